// Single-token (decode) GQA attention over a KV cache, and the RoPE + cache-append step before it.
//
// Cache of one layer: K and V as [B, Hkv, Smax, 128] bf16, every (b, kv_head) a contiguous run of
// 256-byte rows; the entry points take the layer's K / V base pointers and the b / head strides
// in elements.  Head dim 128 only.
//
// th_decode_rope_append  rotates the new token's q and k at pos[b] (rotate-half pairs (i, i+64),
//                        as rope.hip), writes q to q_out and k / v into cache row pos[b].
// th_decode_attn         split-KV attention: grid (nsplit, Hkv, B), one workgroup serves all
//                        rep = Hq/Hkv query heads of its KV head over one chunk of keys, so K and V
//                        are read from HBM once per KV head.  This is an HBM-bound stream with at
//                        most 8 query rows: K/V rows go straight to VGPRs with 16-byte loads (a
//                        wave reads 4 whole rows per instruction), each register is refilled for
//                        the next tile right after its last use (a full tile stays in flight, the
//                        compiler counts vmcnt down), no LDS staging.  The 16 lanes of a row hold
//                        8 dims each; QK^T is reduced over them with DPP adds.  Each 16-lane group
//                        of each wave runs its own online softmax (f32, base 2) over the keys it
//                        owns; the 16 partial states of a workgroup are merged once at the end
//                        (shuffles inside the wave, LDS across waves) and written as
//                        (m, l, acc[rep][128]) f32 to the caller's workspace.
//                        th_decode_attn then runs the combine kernel: the nsplit partials of every
//                        (b, q_head) merged in split order, no atomics -> bit-reproducible bf16 o.
// th_decode_attn_dev     the same kernel body under a grid fixed by the caller, (nsplit_cap, Hkv, B), for
//                        a launch captured into a graph: the split geometry is derived on the device
//                        from kv_len, which grows between replays.  Every workgroup reduces the B
//                        lengths itself (each wave: a strided loop over kv_len and a cross-lane max in DPP steps, so
//                        no LDS, no barrier and no second kernel; B <= 65535, in practice <= 64, and the
//                        lengths are L2 hits) and applies the host rule of ops/decode_attention.py:
//                          longest = max_b clamp(kv_len[b] + extra, 0, Smax)
//                          ns_eff  = max(1, min(want, longest / min_keys, nsplit_cap))
//                          chunk   = max(1, ceil(longest / ns_eff))
//                        Splits >= ns_eff read nothing and write the neutral element, which the
//                        combine kernel (run over nsplit_cap partials) skips, so the live partials and
//                        their merge order are those of th_decode_attn with (ns_eff, chunk): the same
//                        bits.
#include "th_common.h"

namespace {

constexpr int DH = 128;
constexpr int NWAVE = 4;

template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  const int t = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true);
  return v + __int_as_float(t);
}
// sum over the 16 lanes of a DPP row, result in every lane: xor 1, xor 2, half mirror, mirror
__device__ __forceinline__ float row16_sum(float v) {
  v = dpp_add<0xB1>(v);   // quad_perm [1,0,3,2]
  v = dpp_add<0x4E>(v);   // quad_perm [2,3,0,1]
  v = dpp_add<0x141>(v);  // row_half_mirror
  v = dpp_add<0x140>(v);  // row_mirror
  return v;
}

template <int CTRL>
__device__ __forceinline__ int dpp_max(int v) {
  const int t = __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
  return v > t ? v : t;
}
// max of a non-negative value over the 64 lanes of the wave, as a scalar: the DPP steps of row16_sum,
// then one lane of each of the 4 rows
__device__ __forceinline__ int wave_max(int v) {
  v = dpp_max<0xB1>(v);
  v = dpp_max<0x4E>(v);
  v = dpp_max<0x141>(v);
  v = dpp_max<0x140>(v);
  const int a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
  const int c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
  const int ab = a > b ? a : b, cd = c > d ? c : d;
  return ab > cd ? ab : cd;
}

__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }

// Workspace: acc[B*Hq*nsplit][128] f32, then (m, l)[B*Hq*nsplit] f32 pairs; m in the base-2 domain.
// DEVGEO: nsplit is the grid's split count (the workspace stride) only, `chunk` is not read, and the
// live split count and chunk come from kv_len, want and min_keys (header comment).
template <int REP, int KT, bool DEVGEO>
__global__ __launch_bounds__(256) void decode_attn_kernel(
    const ushort* __restrict__ q, const ushort* __restrict__ kc, const ushort* __restrict__ vc,
    const int* __restrict__ kv_len, float* __restrict__ ws, int Hq, int Hkv, int Smax, long stride_b,
    long stride_h, int nsplit, int chunk, int extra, float qscale, int want, int min_keys) {
  const int split = blockIdx.x, hkv = blockIdx.y, b = blockIdx.z;
  const int B = gridDim.z;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int grp = lane >> 4, dl = lane & 15;  // key sub-index in a 4-row load, 8-dim slice

  float* ws_acc = ws;
  float* ws_ml = ws + (long)B * Hq * nsplit * DH;
  const long part0 = ((long)b * Hq + (long)hkv * REP) * nsplit + split;  // + h * nsplit per head

  long len = (long)kv_len[b] + extra;
  len = len < 0 ? 0 : (len > Smax ? Smax : len);  // before any address is formed
  int ns_eff = nsplit;
  if constexpr (DEVGEO) {
    int longest = 0;
    for (int i = lane; i < B; i += 64) {
      long n = (long)kv_len[i] + extra;
      n = n < 0 ? 0 : (n > Smax ? Smax : n);
      longest = longest > (int)n ? longest : (int)n;
    }
    longest = wave_max(longest);  // a scalar: the geometry below stays in SGPRs
    ns_eff = (int)((unsigned)longest / (unsigned)min_keys);
    ns_eff = ns_eff < want ? ns_eff : want;
    ns_eff = ns_eff < nsplit ? ns_eff : nsplit;  // the last live split must be in the grid
    ns_eff = ns_eff > 1 ? ns_eff : 1;
    chunk = (int)((unsigned)(longest + ns_eff - 1) / (unsigned)ns_eff);
    chunk = chunk > 1 ? chunk : 1;
  }
  const long start = (long)split * chunk;
  long end = split == ns_eff - 1 ? len : start + chunk;
  end = end > len ? len : end;
  if ((DEVGEO && split >= ns_eff) || start >= end) {  // nothing to read: the neutral element
    for (int i = tid; i < REP * DH; i += 256) ws_acc[(part0 + (long)(i >> 7) * nsplit) * DH + (i & 127)] = 0.f;
    if (tid < REP) {
      ws_ml[(part0 + (long)tid * nsplit) * 2] = -INFINITY;
      ws_ml[(part0 + (long)tid * nsplit) * 2 + 1] = 0.f;
    }
    return;
  }

  float qf[REP][8];
#pragma unroll
  for (int h = 0; h < REP; ++h) {
    const ushort8 x = *reinterpret_cast<const ushort8*>(q + ((long)b * Hq + hkv * REP + h) * DH + dl * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[h][j] = bf2f(x[j]) * qscale;
  }

  const ushort* kbase = kc + b * stride_b + hkv * stride_h + dl * 8;
  const ushort* vbase = vc + b * stride_b + hkv * stride_h + dl * 8;
  const int last = (int)end - 1;
  // rows past the chunk are loaded from its last row instead (always a valid one) and masked
  auto row = [&](int key) { return (long)(key < last ? key : last) * DH; };

  float m[REP], l[REP], acc[REP][8];
#pragma unroll
  for (int h = 0; h < REP; ++h) {
    m[h] = -INFINITY;
    l[h] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[h][j] = 0.f;
  }

  constexpr int TILE = NWAVE * 4 * KT;  // keys per workgroup step
  int key0 = (int)start + wid * 4 * KT + grp;  // this lane's key of load i: key0 + 4 * i
  ushort8 kr[KT], vr[KT];
#pragma unroll
  for (int i = 0; i < KT; ++i) kr[i] = *reinterpret_cast<const ushort8*>(kbase + row(key0 + 4 * i));
#pragma unroll
  for (int i = 0; i < KT; ++i) vr[i] = *reinterpret_cast<const ushort8*>(vbase + row(key0 + 4 * i));

  for (int t0 = (int)start; t0 < (int)end; t0 += TILE, key0 += TILE) {
    const bool full = t0 + TILE <= (int)end;
    const int nkey = key0 + TILE;
    float s[KT][REP];
#pragma unroll
    for (int i = 0; i < KT; ++i) {
      float kf[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) kf[j] = bf2f(kr[i][j]);
      kr[i] = *reinterpret_cast<const ushort8*>(kbase + row(nkey + 4 * i));  // refill for the next tile
#pragma unroll
      for (int h = 0; h < REP; ++h) {
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) d = fmaf(qf[h][j], kf[j], d);
        s[i][h] = row16_sum(d);
      }
    }
    if (!full) {
#pragma unroll
      for (int i = 0; i < KT; ++i) {
        const bool dead = key0 + 4 * i >= (int)end;
#pragma unroll
        for (int h = 0; h < REP; ++h) s[i][h] = dead ? -INFINITY : s[i][h];
      }
    }
#pragma unroll
    for (int h = 0; h < REP; ++h) {
      float mx = m[h];
#pragma unroll
      for (int i = 0; i < KT; ++i) mx = fmaxf(mx, s[i][h]);
      const float ms = mx == -INFINITY ? 0.f : mx;  // a group that has seen no live key yet
      const float alpha = fexp2(m[h] - ms);
      float ps = 0.f;
#pragma unroll
      for (int i = 0; i < KT; ++i) {
        s[i][h] = fexp2(s[i][h] - ms);
        ps += s[i][h];
      }
      l[h] = l[h] * alpha + ps;
      m[h] = mx;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[h][j] *= alpha;
    }
#pragma unroll
    for (int i = 0; i < KT; ++i) {
      float vf[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) vf[j] = bf2f(vr[i][j]);
      vr[i] = *reinterpret_cast<const ushort8*>(vbase + row(nkey + 4 * i));
#pragma unroll
      for (int h = 0; h < REP; ++h)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[h][j] = fmaf(s[i][h], vf[j], acc[h][j]);
    }
  }

  // merge the 4 lane groups of the wave, then the 4 waves through LDS
  __shared__ float red_acc[NWAVE][REP][DH];
  __shared__ float red_ml[NWAVE][REP][2];
#pragma unroll
  for (int h = 0; h < REP; ++h) {
    float mx = fmaxf(m[h], __shfl_xor(m[h], 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float f = mx == -INFINITY ? 0.f : fexp2(m[h] - mx);
    float lv = l[h] * f;
    lv += __shfl_xor(lv, 16, 64);
    lv += __shfl_xor(lv, 32, 64);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float a = acc[h][j] * f;
      a += __shfl_xor(a, 16, 64);
      a += __shfl_xor(a, 32, 64);
      acc[h][j] = a;
    }
    if (grp == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) red_acc[wid][h][dl * 8 + j] = acc[h][j];
      if (dl == 0) {
        red_ml[wid][h][0] = mx;
        red_ml[wid][h][1] = lv;
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < REP * DH; i += 256) {
    const int h = i >> 7, d = i & 127;
    float mx = red_ml[0][h][0];
#pragma unroll
    for (int w = 1; w < NWAVE; ++w) mx = fmaxf(mx, red_ml[w][h][0]);
    float a = 0.f, lv = 0.f;
#pragma unroll
    for (int w = 0; w < NWAVE; ++w) {
      const float mw = red_ml[w][h][0];
      const float f = mw == -INFINITY ? 0.f : fexp2(mw - mx);
      a += red_acc[w][h][d] * f;
      lv += red_ml[w][h][1] * f;
    }
    const long p = part0 + (long)h * nsplit;
    ws_acc[p * DH + d] = a;
    if (d == 0) {
      ws_ml[p * 2] = mx;
      ws_ml[p * 2 + 1] = lv;
    }
  }
}

// one block of 128 threads per (b, q_head): partials merged in split order
__global__ __launch_bounds__(128) void decode_combine_kernel(const float* __restrict__ ws,
                                                             ushort* __restrict__ o, long nparts,
                                                             int nsplit) {
  const long bh = blockIdx.x;
  const int d = threadIdx.x;
  const float* acc = ws + bh * nsplit * DH;
  const float* ml = ws + nparts * DH + bh * nsplit * 2;
  float mx = -INFINITY;
  for (int s = 0; s < nsplit; ++s) mx = fmaxf(mx, ml[2 * s]);
  float a = 0.f, lv = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float ms = ml[2 * s];
    if (ms == -INFINITY) continue;  // an empty split
    const float f = fexp2(ms - mx);
    a += acc[(long)s * DH + d] * f;
    lv += ml[2 * s + 1] * f;
  }
  o[bh * DH + d] = f2bf(lv > 0.f ? a / lv : 0.f);  // no live key at all: zeros
}

__global__ __launch_bounds__(256) void decode_rope_append_kernel(
    const ushort* __restrict__ qkv, const int* __restrict__ pos, const float* __restrict__ cosT,
    const float* __restrict__ sinT, ushort* __restrict__ q_out, ushort* __restrict__ kc,
    ushort* __restrict__ vc, int Hq, int Hkv, int Smax, long stride_b, long stride_h) {
  const int b = blockIdx.x;
  const int p = pos[b];
  if (p < 0 || p >= Smax) return;  // never a table or cache row out of range
  const ushort* in = qkv + (long)b * (Hq + 2 * Hkv) * DH;
  const int nrot = (Hq + Hkv) * 8;  // 8-pair chunks of the rotated heads
  const int total = nrot + Hkv * 16;  // + 16-byte chunks of v
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    if (i < nrot) {
      const int h = i >> 3, c = i & 7;
      const ushort8 x1 = *reinterpret_cast<const ushort8*>(in + h * DH + c * 8);
      const ushort8 x2 = *reinterpret_cast<const ushort8*>(in + h * DH + 64 + c * 8);
      const float4v* cp = reinterpret_cast<const float4v*>(cosT + (long)p * 64 + c * 8);
      const float4v* sp = reinterpret_cast<const float4v*>(sinT + (long)p * 64 + c * 8);
      const float4v c0 = cp[0], c1 = cp[1], s0 = sp[0], s1 = sp[1];
      const float cs[8] = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]};
      const float sn[8] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};
      ushort8 y1, y2;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float a = bf2f(x1[j]), bb = bf2f(x2[j]);
        y1[j] = f2bf(a * cs[j] - bb * sn[j]);
        y2[j] = f2bf(bb * cs[j] + a * sn[j]);
      }
      ushort* out = h < Hq ? q_out + ((long)b * Hq + h) * DH
                           : kc + b * stride_b + (h - Hq) * stride_h + (long)p * DH;
      *reinterpret_cast<ushort8*>(out + c * 8) = y1;
      *reinterpret_cast<ushort8*>(out + 64 + c * 8) = y2;
    } else {
      const int h = (i - nrot) >> 4, c = (i - nrot) & 15;
      const ushort8 x = *reinterpret_cast<const ushort8*>(in + (Hq + Hkv + h) * DH + c * 8);
      *reinterpret_cast<ushort8*>(vc + b * stride_b + h * stride_h + (long)p * DH + c * 8) = x;
    }
  }
}

bool cache_geometry_ok(int B, int Hq, int Hkv, int Dh, int Smax, long stride_b, long stride_h) {
  if (Dh != DH || B <= 0 || B > 65535 || Hq <= 0 || Hkv <= 0 || Hkv > 65535 || Hq % Hkv || Smax <= 0) return false;
  const int rep = Hq / Hkv;
  if (rep != 1 && rep != 2 && rep != 4 && rep != 8) return false;
  // rows are 16-byte aligned and heads / sequences do not overlap
  if (stride_h % 8 || stride_b % 8 || stride_h < (long)Smax * DH || stride_b < Hkv * stride_h) return false;
  return true;
}

}  // namespace

extern "C" int th_decode_rope_append(const void* qkv, const int* pos, const float* cosT, const float* sinT,
                                     void* q_out, void* kcache, void* vcache, int B, int Hq, int Hkv,
                                     int Dh, int Smax, long stride_b, long stride_h, hipStream_t s) {
  if (!cache_geometry_ok(B, Hq, Hkv, Dh, Smax, stride_b, stride_h)) return -1;
  decode_rope_append_kernel<<<B, 256, 0, s>>>((const ushort*)qkv, pos, cosT, sinT, (ushort*)q_out,
                                              (ushort*)kcache, (ushort*)vcache, Hq, Hkv, Smax,
                                              stride_b, stride_h);
  TH_CHECK_LAUNCH();
}

namespace {

template <bool DEVGEO>
int launch_decode_attn(const void* q, const void* kcache, const void* vcache, const int* kv_len, void* o,
                       float* ws, int B, int Hq, int Hkv, int Smax, long stride_b, long stride_h,
                       int nsplit, int chunk, int extra, float scale, int want, int min_keys,
                       hipStream_t s) {
  const dim3 grid(nsplit, Hkv, B);
  const float qscale = scale * 1.4426950408889634f;  // scores in the base-2 domain
  const ushort *qp = (const ushort*)q, *kp = (const ushort*)kcache, *vp = (const ushort*)vcache;
#define TH_DECODE_LAUNCH(REP, KT)                                                                      \
  decode_attn_kernel<REP, KT, DEVGEO><<<grid, 256, 0, s>>>(qp, kp, vp, kv_len, ws, Hq, Hkv, Smax,      \
                                                           stride_b, stride_h, nsplit, chunk, extra,   \
                                                           qscale, want, min_keys)
  switch (Hq / Hkv) {
    case 1: TH_DECODE_LAUNCH(1, 8); break;
    case 2: TH_DECODE_LAUNCH(2, 8); break;
    case 4: TH_DECODE_LAUNCH(4, 8); break;
    default: TH_DECODE_LAUNCH(8, 4); break;
  }
#undef TH_DECODE_LAUNCH
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  decode_combine_kernel<<<B * Hq, 128, 0, s>>>(ws, (ushort*)o, (long)B * Hq * nsplit, nsplit);
  TH_CHECK_LAUNCH();
}

}  // namespace

// ws: B * Hq * nsplit * 130 floats.  Keys [split * chunk, +chunk) go to split `split` (the last one
// takes the rest); kv_len[b] + extra keys are valid, clamped to [0, Smax] on the device.
extern "C" int th_decode_attn(const void* q, const void* kcache, const void* vcache, const int* kv_len,
                              void* o, float* ws, int B, int Hq, int Hkv, int Dh, int Smax,
                              long stride_b, long stride_h, int nsplit, int chunk, int extra,
                              float scale, hipStream_t s) {
  if (!cache_geometry_ok(B, Hq, Hkv, Dh, Smax, stride_b, stride_h)) return -1;
  if (nsplit <= 0 || nsplit > 1024 || chunk <= 0 || (long)nsplit * chunk > (1L << 30)) return -1;
  return launch_decode_attn<false>(q, kcache, vcache, kv_len, o, ws, B, Hq, Hkv, Smax, stride_b, stride_h,
                                   nsplit, chunk, extra, scale, 0, 1, s);
}

// The same with the geometry taken from kv_len on the device (header comment): the grid and the
// workspace (B * Hq * nsplit_cap * 130 floats) are fixed by nsplit_cap, whatever the lengths become.
extern "C" int th_decode_attn_dev(const void* q, const void* kcache, const void* vcache, const int* kv_len,
                                  void* o, float* ws, int B, int Hq, int Hkv, int Dh, int Smax,
                                  long stride_b, long stride_h, int nsplit_cap, int want, int min_keys,
                                  int extra, float scale, hipStream_t s) {
  if (!cache_geometry_ok(B, Hq, Hkv, Dh, Smax, stride_b, stride_h)) return -1;
  if (nsplit_cap <= 0 || nsplit_cap > 1024 || want <= 0 || min_keys <= 0) return -1;
  return launch_decode_attn<true>(q, kcache, vcache, kv_len, o, ws, B, Hq, Hkv, Smax, stride_b, stride_h,
                                  nsplit_cap, 0, extra, scale, want, min_keys, s);
}
