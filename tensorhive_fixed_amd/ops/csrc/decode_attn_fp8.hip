// Decode GQA attention over an FP8 (OCP e4m3fn) KV cache, and the RoPE + quantizing append before it:
// the FP8-cache forms of decode_attn.hip, which stays as it is.
//
// Cache of one layer: K and V codes as [B, Hkv, Smax, 128] bytes, every (b, kv_head) a contiguous run
// of 128-byte rows, and one f32 scale per row, [B, Hkv, Smax]: row = codes * scale, with
// scale = absmax(row) / 448 (1.0 for a row of zeros; ops/decode_attention.quantize_kv_rows).  The
// entry points take the layer's code and scale base pointers, the b / head strides of the codes in
// bytes and those of the scales in floats.  Head dim 128 only.
//
// th_decode_rope_append_fp8  the math of decode_rope_append_kernel (rotated q goes out as bf16, the
//                        same bits); the rotated k row is rounded to bf16 first and then quantized,
//                        the v row is quantized as it comes.  8 lanes own a head row, 16 elements
//                        each (chunk c of both halves, for v too), so every group that reduces the
//                        row's absmax is 8 aligned lanes of one loop trip, all of them active, for
//                        any head counts.  absmax / 448 and x / scale are true f32 divisions (a
//                        reciprocal multiply gives other bits than the CPU rule), the quotient is
//                        clamped to +-448 before v_cvt_pk_fp8_f32.
// th_decode_attn_fp8     decode_attn_kernel's structure on half the bytes: grid (nsplit, Hkv, B), one
//                        workgroup for the rep = Hq/Hkv query heads of its KV head, rows straight to
//                        VGPRs, no LDS staging, a per-lane-group f32 online softmax in base 2, the
//                        wave and LDS merge, the same workspace, split rule and combine kernel (a
//                        copy of its 20 lines: decode_attn.hip is not touched).
//                        Load form, a template parameter (LPR, lanes per row).  rep <= 4: 16-byte
//                        loads with 8 lanes per row (a lane holds 16 dims, a wave reads 8 whole rows
//                        per instruction, QK^T takes 3 DPP steps).  The kernel is bound by VALU work,
//                        not by bytes, and what the 8 or 16 lanes of a row do alike for every
//                        (key, head) (the DPP reduction, the scale, max, exp2, sum) halves per key
//                        with half the lanes: 8-byte loads in the 16-lane layout measured 29.7 / 47.9
//                        us at 4096 / 8192 keys (B 8, 32 / 8 heads) against 25.7 / 39.9 us for this
//                        form and 31.0 / 52.3 us for the bf16 kernel (profiles/decode_kv_fp8/).
//                        rep = 8 keeps 8-byte loads with 16 lanes per row: 16 dims per lane would take
//                        256 VGPRs for q and the accumulators alone.  Both forms keep the bf16
//                        kernel's bytes in flight per lane as two tiles of KT loads: the loop body
//                        handles tile 0 and tile 1 in turn, each with a softmax step over KT keys per
//                        lane group, and refills a register for the tile after next right after its
//                        last use.  Codes are decoded with v_cvt_scalef32_pk_f32_fp8 at scale 1.0
//                        (exact: every finite e4m3 code is an f32), two per instruction, and the pairs
//                        feed v_pk_fma_f32 (QK^T sums even and odd dims apart, then adds the two).
//                        The scales are applied once per key: s = (q . k_codes) * kscale[key], and
//                        p * vscale[key] before the PV FMAs; a key's scale is one 4-byte load shared
//                        by the lanes of its row.  K/V and scale addresses are a uniform base plus a
//                        32-bit lane offset, hence Smax <= 2^24 (host check).
// th_decode_attn_fp8_dev the same body with the split geometry derived on the device from kv_len
//                        (decode_attn.hip's header): same live partials and merge order, same bits.
#include "th_common.h"

#include <type_traits>

namespace {

constexpr int DH = 128;
constexpr int NWAVE = 4;
constexpr float FP8_MAX = 448.f;

typedef unsigned uint2v __attribute__((ext_vector_type(2)));
typedef unsigned uint4v __attribute__((ext_vector_type(4)));
typedef float float2v __attribute__((ext_vector_type(2)));

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
// max of a non-negative value over the 64 lanes of the wave, as a scalar
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

// sum over the aligned groups of 8 lanes, result in every lane: the first three steps of row16_sum
__device__ __forceinline__ float row8_sum(float v) {
  v = dpp_add<0xB1>(v);
  v = dpp_add<0x4E>(v);
  v = dpp_add<0x141>(v);
  return v;
}

// the 4 * W codes of W dwords -> 2 * W pairs of f32 in byte order, exact
template <int W, typename V>
__device__ __forceinline__ void decode(V r, float2v* f) {
#pragma unroll
  for (int w = 0; w < W; ++w) {
    f[2 * w] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8((int)r[w], 1.0f, false);
    f[2 * w + 1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8((int)r[w], 1.0f, true);
  }
}

__device__ __forceinline__ float2v pk_fma(float2v a, float2v b, float2v c) {
  return __builtin_elementwise_fma(a, b, c);  // v_pk_fma_f32: each half is the fmaf of its operands
}

template <int LPR>
struct RowLoad;  // the lane's slice of a 128-byte row
template <>
struct RowLoad<16> {
  typedef uint2v type;
};
template <>
struct RowLoad<8> {
  typedef uint4v type;
};

// Workspace: acc[B*Hq*nsplit][128] f32, then (m, l)[B*Hq*nsplit] f32 pairs; m in the base-2 domain:
// the format of decode_attn.hip.  DEVGEO as there.  LPR: lanes per row, 16 (8-byte loads, 8 dims per
// lane, a wave reads 4 rows per instruction) or 8 (16-byte loads, 16 dims, 8 rows).  KT: keys per lane
// group and softmax step; two such tiles are in flight.
template <int REP, int LPR, int KT, bool DEVGEO>
__global__ __launch_bounds__(256) void decode_attn_fp8_kernel(
    const ushort* __restrict__ q, const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vc,
    const float* __restrict__ ksc, const float* __restrict__ vsc, const int* __restrict__ kv_len,
    float* __restrict__ ws, int Hq, int Hkv, int Smax, long stride_b, long stride_h, long sstride_b,
    long sstride_h, int nsplit, int chunk, int extra, float qscale, int want, int min_keys) {
  const int split = blockIdx.x, hkv = blockIdx.y, b = blockIdx.z;
  const int B = gridDim.z;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  constexpr int DPL = DH / LPR, NP = DPL / 2;  // dims per lane, f32 pairs per lane
  constexpr int RPL = 64 / LPR;                // rows a wave reads per load instruction
  typedef typename RowLoad<LPR>::type rowv;
  const int grp = lane / LPR, dl = lane % LPR;  // key sub-index in a load of RPL rows, DPL-dim slice

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

  float2v qf[REP][NP];
#pragma unroll
  for (int h = 0; h < REP; ++h) {
#pragma unroll
    for (int c = 0; c < DPL / 8; ++c) {
      const ushort8 x =
          *reinterpret_cast<const ushort8*>(q + ((long)b * Hq + hkv * REP + h) * DH + dl * DPL + c * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) qf[h][4 * c + j] = float2v{bf2f(x[2 * j]) * qscale, bf2f(x[2 * j + 1]) * qscale};
    }
  }

  // uniform bases and 32-bit lane offsets (Smax <= 2^24 rows, checked on the host): one address VGPR per load
  const uint8_t* kbase = kc + b * stride_b + hkv * stride_h;
  const uint8_t* vbase = vc + b * stride_b + hkv * stride_h;
  const float* ksbase = ksc + b * sstride_b + hkv * sstride_h;
  const float* vsbase = vsc + b * sstride_b + hkv * sstride_h;
  const int last = (int)end - 1;
  // rows past the chunk are loaded from its last row instead (always a valid one) and masked
  auto row = [&](int key) { return (unsigned)(key < last ? key : last); };
  auto ldc = [&](const uint8_t* base, int key) {
    return *reinterpret_cast<const rowv*>(base + (row(key) * (unsigned)DH + (unsigned)(dl * DPL)));
  };

  float m[REP], l[REP];
  float2v acc[REP][NP];
#pragma unroll
  for (int h = 0; h < REP; ++h) {
    m[h] = -INFINITY;
    l[h] = 0.f;
#pragma unroll
    for (int j = 0; j < NP; ++j) acc[h][j] = float2v{0.f, 0.f};
  }

  constexpr int TILE = NWAVE * RPL * KT;  // keys per workgroup and softmax step
  int key0 = (int)start + wid * RPL * KT + grp;  // this lane's key of load i of tile u: key0 + u * TILE + RPL * i
  rowv kr[2][KT], vr[2][KT];
  float ks[2][KT], vs[2][KT];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
#pragma unroll
    for (int i = 0; i < KT; ++i) {
      kr[u][i] = ldc(kbase, key0 + u * TILE + RPL * i);
      ks[u][i] = ksbase[row(key0 + u * TILE + RPL * i)];
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
#pragma unroll
    for (int i = 0; i < KT; ++i) {
      vr[u][i] = ldc(vbase, key0 + u * TILE + RPL * i);
      vs[u][i] = vsbase[row(key0 + u * TILE + RPL * i)];
    }
  }

  // one softmax step over tile u, whose first key of this lane is k0; refills for the tile at k0 + 2 * TILE
  auto step = [&](auto U, int t0, int k0) {
    constexpr int u = decltype(U)::value;
    const bool full = t0 + TILE <= (int)end;
    const int nkey = k0 + 2 * TILE;
    float s[KT][REP];
#pragma unroll
    for (int i = 0; i < KT; ++i) {
      float2v kf[NP];
      decode<DPL / 4>(kr[u][i], kf);
      const float sc = ks[u][i];
      kr[u][i] = ldc(kbase, nkey + RPL * i);  // refill for the tile after next
      ks[u][i] = ksbase[row(nkey + RPL * i)];
#pragma unroll
      for (int h = 0; h < REP; ++h) {
        float2v d = qf[h][0] * kf[0];  // even and odd dims summed apart, two per instruction
#pragma unroll
        for (int j = 1; j < NP; ++j) d = pk_fma(qf[h][j], kf[j], d);
        const float dd = d[0] + d[1];
        s[i][h] = (LPR == 16 ? row16_sum(dd) : row8_sum(dd)) * sc;
      }
    }
    if (!full) {
#pragma unroll
      for (int i = 0; i < KT; ++i) {
        const bool dead = k0 + RPL * i >= (int)end;
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
        s[i][h] *= vs[u][i];  // p * vscale[key], once per key
      }
      l[h] = l[h] * alpha + ps;
      m[h] = mx;
#pragma unroll
      for (int j = 0; j < NP; ++j) acc[h][j] *= alpha;
    }
#pragma unroll
    for (int i = 0; i < KT; ++i) {
      float2v vf[NP];
      decode<DPL / 4>(vr[u][i], vf);
      vr[u][i] = ldc(vbase, nkey + RPL * i);
      vs[u][i] = vsbase[row(nkey + RPL * i)];
#pragma unroll
      for (int h = 0; h < REP; ++h) {
        const float2v p = float2v{s[i][h], s[i][h]};
#pragma unroll
        for (int j = 0; j < NP; ++j) acc[h][j] = pk_fma(p, vf[j], acc[h][j]);
      }
    }
  };

  for (int t0 = (int)start; t0 < (int)end; t0 += 2 * TILE, key0 += 2 * TILE) {
    step(std::integral_constant<int, 0>{}, t0, key0);
    if (t0 + TILE < (int)end) step(std::integral_constant<int, 1>{}, t0 + TILE, key0 + TILE);
  }

  // merge the lane groups of the wave, then the 4 waves through LDS
  __shared__ float red_acc[NWAVE][REP][DH];
  __shared__ float red_ml[NWAVE][REP][2];
#pragma unroll
  for (int h = 0; h < REP; ++h) {
    float mx = m[h];
#pragma unroll
    for (int o = LPR; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    const float f = mx == -INFINITY ? 0.f : fexp2(m[h] - mx);
    float lv = l[h] * f;
#pragma unroll
    for (int o = LPR; o < 64; o <<= 1) lv += __shfl_xor(lv, o, 64);
    float av[DPL];
#pragma unroll
    for (int j = 0; j < DPL; ++j) {
      float a = acc[h][j >> 1][j & 1] * f;
#pragma unroll
      for (int o = LPR; o < 64; o <<= 1) a += __shfl_xor(a, o, 64);
      av[j] = a;
    }
    if (grp == 0) {
#pragma unroll
      for (int j = 0; j < DPL; ++j) red_acc[wid][h][dl * DPL + j] = av[j];
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

// decode_attn.hip's combine kernel: one block of 128 threads per (b, q_head), partials merged in split order
__global__ __launch_bounds__(128) void decode_combine_fp8_kernel(const float* __restrict__ ws,
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

// 16 f32 -> scale = absmax over the 8 lanes of the row / 448 (1.0 for zeros) and the row's 16 codes of
// this lane, as ops/decode_attention.quantize_kv_rows computes them on the CPU
__device__ __forceinline__ void quantize16(const float* x, float& scale, uint2v& lo, uint2v& hi) {
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) amax = fmaxf(amax, fabsf(x[j]));
  amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
  amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
  amax = fmaxf(amax, __shfl_xor(amax, 4, 64));
  scale = amax / FP8_MAX;  // a true division, as the CPU's
  scale = scale > 0.f ? scale : 1.f;
  float c[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const float v = x[j] / scale;
    c[j] = v != v ? v : fminf(fmaxf(v, -FP8_MAX), FP8_MAX);  // clamp before the cast, NaN stays NaN
  }
  int w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    w[k] = __builtin_amdgcn_cvt_pk_fp8_f32(c[4 * k], c[4 * k + 1], 0, false);
    w[k] = __builtin_amdgcn_cvt_pk_fp8_f32(c[4 * k + 2], c[4 * k + 3], w[k], true);
  }
  lo = uint2v{(unsigned)w[0], (unsigned)w[1]};
  hi = uint2v{(unsigned)w[2], (unsigned)w[3]};
}

__global__ __launch_bounds__(256) void decode_rope_append_fp8_kernel(
    const ushort* __restrict__ qkv, const int* __restrict__ pos, const float* __restrict__ cosT,
    const float* __restrict__ sinT, ushort* __restrict__ q_out, uint8_t* __restrict__ kc,
    uint8_t* __restrict__ vc, float* __restrict__ ksc, float* __restrict__ vsc, int Hq, int Hkv, int Smax,
    long stride_b, long stride_h, long sstride_b, long sstride_h) {
  const int b = blockIdx.x;
  const int p = pos[b];
  if (p < 0 || p >= Smax) return;  // never a table or cache row out of range
  const ushort* in = qkv + (long)b * (Hq + 2 * Hkv) * DH;
  const int nrot = (Hq + Hkv) * 8;  // 8 lanes per rotated head: pair chunk c of both halves
  const int total = nrot + Hkv * 8;  // 8 lanes per v head: chunk c and chunk 8 + c
  // total is a multiple of 8 and blockDim.x one of 64: the 8 lanes of a head row are in one wave and
  // in the same trip, so the absmax shuffles below read active lanes only
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    const int h = i >> 3, c = i & 7;  // h counts q heads, then k heads, then v heads
    const ushort8 x1 = *reinterpret_cast<const ushort8*>(in + h * DH + c * 8);
    const ushort8 x2 = *reinterpret_cast<const ushort8*>(in + h * DH + 64 + c * 8);
    float r[16];     // the row's elements c*8 .. +7 and 64 + c*8 .. +7 as they go to the cache, before quantization
    ushort8 y1, y2;  // the same as bf16, for q
    if (i < nrot) {
      const float4v* cp = reinterpret_cast<const float4v*>(cosT + (long)p * 64 + c * 8);
      const float4v* sp = reinterpret_cast<const float4v*>(sinT + (long)p * 64 + c * 8);
      const float4v c0 = cp[0], c1 = cp[1], s0 = sp[0], s1 = sp[1];
      const float cs[8] = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]};
      const float sn[8] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float a = bf2f(x1[j]), bb = bf2f(x2[j]);
        y1[j] = f2bf(a * cs[j] - bb * sn[j]);
        y2[j] = f2bf(bb * cs[j] + a * sn[j]);
      }
    } else {
      y1 = x1;
      y2 = x2;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      r[j] = bf2f(y1[j]);
      r[8 + j] = bf2f(y2[j]);
    }
    float scale;
    uint2v lo, hi;
    quantize16(r, scale, lo, hi);  // q lanes too: the shuffles stay outside divergent control flow
    if (h < Hq) {
      ushort* out = q_out + ((long)b * Hq + h) * DH;
      *reinterpret_cast<ushort8*>(out + c * 8) = y1;
      *reinterpret_cast<ushort8*>(out + 64 + c * 8) = y2;
    } else {
      const bool isk = h < Hq + Hkv;
      const int hk = isk ? h - Hq : h - Hq - Hkv;
      uint8_t* out = (isk ? kc : vc) + b * stride_b + hk * stride_h + (long)p * DH;
      *reinterpret_cast<uint2v*>(out + c * 8) = lo;
      *reinterpret_cast<uint2v*>(out + 64 + c * 8) = hi;
      if (c == 0) (isk ? ksc : vsc)[b * sstride_b + hk * sstride_h + p] = scale;
    }
  }
}

// cache_geometry_ok of decode_attn.hip with the code strides in bytes (rows 16-byte aligned) and the
// scale strides in floats
bool cache_geometry_fp8_ok(int B, int Hq, int Hkv, int Dh, int Smax, long stride_b, long stride_h,
                           long sstride_b, long sstride_h) {
  if (Dh != DH || B <= 0 || B > 65535 || Hq <= 0 || Hkv <= 0 || Hkv > 65535 || Hq % Hkv || Smax <= 0) return false;
  if (Smax > (1 << 24)) return false;  // the attention kernel's byte offsets inside a (b, head) run are 32-bit
  const int rep = Hq / Hkv;
  if (rep != 1 && rep != 2 && rep != 4 && rep != 8) return false;
  if (stride_h % 16 || stride_b % 16 || stride_h < (long)Smax * DH || stride_b < Hkv * stride_h) return false;
  if (sstride_h < Smax || sstride_b < Hkv * sstride_h) return false;  // heads / sequences do not overlap
  return true;
}

bool pointers_fp8_ok(const void* kc, const void* vc, const void* ksc, const void* vsc) {
  return kc && vc && ksc && vsc && (uintptr_t)kc % 16 == 0 && (uintptr_t)vc % 16 == 0 &&
         (uintptr_t)ksc % 4 == 0 && (uintptr_t)vsc % 4 == 0;
}

}  // namespace

extern "C" int th_decode_rope_append_fp8(const void* qkv, const int* pos, const float* cosT, const float* sinT,
                                         void* q_out, void* kcache, void* vcache, float* kscale, float* vscale,
                                         int B, int Hq, int Hkv, int Dh, int Smax, long stride_b, long stride_h,
                                         long sstride_b, long sstride_h, hipStream_t s) {
  if (!cache_geometry_fp8_ok(B, Hq, Hkv, Dh, Smax, stride_b, stride_h, sstride_b, sstride_h)) return -1;
  if (!pointers_fp8_ok(kcache, vcache, kscale, vscale)) return -1;
  decode_rope_append_fp8_kernel<<<B, 256, 0, s>>>((const ushort*)qkv, pos, cosT, sinT, (ushort*)q_out,
                                                  (uint8_t*)kcache, (uint8_t*)vcache, kscale, vscale, Hq, Hkv,
                                                  Smax, stride_b, stride_h, sstride_b, sstride_h);
  TH_CHECK_LAUNCH();
}

namespace {

template <bool DEVGEO>
int launch_decode_attn_fp8(const void* q, const void* kcache, const void* vcache, const float* kscale,
                           const float* vscale, const int* kv_len, void* o, float* ws, int B, int Hq, int Hkv,
                           int Smax, long stride_b, long stride_h, long sstride_b, long sstride_h, int nsplit,
                           int chunk, int extra, float scale, int want, int min_keys, hipStream_t s) {
  const dim3 grid(nsplit, Hkv, B);
  const float qscale = scale * 1.4426950408889634f;  // scores in the base-2 domain
  const ushort* qp = (const ushort*)q;
  const uint8_t *kp = (const uint8_t*)kcache, *vp = (const uint8_t*)vcache;
#define TH_DECODE_LAUNCH(REP, LPR, KT)                                                                    \
  decode_attn_fp8_kernel<REP, LPR, KT, DEVGEO><<<grid, 256, 0, s>>>(                                      \
      qp, kp, vp, kscale, vscale, kv_len, ws, Hq, Hkv, Smax, stride_b, stride_h, sstride_b, sstride_h,    \
      nsplit, chunk, extra, qscale, want, min_keys)
  switch (Hq / Hkv) {  // 2 tiles x KT loads x 128 / LPR bytes of K and of V in flight per lane, as decode_attn.hip
    case 1: TH_DECODE_LAUNCH(1, 8, 4); break;
    case 2: TH_DECODE_LAUNCH(2, 8, 4); break;
    case 4: TH_DECODE_LAUNCH(4, 8, 4); break;
    default: TH_DECODE_LAUNCH(8, 16, 4); break;  // 16 dims per lane would take 256 VGPRs for q and o alone
  }
#undef TH_DECODE_LAUNCH
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  decode_combine_fp8_kernel<<<B * Hq, 128, 0, s>>>(ws, (ushort*)o, (long)B * Hq * nsplit, nsplit);
  TH_CHECK_LAUNCH();
}

}  // namespace

// ws: B * Hq * nsplit * 130 floats.  Keys [split * chunk, +chunk) go to split `split` (the last one
// takes the rest); kv_len[b] + extra keys are valid, clamped to [0, Smax] on the device.
extern "C" int th_decode_attn_fp8(const void* q, const void* kcache, const void* vcache, const float* kscale,
                                  const float* vscale, const int* kv_len, void* o, float* ws, int B, int Hq,
                                  int Hkv, int Dh, int Smax, long stride_b, long stride_h, long sstride_b,
                                  long sstride_h, int nsplit, int chunk, int extra, float scale, hipStream_t s) {
  if (!cache_geometry_fp8_ok(B, Hq, Hkv, Dh, Smax, stride_b, stride_h, sstride_b, sstride_h)) return -1;
  if (!pointers_fp8_ok(kcache, vcache, kscale, vscale)) return -1;
  if (nsplit <= 0 || nsplit > 1024 || chunk <= 0 || (long)nsplit * chunk > (1L << 30)) return -1;
  return launch_decode_attn_fp8<false>(q, kcache, vcache, kscale, vscale, kv_len, o, ws, B, Hq, Hkv, Smax,
                                       stride_b, stride_h, sstride_b, sstride_h, nsplit, chunk, extra, scale, 0,
                                       1, s);
}

// The same with the geometry taken from kv_len on the device: the grid and the workspace
// (B * Hq * nsplit_cap * 130 floats) are fixed by nsplit_cap, whatever the lengths become.
extern "C" int th_decode_attn_fp8_dev(const void* q, const void* kcache, const void* vcache, const float* kscale,
                                      const float* vscale, const int* kv_len, void* o, float* ws, int B, int Hq,
                                      int Hkv, int Dh, int Smax, long stride_b, long stride_h, long sstride_b,
                                      long sstride_h, int nsplit_cap, int want, int min_keys, int extra,
                                      float scale, hipStream_t s) {
  if (!cache_geometry_fp8_ok(B, Hq, Hkv, Dh, Smax, stride_b, stride_h, sstride_b, sstride_h)) return -1;
  if (!pointers_fp8_ok(kcache, vcache, kscale, vscale)) return -1;
  if (nsplit_cap <= 0 || nsplit_cap > 1024 || want <= 0 || min_keys <= 0) return -1;
  return launch_decode_attn_fp8<true>(q, kcache, vcache, kscale, vscale, kv_len, o, ws, B, Hq, Hkv, Smax,
                                      stride_b, stride_h, sstride_b, sstride_h, nsplit_cap, 0, extra, scale,
                                      want, min_keys, s);
}
