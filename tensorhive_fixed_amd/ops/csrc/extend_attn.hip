// Multi-token ("block") decode: T new tokens per sequence on top of a bf16 KV cache, T = 1..8.
//
// Cache of one layer as in decode_attn.hip: K and V as [B, Hkv, Smax, 128] bf16, the entry points
// take the layer's K / V base pointers and the b / head strides in elements.  Head dim 128 only.
//
// th_decode_rope_append_block  row (b, t) of qkv [B, T, (Hq+2*Hkv)*128] is rotated at pos[b] + t; its
//                        k / v go into cache row pos[b] + t and its q into q_out [B, T, Hq*128].  The
//                        arithmetic per element is that of th_decode_rope_append, so the bits are
//                        those of T single appends.
// th_extend_attn         query row (b, t, h) attends over cache rows [0, kv_len[b] + t + 1) of its KV
//                        head (causal inside the new block, which was appended before the call; the
//                        lengths have not moved yet).  Grid (nsplit, Hkv, B) and the split rule of
//                        th_decode_attn; one workgroup serves all R = rep * T query rows of its KV head
//                        (row r = t * rep + h, padded to NQ tiles of 16 by repeating the last row) over
//                        its chunk, so K and V leave HBM once per KV head whatever T is.
//
//   Both products run on v_mfma_f32_16x16x32_bf16, with the query on the lane:
//     S^T = K Q^T      A = 16 K rows, 16-byte loads straight from HBM to VGPRs (lane l: row l & 15,
//                      dims 32 s + 8 (l >> 4) + j in k-step s), B = Q rows, in registers for the whole
//                      kernel (unscaled: the scale goes into the exp2 argument in f32).
//     O^T += V^T P^T   B = P^T, packed to bf16 in place from the S^T accumulators of two 16-key
//                      tiles: element j of lane group g is key 4 g + j of the first tile (j < 4) or
//                      key 4 g + j - 4 of the second.  A = V^T in that key order: every wave stages
//                      its 32 V rows in its own LDS slab (288-byte pitch: the transposed reads of a
//                      32-lane half then cover all 64 banks once) and reads them back with
//                      ds_read_b64_tr_b16.  The slab is private to the wave, so the key loop has no
//                      barrier.
//   A wave owns 32 keys per step, the workgroup 128.  K and V registers are refilled for the next
//   step right after their last use.  Running max and sum (f32, base 2) are per lane and q tile; the
//   max is made uniform over the 4 lane groups each step (2 shuffles), the sum once at the end.  Keys
//   past the chunk are loaded from its last row and masked; only steps that reach the last T keys
//   or the chunk's end run the mask.  A query row with no live key in the chunk keeps
//   (m, l, acc) = (-inf, 0, 0), the neutral element.  The 4 waves are merged through LDS in wave
//   order and written as (m, l, acc[128]) f32 per (b, t, q_head, split); the combine kernel merges the
//   splits in split order, no atomics: two runs give the same bits.
// th-build-flags: -fno-slp-vectorize
#include "th_common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef unsigned uint4v __attribute__((ext_vector_type(4)));
#define LDS_AS __attribute__((address_space(3)))

namespace {

constexpr int DH = 128;
constexpr int NWAVE = 4;
constexpr int WKEYS = 32;             // keys of one wave per step: two 16-key MFMA tiles
constexpr int TILE = NWAVE * WKEYS;   // keys of the workgroup per step
constexpr int VPITCH = 288;           // bytes per staged V row
constexpr int MAX_T = 8;

__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ float4v mfma(ushort8 a, ushort8 b, float4v c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
                                                 c, 0, 0, 0);
}

// Workspace: acc[B*T*Hq*nsplit][128] f32, then (m, l)[B*T*Hq*nsplit] f32 pairs; m in the base-2 domain.
template <int NQ>
__global__ __launch_bounds__(256) void extend_attn_kernel(
    const ushort* __restrict__ q, const ushort* __restrict__ kc, const ushort* __restrict__ vc,
    const int* __restrict__ kv_len, float* __restrict__ ws, int Hq, int Hkv, int Smax, long stride_b,
    long stride_h, int nsplit, int chunk, int T, int rep_shift, float qscale) {
  const int split = blockIdx.x, hkv = blockIdx.y, b = blockIdx.z;
  const int B = gridDim.z;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int rep = 1 << rep_shift, R = rep * T;  // R <= 16 * NQ

  float* ws_acc = ws;
  float* ws_ml = ws + (long)B * T * Hq * nsplit * DH;
  auto part = [&](int r) {  // the partial of query row r
    const int t = r >> rep_shift, hh = r & (rep - 1);
    return (((long)b * T + t) * Hq + hkv * rep + hh) * nsplit + split;
  };

  long len0 = kv_len[b];
  len0 = len0 < 0 ? 0 : (len0 > Smax ? Smax : len0);  // before any address is formed
  const long lenT = len0 + T > Smax ? Smax : len0 + T;
  const long start = (long)split * chunk;
  const int end = (int)(start + chunk > lenT ? lenT : start + chunk);
  if (start >= end) {  // nothing to read: the neutral element
    for (int i = tid; i < R * DH; i += 256) ws_acc[part(i >> 7) * DH + (i & 127)] = 0.f;
    if (tid < R) {
      ws_ml[part(tid) * 2] = -INFINITY;
      ws_ml[part(tid) * 2 + 1] = 0.f;
    }
    return;
  }

  // staged V rows of the 4 waves; after the key loop the merge buffer [dim][query] (odd pitch)
  constexpr int PQ = NQ * 16 + 1;
  constexpr int SMEM = NWAVE * WKEYS * VPITCH > DH * PQ * 4 ? NWAVE * WKEYS * VPITCH : DH * PQ * 4;
  __shared__ __attribute__((aligned(16))) char smem[SMEM];
  __shared__ float red_m[NWAVE][NQ * 16], red_l[NWAVE][NQ * 16];

  ushort8 qf[NQ][4];
  int tq[NQ];  // this lane's query's index in the block: it attends to keys < min(len0 + tq + 1, end)
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    int r = n * 16 + c;
    r = r < R ? r : R - 1;  // padding rows repeat the last real one and are never written
    const int t = r >> rep_shift, hh = r & (rep - 1);
    const ushort* qp = q + (((long)b * T + t) * Hq + hkv * rep + hh) * DH + 8 * g;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[n][s] = *reinterpret_cast<const ushort8*>(qp + 32 * s);
    tq[n] = t;
  }
  const int lim_min = len0 + 1 < end ? (int)(len0 + 1) : end;  // steps below it need no mask

  const ushort* kbase = kc + b * stride_b + hkv * stride_h + 8 * g;
  const ushort* vbase = vc + b * stride_b + hkv * stride_h + 8 * c;
  const int last = end - 1;
  // rows past the chunk are loaded from its last row instead (always a valid one) and masked
  auto row = [&](int key) { return (long)(key < last ? key : last) * DH; };

  char* vl = smem + wid * (WKEYS * VPITCH);
  // transposed read: lane 4 q + p of a group addresses row q, dims 4 p .. 4 p + 3 of the block
  const char* vt = vl + (4 * g + (c >> 2)) * VPITCH + (c & 3) * 8;

  float m[NQ], l[NQ];
  float4v acc[NQ][8];
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    m[n] = -INFINITY;
    l[n] = 0.f;
#pragma unroll
    for (int d = 0; d < 8; ++d) acc[n][d] = float4v{0.f, 0.f, 0.f, 0.f};
  }

  int kb = (int)start + wid * WKEYS;  // first key of this wave's step
  ushort8 kr[2][4], vr[8];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int s = 0; s < 4; ++s) kr[x][s] = *reinterpret_cast<const ushort8*>(kbase + row(kb + 16 * x + c) + 32 * s);
#pragma unroll
  for (int i = 0; i < 8; ++i) vr[i] = *reinterpret_cast<const ushort8*>(vbase + row(kb + 4 * i + g));

  for (int t0 = (int)start; t0 < end; t0 += TILE, kb += TILE) {
    const bool live = kb < end;  // wave-uniform; otherwise every key of the step is past the chunk
    const bool masked = kb + WKEYS > lim_min;  // wave-uniform: the step reaches the new block or the chunk's end
    ushort8 pf[NQ];
    if (live) {
#pragma unroll
      for (int n = 0; n < NQ; ++n) {
        float4v sc[2];
#pragma unroll
        for (int x = 0; x < 2; ++x) {
          sc[x] = float4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < 4; ++s) sc[x] = mfma(kr[x][s], qf[n][s], sc[x]);
        }
        if (masked) {
          const int lt = (int)len0 + tq[n] + 1, lim = lt < end ? lt : end;
#pragma unroll
          for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int j = 0; j < 4; ++j) sc[x][j] = kb + 16 * x + 4 * g + j < lim ? sc[x][j] : -INFINITY;
        }
        float mx = fmaxf(fmaxf(sc[0][0], sc[0][1]), fmaxf(sc[0][2], sc[0][3]));
        mx = fmaxf(mx, fmaxf(fmaxf(sc[1][0], sc[1][1]), fmaxf(sc[1][2], sc[1][3])));
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        mx = fmaxf(m[n], mx * qscale);
        const float ms = mx == -INFINITY ? 0.f : mx;  // no live key yet
        const float alpha = fexp2(m[n] - ms);
        float ps = 0.f;
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float p = fexp2(fmaf(sc[x][j], qscale, -ms));
            ps += p;
            pf[n][4 * x + j] = f2bf(p);
          }
        l[n] = l[n] * alpha + ps;
        m[n] = mx;
#pragma unroll
        for (int d = 0; d < 8; ++d) acc[n][d] *= alpha;
      }
    }
#pragma unroll
    for (int x = 0; x < 2; ++x) {  // refill for the next step
      const ushort* kp = kbase + row(kb + TILE + 16 * x + c);
#pragma unroll
      for (int s = 0; s < 4; ++s) kr[x][s] = *reinterpret_cast<const ushort8*>(kp + 32 * s);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      *reinterpret_cast<ushort8*>(vl + (4 * i + g) * VPITCH + c * 16) = vr[i];
      vr[i] = *reinterpret_cast<const ushort8*>(vbase + row(kb + TILE + 4 * i + g));
    }
    if (!live) continue;

    // the slab is this wave's own: its stores above are ordered before these reads, and the reads
    // before the next step's stores, by the wave's in-order LDS queue
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    auto vfrag = [&](int d) {
      const i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS i16x4*)(vt + d * 32));
      const i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS i16x4*)(vt + 16 * VPITCH + d * 32));
      return uint4v{(unsigned)(ushort)lo[0] | (unsigned)lo[1] << 16, (unsigned)(ushort)lo[2] | (unsigned)lo[3] << 16,
                    (unsigned)(ushort)hi[0] | (unsigned)hi[1] << 16, (unsigned)(ushort)hi[2] | (unsigned)hi[3] << 16};
    };
    if (kb + WKEYS <= len0 + 1) {  // wave-uniform: every query sees every key of the step below the chunk's end
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        const ushort8 vf = __builtin_bit_cast(ushort8, vfrag(d));
#pragma unroll
        for (int n = 0; n < NQ; ++n) acc[n][d] = mfma(vf, pf[n], acc[n][d]);
      }
    } else {
      // The step holds keys of the new block that some queries must not see.  A zero in P does not
      // keep such a V row out of the product (0 * NaN), so the step runs once per block index tt, on V
      // with the rows past key len0 + tt zeroed, and a lane takes the result only where its query is tt.
      for (int tt = 0; tt < T; ++tt) {
        const int vis = (int)len0 + tt;  // the last key a query at tt sees
        uint4v vmask;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const int key = kb + 16 * (w >> 1) + 4 * g + 2 * (w & 1);  // of elements 2 w and 2 w + 1
          vmask[w] = (key <= vis ? 0xFFFFu : 0u) | (key + 1 <= vis ? 0xFFFF0000u : 0u);
        }
#pragma unroll
        for (int d = 0; d < 8; ++d) {
          const ushort8 vf = __builtin_bit_cast(ushort8, vfrag(d) & vmask);
#pragma unroll
          for (int n = 0; n < NQ; ++n) {
            const int rlast = n * 16 + 15 < R - 1 ? n * 16 + 15 : R - 1;
            if (tt < (n * 16) >> rep_shift || tt > rlast >> rep_shift) continue;  // no query of tile n is at tt
            const float4v x = mfma(vf, pf[n], float4v{0.f, 0.f, 0.f, 0.f});
            const bool mine = tq[n] == tt;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[n][d][j] += mine ? x[j] : 0.f;
          }
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }

  // the sum over the 4 lane groups (the max is uniform already), then the 4 waves through LDS
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    l[n] += __shfl_xor(l[n], 16, 64);
    l[n] += __shfl_xor(l[n], 32, 64);
    if (g == 0) {
      red_m[wid][n * 16 + c] = m[n];
      red_l[wid][n * 16 + c] = l[n];
    }
  }
  __syncthreads();  // also: every wave is done with its V slab
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    float mx = red_m[0][n * 16 + c];
#pragma unroll
    for (int w = 1; w < NWAVE; ++w) mx = fmaxf(mx, red_m[w][n * 16 + c]);
    const float f = m[n] == -INFINITY ? 0.f : fexp2(m[n] - mx);
#pragma unroll
    for (int d = 0; d < 8; ++d) acc[n][d] *= f;
  }
  float* red = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int w = 0; w < NWAVE; ++w) {
    if (wid == w) {
#pragma unroll
      for (int n = 0; n < NQ; ++n)
#pragma unroll
        for (int d = 0; d < 8; ++d)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float* p = red + (16 * d + 4 * g + j) * PQ + n * 16 + c;
            *p = w == 0 ? acc[n][d][j] : *p + acc[n][d][j];
          }
    }
    __syncthreads();
  }
  for (int i = tid; i < R * DH; i += 256) {
    const int r = i >> 7, d = i & 127;
    const long p = part(r);
    ws_acc[p * DH + d] = red[d * PQ + r];
    if (d == 0) {
      float mx = red_m[0][r];
#pragma unroll
      for (int w = 1; w < NWAVE; ++w) mx = fmaxf(mx, red_m[w][r]);
      float lv = 0.f;
#pragma unroll
      for (int w = 0; w < NWAVE; ++w) {
        const float mw = red_m[w][r];
        lv += red_l[w][r] * (mw == -INFINITY ? 0.f : fexp2(mw - mx));
      }
      ws_ml[p * 2] = mx;
      ws_ml[p * 2 + 1] = lv;
    }
  }
}

// one block of 128 threads per (b, t, q_head): partials merged in split order
__global__ __launch_bounds__(128) void extend_combine_kernel(const float* __restrict__ ws,
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

__global__ __launch_bounds__(256) void rope_append_block_kernel(
    const ushort* __restrict__ qkv, const int* __restrict__ pos, const float* __restrict__ cosT,
    const float* __restrict__ sinT, ushort* __restrict__ q_out, ushort* __restrict__ kc,
    ushort* __restrict__ vc, int T, int Hq, int Hkv, int Smax, long stride_b, long stride_h) {
  const int bt = blockIdx.x, b = bt / T;
  const long pl = (long)pos[b] + (bt - b * T);
  if (pl < 0 || pl >= Smax) return;  // never a table or cache row out of range
  const int p = (int)pl;
  const ushort* in = qkv + (long)bt * (Hq + 2 * Hkv) * DH;
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
      ushort* out = h < Hq ? q_out + ((long)bt * Hq + h) * DH
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

bool block_geometry_ok(int B, int T, int Hq, int Hkv, int Dh, int Smax, long stride_b, long stride_h) {
  if (Dh != DH || B <= 0 || B > 65535 || T < 1 || T > MAX_T || Hq <= 0 || Hkv <= 0 || Hkv > 65535 ||
      Hq % Hkv || Smax <= 0)
    return false;
  const int rep = Hq / Hkv;
  if (rep != 1 && rep != 2 && rep != 4 && rep != 8) return false;
  // rows are 16-byte aligned and heads / sequences do not overlap
  if (stride_h % 8 || stride_b % 8 || stride_h < (long)Smax * DH || stride_b < Hkv * stride_h) return false;
  return true;
}

}  // namespace

extern "C" int th_decode_rope_append_block(const void* qkv, const int* pos, const float* cosT,
                                           const float* sinT, void* q_out, void* kcache, void* vcache, int B,
                                           int T, int Hq, int Hkv, int Dh, int Smax, long stride_b,
                                           long stride_h, hipStream_t s) {
  if (!block_geometry_ok(B, T, Hq, Hkv, Dh, Smax, stride_b, stride_h)) return -1;
  rope_append_block_kernel<<<B * T, 256, 0, s>>>((const ushort*)qkv, pos, cosT, sinT, (ushort*)q_out,
                                                 (ushort*)kcache, (ushort*)vcache, T, Hq, Hkv, Smax,
                                                 stride_b, stride_h);
  TH_CHECK_LAUNCH();
}

// ws: B * T * Hq * nsplit * 130 floats.  Keys [split * chunk, +chunk) go to split `split`; query row
// (b, t, .) sees the first kv_len[b] + t + 1 keys, clamped to [0, Smax] on the device.
extern "C" int th_extend_attn(const void* q, const void* kcache, const void* vcache, const int* kv_len,
                              void* o, float* ws, int B, int T, int Hq, int Hkv, int Dh, int Smax,
                              long stride_b, long stride_h, int nsplit, int chunk, float scale,
                              hipStream_t s) {
  if (!block_geometry_ok(B, T, Hq, Hkv, Dh, Smax, stride_b, stride_h)) return -1;
  if (nsplit <= 0 || nsplit > 1024 || chunk <= 0 || (long)nsplit * chunk > (1L << 30)) return -1;
  const int rep = Hq / Hkv;
  const int rep_shift = rep == 1 ? 0 : rep == 2 ? 1 : rep == 4 ? 2 : 3;
  const dim3 grid(nsplit, Hkv, B);
  const float qscale = scale * 1.4426950408889634f;  // scores in the base-2 domain
  const ushort *qp = (const ushort*)q, *kp = (const ushort*)kcache, *vp = (const ushort*)vcache;
#define TH_EXTEND_LAUNCH(NQ)                                                                             \
  extend_attn_kernel<NQ><<<grid, 256, 0, s>>>(qp, kp, vp, kv_len, ws, Hq, Hkv, Smax, stride_b, stride_h, \
                                              nsplit, chunk, T, rep_shift, qscale)
  switch ((rep * T + 15) / 16) {
    case 1: TH_EXTEND_LAUNCH(1); break;
    case 2: TH_EXTEND_LAUNCH(2); break;
    case 3: TH_EXTEND_LAUNCH(3); break;
    default: TH_EXTEND_LAUNCH(4); break;
  }
#undef TH_EXTEND_LAUNCH
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  extend_combine_kernel<<<B * T * Hq, 128, 0, s>>>(ws, (ushort*)o, (long)B * T * Hq * nsplit, nsplit);
  TH_CHECK_LAUNCH();
}
