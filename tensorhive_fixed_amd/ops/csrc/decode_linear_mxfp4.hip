// Weight-streaming linear for decode steps on OCP MXFP4 weights:
//   y[M, N] = x[M, K] . dequant(codes[N, K/2], scales[N, K/32])^T   with 1 <= M <= 16.
//
// x is contiguous bf16.  codes holds two E2M1 codes per byte (element 2j in the low nibble of byte j,
// 2j+1 in the high one) in the [out, in] layout of the bf16 weight; scales holds one E8M0 byte per
// 32 elements along K: block j of row n is scaled by 2^(scales[n, j] - 127), bytes in [2, 252]
// (ops/decode_linear_mxfp4.py).  0.53125 bytes per weight.  Accumulation is f32.  The epilogues of
// decode_linear_fp8.hip:
//   mode 0  y bf16 [M, N]
//   mode 1  y f32  [M, N]
//   mode 2  codes is the packed gate|up weight [2F, K/2] (N = 2F, F a multiple of 8); y bf16 [M, F] =
//           silu(g) * u, g and u never rounded or stored
//
// A workgroup of 4 waves owns CT = 1, 2 or 4 tiles of 16 output columns, i.e. R = CT tiles of 16
// weight rows (mode 2: R = 2 CT), and splits K across the waves in contiguous runs of 256-wide
// k-steps (a wave may get none: it contributes zeros to the merge).  Per k-step a lane (r, g) loads
// 32 contiguous bytes of row r of every tile, the k-elements 64 g .. 64 g + 63 of the step, as two
// 16-byte loads: a wave reads whole 128-byte lines of 16 rows.  A 16-byte load is exactly one MX
// block, so the lane's two scale bytes sit side by side and come as one 2-byte load issued with the
// weight loads of the same k-step, U k-steps ahead of their use: no load stands in front of a
// conversion.  v_cvt_scalef32_pk_bf16_fp4 turns one byte of a dword into two bf16 with the block
// scale applied (passed as the f32 with bits byte << 23, always an exact power of two); its four
// byte selects make one dword the 8 bf16 of a B fragment of v_mfma_f32_16x16x32_bf16 in memory
// order, and the A fragment is the matching 8 contiguous bf16 of x: 8 MFMAs per tile and k-step.
// code * 2^e is always a bf16 value, so the MFMA sees exactly the dequantized weight.
//
// Per k-step a lane also reads 128 bytes of one x row (L2 hits): per weight byte four times the x
// bytes of the bf16 kernel.  More column tiles per workgroup read x once for more columns; the
// caller picks CT (pick_tiles_mxfp4).  In flight per lane: U = 4, 4, 2, 1 k-steps at R = 1, 2, 4, 8,
// i.e. 16 weight loads of 16 bytes for R >= 2.  R = 1 keeps 8: the x of 8 k-steps, 256 VGPRs, would
// not fit beside them, and two workgroups share a CU at every R (188-235 VGPRs, no spills).  Every
// register is refilled for the next tile right after its MFMAs.  Nothing is staged through LDS, every weight byte is
// read once.
//
// Lanes of the padded rows m >= M read x row M-1 instead; rows >= M are not written.  Weight rows
// past the last one re-read the last row (codes and scales alike, so scales are read only inside
// [N, K/32]) and are not written.  The waves' partial tiles are merged through LDS in wave order.
// No atomics: bit-identical from call to call.
//
// Longest chain of dependent f32 additions behind one output, counting an MFMA as its 32 products
// added one after the other: 128 * ceil(K / 256 / 4) + 4 (two accumulators per tile, each takes
// four MFMAs per k-step, the even or the odd dwords of both 16-byte loads; then their sum and 3
// additions to merge the waves).
#include "th_common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned uint4v __attribute__((ext_vector_type(4)));

enum { OUT_BF16 = 0, OUT_F32 = 1, OUT_SWIGLU = 2 };

__device__ __forceinline__ float4v mfma(bf16x8 a, bf16x8 b, float4v c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ bf16x8 ldx(const ushort* p) { return *reinterpret_cast<const bf16x8*>(p); }
__device__ __forceinline__ uint4v ldw(const uint8_t* p) { return *reinterpret_cast<const uint4v*>(p); }

// the 8 codes of one dword -> 8 bf16 in element order, each times scale (a power of two): exact
__device__ __forceinline__ bf16x8 cvt8(unsigned v, float scale) {
  uint4v r;
  r[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, scale, 0));
  r[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, scale, 1));
  r[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, scale, 2));
  r[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, scale, 3));
  return __builtin_bit_cast(bf16x8, r);
}

constexpr int NW = 4;     // waves per workgroup
constexpr int KS = 256;   // k-elements per k-step
constexpr int BLK = 32;   // k-elements per MX block

__device__ __forceinline__ float silu_mul(float g, float u) { return g / (1.f + __expf(-g)) * u; }

// R: weight tiles of 16 rows per workgroup
template <int MODE, int R>
__global__ __launch_bounds__(NW * 64) void decode_linear_mxfp4_kernel(const ushort* __restrict__ x,
                                                                      const uint8_t* __restrict__ w,
                                                                      const uint8_t* __restrict__ sc,
                                                                      void* __restrict__ y, int M, long N, int K) {
  constexpr int NT = R;
  constexpr int U = R <= 2 ? 4 : 8 / R;                 // k-steps in flight per wave
  constexpr int CT = MODE == OUT_SWIGLU ? R / 2 : R;    // tiles of 16 output columns per workgroup
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: the k-loop branches are scalar
  const int r = lane & 15, g = lane >> 4;  // operand row, 64-element slice of the k-step
  const long n0 = (long)blockIdx.x * (16 * CT);
  const long ncols = MODE == OUT_SWIGLU ? N / 2 : N;  // width of y

  const int S = K / KS;  // k-steps; wave wid owns [s0, s1), possibly none
  const int s0 = S * wid / NW, s1 = S * (wid + 1) / NW;

  const ushort* xp = x + (long)(r < M ? r : M - 1) * K + g * 64;
  const uint8_t* wp[NT];
  const uint8_t* sp[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {  // tile t: column tile t % CT, of the gate (t < CT) or the up half
    const long col = n0 + (t % CT) * 16 + r;
    const long row = (col < ncols ? col : ncols - 1) + (t / CT) * ncols;
    wp[t] = w + row * (K / 2) + g * 32;
    sp[t] = sc + row * (K / BLK) + g * 2;
  }

  float4v acc[NT][2];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t][0] = acc[t][1] = float4v{0.f, 0.f, 0.f, 0.f};

  bf16x8 xr[U][8];
  uint4v wr[U][NT][2];
  unsigned er[U][NT];  // the lane's two scale bytes of the k-step
  auto load = [&](int i, int s) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      wr[i][t][0] = ldw(wp[t] + (long)s * (KS / 2));
      wr[i][t][1] = ldw(wp[t] + (long)s * (KS / 2) + 16);
      er[i][t] = *reinterpret_cast<const ushort*>(sp[t] + s * (KS / BLK));
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) xr[i][q] = ldx(xp + (long)s * KS + 8 * q);
  };
  auto fma = [&](int i) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int h = 0; h < 2; ++h) {  // 16-byte half h: MX block h of the lane's slice, k-elements 32 h .. 32 h + 31
        const uint4v v = wr[i][t][h];
        const float e = __uint_as_float(((er[i][t] >> (8 * h)) & 0xffu) << 23);
#pragma unroll
        for (int d = 0; d < 4; ++d) acc[t][d & 1] = mfma(xr[i][4 * h + d], cvt8(v[d], e), acc[t][d & 1]);
      }
  };

  int s = s0;
  const int nfull = (s1 - s0) / U;
  if (nfull > 0) {
#pragma unroll
    for (int i = 0; i < U; ++i) load(i, s + i);
    for (int t = 1; t < nfull; ++t, s += U) {
#pragma unroll
      for (int i = 0; i < U; ++i) {
        fma(i);
        load(i, s + U + i);  // refill for the next tile
      }
    }
#pragma unroll
    for (int i = 0; i < U; ++i) fma(i);
    s += U;
  }
  const int rem = s1 - s;  // < U k-steps left: all of their loads first
  if (rem > 0) {
#pragma unroll
    for (int i = 0; i < U - 1; ++i)
      if (i < rem) load(i, s + i);
#pragma unroll
    for (int i = 0; i < U - 1; ++i)
      if (i < rem) fma(i);
  }

  // lane (r, g) holds D[m = 4 g + j][n = r]; merge the waves in wave order
  __shared__ float red[NW][NT][256];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) red[wid][t][(g * 4 + j) * 16 + r] = acc[t][0][j] + acc[t][1][j];
  __syncthreads();
  const int m = tid >> 4, n = tid & 15;
  float v[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    v[t] = red[0][t][tid];
#pragma unroll
    for (int q = 1; q < NW; ++q) v[t] += red[q][t][tid];
  }
  if (m >= M) return;
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const long col = n0 + c * 16 + n;
    if (col >= ncols) continue;
    const long o = (long)m * ncols + col;
    if constexpr (MODE == OUT_BF16) {
      reinterpret_cast<ushort*>(y)[o] = f2bf(v[c]);
    } else if constexpr (MODE == OUT_F32) {
      reinterpret_cast<float*>(y)[o] = v[c];
    } else {
      reinterpret_cast<ushort*>(y)[o] = f2bf(silu_mul(v[c], v[CT + c]));
    }
  }
}

template <int MODE>
int launch(const ushort* x, const uint8_t* w, const uint8_t* sc, void* y, int M, long N, int K, int tiles,
           hipStream_t s) {
  constexpr int PER = MODE == OUT_SWIGLU ? 2 : 1;  // weight tiles per tile of output columns
  const long ncols = N / PER;
  const unsigned grid = (unsigned)((ncols + 16 * tiles - 1) / (16 * tiles));
  if (tiles == 1)
    decode_linear_mxfp4_kernel<MODE, PER><<<grid, NW * 64, 0, s>>>(x, w, sc, y, M, N, K);
  else if (tiles == 2)
    decode_linear_mxfp4_kernel<MODE, 2 * PER><<<grid, NW * 64, 0, s>>>(x, w, sc, y, M, N, K);
  else
    decode_linear_mxfp4_kernel<MODE, 4 * PER><<<grid, NW * 64, 0, s>>>(x, w, sc, y, M, N, K);
  TH_CHECK_LAUNCH();
}

}  // namespace

// tiles: tiles of 16 output columns per workgroup, 1, 2 or 4, the caller's policy (ops/decode_linear_mxfp4.py).
extern "C" int th_decode_linear_mxfp4(const void* x, const void* codes, const void* scales, void* y, int M, long N,
                                      int K, int mode, int tiles, hipStream_t s) {
  if (M < 1 || M > 16 || K < 256 || K % 256 || N < 16 || N % 16 || N > (1L << 31)) return -1;
  if (mode < OUT_BF16 || mode > OUT_SWIGLU || (tiles != 1 && tiles != 2 && tiles != 4)) return -1;
  const ushort* xp = (const ushort*)x;
  const uint8_t* wp = (const uint8_t*)codes;
  const uint8_t* sp = (const uint8_t*)scales;
  switch (mode) {
    case OUT_BF16: return launch<OUT_BF16>(xp, wp, sp, y, M, N, K, tiles, s);
    case OUT_F32: return launch<OUT_F32>(xp, wp, sp, y, M, N, K, tiles, s);
    default: return launch<OUT_SWIGLU>(xp, wp, sp, y, M, N, K, tiles, s);
  }
}
