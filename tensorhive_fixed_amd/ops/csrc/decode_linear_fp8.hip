// Weight-streaming linear for decode steps on FP8 weights:
//   y[M, N] = (x[M, K] . Wq[N, K]^T) * scale[N]   with 1 <= M <= 16.
//
// x is contiguous bf16; Wq is contiguous OCP FP8 (e4m3fn, one byte per element) in the [out, in]
// layout of the bf16 weight it was quantized from (ops/decode_linear_fp8.py), scale is one f32 per
// weight row.  Accumulation is f32.  The three epilogues of decode_linear.hip:
//   mode 0  y bf16 [M, N]
//   mode 1  y f32  [M, N]
//   mode 2  Wq is the packed gate|up weight [2F, K] (N = 2F, F a multiple of 8); y bf16 [M, F] =
//           silu(g) * u, g and u each scaled by their own row's scale first, never rounded or stored
//
// The structure is that of decode_linear.hip at half the weight bytes.  A workgroup of 4 waves owns
// 1 or 2 tiles of 16 output columns, i.e. R = 1 or 2 tiles of 16 weight rows (mode 2: R = 2 or 4),
// and splits K across the waves in contiguous runs of 128-wide k-steps (K = 256 has two k-steps:
// waves 0 and 2 get none and contribute zeros to the merge).  Per k-step a lane loads 32
// contiguous bytes of one row of every tile (two 16-byte loads straight into VGPRs: a wave reads
// whole 128-byte lines of 16 rows) and the same 32 k-elements, 64 bytes, of one x row.  A 16-byte
// weight load holds 16 k-elements; v_cvt_scalef32_pk_bf16_fp8 with scale 1.0 turns each byte pair
// of a dword into packed bf16 (low byte pair first, then op_sel the high one), so dwords 0-1 and
// 2-3 become the B fragments of two v_mfma_f32_16x16x32_bf16 in memory order, and the A fragments
// are the matching 8 contiguous bf16 of x.  Every finite e4m3 code is a bf16 value, so the
// conversion rounds nothing and the MFMA sees the operands the bf16 kernel would see for the
// dequantized-without-scale weight.  The k-order inside a fragment is free as long as both operands
// use the same one; here both are in memory order.  16 weight loads per lane are in flight (U = 8 / R
// k-steps, as many bytes as the bf16 kernel keeps, twice the k-elements); every register is
// refilled for the next tile right after its MFMAs.  Nothing is staged through LDS, every weight
// byte is read once, default cache policy.
//
// Lanes of the padded rows m >= M read x row M-1 instead (never past x's M rows); rows >= M are not
// written.  Weight rows past the last one re-read the last row and are not written; scale is read
// only for live columns.  The waves' partial tiles are merged through LDS in wave order.  No
// atomics: bit-identical from call to call.  The scale is applied once per output: one f32
// multiplication of the merged sum by scale[col] in the epilogue.
//
// Longest chain of dependent f32 additions behind one output, counting an MFMA as its 32 products
// added one after the other: 64 * ceil(K / 128 / 4) + 4 (two accumulators per tile, each takes two
// MFMAs per k-step, one per 16-byte weight load half; then their sum and 3 additions to merge the
// waves), followed by the one multiplication by the scale.
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

// bytes 0..7 of two dwords -> 8 bf16 in byte order, exact
__device__ __forceinline__ bf16x8 cvt8(unsigned lo, unsigned hi) {
  uint4v r;
  r[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)lo, 1.0f, false));
  r[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)lo, 1.0f, true));
  r[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)hi, 1.0f, false));
  r[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)hi, 1.0f, true));
  return __builtin_bit_cast(bf16x8, r);
}

constexpr int NW = 4;      // waves per workgroup
constexpr int LOADS = 16;  // 16-byte weight loads in flight per lane
constexpr int KS = 128;    // k-elements per k-step

__device__ __forceinline__ float silu_mul(float g, float u) { return g / (1.f + __expf(-g)) * u; }

// R: weight tiles of 16 rows per workgroup
template <int MODE, int R>
__global__ __launch_bounds__(NW * 64) void decode_linear_fp8_kernel(const ushort* __restrict__ x,
                                                                    const uint8_t* __restrict__ w,
                                                                    const float* __restrict__ scale,
                                                                    void* __restrict__ y, int M, long N, int K) {
  constexpr int NT = R;
  constexpr int U = LOADS / (2 * R);                    // k-steps in flight per wave
  constexpr int CT = MODE == OUT_SWIGLU ? R / 2 : R;    // tiles of 16 output columns per workgroup
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: the k-loop branches are scalar
  const int r = lane & 15, g = lane >> 4;  // operand row, 32-element slice of the k-step
  const long n0 = (long)blockIdx.x * (16 * CT);
  const long ncols = MODE == OUT_SWIGLU ? N / 2 : N;  // width of y

  const int S = K / KS;  // k-steps; wave wid owns [s0, s1), possibly none
  const int s0 = S * wid / NW, s1 = S * (wid + 1) / NW;

  const ushort* xp = x + (long)(r < M ? r : M - 1) * K + g * 32;
  const uint8_t* wp[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {  // tile t: column tile t % CT, of the gate (t < CT) or the up half
    const long col = n0 + (t % CT) * 16 + r;
    wp[t] = w + ((col < ncols ? col : ncols - 1) + (t / CT) * ncols) * K + g * 32;
  }

  float4v acc[NT][2];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t][0] = acc[t][1] = float4v{0.f, 0.f, 0.f, 0.f};

  bf16x8 xr[U][4];
  uint4v wr[U][NT][2];
  auto load = [&](int i, int s) {
    const long k = (long)s * KS;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      wr[i][t][0] = ldw(wp[t] + k);
      wr[i][t][1] = ldw(wp[t] + k + 16);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) xr[i][q] = ldx(xp + k + 8 * q);
  };
  auto fma = [&](int i) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int h = 0; h < 2; ++h) {  // 16-byte half h: k-elements 16 h .. 16 h + 15 of the lane's slice
        const uint4v v = wr[i][t][h];
        acc[t][0] = mfma(xr[i][2 * h], cvt8(v[0], v[1]), acc[t][0]);
        acc[t][1] = mfma(xr[i][2 * h + 1], cvt8(v[2], v[3]), acc[t][1]);
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
    const float a = v[c] * scale[col];
    if constexpr (MODE == OUT_BF16) {
      reinterpret_cast<ushort*>(y)[o] = f2bf(a);
    } else if constexpr (MODE == OUT_F32) {
      reinterpret_cast<float*>(y)[o] = a;
    } else {
      reinterpret_cast<ushort*>(y)[o] = f2bf(silu_mul(a, v[CT + c] * scale[ncols + col]));
    }
  }
}

template <int MODE>
int launch(const ushort* x, const uint8_t* w, const float* scale, void* y, int M, long N, int K, int tiles,
           hipStream_t s) {
  constexpr int PER = MODE == OUT_SWIGLU ? 2 : 1;  // weight tiles per tile of output columns
  const long ncols = N / PER;
  const unsigned grid = (unsigned)((ncols + 16 * tiles - 1) / (16 * tiles));
  if (tiles == 1)
    decode_linear_fp8_kernel<MODE, PER><<<grid, NW * 64, 0, s>>>(x, w, scale, y, M, N, K);
  else
    decode_linear_fp8_kernel<MODE, 2 * PER><<<grid, NW * 64, 0, s>>>(x, w, scale, y, M, N, K);
  TH_CHECK_LAUNCH();
}

}  // namespace

// tiles: tiles of 16 output columns per workgroup, 1 or 2, the caller's policy (ops/decode_linear_fp8.py).
extern "C" int th_decode_linear_fp8(const void* x, const void* wq, const void* scale, void* y, int M, long N, int K,
                                    int mode, int tiles, hipStream_t s) {
  if (M < 1 || M > 16 || K < 256 || K % 256 || N < 16 || N % 16 || N > (1L << 31)) return -1;
  if (mode < OUT_BF16 || mode > OUT_SWIGLU || (tiles != 1 && tiles != 2)) return -1;
  const ushort* xp = (const ushort*)x;
  const uint8_t* wp = (const uint8_t*)wq;
  const float* sp = (const float*)scale;
  switch (mode) {
    case OUT_BF16: return launch<OUT_BF16>(xp, wp, sp, y, M, N, K, tiles, s);
    case OUT_F32: return launch<OUT_F32>(xp, wp, sp, y, M, N, K, tiles, s);
    default: return launch<OUT_SWIGLU>(xp, wp, sp, y, M, N, K, tiles, s);
  }
}
