// Weight-streaming linear for decode steps: y[M, N] = x[M, K] . W[N, K]^T with 1 <= M <= 16.
//
// x and W are contiguous bf16, W in the [out, in] layout of every nn.Parameter (nothing is
// transposed or repacked); accumulation is f32.  Three epilogues:
//   mode 0  y bf16 [M, N]
//   mode 1  y f32  [M, N]   (LM head: the logits leave the f32 accumulator unrounded)
//   mode 2  W is the packed gate|up weight [2F, K] (N = 2F, F a multiple of 8); y bf16 [M, F] =
//           silu(g) * u from the two f32 accumulators, g and u are never rounded or stored
//
// This is an HBM stream of W with next to no arithmetic.  A workgroup of 4 waves owns 1 or 2 tiles of
// 16 output columns, i.e. R = 1 or 2 tiles of 16 weight rows (mode 2: R = 2 or 4, the gate rows n
// and the up rows F + n of the same columns), and splits K across the waves in contiguous runs
// of 64-wide k-steps.  Per k-step a lane loads 32
// contiguous bytes of one row of every tile (two 16-byte loads straight into VGPRs: a wave reads
// whole 128-byte lines of 16 rows) and the same 32 bytes of one x row; each 16-byte half is the
// operand fragment of one v_mfma_f32_16x16x32_bf16 (A = x padded to 16 rows, B = W^T) -- the
// k-order inside a fragment is free as long as both operands use the same one.  The x fragment
// serves all R tiles: x comes out of L2 once per workgroup, so R divides that traffic, which the
// kernel's time grows with as M grows.  16 weight loads per lane are in flight (U = 8 / R
// k-steps); every register is refilled for the next tile right after its MFMA, so the compiler
// counts vmcnt down and a full tile stays in flight.  Nothing is staged through LDS, every weight
// byte is read once.  The weight loads use the default cache policy: non-temporal loads measured
// 5 to 15 % slower on the Llama-3-8B shapes (profiles/decode_linear/README.md).
//
// Lanes of the padded rows m >= M read x row M-1 instead (never past x's M rows); row m of the
// MFMA result depends on row m of A only, and rows >= M are not written.  Weight rows past the last
// one (a partial or dead tile of the last workgroup) re-read the last row and are not written.
// The waves' partial tiles are merged through LDS in wave order.  No atomics: bit-identical from
// call to call.  (K split over workgroups as well, with f32 partials merged by a second kernel,
// measured no faster on any Llama-3-8B shape and is not kept: profiles/decode_linear/README.md.)
//
// Longest chain of dependent f32 additions behind one output, counting an MFMA as its 32 products
// added one after the other: 32 * ceil(K / 64 / 4) + 4 (two accumulators per tile, one per 16-byte
// half, then their sum and 3 additions to merge the waves).
#include "th_common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

enum { OUT_BF16 = 0, OUT_F32 = 1, OUT_SWIGLU = 2 };

__device__ __forceinline__ float4v mfma(ushort8 a, ushort8 b, float4v c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
                                                 c, 0, 0, 0);
}
__device__ __forceinline__ ushort8 ld(const ushort* p) { return *reinterpret_cast<const ushort8*>(p); }

constexpr int NW = 4;      // waves per workgroup
constexpr int LOADS = 16;  // 16-byte weight loads in flight per lane

__device__ __forceinline__ float silu_mul(float g, float u) { return g / (1.f + __expf(-g)) * u; }

// R: weight tiles of 16 rows per workgroup
template <int MODE, int R>
__global__ __launch_bounds__(NW * 64) void decode_linear_kernel(const ushort* __restrict__ x,
                                                                const ushort* __restrict__ w,
                                                                void* __restrict__ y, int M, long N, int K) {
  constexpr int NT = R;
  constexpr int U = LOADS / (2 * R);                    // k-steps in flight per wave
  constexpr int CT = MODE == OUT_SWIGLU ? R / 2 : R;    // tiles of 16 output columns per workgroup
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: the k-loop branches are scalar
  const int r = lane & 15, g = lane >> 4;  // operand row, 32-byte slice of the k-step
  const long n0 = (long)blockIdx.x * (16 * CT);
  const long ncols = MODE == OUT_SWIGLU ? N / 2 : N;  // width of y

  const int S = K / 64;  // k-steps; wave wid owns [s0, s1)
  const int s0 = S * wid / NW, s1 = S * (wid + 1) / NW;

  const ushort* xp = x + (long)(r < M ? r : M - 1) * K + g * 16;
  const ushort* wp[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {  // tile t: column tile t % CT, of the gate (t < CT) or the up half
    const long col = n0 + (t % CT) * 16 + r;
    wp[t] = w + ((col < ncols ? col : ncols - 1) + (t / CT) * ncols) * K + g * 16;
  }

  float4v acc[NT][2];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t][0] = acc[t][1] = float4v{0.f, 0.f, 0.f, 0.f};

  ushort8 xr[U][2], wr[U][NT][2];
  auto load = [&](int i, int s) {
    const long k = (long)s * 64;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      wr[i][t][0] = ld(wp[t] + k);
      wr[i][t][1] = ld(wp[t] + k + 8);
    }
    xr[i][0] = ld(xp + k);
    xr[i][1] = ld(xp + k + 8);
  };
  auto fma = [&](int i) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      acc[t][0] = mfma(xr[i][0], wr[i][t][0], acc[t][0]);
      acc[t][1] = mfma(xr[i][1], wr[i][t][1], acc[t][1]);
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
int launch(const ushort* x, const ushort* w, void* y, int M, long N, int K, int tiles, hipStream_t s) {
  constexpr int PER = MODE == OUT_SWIGLU ? 2 : 1;  // weight tiles per tile of output columns
  const long ncols = N / PER;
  const unsigned grid = (unsigned)((ncols + 16 * tiles - 1) / (16 * tiles));
  if (tiles == 1)
    decode_linear_kernel<MODE, PER><<<grid, NW * 64, 0, s>>>(x, w, y, M, N, K);
  else
    decode_linear_kernel<MODE, 2 * PER><<<grid, NW * 64, 0, s>>>(x, w, y, M, N, K);
  TH_CHECK_LAUNCH();
}

}  // namespace

// tiles: tiles of 16 output columns per workgroup, 1 or 2, the caller's policy (ops/decode_linear.py).
extern "C" int th_decode_linear(const void* x, const void* w, void* y, int M, long N, int K, int mode, int tiles,
                                hipStream_t s) {
  if (M < 1 || M > 16 || K < 256 || K % 256 || N < 16 || N % 16 || N > (1L << 31)) return -1;
  if (mode < OUT_BF16 || mode > OUT_SWIGLU || (tiles != 1 && tiles != 2)) return -1;
  const ushort *xp = (const ushort*)x, *wp = (const ushort*)w;
  switch (mode) {
    case OUT_BF16: return launch<OUT_BF16>(xp, wp, y, M, N, K, tiles, s);
    case OUT_F32: return launch<OUT_F32>(xp, wp, y, M, N, K, tiles, s);
    default: return launch<OUT_SWIGLU>(xp, wp, y, M, N, K, tiles, s);
  }
}
