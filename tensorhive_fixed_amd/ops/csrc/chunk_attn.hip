// Chunked prefill: a long block of T new tokens per sequence on top of a bf16 KV cache that already
// holds kv_len[b] rows (any number, 0 included).  new_len[b] in 0..T of the block's tokens are live.
//
// Cache of one layer as in decode_attn.hip: K and V as [B, Hkv, Smax, 128] bf16, the entry points
// take the layer's K / V base pointers and the b / head strides in elements.  Head dim 128 only.
// th-build-flags: -fno-slp-vectorize -Xclang -target-feature -Xclang -packed-fp32-ops
//   (no v_pk_*_f32 in the f32 softmax math beside the MFMAs; the host pass ignores the feature.  The build
//   reads this line from the file's first 40 lines only: it stays up here)
//
// th_chunk_rope_append  row (b, t < new_len[b]) of qkv [B, T, (Hq+2*Hkv)*128] is rotated at
//                        kv_len[b] + t; its k / v go into cache row kv_len[b] + t and its q into
//                        q_out [B, T, Hq*128], with the arithmetic of th_decode_rope_append.  A row
//                        t >= new_len[b] writes nothing to the cache and zeros to q_out.
// th_chunk_attn          query row (b, t < new_len[b], h) attends over cache rows
//                        [0, kv_len[b] + t + 1) of its KV head; rows t >= new_len[b] get zeros.
//
// Where extend_attn.hip keeps all (<= 64) query rows in every wave and splits the keys over the waves,
// this kernel splits the QUERY rows: grid (query tile, Hkv, B), the tiles that reach furthest down the
// cache first.  A workgroup of 4 waves serves QTILE = 128 query rows of one KV head, row r = t * rep + h
// (128 / rep consecutive tokens x the rep query heads of the group, so the causal limit of a wave's 32
// rows spans at most 32 / rep tokens); every wave owns 32 rows for the whole key loop and there is no
// merge, no workspace and no atomic: every output element is written once.
//
//   K / V tiles of KTILE = 64 keys are staged once per workgroup (global_load_dwordx4 -> registers ->
//   ds_write_b128) into double-buffered LDS images and shared by the four waves: tile j + 1 is written
//   into the other image and tile j + 2 is in flight while tile j is computed, one barrier per tile.
//   The image is flash_attn.hip's 8-row x 32-column subtile swizzle, conflict-free for both the
//   16-byte row reads and the ds_read_b64_tr_b16 transposed reads of 32x32x16 MFMAs.
//     S^T = K Q^T      A = K rows from LDS, B = Q rows in registers, unscaled (the scale goes into the
//                      exp2 argument in f32).  Lane (c = lane & 31, h = lane >> 5) holds query c and
//                      the 32 keys 32 kb + 8 (r >> 2) + 4 h + (r & 3) of the tile.
//     O^T += V^T P^T   B = P^T, packed to bf16 in place from the S^T accumulators, A = V^T through
//                      transposed LDS reads in the same key order.  O (32 rows x 128, f32) stays in
//                      registers.
//   Running max and sum are per lane, f32, base 2; the max is made uniform over the lane pair (c, c+32)
//   each tile (one v_permlane32_swap), the sum once at the end.  The key loop of a workgroup ends at
//   the last key its last live row sees; a wave skips the tiles past its own last row's limit and runs
//   the mask (key < kv_len + t + 1) only on tiles that reach its first row's limit.  Keys past the loop's
//   end are loaded from its last row and masked; query rows t >= new_len[b] are loaded from the last live
//   row and written as zeros; cache rows at or past kv_len[b] + new_len[b] are never loaded.  A tile
//   with no live row writes zeros and reads no K / V.  kv_len and new_len are clamped on the device
//   (kv_len + new_len <= Smax) before any address is formed.
//
// th_chunk_attn_split    the same rows for a short chunk on a long cache, where (query tile, Hkv, B) leaves
//                        most CUs idle: chunk_attn_kernel<true> on a grid (nsplit x query tile, Hkv, B) and
//                        chunk_attn_combine_kernel.  chunk_attn_kernel<false> is the kernel described above,
//                        with its argument block and its instructions.
//   A workgroup (tile, split s) derives kv_end and ntiles of its tile as above and serves the key tiles
//   [s * tps, min((s + 1) * tps, ntiles)), tps = ceil(ntiles / nsplit): every tile of every sequence is cut
//   into equal parts of its own causal range, in whole key tiles, so the loop, its masks and its wave skip
//   are the unsplit ones and only nsplit depends on the lengths.  A partial is unnormalised f32 in a
//   workspace slot of WS_SLOT floats per (b, hkv, tile, split): 128 x (m, l) (m scaled, base 2, uniform
//   over the lane pair; l pair-summed), then per wave its 32 x 128 accumulators in register order, piece
//   (d, g) = acc[d][4 g .. 4 g + 3] of lane L at float 4 * ((4 d + g) * 64 + L): a store instruction of a
//   wave covers 1024 contiguous bytes and nothing passes through LDS.  A workgroup with no key tile (or a
//   tile with no live row) writes (-inf, 0) and returns before any K / V or Q load; a wave that computed
//   no tile writes its (m, l) = (-inf, 0) only.
//   The combine workgroup serves the 32 rows of one wave block: thread (wave d, lane L) reads the pieces
//   (d, 0..3) of lane L of every split, whole 1024-byte runs per wave as they were written, skips every
//   partial with l == 0 without reading its accumulators (the workspace is not cleared), weights the
//   others by exp2(m_s - max m) in split order, swaps halves with lane L ^ 32 (which holds the other 4 of
//   every 8 dims of the same row) and writes 2 x 16 bytes of bf16; rows t >= new_len[b] and rows with no
//   key are exact zeros.  No atomic and no counter: two runs give the same bits.
//
// th_paged_chunk_rope_append / th_paged_chunk_attn / th_paged_chunk_attn_split    the same three on the PAGED
//   cache of paged_attn.hip: pool [n_pages, Hkv, 64, 128] per K / V, table [B, table_stride] int32, logical row r
//   of sequence b in row r & 63 of page table[b][r >> 6].  A page is KTILE rows, so key tile j of sequence b IS
//   page table[b][j]: one contiguous 16 KB run per KV head.  chunk_attn_kernel<SPLIT, true> keeps the grid, the
//   images, the MFMA products, the masks, the softmax and the epilogues of the dense kernel and changes only how
//   a tile's rows are found, so it gives the dense kernel's bits on the same rows through any table:
//     the page id of a tile is workgroup-uniform: a scalar load from table + b * table_stride, clamped to
//     [0, n_pages) (a bad id is never followed) and turned into the 64-bit pool offset id * stride_page +
//     hkv * stride_h, all in SGPRs; a lane adds a 32-bit offset inside the 16 KB run (row x 256 B + its chunk).
//     The global loads of tile j + 2 are issued in iteration j, so the entry of tile j + 2 is read in
//     iteration j - 1 (that of j + 3 in iteration j, right behind the loads) and clamped only where it is used:
//     the key loop never waits on a table entry.  Only the entries of the workgroup's own tiles [j0, j1) are
//     read (the read-ahead index is clamped to j1 - 1), never one at or past ceil(kv_end / 64).  Rows past
//     kv_end - 1 of the last tile come from row kv_end - 1, which lies in the same page.  The append checks the
//     page id against [0, n_pages) before an address is formed: a row whose id fails stores nothing in the pool,
//     its q still goes out.
#include "th_common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef short i16x8 __attribute__((ext_vector_type(8)));
#define LDS_AS __attribute__((address_space(3)))
#define CONST_AS __attribute__((address_space(4)))

namespace {

constexpr int DH = 128;
constexpr int QTILE = 128;         // query rows of a workgroup: 4 waves x 32
constexpr int KTILE = 64;          // keys per staged tile
constexpr int IMG = KTILE * DH * 2;  // bytes of one K or V image
constexpr int MAX_CHUNK_SPLITS = 16;
constexpr int WS_ML = 2 * QTILE;                 // floats of a slot's (m, l) pairs
constexpr int WS_SLOT = WS_ML + QTILE * DH;      // floats of one (b, hkv, tile, split) partial

// byte offset of (row, 16-byte chunk) in an image: 8-row x 32-column subtiles of 512 B, the slot of a
// chunk inside its 64 B is xor-ed with (row >> 2) & 3 (flash_attn.hip's img_off)
__device__ __forceinline__ int img_off(int row, int ch) {
  return ((row >> 3) << 11) + ((ch >> 2) << 9) + ((row & 7) << 6) + (((ch & 3) ^ ((row >> 2) & 3)) << 4);
}

__device__ __forceinline__ bf16x8 lds_row(const char* img, int row, int ch) {
  return *reinterpret_cast<const bf16x8*>(img + img_off(row, ch));
}

// A = X^T of the image X[key][dim]: lane (c, h) gets X[rbase + 8 (j >> 2) + 4 h + (j & 3)][cbase + c] in
// element j, the key order of the S^T accumulators
__device__ __forceinline__ bf16x8 lds_tr(const char* img, int rbase, int cbase, int lane) {
  const int h = lane >> 5, grp = (lane >> 4) & 1, i = lane & 15;
  const int row = rbase + 4 * h + (i >> 2);
  const int col = cbase + 16 * grp + 4 * (i & 3);
  const char* p0 = img + img_off(row, col >> 3) + ((col & 7) << 1);
  const char* p1 = img + img_off(row + 8, col >> 3) + ((col & 7) << 1);
  const i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS i16x4*)(p0));
  const i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS i16x4*)(p1));
  const i16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}

__device__ __forceinline__ f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }

// accumulator row (register r of lane half h) of a 32x32 MFMA tile
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ bf16x8 pack8(const f32x16& x, int base) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (__bf16)x[base + j];
  return r;
}

// lane <-> lane ^ 32
__device__ __forceinline__ float pair_max(float x) {
  const int xi = __builtin_bit_cast(int, x);
  const auto r = __builtin_amdgcn_permlane32_swap(xi, xi, false, false);
  return fmaxf(__builtin_bit_cast(float, (int)r[0]), __builtin_bit_cast(float, (int)r[1]));
}
__device__ __forceinline__ float pair_sum(float x) {
  const int xi = __builtin_bit_cast(int, x);
  const auto r = __builtin_amdgcn_permlane32_swap(xi, xi, false, false);
  return __builtin_bit_cast(float, (int)r[0]) + __builtin_bit_cast(float, (int)r[1]);
}

// the lane's half of an output row: dims 32 d + 8 g + 4 h + 0..3; `live` false writes zeros
__device__ __forceinline__ void store_row(ushort* row, const f32x16 (&acc)[4], float f, bool live, int h) {
#pragma unroll
  for (int d = 0; d < 4; ++d)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      ushort4v v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = live ? f2bf(acc[d][4 * g + e] * f) : (ushort)0;
      *reinterpret_cast<ushort4v*>(row + 32 * d + 8 * g + 4 * h) = v;
    }
}

// old and live-new length of sequence b, clamped so that len0 + nw <= Smax and nw <= T
__device__ __forceinline__ void chunk_lens(const int* kv_len, const int* new_len, int b, int T, int Smax,
                                           int& len0, int& nw) {
  int l = kv_len[b], n = new_len[b];
  l = l < 0 ? 0 : (l > Smax ? Smax : l);
  n = n < 0 ? 0 : (n > T ? T : n);
  len0 = l;
  nw = n > Smax - l ? Smax - l : n;
}

// the page table of a paged launch: the first member of the kernels' trailing argument pack
struct PageMap {
  const int* table;
  int n_pages, table_stride;
};

__device__ __forceinline__ float* split_ws(float* ws, int) { return ws; }
__device__ __forceinline__ int split_count(float*, int nsplit) { return nsplit; }
__device__ __forceinline__ float* split_ws(PageMap, float* ws, int) { return ws; }
__device__ __forceinline__ int split_count(PageMap, float*, int nsplit) { return nsplit; }
template <typename... R>
__device__ __forceinline__ PageMap page_map(PageMap pm, R...) { return pm; }

// a row's (m, l) = (-inf, 0): the neutral partial, which the combine pass skips
__device__ __forceinline__ void store_neutral(float* slot, int w, int c32, int h) {
  if (h == 0) *reinterpret_cast<float2*>(slot + 2 * (w * 32 + c32)) = make_float2(-INFINITY, 0.f);
}

// SPLIT: `sp...` ends in (float* ws, int nsplit) and `o` is not written.  PAGED: `sp...` starts with a PageMap,
// kc / vc are the pools and stride_b is the page stride.  <false, false> has no `sp`.
template <bool SPLIT, bool PAGED, typename... SP>
__global__ __launch_bounds__(256, 2) void chunk_attn_kernel(
    const ushort* __restrict__ q, const ushort* __restrict__ kc, const ushort* __restrict__ vc,
    const int* __restrict__ kv_len, const int* __restrict__ new_len, ushort* __restrict__ o, int T, int Hq,
    int Smax, long stride_b, long stride_h, int rep_shift, float qscale, SP... sp) {
  __shared__ __attribute__((aligned(16))) char smem[2 * 2 * IMG];  // (K, V) x 2 buffers
  int nsplit = 1, split = 0, xt = blockIdx.x, qtiles = gridDim.x;
  float* slot = nullptr;
  if constexpr (SPLIT) {
    nsplit = split_count(sp...);
    xt = blockIdx.x / nsplit;
    split = blockIdx.x - xt * nsplit;
    qtiles = gridDim.x / nsplit;
  }
  const int qt = qtiles - 1 - xt, hkv = blockIdx.y, b = blockIdx.z;  // furthest tile first
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, c32 = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rep = 1 << rep_shift;

  int len0, nw;
  chunk_lens(kv_len, new_len, b, T, Smax, len0, nw);  // before any address is formed

  const int r = qt * QTILE + w * 32 + c32;  // this lane's query row of the KV head
  const int t = r >> rep_shift, hh = r & (rep - 1);
  const int tok0 = (qt * QTILE) >> rep_shift;  // first token of the tile
  ushort* orow = o + (((long)b * T + (t < T ? t : 0)) * Hq + hkv * rep + hh) * DH;

  f32x16 acc[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) acc[d] = f32x16(0.f);

  if constexpr (SPLIT)
    slot = split_ws(sp...) + ((((long)b * gridDim.y + hkv) * qtiles + qt) * nsplit + split) * WS_SLOT;
  if (tok0 >= nw) {  // no live row: zeros, no K / V read
    if constexpr (SPLIT)
      store_neutral(slot, w, c32, h);
    else if (t < T)
      store_row(orow, acc, 0.f, false, h);
    return;
  }

  const int tl = min(tok0 + (QTILE >> rep_shift), nw) - 1;  // last live token of the tile
  const int kv_end = len0 + tl + 1;                         // keys the tile's last live row sees (>= 1)
  const int ntiles = (kv_end + KTILE - 1) / KTILE;
  int j0 = 0, j1 = ntiles;  // this workgroup's key tiles
  if constexpr (SPLIT) {
    const int tps = (ntiles + nsplit - 1) / nsplit;
    j0 = split * tps;
    j1 = min(j0 + tps, ntiles);
    if (j0 >= j1) {  // fewer key tiles than splits: nothing to read
      store_neutral(slot, w, c32, h);
      return;
    }
  }
  const int tc = t < nw ? t : nw - 1;  // dead rows are loaded from the last live one
  const int lim = len0 + tc + 1;       // this row sees keys < lim
  // wave-uniform: the wave's first and last live token
  const int tw0 = (qt * QTILE + w * 32) >> rep_shift;
  const bool wave_live = tw0 < nw;
  const int wfirst = len0 + tw0 + 1;                                                    // smallest limit
  const int wlast = len0 + min((qt * QTILE + w * 32 + 31) >> rep_shift, nw - 1) + 1;  // largest limit

  bf16x8 qf[8];
  {
    const ushort* qp = q + (((long)b * T + tc) * Hq + hkv * rep + hh) * DH + 8 * h;
#pragma unroll
    for (int s = 0; s < 8; ++s) qf[s] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const ushort8*>(qp + 16 * s));
  }

  // staging: thread `tid` covers rows 16 i + srow, 16-byte chunk sch; 8 contiguous lanes write 2 adjacent
  // rows x 4 chunks = 128 contiguous bytes of the image
  const int srow = 2 * ((tid >> 3) & 7) + ((tid >> 2) & 1), sch = 4 * ((tid >> 6) & 3) + (tid & 3);
  const ushort* kb = kc + b * stride_b + hkv * stride_h + sch * 8;
  const ushort* vb = vc + b * stride_b + hkv * stride_h + sch * 8;
  ushort8 kr[4], vr[4];
  // PAGED: the table entry of key tile min(j, j1 - 1), scalar and still unclamped (the clamp waits for the load,
  // so it is left to the entry's use).  Only entries of [j0, j1) are read: they exist (j1 <= ceil(Smax / 64) <=
  // table_stride) and belong to the sequence.
  auto page_id = [&](int j) -> int {
    if constexpr (PAGED) {
      const PageMap pm = page_map(sp...);
      // read through the constant address space: nothing writes the table while the kernel runs, and the split
      // form's workspace stores would otherwise turn this scalar load into a vector load the loop waits on
      const CONST_AS int* trow = (const CONST_AS int*)pm.table + (long)b * pm.table_stride;
      return __builtin_amdgcn_readfirstlane(trow[min(j, j1 - 1)]);
    }
    return 0;
  };
  // rows past the loop's end come from its last row (live, and in the same page) and are masked
  auto load_tile = [&](int j, int id) {
    if constexpr (PAGED) {
      const int n_pages = page_map(sp...).n_pages;
      id = id < 0 ? 0 : (id >= n_pages ? n_pages - 1 : id);  // a bad id is clamped, never followed
      const long off = (long)id * stride_b + hkv * stride_h;  // the (page, kv head) run: 64 bits, scalar
      const char* kp = reinterpret_cast<const char*>(kc + off);
      const char* vp = reinterpret_cast<const char*>(vc + off);
      const int last = kv_end - 1 - j * KTILE;  // >= 63 except in the last tile
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned x = (unsigned)min(16 * i + srow, last) * (DH * 2) + sch * 16;  // inside the 16 KB run
        kr[i] = *reinterpret_cast<const ushort8*>(kp + x);
        vr[i] = *reinterpret_cast<const ushort8*>(vp + x);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long row = min(j * KTILE + 16 * i + srow, kv_end - 1);
        kr[i] = *reinterpret_cast<const ushort8*>(kb + row * DH);
        vr[i] = *reinterpret_cast<const ushort8*>(vb + row * DH);
      }
    }
  };
  auto store_tile = [&](int buf) {
    char* img = smem + buf * (2 * IMG);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<ushort8*>(img + img_off(16 * i + srow, sch)) = kr[i];
      *reinterpret_cast<ushort8*>(img + IMG + img_off(16 * i + srow, sch)) = vr[i];
    }
  };

  int pnext = 0;  // PAGED: page_id of the tile whose loads are issued next, read one iteration before them
  if constexpr (PAGED) {
    const int p0 = page_id(j0), p1 = page_id(j0 + 1);
    pnext = page_id(j0 + 2);
    load_tile(j0, p0);
    store_tile(j0 & 1);
    if (j0 + 1 < j1) load_tile(j0 + 1, p1);
  } else {
    load_tile(j0, 0);
    store_tile(j0 & 1);
    if (j0 + 1 < j1) load_tile(j0 + 1, 0);
  }
  __syncthreads();

  float m_i = -INFINITY, l_i = 0.f;  // l_i: this lane's 32 keys per tile; the pair is summed at the end
  for (int j = j0; j < j1; ++j) {
    // the other image was last read in iteration j - 1, which ended with a barrier
    if (j + 1 < j1) {
      store_tile((j + 1) & 1);
      if (j + 2 < j1) load_tile(j + 2, pnext);
    }
    if constexpr (PAGED) pnext = page_id(j + 3);  // right behind the loads of tile j + 2, used in iteration j + 1
    const int kbase = j * KTILE;
    if (wave_live && kbase < wlast) {  // wave-uniform
      const char* ks = smem + (j & 1) * (2 * IMG);
      const char* vs = ks + IMG;
      f32x16 sacc[2] = {f32x16(0.f), f32x16(0.f)};
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        sacc[0] = mfma(lds_row(ks, c32, 2 * s + h), qf[s], sacc[0]);
        sacc[1] = mfma(lds_row(ks, 32 + c32, 2 * s + h), qf[s], sacc[1]);
      }
      if (kbase + KTILE > wfirst) {  // the tile reaches the wave's first row's limit (or the end)
        const int kmax = lim - kbase - 4 * h;  // tile-relative, exclusive
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
          for (int i = 0; i < 16; ++i)
            sacc[x][i] = (32 * x + (i & 3) + 8 * (i >> 2) < kmax) ? sacc[x][i] : -INFINITY;
      }
      float mt = -INFINITY;
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int i = 0; i < 16; ++i) mt = fmaxf(mt, sacc[x][i]);
      mt = pair_max(mt);
      const float m_new = fmaxf(m_i, mt * qscale);
      const float ms = m_new == -INFINITY ? 0.f : m_new;  // no live key yet
      const float alpha = fexp2(m_i - ms);
      m_i = m_new;
      float ps[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float p = fexp2(fmaf(sacc[x][i], qscale, -ms));
          sacc[x][i] = p;
          ps[i & 3] += p;
        }
      l_i = l_i * alpha + ((ps[0] + ps[1]) + (ps[2] + ps[3]));
#pragma unroll
      for (int d = 0; d < 4; ++d) acc[d] *= alpha;
      const bf16x8 pf[4] = {pack8(sacc[0], 0), pack8(sacc[0], 8), pack8(sacc[1], 0), pack8(sacc[1], 8)};
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int d = 0; d < 4; ++d) acc[d] = mfma(lds_tr(vs, 16 * s, 32 * d, lane), pf[s], acc[d]);
    }
    __syncthreads();
  }

  if constexpr (SPLIT) {
    const float l = pair_sum(l_i);
    if (h == 0) *reinterpret_cast<float2*>(slot + 2 * (w * 32 + c32)) = make_float2(m_i, l);
    if (wave_live && j0 * KTILE < wlast) {  // wave-uniform: the wave computed a tile
      float* ap = slot + WS_ML + w * (32 * DH) + 4 * lane;
#pragma unroll
      for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4v v = {acc[d][4 * g], acc[d][4 * g + 1], acc[d][4 * g + 2], acc[d][4 * g + 3]};
          *reinterpret_cast<float4v*>(ap + (4 * d + g) * 256) = v;
        }
    }
  } else if (t < T) {
    const float l = pair_sum(l_i);
    store_row(orow, acc, l > 0.f ? 1.f / l : 0.f, t < nw, h);
  }
}

// lanes 0..31 get {x, x of lane + 32}, lanes 32..63 get {y of lane - 32, y}
__device__ __forceinline__ void pair_swap(float x, float y, float& lo, float& hi) {
  const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(int, x), __builtin_bit_cast(int, y), false, false);
  lo = __builtin_bit_cast(float, (int)r[0]);
  hi = __builtin_bit_cast(float, (int)r[1]);
}

// grid (4 x query tile, Hkv, B): the 32 rows of wave block blockIdx.x & 3; header comment
__global__ __launch_bounds__(256) void chunk_attn_combine_kernel(
    const float* __restrict__ ws, const int* __restrict__ kv_len, const int* __restrict__ new_len,
    ushort* __restrict__ o, int T, int Hq, int Smax, int rep_shift, int nsplit) {
  const int qt = blockIdx.x >> 2, wb = blockIdx.x & 3, hkv = blockIdx.y, b = blockIdx.z;
  const int qtiles = gridDim.x >> 2;
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, d = tid >> 6;
  const int rep = 1 << rep_shift;
  int len0, nw;
  chunk_lens(kv_len, new_len, b, T, Smax, len0, nw);
  const int r = qt * QTILE + wb * 32 + (lane & 31);  // both lanes of a pair serve this row
  const int t = r >> rep_shift, hh = r & (rep - 1);
  if (t >= T) return;
  const float* slot = ws + (((long)b * gridDim.y + hkv) * qtiles + qt) * nsplit * WS_SLOT;
  const float* ml = slot + 2 * (wb * 32 + (lane & 31));
  const float* ap = slot + WS_ML + wb * (32 * DH) + (4 * d) * 256 + 4 * lane;

  float4v a[4] = {float4v(0.f), float4v(0.f), float4v(0.f), float4v(0.f)};
  float L = 0.f;
  if (t < nw) {
    float M = -INFINITY;
    for (int s = 0; s < nsplit; ++s) {
      const float2 x = *reinterpret_cast<const float2*>(ml + (long)s * WS_SLOT);
      if (x.y != 0.f) M = fmaxf(M, x.x);
    }
    for (int s = 0; s < nsplit; ++s) {
      const float2 x = *reinterpret_cast<const float2*>(ml + (long)s * WS_SLOT);
      if (x.y == 0.f) continue;  // a neutral partial: its accumulators were never written
      const float wgt = fexp2(x.x - M);
      L += wgt * x.y;
#pragma unroll
      for (int g = 0; g < 4; ++g) a[g] += wgt * *reinterpret_cast<const float4v*>(ap + (long)s * WS_SLOT + g * 256);
    }
  }
  const bool live = L > 0.f;  // false for t >= nw and for a row that saw no key (never NaN: L is then 0)
  const float f = live ? 1.f / L : 0.f;
  // a[g] holds dims 32 d + 8 g + 4 h + 0..3 of the row; after the swap this lane has 32 d + 16 h + 0..15
  ushort* orow = o + (((long)b * T + t) * Hq + hkv * rep + hh) * DH + 32 * d + 16 * h;
#pragma unroll
  for (int x = 0; x < 2; ++x) {
    ushort8 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float lo, hi;
      pair_swap(a[x][e], a[2 + x][e], lo, hi);
      v[e] = live ? f2bf(lo * f) : (ushort)0;
      v[4 + e] = live ? f2bf(hi * f) : (ushort)0;
    }
    *reinterpret_cast<ushort8*>(orow + 8 * x) = v;
  }
}

// PAGED: `pg` is one PageMap, kc / vc are the pools and stride_b is the page stride
template <bool PAGED, typename... PG>
__global__ __launch_bounds__(256) void chunk_rope_append_kernel(
    const ushort* __restrict__ qkv, const int* __restrict__ kv_len, const int* __restrict__ new_len,
    const float* __restrict__ cosT, const float* __restrict__ sinT, ushort* __restrict__ q_out,
    ushort* __restrict__ kc, ushort* __restrict__ vc, int T, int Hq, int Hkv, int Smax, long stride_b,
    long stride_h, PG... pg) {
  const long bt = blockIdx.x;
  const int b = (int)(bt / T), t = (int)(bt - (long)b * T);
  int len0, nw;
  chunk_lens(kv_len, new_len, b, T, Smax, len0, nw);
  if (t >= nw) {  // a dead row: nothing to the cache, zeros to q_out
    for (int i = threadIdx.x; i < Hq * 16; i += blockDim.x)
      *reinterpret_cast<ushort8*>(q_out + bt * Hq * DH + i * 8) = ushort8(0);
    return;
  }
  const int p = len0 + t;  // < Smax by the clamp: never a table or cache row out of range
  long row = b * stride_b + (long)p * DH;  // of KV head 0
  bool stored = true;
  if constexpr (PAGED) {
    const PageMap pm = page_map(pg...);
    const int id = pm.table[(long)b * pm.table_stride + (p >> 6)];  // p >> 6 < ceil(Smax / 64) <= table_stride
    stored = id >= 0 && id < pm.n_pages;  // a bad id: nothing of this row goes to the pool
    row = stored ? (long)id * stride_b + (long)(p & 63) * DH : 0;
  }
  const ushort* in = qkv + bt * (Hq + 2 * Hkv) * DH;
  const int nrot = (Hq + Hkv) * 8;    // 8-pair chunks of the rotated heads
  const int total = nrot + Hkv * 16;  // + 16-byte chunks of v
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    if (i < nrot) {
      const int hd = i >> 3, c = i & 7;
      const ushort8 x1 = *reinterpret_cast<const ushort8*>(in + hd * DH + c * 8);
      const ushort8 x2 = *reinterpret_cast<const ushort8*>(in + hd * DH + 64 + c * 8);
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
      if (hd >= Hq && !stored) continue;
      ushort* out = hd < Hq ? q_out + (bt * Hq + hd) * DH : kc + row + (hd - Hq) * stride_h;
      *reinterpret_cast<ushort8*>(out + c * 8) = y1;
      *reinterpret_cast<ushort8*>(out + 64 + c * 8) = y2;
    } else if (stored) {
      const int hd = (i - nrot) >> 4, c = (i - nrot) & 15;
      const ushort8 x = *reinterpret_cast<const ushort8*>(in + (Hq + Hkv + hd) * DH + c * 8);
      *reinterpret_cast<ushort8*>(vc + row + hd * stride_h + c * 8) = x;
    }
  }
}

bool chunk_geometry_ok(int B, int T, int Hq, int Hkv, int Dh, int Smax, long stride_b, long stride_h) {
  if (Dh != DH || B <= 0 || B > 65535 || T < 1 || T > (1 << 24) || (long)B * T > 0x7fffffffL || Hq <= 0 ||
      Hkv <= 0 || Hkv > 65535 || Hq % Hkv || Smax <= 0 || Smax > (1 << 30))
    return false;
  const int rep = Hq / Hkv;
  if (rep != 1 && rep != 2 && rep != 4 && rep != 8) return false;
  // rows are 16-byte aligned and heads / sequences do not overlap
  if (stride_h % 8 || stride_b % 8 || stride_h < (long)Smax * DH || stride_b < Hkv * stride_h) return false;
  return true;
}

// chunk_geometry_ok for a pool: every row of a sequence has a table entry; the table's rows, the pages and the
// heads of a page do not overlap
bool paged_chunk_geometry_ok(int B, int T, int Hq, int Hkv, int Dh, int Smax, int n_pages, int max_pages,
                             int table_stride, long stride_page, long stride_h) {
  if (Dh != DH || B <= 0 || B > 65535 || T < 1 || T > (1 << 24) || (long)B * T > 0x7fffffffL || Hq <= 0 ||
      Hkv <= 0 || Hkv > 65535 || Hq % Hkv || Smax <= 0 || Smax > (1 << 30))
    return false;
  const int rep = Hq / Hkv;
  if (rep != 1 && rep != 2 && rep != 4 && rep != 8) return false;
  if (n_pages <= 0 || max_pages <= 0 || (long)max_pages * KTILE < Smax || table_stride < max_pages) return false;
  if (stride_h % 8 || stride_page % 8 || stride_h < (long)KTILE * DH || stride_page < Hkv * stride_h) return false;
  return true;
}

int rep_shift_of(int rep) { return rep == 1 ? 0 : rep == 2 ? 1 : rep == 4 ? 2 : 3; }

}  // namespace

extern "C" int th_chunk_rope_append(const void* qkv, const int* kv_len, const int* new_len, const float* cosT,
                                    const float* sinT, void* q_out, void* kcache, void* vcache, int B, int T,
                                    int Hq, int Hkv, int Dh, int Smax, long stride_b, long stride_h,
                                    hipStream_t s) {
  if (!chunk_geometry_ok(B, T, Hq, Hkv, Dh, Smax, stride_b, stride_h)) return -1;
  chunk_rope_append_kernel<false><<<B * T, 256, 0, s>>>((const ushort*)qkv, kv_len, new_len, cosT, sinT,
                                                 (ushort*)q_out, (ushort*)kcache, (ushort*)vcache, T, Hq, Hkv,
                                                 Smax, stride_b, stride_h);
  TH_CHECK_LAUNCH();
}

// Query row (b, t, .) sees the first kv_len[b] + t + 1 keys where t < new_len[b]; both lengths are clamped
// on the device.
extern "C" int th_chunk_attn(const void* q, const void* kcache, const void* vcache, const int* kv_len,
                             const int* new_len, void* o, int B, int T, int Hq, int Hkv, int Dh, int Smax,
                             long stride_b, long stride_h, float scale, hipStream_t s) {
  if (!chunk_geometry_ok(B, T, Hq, Hkv, Dh, Smax, stride_b, stride_h)) return -1;
  const int rep = Hq / Hkv;
  const int rep_shift = rep == 1 ? 0 : rep == 2 ? 1 : rep == 4 ? 2 : 3;
  const dim3 grid((T * rep + QTILE - 1) / QTILE, Hkv, B);
  const float qscale = scale * 1.4426950408889634f;  // scores in the base-2 domain
  chunk_attn_kernel<false, false><<<grid, 256, 0, s>>>((const ushort*)q, (const ushort*)kcache, (const ushort*)vcache, kv_len,
                                         new_len, (ushort*)o, T, Hq, Smax, stride_b, stride_h, rep_shift, qscale);
  TH_CHECK_LAUNCH();
}

// th_chunk_attn on a grid of nsplit x as many workgroups; ws: B * Hkv * ceil(T * rep / 128) * nsplit * 128 * 130
// floats, which need not be cleared.
extern "C" int th_chunk_attn_split(const void* q, const void* kcache, const void* vcache, const int* kv_len,
                                   const int* new_len, void* o, void* ws, int B, int T, int Hq, int Hkv, int Dh,
                                   int Smax, long stride_b, long stride_h, int nsplit, float scale, hipStream_t s) {
  if (!chunk_geometry_ok(B, T, Hq, Hkv, Dh, Smax, stride_b, stride_h) || nsplit < 2 || nsplit > MAX_CHUNK_SPLITS)
    return -1;
  const int rep = Hq / Hkv;
  const int rep_shift = rep == 1 ? 0 : rep == 2 ? 1 : rep == 4 ? 2 : 3;
  const int qtiles = (int)(((long)T * rep + QTILE - 1) / QTILE);
  const float qscale = scale * 1.4426950408889634f;  // scores in the base-2 domain
  chunk_attn_kernel<true, false><<<dim3(qtiles * nsplit, Hkv, B), 256, 0, s>>>(
      (const ushort*)q, (const ushort*)kcache, (const ushort*)vcache, kv_len, new_len, (ushort*)o, T, Hq, Smax,
      stride_b, stride_h, rep_shift, qscale, (float*)ws, nsplit);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  chunk_attn_combine_kernel<<<dim3(qtiles * 4, Hkv, B), 256, 0, s>>>((const float*)ws, kv_len, new_len, (ushort*)o,
                                                                     T, Hq, Smax, rep_shift, nsplit);
  TH_CHECK_LAUNCH();
}

// th_chunk_rope_append through the page table: row p = kv_len[b] + t goes to row p & 63 of page table[b][p >> 6].
extern "C" int th_paged_chunk_rope_append(const void* qkv, const int* kv_len, const int* new_len, const int* table,
                                          const float* cosT, const float* sinT, void* q_out, void* kpool,
                                          void* vpool, int B, int T, int Hq, int Hkv, int Dh, int Smax, int n_pages,
                                          int max_pages, int table_stride, long stride_page, long stride_h,
                                          hipStream_t s) {
  if (!paged_chunk_geometry_ok(B, T, Hq, Hkv, Dh, Smax, n_pages, max_pages, table_stride, stride_page, stride_h))
    return -1;
  chunk_rope_append_kernel<true><<<B * T, 256, 0, s>>>((const ushort*)qkv, kv_len, new_len, cosT, sinT,
                                                       (ushort*)q_out, (ushort*)kpool, (ushort*)vpool, T, Hq, Hkv,
                                                       Smax, stride_page, stride_h,
                                                       PageMap{table, n_pages, table_stride});
  TH_CHECK_LAUNCH();
}

// th_chunk_attn on the pool: the rows of sequence b are those its table row names; the bits of th_chunk_attn.
extern "C" int th_paged_chunk_attn(const void* q, const void* kpool, const void* vpool, const int* table,
                                   const int* kv_len, const int* new_len, void* o, int B, int T, int Hq, int Hkv,
                                   int Dh, int Smax, int n_pages, int max_pages, int table_stride, long stride_page,
                                   long stride_h, float scale, hipStream_t s) {
  if (!paged_chunk_geometry_ok(B, T, Hq, Hkv, Dh, Smax, n_pages, max_pages, table_stride, stride_page, stride_h))
    return -1;
  const int rep = Hq / Hkv;
  const dim3 grid((int)(((long)T * rep + QTILE - 1) / QTILE), Hkv, B);
  const float qscale = scale * 1.4426950408889634f;  // scores in the base-2 domain
  chunk_attn_kernel<false, true><<<grid, 256, 0, s>>>(
      (const ushort*)q, (const ushort*)kpool, (const ushort*)vpool, kv_len, new_len, (ushort*)o, T, Hq, Smax,
      stride_page, stride_h, rep_shift_of(rep), qscale, PageMap{table, n_pages, table_stride});
  TH_CHECK_LAUNCH();
}

// th_chunk_attn_split on the pool (ws as there); the bits of th_chunk_attn_split at the same nsplit.
extern "C" int th_paged_chunk_attn_split(const void* q, const void* kpool, const void* vpool, const int* table,
                                         const int* kv_len, const int* new_len, void* o, void* ws, int B, int T,
                                         int Hq, int Hkv, int Dh, int Smax, int n_pages, int max_pages,
                                         int table_stride, long stride_page, long stride_h, int nsplit, float scale,
                                         hipStream_t s) {
  if (!paged_chunk_geometry_ok(B, T, Hq, Hkv, Dh, Smax, n_pages, max_pages, table_stride, stride_page, stride_h) ||
      nsplit < 2 || nsplit > MAX_CHUNK_SPLITS)
    return -1;
  const int rep = Hq / Hkv, rep_shift = rep_shift_of(rep);
  const int qtiles = (int)(((long)T * rep + QTILE - 1) / QTILE);
  const float qscale = scale * 1.4426950408889634f;  // scores in the base-2 domain
  chunk_attn_kernel<true, true><<<dim3(qtiles * nsplit, Hkv, B), 256, 0, s>>>(
      (const ushort*)q, (const ushort*)kpool, (const ushort*)vpool, kv_len, new_len, (ushort*)o, T, Hq, Smax,
      stride_page, stride_h, rep_shift, qscale, PageMap{table, n_pages, table_stride}, (float*)ws, nsplit);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  chunk_attn_combine_kernel<<<dim3(qtiles * 4, Hkv, B), 256, 0, s>>>((const float*)ws, kv_len, new_len, (ushort*)o,
                                                                     T, Hq, Smax, rep_shift, nsplit);
  TH_CHECK_LAUNCH();
}
