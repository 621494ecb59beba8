// Cascade decode attention over a PAGED KV cache whose sequences share their first pages.
//
// Pool, table and page size as in paged_attn.hip: K and V as [n_pages, Hkv, 64, 128] bf16, logical row
// r of sequence b in row r & 63 of page table[b][r >> 6].  The first `shared_pages` table entries of
// every sequence are the same (the host checks it), so those pages are read through the table row of
// sequence 0, once for the whole batch.  Head dim 128 only.
// th-build-flags: -fno-slp-vectorize -Xclang -target-feature -Xclang -packed-fp32-ops
//   (no v_pk_*_f32 in the f32 softmax math beside the MFMAs; the host pass ignores the feature)
//
// th_paged_cascade_decode_attn  three launches on one stream:
//
//   prefix   grid (prefix_splits, Hkv, row_groups).  All R = B * rep query rows of a KV head (row
//            r = b * rep + h, gathered from q[b, (kvh * rep + h) * 128 ..]) attend the shared pages.  A
//            workgroup serves the rows_per_group <= 64 rows of its group, NQ tiles of 16 (padding rows
//            repeat the group's last row and are never written), over the pages [split * chunk,
//            + chunk) of the prefix: the prefix leaves HBM once per group, not once per sequence.
//            Both products run on v_mfma_f32_16x16x32_bf16 with the query on the lane, as in
//            extend_attn.hip: S^T = K Q^T (A = 16 K rows, 16-byte loads HBM -> VGPR; B = Q, in
//            registers for the whole kernel) and O^T += V^T P^T (B = P^T packed to bf16 in place, A =
//            V^T read back transposed from the wave's private LDS slab, so the key loop has no
//            barrier).  A WAVE owns whole pages (wave w: pages w, w + 4, ... of the split), two steps
//            of 32 keys each; the page id is wave-uniform, read one page ahead, clamped to
//            [0, n_pages) and made scalar, so the K / V bases are SGPR pairs.  Registers are refilled
//            for the next step right after their last use, in a page's second step from the next
//            page.  Every prefix row is live for every sequence: no mask, no tail.  A column of
//            either product is one query, so rows of one tile never mix.
//   suffix   grid (nsplit, Hkv, B): the split-KV body of paged_attn.hip (VALU dot products, one
//            sequence per workgroup) over logical pages [shared_pages, ceil(len / 64)).  A sequence
//            with no row past the prefix writes the neutral element and reads nothing.
//   combine  one block per (b, q_head) merges its prefix_splits + nsplit partials, prefix first, in
//            index order: no atomics, so two runs give the same bits.
//
// Workspace: acc[B*Hq*NP][128] f32, then (m, l)[B*Hq*NP] f32 pairs, NP = prefix_splits + nsplit; the
// partial of (b, q_head, part) is (b * Hq + q_head) * NP + part; m in the base-2 domain.
#include "th_common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef unsigned uint4v __attribute__((ext_vector_type(4)));
#define LDS_AS __attribute__((address_space(3)))

namespace {

constexpr int DH = 128;
constexpr int NWAVE = 4;
constexpr int PAGE = 64;
constexpr int ROW_BYTES = DH * 2;
constexpr int WKEYS = 32;        // keys of one wave per step: two 16-key MFMA tiles, half a page
constexpr int VPITCH = 288;      // bytes per staged V row (extend_attn.hip)
constexpr int GROUP_ROWS = 64;   // most query rows of one workgroup
constexpr int LOADS = PAGE / 4;  // suffix: 4-row load instructions per page

__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ float4v mfma(ushort8 a, ushort8 b, float4v c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
                                                 c, 0, 0, 0);
}

// ---------------------------------------------------------------------------------------- prefix
template <int NQ>
__global__ __launch_bounds__(256) void cascade_prefix_kernel(
    const ushort* __restrict__ q, const ushort* __restrict__ kpool, const ushort* __restrict__ vpool,
    const int* __restrict__ table, float* __restrict__ ws, int B, int Hq, int n_pages, long stride_page,
    long stride_h, int shared_pages, int chunk_pages, int nparts, int rep_shift, int rows_per_group,
    float qscale) {
  const int split = blockIdx.x, hkv = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: so is everything about a page
  const int g = lane >> 4, c = lane & 15;
  const int rep = 1 << rep_shift;
  const int r0 = blockIdx.z * rows_per_group;  // first row of the group; the host leaves no group empty
  const int Rg = B * rep - r0 < rows_per_group ? B * rep - r0 : rows_per_group;  // 1 .. 16 * NQ

  float* ws_acc = ws;
  float* ws_ml = ws + (long)B * Hq * nparts * DH;
  auto q_head = [&](int r) {  // (b * Hq + q head) of row r of the group
    const int rr = r0 + r;
    return (long)(rr >> rep_shift) * Hq + hkv * rep + (rr & (rep - 1));
  };
  auto part = [&](int r) { return q_head(r) * nparts + split; };

  const int p0 = split * chunk_pages;
  const int p1 = p0 + chunk_pages < shared_pages ? p0 + chunk_pages : shared_pages;
  if (p0 >= p1) {  // no page: the neutral element, nothing read
    for (int i = tid; i < Rg * DH; i += 256) ws_acc[part(i >> 7) * DH + (i & 127)] = 0.f;
    if (tid < Rg) {
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
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    int r = n * 16 + c;
    r = r < Rg ? r : Rg - 1;  // padding rows repeat the last real one and are never written
    const ushort* qp = q + q_head(r) * DH + 8 * g;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[n][s] = *reinterpret_cast<const ushort8*>(qp + 32 * s);
  }

  float m[NQ], l[NQ];
  float4v acc[NQ][8];
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    m[n] = -INFINITY;
    l[n] = 0.f;
#pragma unroll
    for (int d = 0; d < 8; ++d) acc[n][d] = float4v{0.f, 0.f, 0.f, 0.f};
  }

  int pg = p0 + wid;
  if (pg < p1) {  // a wave without a page keeps the neutral state and joins the merge below
    const int* trow = table;  // sequence 0's row: the first shared_pages entries of every row are equal
    const long head_off = (long)hkv * stride_h;
    // logical page pg (< p1 <= shared_pages) -> byte bases of its K and V runs; a bad id is clamped
    auto k_base = [&](int id) { return (const char*)(kpool + (long)id * stride_page + head_off); };
    auto v_base = [&](int id) { return (const char*)(vpool + (long)id * stride_page + head_off); };
    auto page_id = [&](int p) {
      const int id = __builtin_amdgcn_readfirstlane(trow[p]);
      return id < 0 ? 0 : (id >= n_pages ? n_pages - 1 : id);
    };
    // this lane's bytes inside a 32-row half page: K row c (+ 16 x), dims 8 g (+ 32 s); V row g (+ 4 i), dims 8 c
    const unsigned klane = (unsigned)c * ROW_BYTES + 16 * g;
    const unsigned vlane = (unsigned)g * ROW_BYTES + 16 * c;
    char* vl = smem + wid * (WKEYS * VPITCH);
    // transposed read: lane 4 q + p of a group addresses row q, dims 4 p .. 4 p + 3 of the block
    const char* vt = vl + (4 * g + (c >> 2)) * VPITCH + (c & 3) * 8;

    int id = page_id(pg);
    const char *ck = k_base(id), *cv = v_base(id);
    ushort8 kr[2][4], vr[8];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int s = 0; s < 4; ++s)
        kr[x][s] = *reinterpret_cast<const ushort8*>(ck + klane + 16 * x * ROW_BYTES + 64 * s);
#pragma unroll
    for (int i = 0; i < 8; ++i) vr[i] = *reinterpret_cast<const ushort8*>(cv + vlane + 4 * i * ROW_BYTES);

    for (;;) {
      const int npg = pg + NWAVE;
      const bool more = npg < p1;
      // one page ahead; after the last page the refills re-read its first half and are dropped
      const int nid = more ? page_id(npg) : id;
      const char *nk = k_base(nid), *nv = v_base(nid);
#pragma unroll 1
      for (int hf = 0; hf < 2; ++hf) {  // the page's second step refills from the next page
        const char* fk = hf ? nk : ck + WKEYS * ROW_BYTES;
        const char* fv = hf ? nv : cv + WKEYS * ROW_BYTES;
        ushort8 pf[NQ];
#pragma unroll
        for (int n = 0; n < NQ; ++n) {
          float4v sc[2];
#pragma unroll
          for (int x = 0; x < 2; ++x) {
            sc[x] = float4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 4; ++s) sc[x] = mfma(kr[x][s], qf[n][s], sc[x]);
          }
          float mx = fmaxf(fmaxf(sc[0][0], sc[0][1]), fmaxf(sc[0][2], sc[0][3]));
          mx = fmaxf(mx, fmaxf(fmaxf(sc[1][0], sc[1][1]), fmaxf(sc[1][2], sc[1][3])));
          mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
          mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
          mx = fmaxf(m[n], mx * qscale);
          const float ms = mx == -INFINITY ? 0.f : mx;
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
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
          for (int s = 0; s < 4; ++s)
            kr[x][s] = *reinterpret_cast<const ushort8*>(fk + klane + 16 * x * ROW_BYTES + 64 * s);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          *reinterpret_cast<ushort8*>(vl + (4 * i + g) * VPITCH + c * 16) = vr[i];
          vr[i] = *reinterpret_cast<const ushort8*>(fv + vlane + 4 * i * ROW_BYTES);
        }
        // the slab is this wave's own: its stores above are ordered before these reads, and the reads
        // before the next step's stores, by the wave's in-order LDS queue
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int d = 0; d < 8; ++d) {
          const i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS i16x4*)(vt + d * 32));
          const i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS i16x4*)(vt + 16 * VPITCH + d * 32));
          const uint4v vv{(unsigned)(ushort)lo[0] | (unsigned)lo[1] << 16, (unsigned)(ushort)lo[2] | (unsigned)lo[3] << 16,
                          (unsigned)(ushort)hi[0] | (unsigned)hi[1] << 16, (unsigned)(ushort)hi[2] | (unsigned)hi[3] << 16};
          const ushort8 vf = __builtin_bit_cast(ushort8, vv);
#pragma unroll
          for (int n = 0; n < NQ; ++n) acc[n][d] = mfma(vf, pf[n], acc[n][d]);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
      if (!more) break;
      pg = npg;
      id = nid;
      ck = nk;
      cv = nv;
    }
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
  for (int i = tid; i < Rg * DH; i += 256) {
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

// ---------------------------------------------------------------------------------------- suffix
// The body of paged_attn.hip's paged_decode_attn_kernel, started at logical page `first_page` and
// writing its partials behind the prefix's: see that file for the work split and the data movement.
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

// One page as a wave sees it: scalar K / V bases of its (page, kv_head) run and the last live row.
struct PageRef {
  const char* k;
  const char* v;
  int lastrow;  // 63, less in a sequence's last page
};

// byte offset of this lane's 16 bytes of row min(r, lastrow): 32 bits beside the scalar base
__device__ __forceinline__ unsigned row_off(int r, int lastrow, int dl16) {
  return (unsigned)(r < lastrow ? r : lastrow) * ROW_BYTES + dl16;
}

// Consume the sub-tile in kr / vr (rows r0 + 4 * i + grp of page `cur`) and refill every register, right
// after its last use, with row nr0 + 4 * i + grp of page `src`.
template <int REP, int ST>
__device__ __forceinline__ void subtile(ushort8 (&kr)[ST], ushort8 (&vr)[ST], const float (&qf)[REP][8],
                                        float (&m)[REP], float (&l)[REP], float (&acc)[REP][8],
                                        const PageRef& cur, int r0, const PageRef& src, int nr0, int grp,
                                        int dl16) {
  float s[ST][REP];
#pragma unroll
  for (int i = 0; i < ST; ++i) {
    float kf[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) kf[j] = bf2f(kr[i][j]);
    kr[i] = *reinterpret_cast<const ushort8*>(src.k + row_off(nr0 + 4 * i + grp, src.lastrow, dl16));
#pragma unroll
    for (int h = 0; h < REP; ++h) {
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) d = fmaf(qf[h][j], kf[j], d);
      s[i][h] = row16_sum(d);
    }
  }
  if (cur.lastrow < PAGE - 1) {  // wave-uniform: only a sequence's last page has dead rows
#pragma unroll
    for (int i = 0; i < ST; ++i) {
      const bool dead = r0 + 4 * i + grp > cur.lastrow;
#pragma unroll
      for (int h = 0; h < REP; ++h) s[i][h] = dead ? -INFINITY : s[i][h];
    }
  }
#pragma unroll
  for (int h = 0; h < REP; ++h) {
    float mx = m[h];
#pragma unroll
    for (int i = 0; i < ST; ++i) mx = fmaxf(mx, s[i][h]);
    const float ms = mx == -INFINITY ? 0.f : mx;  // a group that has seen no live key yet
    const float alpha = fexp2(m[h] - ms);
    float ps = 0.f;
#pragma unroll
    for (int i = 0; i < ST; ++i) {
      s[i][h] = fexp2(s[i][h] - ms);
      ps += s[i][h];
    }
    l[h] = l[h] * alpha + ps;
    m[h] = mx;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[h][j] *= alpha;
  }
#pragma unroll
  for (int i = 0; i < ST; ++i) {
    float vf[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) vf[j] = bf2f(vr[i][j]);
    vr[i] = *reinterpret_cast<const ushort8*>(src.v + row_off(nr0 + 4 * i + grp, src.lastrow, dl16));
#pragma unroll
    for (int h = 0; h < REP; ++h)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[h][j] = fmaf(s[i][h], vf[j], acc[h][j]);
  }
}

template <int REP, int ST>
__global__ __launch_bounds__(256) void cascade_suffix_kernel(
    const ushort* __restrict__ q, const ushort* __restrict__ kpool, const ushort* __restrict__ vpool,
    const int* __restrict__ table, const int* __restrict__ kv_len, float* __restrict__ ws, int Hq, int Smax,
    int n_pages, int table_stride, long stride_page, long stride_h, int first_page, int part_base, int nparts,
    int chunk_pages, int extra, float qscale) {
  const int split = blockIdx.x, hkv = blockIdx.y, b = blockIdx.z;
  const int nsplit = gridDim.x, B = gridDim.z;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = lane >> 4, dl = lane & 15;  // row sub-index in a 4-row load, 8-dim slice

  float* ws_acc = ws;
  float* ws_ml = ws + (long)B * Hq * nparts * DH;
  const long part0 = ((long)b * Hq + (long)hkv * REP) * nparts + part_base + split;  // + h * nparts per head

  long len = (long)kv_len[b] + extra;
  len = len < 0 ? 0 : (len > Smax ? Smax : len);  // before any table entry or address is formed
  const int live_pages = (int)((len + PAGE - 1) / PAGE);  // <= max_pages <= table_stride (entry point)
  const int p0 = first_page + split * chunk_pages;
  int p1 = split == nsplit - 1 ? live_pages : p0 + chunk_pages;
  p1 = p1 > live_pages ? live_pages : p1;
  if (p0 >= p1) {  // no page (every split of a sequence that ends with the prefix): the neutral element
    for (int i = tid; i < REP * DH; i += 256) ws_acc[(part0 + (long)(i >> 7) * nparts) * DH + (i & 127)] = 0.f;
    if (tid < REP) {
      ws_ml[(part0 + (long)tid * nparts) * 2] = -INFINITY;
      ws_ml[(part0 + (long)tid * nparts) * 2 + 1] = 0.f;
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
  float m[REP], l[REP], acc[REP][8];
#pragma unroll
  for (int h = 0; h < REP; ++h) {
    m[h] = -INFINITY;
    l[h] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[h][j] = 0.f;
  }

  const int* trow = table + (long)b * table_stride;
  const long head_off = (long)hkv * stride_h;
  // logical page pg (< p1 <= live_pages) -> its scalar bases; a bad id is clamped, never followed
  auto page_ref = [&](int pg) {
    int id = __builtin_amdgcn_readfirstlane(trow[pg]);
    id = id < 0 ? 0 : (id >= n_pages ? n_pages - 1 : id);
    const long off = (long)id * stride_page + head_off;
    return PageRef{(const char*)(kpool + off), (const char*)(vpool + off),
                   pg == live_pages - 1 ? (int)len - 1 - pg * PAGE : PAGE - 1};
  };

  int pg = p0 + wid;
  if (pg < p1) {  // a wave without a page keeps the neutral state and joins the merge below
    const int dl16 = dl * 16;
    PageRef cur = page_ref(pg);
    ushort8 kr[ST], vr[ST];
#pragma unroll
    for (int i = 0; i < ST; ++i) kr[i] = *reinterpret_cast<const ushort8*>(cur.k + row_off(4 * i + grp, cur.lastrow, dl16));
#pragma unroll
    for (int i = 0; i < ST; ++i) vr[i] = *reinterpret_cast<const ushort8*>(cur.v + row_off(4 * i + grp, cur.lastrow, dl16));
    for (;;) {
      const int npg = pg + NWAVE;
      const bool more = npg < p1;
      // one page ahead; after the last page the refills re-read row 0 of it and are dropped
      const PageRef nxt = more ? page_ref(npg) : PageRef{cur.k, cur.v, 0};
#pragma unroll 1
      for (int t = 0; t < LOADS / ST; ++t) {  // the page's last sub-tile refills from the next page
        const bool last = t == LOADS / ST - 1;
        subtile<REP, ST>(kr, vr, qf, m, l, acc, cur, t * ST * 4, last ? nxt : cur, last ? 0 : (t + 1) * ST * 4,
                         grp, dl16);
      }
      if (!more) break;
      pg = npg;
      cur = nxt;
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
    const long p = part0 + (long)h * nparts;
    ws_acc[p * DH + d] = a;
    if (d == 0) {
      ws_ml[p * 2] = mx;
      ws_ml[p * 2 + 1] = lv;
    }
  }
}

// ---------------------------------------------------------------------------------------- combine
// one block of 128 threads per (b, q_head): the prefix partials, then the suffix partials, in index order
__global__ __launch_bounds__(128) void cascade_combine_kernel(const float* __restrict__ ws, ushort* __restrict__ o,
                                                              long nrows, int nparts) {
  const long bh = blockIdx.x;
  const int d = threadIdx.x;
  const float* acc = ws + bh * nparts * DH;
  const float* ml = ws + nrows * nparts * DH + bh * nparts * 2;
  float mx = -INFINITY;
#pragma unroll 4
  for (int s = 0; s < nparts; ++s) mx = fmaxf(mx, ml[2 * s]);
  float a = 0.f, lv = 0.f;
  // no branch in the body: the loads of 4 parts are in flight together.  An empty split holds (-inf, 0, 0)
  // and gets the factor 0.
#pragma unroll 4
  for (int s = 0; s < nparts; ++s) {
    const float ms = ml[2 * s];
    const float f = ms == -INFINITY ? 0.f : fexp2(ms - mx);
    a += acc[(long)s * DH + d] * f;
    lv += ml[2 * s + 1] * f;
  }
  o[bh * DH + d] = f2bf(lv > 0.f ? a / lv : 0.f);  // no live key at all: zeros
}

bool cascade_geometry_ok(int B, int Hq, int Hkv, int Dh, int Smax, int n_pages, int max_pages, int table_stride,
                         long stride_page, long stride_h) {
  if (Dh != DH || B <= 0 || B > 65535 || Hq <= 0 || Hkv <= 0 || Hkv > 65535 || Hq % Hkv || Smax <= 0) return false;
  const int rep = Hq / Hkv;
  if (rep != 1 && rep != 2 && rep != 4 && rep != 8) return false;
  // every row of a sequence has a table entry, and the table's rows do not overlap
  if (n_pages <= 0 || max_pages <= 0 || (long)max_pages * PAGE < Smax || table_stride < max_pages) return false;
  // rows are 16-byte aligned and heads / pages do not overlap
  if (stride_h % 8 || stride_page % 8 || stride_h < (long)PAGE * DH || stride_page < Hkv * stride_h) return false;
  return true;
}

}  // namespace

// ws: B * Hq * (prefix_splits + nsplit) * 130 floats.  The first shared_pages table entries of every
// sequence must be equal (the caller's check): they are read from table row 0.  Prefix split s takes
// the shared pages [s * prefix_chunk_pages, + prefix_chunk_pages); suffix split s the logical pages
// [shared_pages + s * chunk_pages, + chunk_pages) below ceil((kv_len[b] + extra) / 64), the last one the rest.
extern "C" int th_paged_cascade_decode_attn(const void* q, const void* kpool, const void* vpool, const int* table,
                                            const int* kv_len, void* o, float* ws, int B, int Hq, int Hkv, int Dh,
                                            int Smax, int n_pages, int max_pages, int table_stride,
                                            long stride_page, long stride_h, int shared_pages, int prefix_splits,
                                            int prefix_chunk_pages, int nsplit, int chunk_pages, int extra,
                                            float scale, hipStream_t s) {
  if (!cascade_geometry_ok(B, Hq, Hkv, Dh, Smax, n_pages, max_pages, table_stride, stride_page, stride_h)) return -1;
  if (shared_pages < 1 || shared_pages > max_pages) return -1;
  if (prefix_splits <= 0 || prefix_splits > 1024 || prefix_chunk_pages <= 0 || prefix_chunk_pages > max_pages ||
      (long)prefix_splits * prefix_chunk_pages < shared_pages)
    return -1;
  if (nsplit <= 0 || nsplit > 1024 || chunk_pages <= 0 || (long)nsplit * chunk_pages > (1L << 24)) return -1;
  const int rep = Hq / Hkv;
  const int rep_shift = rep == 1 ? 0 : rep == 2 ? 1 : rep == 4 ? 2 : 3;
  const int R = B * rep;
  const int groups = (R + GROUP_ROWS - 1) / GROUP_ROWS;
  const int rows_per_group = ((R + groups - 1) / groups + 15) / 16 * 16;  // <= 64, and no group is empty
  const int nparts = prefix_splits + nsplit;
  const float qscale = scale * 1.4426950408889634f;  // scores in the base-2 domain
  const ushort *qp = (const ushort*)q, *kp = (const ushort*)kpool, *vp = (const ushort*)vpool;

  const dim3 pgrid(prefix_splits, Hkv, groups);
#define TH_CASCADE_PREFIX(NQ)                                                                                 \
  cascade_prefix_kernel<NQ><<<pgrid, 256, 0, s>>>(qp, kp, vp, table, ws, B, Hq, n_pages, stride_page, stride_h, \
                                                  shared_pages, prefix_chunk_pages, nparts, rep_shift,        \
                                                  rows_per_group, qscale)
  switch (rows_per_group / 16) {
    case 1: TH_CASCADE_PREFIX(1); break;
    case 2: TH_CASCADE_PREFIX(2); break;
    case 3: TH_CASCADE_PREFIX(3); break;
    default: TH_CASCADE_PREFIX(4); break;
  }
#undef TH_CASCADE_PREFIX
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;

  const dim3 sgrid(nsplit, Hkv, B);
#define TH_CASCADE_SUFFIX(REP, ST)                                                                       \
  cascade_suffix_kernel<REP, ST><<<sgrid, 256, 0, s>>>(qp, kp, vp, table, kv_len, ws, Hq, Smax, n_pages, \
                                                       table_stride, stride_page, stride_h, shared_pages, \
                                                       prefix_splits, nparts, chunk_pages, extra, qscale)
  switch (rep) {
    case 1: TH_CASCADE_SUFFIX(1, 8); break;
    case 2: TH_CASCADE_SUFFIX(2, 8); break;
    case 4: TH_CASCADE_SUFFIX(4, 8); break;
    default: TH_CASCADE_SUFFIX(8, 4); break;
  }
#undef TH_CASCADE_SUFFIX
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  cascade_combine_kernel<<<B * Hq, 128, 0, s>>>(ws, (ushort*)o, (long)B * Hq, nparts);
  TH_CHECK_LAUNCH();
}
