// Single-token (decode) GQA attention over a PAGED KV cache, and the RoPE + append step before it.
//
// Pool of one layer: K and V as [n_pages, Hkv, 64, 128] bf16, every (page, kv_head) one contiguous
// 16 KB run of 64 rows of 256 bytes.  table [B, table_stride] int32 maps logical page p of sequence
// b to a pool page: logical row r lives in row r & 63 of page table[b][r >> 6].  The entry points
// take the layer's K / V base pointers and the page / head strides in elements.  Head dim 128 only.
//
// th-build-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
//
// th_paged_rope_append  the arithmetic of th_decode_rope_append (decode_attn.hip), so the same bits;
//                       the row address comes from table[b][pos >> 6] and pos & 63.  pos is checked
//                       against [0, Smax) and the page id against [0, n_pages) before any address is
//                       formed; a sequence that fails either check writes nothing at all.
// th_paged_decode_attn  split-KV attention on grid (nsplit, Hkv, B).  Splits cover whole pages:
//                       split s owns logical pages [s * chunk_pages, (s + 1) * chunk_pages) (the last
//                       one takes the rest) below ceil(len / 64); a workgroup with no page writes the
//                       neutral element and reads nothing.
//
//   Work split.  A WAVE owns whole pages: wave w of the workgroup takes pages w, w + 4, ... of the
//   split.  The page id is therefore wave-uniform: it is read once per page, one page ahead of its
//   use, clamped to [0, n_pages) and made scalar (readfirstlane), so the K and V base addresses of
//   a page are two SGPR pairs and nothing per lane depends on the table.
//   Data movement.  Inside a page a load instruction fetches 4 whole rows (lane group g = lane / 16
//   takes row 4 * i + g, lane d of the group its dims 8 * d .. 8 * d + 7): 16-byte loads straight to
//   VGPRs off the scalar base, at offsets inside the 16 KB run (the row clamp of the tail rule
//   below only binds in a sequence's last page).  No LDS staging.  A page is 16
//   loads of K and 16 of V; ST of them (the sub-tile: 8, or 4 at rep 8 to stay inside the register
//   budget of 2 waves per SIMD) are in flight per wave.  Every register is refilled for the next
//   sub-tile right after its last use; in a page's last sub-tile the refills already come from the
//   NEXT page's base, so the stream does not drain at a page boundary.  The refills after a wave's
//   last page hit row 0 of that page again (cache hits, never consumed).
//   Math.  QK^T per 16-lane group with DPP adds; one online softmax state (f32, base 2) per lane
//   group; the 16 states of a workgroup are merged once at the end (shuffles, then LDS) and written
//   as (m, l, acc[rep][128]) f32 partials.  The combine kernel merges the nsplit partials of every
//   (b, q_head) in split order: no atomics, so two runs give the same bits.
//   Tail.  Rows at or past len in a sequence's last page are loaded from its last live row and
//   masked; table entries at or past ceil(len / 64) are never read.
#include "th_common.h"

namespace {

constexpr int DH = 128;
constexpr int NWAVE = 4;
constexpr int PAGE = 64;
constexpr int LOADS = PAGE / 4;  // 4-row load instructions per page, for K and for V

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

__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }

// One page as a wave sees it: scalar K / V bases of its (page, kv_head) run and the last live row.
struct PageRef {
  const char* k;
  const char* v;
  int lastrow;  // 63, less in a sequence's last page
};

// byte offset of this lane's 16 bytes of row min(r, lastrow): 32 bits beside the scalar base
__device__ __forceinline__ unsigned row_off(int r, int lastrow, int dl16) {
  return (unsigned)(r < lastrow ? r : lastrow) * (DH * 2) + dl16;
}

// Consume the sub-tile in kr / vr (rows r0 + 4 * i + grp of page `cur`) and refill every register, right
// after its last use, with row nr0 + 4 * i + grp of page `src`: the same page's next sub-tile, or
// the first one of the wave's next page.
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

// Workspace: acc[B*Hq*nsplit][128] f32, then (m, l)[B*Hq*nsplit] f32 pairs; m in the base-2 domain.
template <int REP, int ST>
__global__ __launch_bounds__(256) void paged_decode_attn_kernel(
    const ushort* __restrict__ q, const ushort* __restrict__ kpool, const ushort* __restrict__ vpool,
    const int* __restrict__ table, const int* __restrict__ kv_len, float* __restrict__ ws, int Hq, int Smax,
    int n_pages, int table_stride, long stride_page, long stride_h, int nsplit, int chunk_pages, int extra,
    float qscale) {
  const int split = blockIdx.x, hkv = blockIdx.y, b = blockIdx.z;
  const int B = gridDim.z;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: so is everything about a page
  const int grp = lane >> 4, dl = lane & 15;                 // row sub-index in a 4-row load, 8-dim slice

  float* ws_acc = ws;
  float* ws_ml = ws + (long)B * Hq * nsplit * DH;
  const long part0 = ((long)b * Hq + (long)hkv * REP) * nsplit + split;  // + h * nsplit per head

  long len = (long)kv_len[b] + extra;
  len = len < 0 ? 0 : (len > Smax ? Smax : len);  // before any table entry or address is formed
  const int live_pages = (int)((len + PAGE - 1) / PAGE);  // <= max_pages <= table_stride (entry point)
  const int p0 = split * chunk_pages;
  int p1 = split == nsplit - 1 ? live_pages : p0 + chunk_pages;
  p1 = p1 > live_pages ? live_pages : p1;
  if (p0 >= p1) {  // no page: the neutral element, nothing read
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
    return PageRef{(const char*)(kpool + off), (const char*)(vpool + off), pg == live_pages - 1 ? (int)len - 1 - pg * PAGE : PAGE - 1};
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
    const long p = part0 + (long)h * nsplit;
    ws_acc[p * DH + d] = a;
    if (d == 0) {
      ws_ml[p * 2] = mx;
      ws_ml[p * 2 + 1] = lv;
    }
  }
}

// one block of 128 threads per (b, q_head): partials merged in split order (as decode_attn.hip's)
__global__ __launch_bounds__(128) void paged_combine_kernel(const float* __restrict__ ws, ushort* __restrict__ o,
                                                            long nparts, int nsplit) {
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

__global__ __launch_bounds__(256) void paged_rope_append_kernel(
    const ushort* __restrict__ qkv, const int* __restrict__ pos, const int* __restrict__ table,
    const float* __restrict__ cosT, const float* __restrict__ sinT, ushort* __restrict__ q_out,
    ushort* __restrict__ kpool, ushort* __restrict__ vpool, int Hq, int Hkv, int Smax, int n_pages,
    int table_stride, long stride_page, long stride_h) {
  const int b = blockIdx.x;
  const int p = pos[b];
  if (p < 0 || p >= Smax) return;  // never a rope table row, page table entry or pool row out of range
  const int id = table[(long)b * table_stride + (p >> 6)];  // p >> 6 < max_pages <= table_stride
  if (id < 0 || id >= n_pages) return;
  const long row = (long)id * stride_page + (long)(p & 63) * DH;  // + head * stride_h
  const ushort* in = qkv + (long)b * (Hq + 2 * Hkv) * DH;
  const int nrot = (Hq + Hkv) * 8;    // 8-pair chunks of the rotated heads
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
      ushort* out = h < Hq ? q_out + ((long)b * Hq + h) * DH : kpool + row + (h - Hq) * stride_h;
      *reinterpret_cast<ushort8*>(out + c * 8) = y1;
      *reinterpret_cast<ushort8*>(out + 64 + c * 8) = y2;
    } else {
      const int h = (i - nrot) >> 4, c = (i - nrot) & 15;
      const ushort8 x = *reinterpret_cast<const ushort8*>(in + (Hq + Hkv + h) * DH + c * 8);
      *reinterpret_cast<ushort8*>(vpool + row + h * stride_h + c * 8) = x;
    }
  }
}

bool pool_geometry_ok(int B, int Hq, int Hkv, int Dh, int Smax, int n_pages, int max_pages, int table_stride,
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

extern "C" int th_paged_rope_append(const void* qkv, const int* pos, const int* table, const float* cosT,
                                    const float* sinT, void* q_out, void* kpool, void* vpool, int B, int Hq,
                                    int Hkv, int Dh, int Smax, int n_pages, int max_pages, int table_stride,
                                    long stride_page, long stride_h, hipStream_t s) {
  if (!pool_geometry_ok(B, Hq, Hkv, Dh, Smax, n_pages, max_pages, table_stride, stride_page, stride_h)) return -1;
  paged_rope_append_kernel<<<B, 256, 0, s>>>((const ushort*)qkv, pos, table, cosT, sinT, (ushort*)q_out,
                                             (ushort*)kpool, (ushort*)vpool, Hq, Hkv, Smax, n_pages,
                                             table_stride, stride_page, stride_h);
  TH_CHECK_LAUNCH();
}

// ws: B * Hq * nsplit * 130 floats.  kv_len[b] + extra rows are valid, clamped to [0, Smax] on the
// device; logical pages [split * chunk_pages, +chunk_pages) go to split `split`, the last takes the rest.
extern "C" int th_paged_decode_attn(const void* q, const void* kpool, const void* vpool, const int* table,
                                    const int* kv_len, void* o, float* ws, int B, int Hq, int Hkv, int Dh,
                                    int Smax, int n_pages, int max_pages, int table_stride, long stride_page,
                                    long stride_h, int nsplit, int chunk_pages, int extra, float scale,
                                    hipStream_t s) {
  if (!pool_geometry_ok(B, Hq, Hkv, Dh, Smax, n_pages, max_pages, table_stride, stride_page, stride_h)) return -1;
  if (nsplit <= 0 || nsplit > 1024 || chunk_pages <= 0 || (long)nsplit * chunk_pages > (1L << 24)) return -1;
  const dim3 grid(nsplit, Hkv, B);
  const float qscale = scale * 1.4426950408889634f;  // scores in the base-2 domain
#define TH_PAGED_LAUNCH(REP, ST)                                                                        \
  paged_decode_attn_kernel<REP, ST><<<grid, 256, 0, s>>>(                                               \
      (const ushort*)q, (const ushort*)kpool, (const ushort*)vpool, table, kv_len, ws, Hq, Smax, n_pages, \
      table_stride, stride_page, stride_h, nsplit, chunk_pages, extra, qscale)
  switch (Hq / Hkv) {
    case 1: TH_PAGED_LAUNCH(1, 8); break;
    case 2: TH_PAGED_LAUNCH(2, 8); break;
    case 4: TH_PAGED_LAUNCH(4, 8); break;
    default: TH_PAGED_LAUNCH(8, 4); break;
  }
#undef TH_PAGED_LAUNCH
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  paged_combine_kernel<<<B * Hq, 128, 0, s>>>(ws, (ushort*)o, (long)B * Hq * nsplit, nsplit);
  TH_CHECK_LAUNCH();
}
