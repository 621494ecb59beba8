"""Cascade decode attention on a paged KV cache whose sequences share their first pages.

``paged_cascade_decode_attention(q, cache, layer, shared_rows)`` has the shapes and meaning of
``paged_decode_attention``.  The first ``shared_rows`` rows (whole pages, at most ``min(lens)``) must be the
same pool pages for every sequence, as ``PagedKVCache.share_prefix`` leaves them.  ``csrc/paged_cascade_attn.hip``
then reads those pages once per KV head for the whole batch: all ``B * rep`` query rows of a KV head go through
them together, on MFMAs, in workgroups of at most 64 rows.  The rows behind the prefix go to a per-sequence
split-KV pass as in ``csrc/paged_attn.hip``, and one combine kernel merges the prefix partials and then the
suffix partials of every ``(b, q_head)`` in a fixed order (no atomics: two runs give the same bits).

Bytes per layer and step for Llama-3-8B, B 8, 4096 keys, 3584 shared: ``2 * 8 * 8 * 4096 * 256`` = 134 MB without,
``2 * 8 * (3584 + 8 * 512) * 256`` = 31.5 MB with (``profiles/decode_cascade/README.md`` has what was measured).

``ops/decode_attention.py::decode_attention`` calls this op for a paged cache with ``cache.cascade_rows > 0``
(``Llama.generate(cascade=True)`` sets it after the shared-prefix prefill).  GPU tensors run the gfx950 kernels
(a missing entry point raises); CPU tensors run ``paged_decode_attention_reference``, the same math, so the CPU
results keep their bits.  Every refusal is a ``ValueError`` before anything is launched or changed.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .decode_attention import HEAD_DIM, MAX_SPLITS, pick_nsplit
from .paged_attention import PAGE, PagedKVCache, _check, paged_decode_attention_reference, split_pages

GROUP_ROWS = 64  # query rows of one prefix workgroup (csrc/paged_cascade_attn.hip)
# fewest pages a prefix split is worth: a wave owns whole pages, so fewer leave some of the 4 waves idle while
# the workgroup still writes and the combine still reads a partial for each of its rows
MIN_PAGES_PER_PREFIX_SPLIT = 4


def pick_prefix_splits(rows: int, n_kv_heads: int, pages: int, n_cus: int) -> int:
    """Smallest split count that gives every CU a prefix workgroup (``splits * n_kv_heads * row_groups >=
    n_cus``), never leaving a split fewer than ``MIN_PAGES_PER_PREFIX_SPLIT`` pages; splits that the whole-page
    chunks leave empty are dropped."""
    groups = -(-rows // GROUP_ROWS)
    want = -(-n_cus // (n_kv_heads * groups))
    splits = max(1, min(want, pages // MIN_PAGES_PER_PREFIX_SPLIT, MAX_SPLITS))
    return -(-pages // -(-pages // splits))


def paged_cascade_decode_attention(q: torch.Tensor, cache: PagedKVCache, layer: int, shared_rows: int,
                                   nsplit: int | None = None, prefix_splits: int | None = None,
                                   new: int = 0) -> torch.Tensor:
    """``q [B, Hq*128]`` against the first ``lens[b] + new`` rows of ``layer`` -> ``o [B, Hq*128]``, the first
    ``shared_rows`` of them read once for all sequences.  ``nsplit`` (suffix) and ``prefix_splits`` override the
    automatic split counts (tests)."""
    Hq, Hkv = cache.n_heads, cache.n_kv_heads
    _check(q, cache, Hq * HEAD_DIM, layer, new, "paged_cascade_decode_attention")
    cache.check_shared_rows(shared_rows, "paged_cascade_decode_attention")
    for name, n in (("nsplit", nsplit), ("prefix_splits", prefix_splits)):
        if n is not None and not 1 <= int(n) <= 1024:
            raise ValueError(f"paged_cascade_decode_attention: {name} must be in [1, 1024]")
    if not q.is_cuda:
        return paged_decode_attention_reference(q, cache, layer, new)
    shared_pages = int(shared_rows) // PAGE
    suffix = max(cache.lens) + new - shared_pages * PAGE  # the longest one; 0 when every sequence ends with the prefix
    cus = torch.cuda.get_device_properties(q.device).multi_processor_count
    if nsplit is None:
        nsplit = pick_nsplit(cache.batch, Hkv, suffix, cus)
    if prefix_splits is None:
        prefix_splits = pick_prefix_splits(cache.batch * (Hq // Hkv), Hkv, shared_pages, cus)
    nsplit, prefix_splits = int(nsplit), int(prefix_splits)
    o = torch.empty_like(q)
    ws = cache.workspace(cache.batch * Hq * (prefix_splits + nsplit) * (HEAD_DIM + 2))
    kp, vp = cache.k(layer), cache.v(layer)
    _lib.call("th_paged_cascade_decode_attn", q.data_ptr(), kp.data_ptr(), vp.data_ptr(),
              cache.table_dev.data_ptr(), cache.lens_dev.data_ptr(), o.data_ptr(), ws.data_ptr(), cache.batch, Hq, Hkv,
              HEAD_DIM, cache.max_len, cache.n_pages, cache.max_pages, cache.table_dev.stride(0), kp.stride(0),
              kp.stride(1), shared_pages, prefix_splits, -(-shared_pages // prefix_splits), nsplit,
              split_pages(suffix, nsplit), int(new), 1.0 / math.sqrt(HEAD_DIM), _lib.stream_ptr(q.device))
    return o
