"""Chunked prefill on a PAGED KV cache: ``rope_append_chunk`` / ``chunk_attention`` (``ops/chunk_attention.py``)
through the page table of a ``PagedKVCache`` (``ops/paged_attention.py``).

This is what makes a shared prefix usable: after ``share_prefix(src, dst, rows)`` the rest of ``dst``'s prompt
goes into the cache as one chunk on top of the shared rows, not as one decode step per token.

``paged_rope_append_chunk(qkv [n, T, (Hq+2*Hkv)*128], cache, layer, new_lens, new_dev=None, seqs=None)`` and
``paged_chunk_attention(q [n, T, Hq*128], cache, layer, new_lens, new_dev=None, nsplit=None, seqs=None)`` have
the meaning of the dense ops.  ``seqs`` is a list of ``n`` distinct sequence indices (default: all
``cache.batch``, in order) saying which sequences the ``n`` rows of the batch dimension belong to, so a prefix
is prefilled for one sequence without running ``batch`` rows through the GEMMs.  The kernels need no
indirection for it: they take ``cache.seq_view(seqs)``, the lengths and table rows of ``seqs``, with ``B = n``.
Neither op moves the lengths; the model then calls ``cache.advance_seqs(seqs, new_lens)``.

The append reserves the pages of rows ``lens .. lens + new_lens - 1`` (it raises, with nothing changed, when
the pool is short) and refuses to write into a page whose reference count is above 1: copy-on-write is out of
scope, and ``share_prefix`` shares whole pages only, so the rows after a shared prefix start a page of their own.

The kernels are the paged instantiations of ``csrc/chunk_attn.hip``: a key tile is a page, its id is a scalar
load issued ahead of the tile's rows, and everything else is the dense kernel, so the output has the dense
kernel's bits on the same rows, at the same ``nsplit``, through any table.  GPU tensors run them (a missing
entry point raises); CPU tensors run the dense fp32 references on the rows gathered through the table, so a
paged and a dense cache with the same content give the same bits on the CPU as well.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .chunk_attention import (MAX_CHUNK_SPLITS, QUERY_TILE, WS_FLOATS_PER_ROW, chunk_attention_reference,
                              pick_chunk_nsplit, rope_append_chunk_reference)
from .decode_attention import HEAD_DIM
from .paged_attention import PAGE, PagedKVCache, pages_for
from .rope import rope_tables


def _check(x: torch.Tensor, cache: PagedKVCache, cols: int, layer: int, new_lens, new_dev, seqs, what: str):
    if not getattr(cache, "is_paged", False):
        raise ValueError(f"{what}: needs a PagedKVCache")
    if not 0 <= layer < cache.pool.shape[0]:
        raise ValueError(f"{what}: no layer {layer} in the cache")
    if cache.pool.dtype != torch.bfloat16 or not cache.pool.is_contiguous():
        raise ValueError(f"{what}: the pool must be a contiguous bf16 tensor")
    if (cache.table_dev.dtype != torch.int32 or not cache.table_dev.is_contiguous()
            or tuple(cache.table_dev.shape) != (cache.batch, cache.max_pages)):
        raise ValueError(f"{what}: table_dev must be contiguous int32 [{cache.batch}, {cache.max_pages}]")
    seqs = list(range(cache.batch)) if seqs is None else [int(s) for s in seqs]
    n = len(seqs)
    if n < 1 or len(set(seqs)) != n or min(seqs) < 0 or max(seqs) >= cache.batch:
        raise ValueError(f"{what}: seqs {seqs} must be distinct sequence indices in [0, {cache.batch})")
    if x.dtype != torch.bfloat16 or not x.is_contiguous() or x.device != cache.pool.device:
        raise ValueError(f"{what}: needs a contiguous bf16 tensor on the cache's device")
    if x.dim() != 3 or x.shape[0] != n or x.shape[1] < 1 or x.shape[2] != cols:
        raise ValueError(f"{what}: expected shape ({n}, T >= 1, {cols}), got {tuple(x.shape)}")
    T = x.shape[1]
    new = [int(k) for k in new_lens]
    if len(new) != n or min(new) < 0 or max(new) > T:
        raise ValueError(f"{what}: new_lens {new} must hold {n} values in [0, {T}]")
    lens = [cache.lens[s] for s in seqs]
    if min(lens) < 0 or max(a + k for a, k in zip(lens, new)) > cache.max_len:
        raise ValueError(f"{what}: lengths {lens} + new_lens {new} exceed the cache's max_len {cache.max_len}")
    if new_dev is None:
        new_dev = torch.tensor(new, dtype=torch.int32, device=x.device)
    elif (new_dev.dtype != torch.int32 or new_dev.device != x.device or tuple(new_dev.shape) != (n,)
          or not new_dev.is_contiguous()):
        raise ValueError(f"{what}: new_dev must be a contiguous int32 tensor [{n}] on the cache's device")
    return T, new, new_dev, seqs, lens


class _Rows:
    """The first ``rows[i]`` rows of sequence ``seqs[i]`` of one layer as a dense cache of ``len(seqs)``
    sequences: what the dense references read (``gather=True``) or write."""

    def __init__(self, cache: PagedKVCache, layer: int, seqs, lens, rows, gather: bool):
        self.cfg, self.max_len, self.lens, self.batch = cache.cfg, cache.max_len, list(lens), len(seqs)
        self.n_heads, self.n_kv_heads = cache.n_heads, cache.n_kv_heads
        self.kv = torch.zeros((2, self.batch, self.n_kv_heads, max(max(rows), 1), HEAD_DIM),
                              device=cache.device, dtype=torch.bfloat16)
        for i, (s, r) in enumerate(zip(seqs, rows)):
            if gather and r:
                self.kv[0, i, :, :r], self.kv[1, i, :, :r] = cache.gather(layer, s, r)

    def k(self, layer: int) -> torch.Tensor:
        return self.kv[0]

    def v(self, layer: int) -> torch.Tensor:
        return self.kv[1]


def paged_rope_append_chunk_reference(qkv, cache: PagedKVCache, layer: int, new, seqs, lens) -> torch.Tensor:
    """``rope_append_chunk_reference`` into a dense block, whose new rows then go through the table."""
    dense = _Rows(cache, layer, seqs, lens, [a + k for a, k in zip(lens, new)], gather=False)
    q = rope_append_chunk_reference(qkv, dense, 0, new)
    for i, (s, a, k) in enumerate(zip(seqs, lens, new)):
        if k == 0:
            continue
        r = torch.arange(a, a + k, device=qkv.device)
        page = torch.tensor(cache.table[s], dtype=torch.long, device=qkv.device)[r // PAGE]
        cache.k(layer)[page, :, r % PAGE] = dense.kv[0, i, :, a: a + k].transpose(0, 1)
        cache.v(layer)[page, :, r % PAGE] = dense.kv[1, i, :, a: a + k].transpose(0, 1)
    return q


def paged_rope_append_chunk(qkv: torch.Tensor, cache: PagedKVCache, layer: int, new_lens,
                            new_dev: torch.Tensor | None = None, seqs=None) -> torch.Tensor:
    """``rope_append_chunk`` on a paged cache for the sequences ``seqs``: reserves the pages of the live rows,
    rotates q / k of ``qkv [n, T, (Hq+2*Hkv)*128]`` at ``lens[seqs[i]] + t``, stores k / v through the table and
    returns the rotated q ``[n, T, Hq*128]`` (zeros in the rows ``t >= new_lens[i]``, which store nothing)."""
    Hq, Hkv = cache.n_heads, cache.n_kv_heads
    T, new, new_dev, seqs, lens = _check(qkv, cache, (Hq + 2 * Hkv) * HEAD_DIM, layer, new_lens, new_dev, seqs,
                                         "paged_rope_append_chunk")
    need = 0
    for s, a, k in zip(seqs, lens, new):
        if k == 0:
            continue
        for p in cache.table[s][a // PAGE: pages_for(a + k)]:
            if cache._refs[p] > 1:
                raise ValueError(f"paged_rope_append_chunk: rows {a}..{a + k - 1} of sequence {s} reach page {p}, "
                                 f"which {cache._refs[p]} sequences share: there is no copy-on-write, share whole "
                                 "pages and append behind them")
        need += max(0, pages_for(a + k) - len(cache.table[s]))
    if need > len(cache.free_pages):  # before the first reserve: a failure leaves every table as it was
        raise ValueError(f"paged_rope_append_chunk: the chunk needs {need} more pages, {len(cache.free_pages)} of "
                         f"{cache.n_pages} are free")
    for s, a, k in zip(seqs, lens, new):
        if k:
            cache.reserve(s, a + k)
    if not qkv.is_cuda:
        return paged_rope_append_chunk_reference(qkv, cache, layer, new, seqs, lens)
    cos, sin = rope_tables(cache.max_len, HEAD_DIM, cache.cfg.rope_theta, qkv.device)
    q = torch.empty((len(seqs), T, Hq * HEAD_DIM), device=qkv.device, dtype=qkv.dtype)
    kp, vp = cache.k(layer), cache.v(layer)
    lens_dev, table_dev = cache.seq_view(seqs)
    _lib.call("th_paged_chunk_rope_append", qkv.data_ptr(), lens_dev.data_ptr(), new_dev.data_ptr(),
              table_dev.data_ptr(), cos.data_ptr(), sin.data_ptr(), q.data_ptr(), kp.data_ptr(), vp.data_ptr(),
              len(seqs), T, Hq, Hkv, HEAD_DIM, cache.max_len, cache.n_pages, cache.max_pages, table_dev.stride(0),
              kp.stride(0), kp.stride(1), _lib.stream_ptr(qkv.device))
    return q


def paged_chunk_attention(q: torch.Tensor, cache: PagedKVCache, layer: int, new_lens,
                          new_dev: torch.Tensor | None = None, nsplit: int | None = None, seqs=None) -> torch.Tensor:
    """``q [n, T, Hq*128]`` (the output of ``paged_rope_append_chunk``) against the rows of ``seqs`` in
    ``layer`` -> ``o`` of the same shape: live row ``(i, t, h)`` attends over rows ``[0, lens[seqs[i]] + t + 1)``.
    ``nsplit`` overrides ``pick_chunk_nsplit`` (1: the unsplit kernel); CPU tensors ignore it."""
    Hq, Hkv = cache.n_heads, cache.n_kv_heads
    T, new, new_dev, seqs, lens = _check(q, cache, Hq * HEAD_DIM, layer, new_lens, new_dev, seqs,
                                         "paged_chunk_attention")
    if nsplit is not None and not 1 <= int(nsplit) <= MAX_CHUNK_SPLITS:
        raise ValueError(f"paged_chunk_attention: nsplit must be in [1, {MAX_CHUNK_SPLITS}], got {nsplit}")
    if any(k and a + k > cache.owned_rows(s) for s, a, k in zip(seqs, lens, new)):
        raise ValueError("paged_chunk_attention: a sequence has fewer pages than its lens + new_lens rows: "
                         "paged_rope_append_chunk() first")
    n = len(seqs)
    if not q.is_cuda:
        rows = [a + k if k else 0 for a, k in zip(lens, new)]
        return chunk_attention_reference(q, _Rows(cache, layer, seqs, lens, rows, gather=True), 0, new)
    rep = Hq // Hkv
    if nsplit is None:
        cus = torch.cuda.get_device_properties(q.device).multi_processor_count
        nsplit = pick_chunk_nsplit(n, Hkv, rep, T, max(a + k for a, k in zip(lens, new)), cus)
    nsplit = int(nsplit)
    o = torch.empty_like(q)
    kp, vp = cache.k(layer), cache.v(layer)
    lens_dev, table_dev = cache.seq_view(seqs)
    geometry = (n, T, Hq, Hkv, HEAD_DIM, cache.max_len, cache.n_pages, cache.max_pages, table_dev.stride(0),
                kp.stride(0), kp.stride(1))
    if nsplit > 1:
        qtiles = -(-T * rep // QUERY_TILE)
        ws = cache.workspace(n * Hkv * qtiles * nsplit * QUERY_TILE * WS_FLOATS_PER_ROW)
        _lib.call("th_paged_chunk_attn_split", q.data_ptr(), kp.data_ptr(), vp.data_ptr(), table_dev.data_ptr(),
                  lens_dev.data_ptr(), new_dev.data_ptr(), o.data_ptr(), ws.data_ptr(), *geometry, nsplit,
                  1.0 / math.sqrt(HEAD_DIM), _lib.stream_ptr(q.device))
        return o
    _lib.call("th_paged_chunk_attn", q.data_ptr(), kp.data_ptr(), vp.data_ptr(), table_dev.data_ptr(),
              lens_dev.data_ptr(), new_dev.data_ptr(), o.data_ptr(), *geometry, 1.0 / math.sqrt(HEAD_DIM),
              _lib.stream_ptr(q.device))
    return o
