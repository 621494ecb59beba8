"""Chunked prefill on a bf16 KV cache: a block of ``T`` new tokens per sequence, of any length, on top
of a cache that already holds ``lens[b]`` rows (0 included).

``new_lens[b]`` in ``0..T`` says how many of sequence ``b``'s ``T`` rows are live; the rows after them are
padding (a shorter prompt in the same batch).  ``rope_append_chunk(qkv [B, T, (Hq+2*Hkv)*128], cache,
layer, new_lens)`` rotates a live row ``(b, t)`` at position ``lens[b] + t``, stores its k / v in cache row
``lens[b] + t`` and returns the rotated q ``[B, T, Hq*128]``, with the bits of single ``rope_append``
calls; a padding row writes nothing to the cache and zeros to q.  ``chunk_attention(q [B, T, Hq*128],
cache, layer, new_lens)`` is called after it: a live query row ``(b, t, h)`` attends over cache rows
``[0, lens[b] + t + 1)`` of its KV head, a padding row gets zeros.  Neither moves the lengths; the model
then calls ``cache.set_lens(lens + new_lens)``.  Both take ``new_dev``, ``new_lens`` as an int32 tensor on
the cache's device, so that a model step uploads it once and not once per layer.

The kernels are in ``csrc/chunk_attn.hip``: a workgroup serves ``QUERY_TILE`` query rows of one KV head
(``QUERY_TILE / rep`` consecutive tokens times the ``rep`` query heads), its four waves share K / V tiles
of ``KEY_TILE`` keys through LDS, and no partial leaves the workgroup, so two runs give the same bits.

A short chunk on a long cache has too few query tiles to fill the device, so ``chunk_attention`` then
splits every tile's own causal key range into ``nsplit`` equal parts of whole key tiles
(``th_chunk_attn_split``): ``nsplit`` times as many workgroups write unnormalised f32 partials into
``cache.workspace`` and a second kernel merges them in split order, with no atomic, so two runs still
give the same bits (they differ from the unsplit kernel's by the f32 rounding of the merge).
``pick_chunk_nsplit`` is the rule; ``nsplit=`` overrides it (tests, benchmarks).  Out of scope here:

* an FP8 cache (a ``ValueError``: chunk steps need a bf16 cache);
* for ``T <= 8`` ``extend_attention`` remains the right call, and nothing dispatches between the two;
* isolation from a NaN in a *live* later row of the same chunk (``0 * NaN`` in the PV product).  Rows at
  or past ``lens[b] + new_lens[b]`` are never read and may hold anything.

GPU tensors run the gfx950 kernels (a missing entry point raises); CPU tensors run the fp32 references
below, which are also the CPU tests' oracle.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .decode_attention import HEAD_DIM, KVCache
from .rope import rope_tables

QUERY_TILE = 128  # query rows (token x query head of one KV head) of a workgroup
KEY_TILE = 64     # keys per staged K / V tile
MAX_CHUNK_SPLITS = 16
# fewest keys of the longest sequence per split.  At or below 1024 keys a call is never split.  Measured
# (profiles/prefill_chunk_split): B 1, 32 / 8 heads, 64 or 128 tokens on 8192 rows take 0.074 ms at 1024
# (8 splits), 0.095 ms at 2048 (4) and 0.150 ms at 4096 (2) against 0.26 ms unsplit; 512 tokens on 3584
# rows take 0.092 ms at 1024 or 2048 (2 splits) against 0.143 ms at 4096 (unsplit).  1024 stays.
MIN_KEYS_PER_CHUNK_SPLIT = 1024
WS_FLOATS_PER_ROW = HEAD_DIM + 2  # a partial: the row's f32 accumulators and (m, l)


def pick_chunk_nsplit(batch: int, n_kv_heads: int, rep: int, T: int, longest_keys: int, n_cus: int) -> int:
    """Smallest split count that gives every CU a workgroup (``qtiles * n_kv_heads * batch * nsplit >=
    n_cus``), never leaving the longest sequence fewer than ``MIN_KEYS_PER_CHUNK_SPLIT`` keys per split
    nor exceeding ``MAX_CHUNK_SPLITS``.  ``longest_keys`` is ``max(lens[b] + new_lens[b])``."""
    qtiles = -(-T * rep // QUERY_TILE)
    want = -(-n_cus // (qtiles * n_kv_heads * batch))
    return max(1, min(want, longest_keys // MIN_KEYS_PER_CHUNK_SPLIT, MAX_CHUNK_SPLITS))


def _check_chunk(x: torch.Tensor, cache: KVCache, cols: int, layer: int, new_lens, new_dev, what: str):
    if not 0 <= layer < cache.kv.shape[0]:
        raise ValueError(f"{what}: no layer {layer} in the cache")
    if cache.is_fp8:
        raise ValueError(f"{what}: chunk steps need a bf16 cache, this one is float8_e4m3fn")
    if cache.kv.dtype != torch.bfloat16 or not cache.kv.is_contiguous():
        raise ValueError(f"{what}: the cache must be a contiguous bf16 tensor")
    if x.dtype != torch.bfloat16 or not x.is_contiguous() or x.device != cache.kv.device:
        raise ValueError(f"{what}: needs a contiguous bf16 tensor on the cache's device")
    if x.dim() != 3 or x.shape[0] != cache.batch or x.shape[1] < 1 or x.shape[2] != cols:
        raise ValueError(f"{what}: expected shape ({cache.batch}, T >= 1, {cols}), got {tuple(x.shape)}")
    T = x.shape[1]
    rep = cache.n_heads // cache.n_kv_heads
    if rep not in (1, 2, 4, 8):
        raise ValueError(f"{what}: rep {rep} query heads per KV head is not supported (1, 2, 4 or 8)")
    new = [int(n) for n in new_lens]
    if len(new) != cache.batch or min(new) < 0 or max(new) > T:
        raise ValueError(f"{what}: new_lens {new} must hold {cache.batch} values in [0, {T}]")
    if min(cache.lens) < 0 or max(a + n for a, n in zip(cache.lens, new)) > cache.max_len:
        raise ValueError(f"{what}: lengths {cache.lens} + new_lens {new} exceed the cache's max_len "
                         f"{cache.max_len}")
    if new_dev is None:
        new_dev = torch.tensor(new, dtype=torch.int32, device=x.device)
    elif (new_dev.dtype != torch.int32 or new_dev.device != x.device or tuple(new_dev.shape) != (cache.batch,)
          or not new_dev.is_contiguous()):
        raise ValueError(f"{what}: new_dev must be a contiguous int32 tensor [{cache.batch}] on the cache's device")
    return T, new, new_dev


def rope_append_chunk_reference(qkv: torch.Tensor, cache: KVCache, layer: int, new_lens) -> torch.Tensor:
    """fp32 math of ``rope_append_reference`` for the live rows ``(b, t < new_lens[b])`` at position
    ``lens[b] + t``; zeros in q for the others."""
    B, T, Hq, Hkv = cache.batch, qkv.shape[1], cache.n_heads, cache.n_kv_heads
    cos, sin = rope_tables(cache.max_len, HEAD_DIM, cache.cfg.rope_theta, qkv.device)
    q = torch.zeros((B, T, Hq * HEAD_DIM), device=qkv.device, dtype=qkv.dtype)
    for b, n in enumerate(new_lens):
        if n == 0:
            continue
        pos = cache.lens[b] + torch.arange(n, device=qkv.device)
        c, s = cos[pos][:, None, :], sin[pos][:, None, :]
        x = qkv[b, :n, : (Hq + Hkv) * HEAD_DIM].view(n, Hq + Hkv, HEAD_DIM).float()
        x1, x2 = x[..., :64], x[..., 64:]
        y = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).to(qkv.dtype)
        cache.k(layer)[b, :, pos] = y[:, Hq:].transpose(0, 1)
        cache.v(layer)[b, :, pos] = qkv[b, :n, (Hq + Hkv) * HEAD_DIM:].view(n, Hkv, HEAD_DIM).transpose(0, 1)
        q[b, :n] = y[:, :Hq].reshape(n, Hq * HEAD_DIM)
    return q


def rope_append_chunk(qkv: torch.Tensor, cache: KVCache, layer: int, new_lens,
                      new_dev: torch.Tensor | None = None) -> torch.Tensor:
    """Rotate q / k of the live rows of ``qkv [B, T, (Hq+2*Hkv)*128]`` at ``lens[b] + t``, store their k / v
    in cache rows ``lens[b] .. lens[b] + new_lens[b] - 1`` of ``layer`` and return the rotated q
    ``[B, T, Hq*128]`` (zeros in the rows ``t >= new_lens[b]``, which leave the cache alone)."""
    Hq, Hkv = cache.n_heads, cache.n_kv_heads
    T, new, new_dev = _check_chunk(qkv, cache, (Hq + 2 * Hkv) * HEAD_DIM, layer, new_lens, new_dev,
                                   "rope_append_chunk")
    if not qkv.is_cuda:
        return rope_append_chunk_reference(qkv, cache, layer, new)
    cos, sin = rope_tables(cache.max_len, HEAD_DIM, cache.cfg.rope_theta, qkv.device)
    q = torch.empty((cache.batch, T, Hq * HEAD_DIM), device=qkv.device, dtype=qkv.dtype)
    kc, vc = cache.k(layer), cache.v(layer)
    _lib.call("th_chunk_rope_append", qkv.data_ptr(), cache.lens_dev.data_ptr(), new_dev.data_ptr(),
              cos.data_ptr(), sin.data_ptr(), q.data_ptr(), kc.data_ptr(), vc.data_ptr(), cache.batch, T, Hq, Hkv,
              HEAD_DIM, cache.max_len, kc.stride(0), kc.stride(1), _lib.stream_ptr(qkv.device))
    return q


def chunk_attention_reference(q: torch.Tensor, cache: KVCache, layer: int, new_lens) -> torch.Tensor:
    """fp32 softmax(q k^T / sqrt(128)) v of every live query row ``(b, t)`` over its first
    ``lens[b] + t + 1`` cache rows; zeros for the others."""
    B, T, Hq, Hkv = cache.batch, q.shape[1], cache.n_heads, cache.n_kv_heads
    rep = Hq // Hkv
    out = torch.zeros((B, T, Hq, HEAD_DIM), device=q.device, dtype=torch.float32)
    qf = q.view(B, T, Hkv, rep, HEAD_DIM).float()
    for b, n in enumerate(new_lens):
        if n == 0:
            continue
        rows = cache.lens[b] + n
        k = cache.k(layer)[b, :, :rows].float()  # dead rows are never touched: they may hold NaN
        v = cache.v(layer)[b, :, :rows].float()
        s = torch.einsum("tgrd,gkd->gtrk", qf[b, :n], k) / math.sqrt(HEAD_DIM)
        seen = torch.arange(rows, device=q.device)[None, :] <= cache.lens[b] + torch.arange(n, device=q.device)[:, None]
        s = s.masked_fill(~seen[None, :, None, :], float("-inf"))
        out[b, :n] = torch.einsum("gtrk,gkd->tgrd", s.softmax(-1), v).reshape(n, Hq, HEAD_DIM)
    return out.reshape(B, T, Hq * HEAD_DIM).to(q.dtype)


def chunk_attention(q: torch.Tensor, cache: KVCache, layer: int, new_lens,
                    new_dev: torch.Tensor | None = None, nsplit: int | None = None) -> torch.Tensor:
    """``q [B, T, Hq*128]`` (the output of ``rope_append_chunk``) against ``layer`` -> ``o`` of the same
    shape; module docstring.  ``nsplit`` overrides ``pick_chunk_nsplit`` (1: the unsplit kernel); CPU
    tensors ignore it."""
    Hq, Hkv = cache.n_heads, cache.n_kv_heads
    T, new, new_dev = _check_chunk(q, cache, Hq * HEAD_DIM, layer, new_lens, new_dev, "chunk_attention")
    if nsplit is not None and not 1 <= int(nsplit) <= MAX_CHUNK_SPLITS:
        raise ValueError(f"chunk_attention: nsplit must be in [1, {MAX_CHUNK_SPLITS}], got {nsplit}")
    if not q.is_cuda:
        return chunk_attention_reference(q, cache, layer, new)
    rep = Hq // Hkv
    if nsplit is None:
        cus = torch.cuda.get_device_properties(q.device).multi_processor_count
        nsplit = pick_chunk_nsplit(cache.batch, Hkv, rep, T, max(a + n for a, n in zip(cache.lens, new)), cus)
    nsplit = int(nsplit)
    o = torch.empty_like(q)
    kc, vc = cache.k(layer), cache.v(layer)
    if nsplit > 1:
        qtiles = -(-T * rep // QUERY_TILE)
        ws = cache.workspace(cache.batch * Hkv * qtiles * nsplit * QUERY_TILE * WS_FLOATS_PER_ROW)
        _lib.call("th_chunk_attn_split", q.data_ptr(), kc.data_ptr(), vc.data_ptr(), cache.lens_dev.data_ptr(),
                  new_dev.data_ptr(), o.data_ptr(), ws.data_ptr(), cache.batch, T, Hq, Hkv, HEAD_DIM, cache.max_len,
                  kc.stride(0), kc.stride(1), nsplit, 1.0 / math.sqrt(HEAD_DIM), _lib.stream_ptr(q.device))
        return o
    _lib.call("th_chunk_attn", q.data_ptr(), kc.data_ptr(), vc.data_ptr(), cache.lens_dev.data_ptr(),
              new_dev.data_ptr(), o.data_ptr(), cache.batch, T, Hq, Hkv, HEAD_DIM, cache.max_len, kc.stride(0),
              kc.stride(1), 1.0 / math.sqrt(HEAD_DIM), _lib.stream_ptr(q.device))
    return o
