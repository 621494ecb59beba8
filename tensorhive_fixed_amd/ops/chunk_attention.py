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
Out of scope here:

* an FP8 cache (a ``ValueError``: chunk steps need a bf16 cache);
* a split over the keys for short chunks on long caches: for ``T <= 8`` ``extend_attention`` remains the
  right call, and nothing dispatches between the two;
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
                    new_dev: torch.Tensor | None = None) -> torch.Tensor:
    """``q [B, T, Hq*128]`` (the output of ``rope_append_chunk``) against ``layer`` -> ``o`` of the same
    shape; module docstring."""
    Hq, Hkv = cache.n_heads, cache.n_kv_heads
    T, new, new_dev = _check_chunk(q, cache, Hq * HEAD_DIM, layer, new_lens, new_dev, "chunk_attention")
    if not q.is_cuda:
        return chunk_attention_reference(q, cache, layer, new)
    o = torch.empty_like(q)
    kc, vc = cache.k(layer), cache.v(layer)
    _lib.call("th_chunk_attn", q.data_ptr(), kc.data_ptr(), vc.data_ptr(), cache.lens_dev.data_ptr(),
              new_dev.data_ptr(), o.data_ptr(), cache.batch, T, Hq, Hkv, HEAD_DIM, cache.max_len, kc.stride(0),
              kc.stride(1), 1.0 / math.sqrt(HEAD_DIM), _lib.stream_ptr(q.device))
    return o
