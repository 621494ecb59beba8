"""Multi-token ("block") decode steps on a bf16 KV cache: T = 1..8 new tokens per sequence at once.

``rope_append_block(qkv [B, T, (Hq+2*Hkv)*128], cache, layer)`` rotates row ``(b, t)`` at position
``lens[b] + t``, stores its k / v in cache row ``lens[b] + t`` and returns the rotated q
``[B, T, Hq*128]``; the bits are those of T single ``rope_append`` calls.  It does not advance the
lengths.  ``extend_attention(q [B, T, Hq*128], cache, layer, nsplit=None)`` is called after it, before
the lengths move: query row ``(b, t, h)`` attends over cache rows ``[0, lens[b] + t + 1)`` of its KV
head, which is causal inside the new block and full over the old rows.  The model then calls
``cache.advance(T)`` (or ``set_lens`` with fewer rows: the rows past a length are dead).

The kernels are in ``csrc/extend_attn.hip``: the split rule is ``decode_attention``'s (``pick_nsplit`` on
``max(lens) + T``), one workgroup serves all ``rep * T`` query rows of a KV head, so K and V are read
once per call whatever T is, and both products run on MFMAs.  ``supported_block(rep, T)`` is the shape
rule.  Out of scope here: an FP8 cache (a ``ValueError``; block steps need a bf16 cache) and a
device-geometry form that a graph could capture (the split geometry comes from the host lengths).

GPU tensors run the gfx950 kernels (a missing entry point raises); CPU tensors run the fp32
references below, which are also the tests' oracle.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .decode_attention import HEAD_DIM, KVCache, pick_nsplit
from .rope import rope_tables

MAX_BLOCK = 8


def supported_block(rep: int, T: int) -> bool:
    """Whether the block kernels take ``T`` new tokens at ``rep = Hq / Hkv`` query heads per KV head:
    rep 1, 2, 4 or 8 and ``1 <= T <= 8`` (at most 64 query rows per workgroup)."""
    return rep in (1, 2, 4, 8) and 1 <= T <= MAX_BLOCK


def _check_block(x: torch.Tensor, cache: KVCache, cols: int, layer: int, what: str) -> int:
    if not 0 <= layer < cache.kv.shape[0]:
        raise ValueError(f"{what}: no layer {layer} in the cache")
    if cache.is_fp8:
        raise ValueError(f"{what}: block steps need a bf16 cache, this one is float8_e4m3fn")
    if cache.kv.dtype != torch.bfloat16 or not cache.kv.is_contiguous():
        raise ValueError(f"{what}: the cache must be a contiguous bf16 tensor")
    if x.dtype != torch.bfloat16 or not x.is_contiguous() or x.device != cache.kv.device:
        raise ValueError(f"{what}: needs a contiguous bf16 tensor on the cache's device")
    if x.dim() != 3 or x.shape[0] != cache.batch or x.shape[2] != cols:
        raise ValueError(f"{what}: expected shape ({cache.batch}, T, {cols}), got {tuple(x.shape)}")
    T = x.shape[1]
    if not 1 <= T <= MAX_BLOCK:
        raise ValueError(f"{what}: a block holds 1 <= T <= {MAX_BLOCK} tokens, got T = {T}")
    if not supported_block(cache.n_heads // cache.n_kv_heads, T):
        raise ValueError(f"{what}: rep {cache.n_heads // cache.n_kv_heads} x T {T} is outside supported_block "
                         "(rep 1, 2, 4 or 8)")
    if min(cache.lens) < 0 or max(cache.lens) + T > cache.max_len:
        raise ValueError(f"{what}: {max(cache.lens)} + {T} rows exceed the cache's max_len {cache.max_len}")
    return T


def rope_append_block_reference(qkv: torch.Tensor, cache: KVCache, layer: int) -> torch.Tensor:
    """fp32 math of ``rope_append_reference`` for row ``(b, t)`` at position ``lens[b] + t``."""
    B, T, Hq, Hkv = cache.batch, qkv.shape[1], cache.n_heads, cache.n_kv_heads
    cos, sin = rope_tables(cache.max_len, HEAD_DIM, cache.cfg.rope_theta, qkv.device)
    pos = (torch.tensor(cache.lens, device=qkv.device, dtype=torch.long)[:, None]
           + torch.arange(T, device=qkv.device)[None, :])  # [B, T]
    c, s = cos[pos][:, :, None, :], sin[pos][:, :, None, :]
    x = qkv[..., : (Hq + Hkv) * HEAD_DIM].view(B, T, Hq + Hkv, HEAD_DIM).float()
    x1, x2 = x[..., :64], x[..., 64:]
    y = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).to(qkv.dtype)
    v = qkv[..., (Hq + Hkv) * HEAD_DIM:].view(B, T, Hkv, HEAD_DIM)
    bi = torch.arange(B, device=qkv.device)[:, None].expand(B, T)
    cache.k(layer)[bi, :, pos] = y[:, :, Hq:]
    cache.v(layer)[bi, :, pos] = v
    return y[:, :, :Hq].reshape(B, T, Hq * HEAD_DIM).contiguous()


def rope_append_block(qkv: torch.Tensor, cache: KVCache, layer: int) -> torch.Tensor:
    """Rotate q / k of the block ``qkv [B, T, (Hq+2*Hkv)*128]`` at ``lens[b] + t``, store k / v in cache
    rows ``lens[b] .. lens[b] + T - 1`` of ``layer`` and return the rotated q ``[B, T, Hq*128]``."""
    Hq, Hkv = cache.n_heads, cache.n_kv_heads
    T = _check_block(qkv, cache, (Hq + 2 * Hkv) * HEAD_DIM, layer, "rope_append_block")
    if not qkv.is_cuda:
        return rope_append_block_reference(qkv, cache, layer)
    cos, sin = rope_tables(cache.max_len, HEAD_DIM, cache.cfg.rope_theta, qkv.device)
    q = torch.empty((cache.batch, T, Hq * HEAD_DIM), device=qkv.device, dtype=qkv.dtype)
    kc, vc = cache.k(layer), cache.v(layer)
    _lib.call("th_decode_rope_append_block", qkv.data_ptr(), cache.lens_dev.data_ptr(), cos.data_ptr(),
              sin.data_ptr(), q.data_ptr(), kc.data_ptr(), vc.data_ptr(), cache.batch, T, Hq, Hkv, HEAD_DIM,
              cache.max_len, kc.stride(0), kc.stride(1), _lib.stream_ptr(qkv.device))
    return q


def extend_attention_reference(q: torch.Tensor, cache: KVCache, layer: int) -> torch.Tensor:
    """fp32 softmax(q k^T / sqrt(128)) v of query row ``(b, t)`` over its first ``lens[b] + t + 1``
    cache rows."""
    B, T, Hq, Hkv = cache.batch, q.shape[1], cache.n_heads, cache.n_kv_heads
    rep = Hq // Hkv
    out = torch.zeros((B, T, Hq, HEAD_DIM), device=q.device, dtype=torch.float32)
    qf = q.view(B, T, Hkv, rep, HEAD_DIM).float()
    for b in range(B):
        for t in range(T):
            n = cache.lens[b] + t + 1
            k = cache.k(layer)[b, :, :n].float()  # dead rows are never touched: they may hold NaN
            v = cache.v(layer)[b, :, :n].float()
            s = qf[b, t] @ k.transpose(-1, -2) / math.sqrt(HEAD_DIM)
            out[b, t] = (s.softmax(-1) @ v).reshape(Hq, HEAD_DIM)
    return out.reshape(B, T, Hq * HEAD_DIM).to(q.dtype)


def extend_attention(q: torch.Tensor, cache: KVCache, layer: int, nsplit: int | None = None) -> torch.Tensor:
    """``q [B, T, Hq*128]`` (the output of ``rope_append_block``) against ``layer`` -> ``o`` of the same
    shape; module docstring.  ``nsplit`` overrides the automatic split count (tests)."""
    Hq, Hkv = cache.n_heads, cache.n_kv_heads
    T = _check_block(q, cache, Hq * HEAD_DIM, layer, "extend_attention")
    if nsplit is not None and not 1 <= int(nsplit) <= 1024:
        raise ValueError("extend_attention: nsplit must be in [1, 1024]")
    if not q.is_cuda:
        return extend_attention_reference(q, cache, layer)
    longest = max(cache.lens) + T
    if nsplit is None:
        cus = torch.cuda.get_device_properties(q.device).multi_processor_count
        nsplit = pick_nsplit(cache.batch, Hkv, longest, cus)
    nsplit = int(nsplit)
    chunk = max(1, -(-longest // nsplit))
    o = torch.empty_like(q)
    ws = cache.workspace(cache.batch * T * Hq * nsplit * (HEAD_DIM + 2))
    kc, vc = cache.k(layer), cache.v(layer)
    _lib.call("th_extend_attn", q.data_ptr(), kc.data_ptr(), vc.data_ptr(), cache.lens_dev.data_ptr(),
              o.data_ptr(), ws.data_ptr(), cache.batch, T, Hq, Hkv, HEAD_DIM, cache.max_len, kc.stride(0),
              kc.stride(1), nsplit, chunk, 1.0 / math.sqrt(HEAD_DIM), _lib.stream_ptr(q.device))
    return o
