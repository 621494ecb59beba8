"""KV cache, RoPE + cache append, and single-token GQA attention over the cache (generation).

Cache layout: one bf16 tensor per model, ``[n_layers, 2, B, Hkv, Smax, 128]`` (K = index 0, V = 1):
every ``(b, kv_head)`` is a contiguous run of 256-byte rows, which is what ``csrc/decode_attn.hip``
streams.  ``KVCache.lens`` (host list) and ``KVCache.lens_dev`` (int32 on the device) hold the
number of valid rows per sequence and are advanced together; rows at or past ``lens[b]`` are dead
and may hold anything.

``rope_append(qkv, cache, layer)`` rotates the new token's q and k at position ``lens[b]``, writes
k and v into cache row ``lens[b]`` and returns the rotated q ``[B, Hq*128]``.  It does not advance
the lengths: every layer appends at the same row, then the model calls ``cache.advance()``.
``decode_attention(q, cache, layer, nsplit=None, new=0)`` attends over the first ``lens[b] + new``
rows (``new=1`` right after ``rope_append``).  Its split geometry comes from the host lengths; with
``device_geometry=True`` the kernel derives it from ``lens_dev`` under a grid sized for ``max_len``
(``device_split_geometry`` is that rule), so the launch can be captured into a graph and replayed
while the lengths grow, with the same bits as the host rule gives.

GPU tensors run the gfx950 kernels (a missing entry point raises, there is no SDPA fallback);
CPU tensors run the fp32 reference below, which is also the tests' oracle.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .rope import rope_tables

HEAD_DIM = 128
# fewest keys a split is worth: below this the partial write + combine outweigh the extra workgroups
MIN_KEYS_PER_SPLIT = 256
MAX_SPLITS = 64


class KVCache:
    """The K/V rows of every layer for ``batch`` sequences of at most ``max_len`` tokens."""

    def __init__(self, cfg, batch: int, max_len: int, device="cpu"):
        if cfg.head_dim != HEAD_DIM:
            raise ValueError(f"KVCache: head_dim {cfg.head_dim} is not supported (128 only)")
        if cfg.n_heads % cfg.n_kv_heads:
            raise ValueError("KVCache: n_heads is not a multiple of n_kv_heads")
        if batch <= 0 or max_len <= 0:
            raise ValueError("KVCache: batch and max_len must be positive")
        if max_len > cfg.max_seq_len:
            raise ValueError(f"KVCache: max_len {max_len} exceeds the model's max_seq_len {cfg.max_seq_len}")
        self.cfg = cfg
        self.batch, self.max_len = batch, max_len
        self.n_heads, self.n_kv_heads = cfg.n_heads, cfg.n_kv_heads
        self.device = torch.device(device)
        self.kv = torch.zeros((cfg.n_layers, 2, batch, cfg.n_kv_heads, max_len, HEAD_DIM),
                              device=self.device, dtype=torch.bfloat16)
        self.lens: list[int] = [0] * batch
        self.lens_dev = torch.zeros(batch, device=self.device, dtype=torch.int32)
        self._ws: torch.Tensor | None = None  # split partials, shared by the layers (stream-ordered)

    def k(self, layer: int) -> torch.Tensor:
        return self.kv[layer, 0]

    def v(self, layer: int) -> torch.Tensor:
        return self.kv[layer, 1]

    def set_lens(self, lens) -> None:
        lens = [int(n) for n in lens]
        if len(lens) != self.batch or min(lens) < 0 or max(lens) > self.max_len:
            raise ValueError(f"KVCache: lengths {lens} do not fit batch {self.batch} x max_len {self.max_len}")
        self.lens = lens
        self.lens_dev.copy_(torch.tensor(lens, dtype=torch.int32))

    def advance(self, n: int = 1) -> None:
        if max(self.lens) + n > self.max_len:
            raise ValueError(f"KVCache: {max(self.lens)} + {n} rows exceed max_len {self.max_len}")
        self.lens = [x + n for x in self.lens]
        self.lens_dev += n

    def advance_host(self, n: int = 1) -> None:
        """Advance the host list only: for a captured step, whose replay advanced ``lens_dev`` itself."""
        if max(self.lens) + n > self.max_len:
            raise ValueError(f"KVCache: {max(self.lens)} + {n} rows exceed max_len {self.max_len}")
        self.lens = [x + n for x in self.lens]

    def workspace(self, floats: int) -> torch.Tensor:
        """At least ``floats`` f32 of scratch.  A larger request replaces the buffer and never touches
        the old one: whoever captured its address into a graph keeps a reference to it."""
        if self._ws is None or self._ws.numel() < floats:
            self._ws = torch.empty(floats, device=self.device, dtype=torch.float32)
        return self._ws


def _check(x: torch.Tensor, cache: KVCache, cols: int, layer: int, new: int, what: str) -> None:
    # head geometry and max_len were checked when the cache was built
    if not 0 <= layer < cache.kv.shape[0]:
        raise ValueError(f"{what}: no layer {layer} in the cache")
    if x.dtype != torch.bfloat16 or not x.is_contiguous() or x.device != cache.kv.device:
        raise ValueError(f"{what}: needs a contiguous bf16 tensor on the cache's device")
    if x.dim() != 2 or tuple(x.shape) != (cache.batch, cols):
        raise ValueError(f"{what}: expected shape {(cache.batch, cols)}, got {tuple(x.shape)}")
    if cache.kv.dtype != torch.bfloat16 or not cache.kv.is_contiguous():
        raise ValueError(f"{what}: the cache must be a contiguous bf16 tensor")
    if new < 0 or min(cache.lens) < 0 or max(cache.lens) + new > cache.max_len:
        raise ValueError(f"{what}: {max(cache.lens)} + {new} rows exceed the cache's max_len {cache.max_len}")


def rope_append_reference(qkv: torch.Tensor, cache: KVCache, layer: int) -> torch.Tensor:
    """fp32 math of ``rope_reference_`` at position ``lens[b]`` of every sequence."""
    B, Hq, Hkv = cache.batch, cache.n_heads, cache.n_kv_heads
    cos, sin = rope_tables(cache.max_len, HEAD_DIM, cache.cfg.rope_theta, qkv.device)
    pos = torch.tensor(cache.lens, device=qkv.device, dtype=torch.long)
    c, s = cos[pos][:, None, :], sin[pos][:, None, :]
    x = qkv[:, : (Hq + Hkv) * HEAD_DIM].view(B, Hq + Hkv, HEAD_DIM).float()
    x1, x2 = x[..., :64], x[..., 64:]
    y = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).to(qkv.dtype)
    v = qkv[:, (Hq + Hkv) * HEAD_DIM:].view(B, Hkv, HEAD_DIM)
    bi = torch.arange(B, device=qkv.device)
    cache.k(layer)[bi, :, pos] = y[:, Hq:]
    cache.v(layer)[bi, :, pos] = v
    return y[:, :Hq].reshape(B, Hq * HEAD_DIM).contiguous()


def rope_append(qkv: torch.Tensor, cache: KVCache, layer: int) -> torch.Tensor:
    """Rotate q / k of the new token rows ``qkv [B, (Hq+2*Hkv)*128]`` at ``lens[b]``, store k / v in
    cache row ``lens[b]`` of ``layer`` and return the rotated q ``[B, Hq*128]``."""
    Hq, Hkv = cache.n_heads, cache.n_kv_heads
    _check(qkv, cache, (Hq + 2 * Hkv) * HEAD_DIM, layer, 1, "rope_append")
    if not qkv.is_cuda:
        return rope_append_reference(qkv, cache, layer)
    cos, sin = rope_tables(cache.max_len, HEAD_DIM, cache.cfg.rope_theta, qkv.device)
    q = torch.empty((cache.batch, Hq * HEAD_DIM), device=qkv.device, dtype=qkv.dtype)
    kc, vc = cache.k(layer), cache.v(layer)
    _lib.call("th_decode_rope_append", qkv.data_ptr(), cache.lens_dev.data_ptr(), cos.data_ptr(),
              sin.data_ptr(), q.data_ptr(), kc.data_ptr(), vc.data_ptr(), cache.batch, Hq, Hkv, HEAD_DIM,
              cache.max_len, kc.stride(0), kc.stride(1), _lib.stream_ptr(qkv.device))
    return q


def decode_attention_reference(q: torch.Tensor, cache: KVCache, layer: int, new: int = 0) -> torch.Tensor:
    """fp32 softmax(q k^T / sqrt(128)) v over the first ``lens[b] + new`` cache rows of every sequence."""
    B, Hq, Hkv = cache.batch, cache.n_heads, cache.n_kv_heads
    rep = Hq // Hkv
    out = torch.zeros((B, Hq, HEAD_DIM), device=q.device, dtype=torch.float32)
    qf = q.view(B, Hkv, rep, HEAD_DIM).float()
    for b in range(B):
        n = cache.lens[b] + new
        if n == 0:
            continue
        k = cache.k(layer)[b, :, :n].float()  # dead rows are never touched: they may hold NaN
        v = cache.v(layer)[b, :, :n].float()
        s = qf[b] @ k.transpose(-1, -2) / math.sqrt(HEAD_DIM)
        out[b] = (s.softmax(-1) @ v).reshape(Hq, HEAD_DIM)
    return out.reshape(B, Hq * HEAD_DIM).to(q.dtype)


def pick_nsplit(batch: int, n_kv_heads: int, max_kv_len: int, n_cus: int) -> int:
    """Smallest split count that gives every CU a workgroup (``batch * n_kv_heads * nsplit >= n_cus``),
    never leaving a split fewer than ``MIN_KEYS_PER_SPLIT`` keys."""
    want = -(-n_cus // (batch * n_kv_heads))
    return max(1, min(want, max_kv_len // MIN_KEYS_PER_SPLIT, MAX_SPLITS))


def device_split_geometry(lens, new: int, want: int, max_len: int, min_keys: int = MIN_KEYS_PER_SPLIT,
                          cap: int = MAX_SPLITS) -> tuple[int, int]:
    """``(ns_eff, chunk)`` as the ``device_geometry`` kernel derives them from the device lengths:
    the rule of ``pick_nsplit`` on the longest sequence, then ``decode_attention``'s ``chunk``.  ``want``
    is ``ceil(CUs / (batch * n_kv_heads))``; ``cap`` is the grid's split count, ``pick_nsplit`` at
    ``max_len`` (never above ``MAX_SPLITS``, and never below what the rule picks at a shorter length).
    A forced split count passes ``want = cap = nsplit`` and ``min_keys = 1``."""
    longest = max(min(max(int(n) + new, 0), max_len) for n in lens)
    ns_eff = max(1, min(want, longest // min_keys, cap))
    return ns_eff, max(1, -(-longest // ns_eff))


def decode_attention(q: torch.Tensor, cache: KVCache, layer: int, nsplit: int | None = None,
                     new: int = 0, device_geometry: bool = False) -> torch.Tensor:
    """``q [B, Hq*128]`` against the first ``lens[b] + new`` rows of ``layer`` -> ``o [B, Hq*128]``.
    ``nsplit`` overrides the automatic split count (tests).  ``device_geometry`` takes the split count
    and chunk from ``lens_dev`` inside the kernel (``device_split_geometry``) under a grid of
    ``pick_nsplit`` at ``max_len`` splits, or of ``nsplit`` where given; nothing the launch is given then
    depends on the current lengths, and the output has the bits of the host rule."""
    Hq, Hkv = cache.n_heads, cache.n_kv_heads
    _check(q, cache, Hq * HEAD_DIM, layer, new, "decode_attention")
    if nsplit is not None and not 1 <= int(nsplit) <= 1024:
        raise ValueError("decode_attention: nsplit must be in [1, 1024]")
    if not q.is_cuda:
        return decode_attention_reference(q, cache, layer, new)
    if device_geometry:
        if nsplit is None:
            cus = torch.cuda.get_device_properties(q.device).multi_processor_count
            want = -(-cus // (cache.batch * Hkv))
            cap, min_keys = pick_nsplit(cache.batch, Hkv, cache.max_len, cus), MIN_KEYS_PER_SPLIT
        else:
            want = cap = int(nsplit)
            min_keys = 1
        o = torch.empty_like(q)
        ws = cache.workspace(cache.batch * Hq * cap * (HEAD_DIM + 2))
        kc, vc = cache.k(layer), cache.v(layer)
        _lib.call("th_decode_attn_dev", q.data_ptr(), kc.data_ptr(), vc.data_ptr(), cache.lens_dev.data_ptr(),
                  o.data_ptr(), ws.data_ptr(), cache.batch, Hq, Hkv, HEAD_DIM, cache.max_len, kc.stride(0),
                  kc.stride(1), cap, want, min_keys, int(new), 1.0 / math.sqrt(HEAD_DIM),
                  _lib.stream_ptr(q.device))
        return o
    longest = max(cache.lens) + new
    if nsplit is None:
        cus = torch.cuda.get_device_properties(q.device).multi_processor_count
        nsplit = pick_nsplit(cache.batch, Hkv, longest, cus)
    nsplit = int(nsplit)
    chunk = max(1, -(-longest // nsplit))
    o = torch.empty_like(q)
    ws = cache.workspace(cache.batch * Hq * nsplit * (HEAD_DIM + 2))
    kc, vc = cache.k(layer), cache.v(layer)
    _lib.call("th_decode_attn", q.data_ptr(), kc.data_ptr(), vc.data_ptr(), cache.lens_dev.data_ptr(),
              o.data_ptr(), ws.data_ptr(), cache.batch, Hq, Hkv, HEAD_DIM, cache.max_len, kc.stride(0),
              kc.stride(1), nsplit, chunk, int(new), 1.0 / math.sqrt(HEAD_DIM), _lib.stream_ptr(q.device))
    return o
