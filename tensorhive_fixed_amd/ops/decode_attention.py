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

FP8 cache (opt-in): ``KVCache(..., dtype=torch.float8_e4m3fn)`` keeps ``kv`` as OCP e4m3fn codes in
the same layout (128-byte rows) and one f32 scale per (token, KV head) row in ``kv_scale
[n_layers, 2, B, Hkv, Smax]``: row = codes * scale.  ``quantize_kv_rows`` is the rule, that of
``decode_linear_fp8.quantize_weight_fp8``: ``scale = absmax(row) / 448`` (1.0 for a row of zeros),
``codes = clamp(row / scale, +-448)`` cast to e4m3fn; it never produces a NaN code.  ``rope_append``
and ``decode_attention`` dispatch on ``cache.kv.dtype``; on an FP8 cache the append rounds the rotated
k row to bf16 and quantizes it (v as it comes), and the attention is over ``codes * scale``
(``csrc/decode_attn_fp8.hip``).  67,584 bytes per token against 131,072 for Llama-3-8B.

GPU tensors run the gfx950 kernels (a missing entry point raises, there is no SDPA fallback);
CPU tensors run the fp32 reference below, which is also the tests' oracle.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .rope import rope_tables

HEAD_DIM = 128
FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0
FP8_MAX_LEN = 1 << 24  # the FP8 attention kernel's byte offsets inside a (b, head) run are 32-bit
# fewest keys a split is worth: below this the partial write + combine outweigh the extra workgroups
MIN_KEYS_PER_SPLIT = 256
MAX_SPLITS = 64


def quantize_kv_rows(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """bf16 ``x [..., 128]`` -> (``codes`` e4m3fn of the same shape, ``scale`` f32 ``[...]``); module
    docstring.  Runs on ``x``'s device; the bytes are those of the CPU run."""
    if x.dtype != torch.bfloat16 or x.dim() < 1 or x.shape[-1] != HEAD_DIM:
        raise ValueError(f"quantize_kv_rows: needs bf16 rows of {HEAD_DIM}, got {x.dtype} {tuple(x.shape)}")
    xf = x.float()
    amax = xf.abs().amax(dim=-1)
    # a tensor divisor: by a Python scalar the GPU multiplies by the rounded reciprocal, which is not the
    # correctly rounded quotient the CPU gives
    scale = amax / torch.full_like(amax, FP8_MAX)
    scale = torch.where(scale > 0, scale, torch.ones_like(scale))
    codes = (xf / scale[..., None]).clamp(-FP8_MAX, FP8_MAX).to(FP8)
    return codes, scale


def kv_cache_bytes(cfg, batch: int, max_len: int, dtype=torch.bfloat16) -> int:
    """Bytes of ``KVCache(cfg, batch, max_len, dtype=dtype)``: rows, plus the scales of an FP8 cache."""
    per_row = HEAD_DIM + 4 if dtype == FP8 else 2 * HEAD_DIM
    return cfg.n_layers * 2 * batch * cfg.n_kv_heads * max_len * per_row


class KVCache:
    """The K/V rows of every layer for ``batch`` sequences of at most ``max_len`` tokens."""

    def __init__(self, cfg, batch: int, max_len: int, device="cpu", dtype=torch.bfloat16):
        if cfg.head_dim != HEAD_DIM:
            raise ValueError(f"KVCache: head_dim {cfg.head_dim} is not supported (128 only)")
        if cfg.n_heads % cfg.n_kv_heads:
            raise ValueError("KVCache: n_heads is not a multiple of n_kv_heads")
        if batch <= 0 or max_len <= 0:
            raise ValueError("KVCache: batch and max_len must be positive")
        if max_len > cfg.max_seq_len:
            raise ValueError(f"KVCache: max_len {max_len} exceeds the model's max_seq_len {cfg.max_seq_len}")
        if dtype not in (torch.bfloat16, FP8):
            raise ValueError(f"KVCache: dtype must be bfloat16 or float8_e4m3fn, got {dtype}")
        if dtype == FP8 and max_len > FP8_MAX_LEN:
            raise ValueError(f"KVCache: an FP8 cache holds at most {FP8_MAX_LEN} rows per sequence, got {max_len}")
        self.cfg = cfg
        self.batch, self.max_len = batch, max_len
        self.n_heads, self.n_kv_heads = cfg.n_heads, cfg.n_kv_heads
        self.device = torch.device(device)
        self.kv = torch.zeros((cfg.n_layers, 2, batch, cfg.n_kv_heads, max_len, HEAD_DIM),
                              device=self.device, dtype=dtype)
        # one f32 scale per row of an FP8 cache (1.0: the scale of a row of zeros)
        self.kv_scale = (torch.ones(self.kv.shape[:-1], device=self.device, dtype=torch.float32)
                         if dtype == FP8 else None)
        self.lens: list[int] = [0] * batch
        self.lens_dev = torch.zeros(batch, device=self.device, dtype=torch.int32)
        self._ws: torch.Tensor | None = None  # split partials, shared by the layers (stream-ordered)

    def k(self, layer: int) -> torch.Tensor:
        return self.kv[layer, 0]

    def v(self, layer: int) -> torch.Tensor:
        return self.kv[layer, 1]

    @property
    def is_fp8(self) -> bool:
        return self.kv.dtype == FP8

    def k_scale(self, layer: int) -> torch.Tensor:
        return self.kv_scale[layer, 0]

    def v_scale(self, layer: int) -> torch.Tensor:
        return self.kv_scale[layer, 1]

    def fill(self, layer: int, k: torch.Tensor, v: torch.Tensor) -> None:
        """Store bf16 ``k`` / ``v [B, Hkv, S, 128]`` (any strides) at rows ``0..S-1`` of ``layer``; an FP8
        cache quantizes the rows first (``quantize_kv_rows``).  Does not touch the lengths."""
        S = k.shape[2]
        want = (self.batch, self.n_kv_heads, S, HEAD_DIM)
        if tuple(k.shape) != want or tuple(v.shape) != want or S > self.max_len:
            raise ValueError(f"KVCache.fill: expected k and v of shape [{self.batch}, {self.n_kv_heads}, "
                             f"S <= {self.max_len}, {HEAD_DIM}], got {tuple(k.shape)} and {tuple(v.shape)}")
        if k.dtype != torch.bfloat16 or v.dtype != torch.bfloat16:
            raise ValueError(f"KVCache.fill: needs bf16 rows, got {k.dtype} and {v.dtype}")
        if not self.is_fp8:
            self.k(layer)[:, :, :S].copy_(k)
            self.v(layer)[:, :, :S].copy_(v)
            return
        for j, x in enumerate((k, v)):
            codes, scale = quantize_kv_rows(x)
            self.kv[layer, j].view(torch.uint8)[:, :, :S].copy_(codes.view(torch.uint8))
            self.kv_scale[layer, j, :, :, :S].copy_(scale)

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
    if cache.kv.dtype not in (torch.bfloat16, FP8) or not cache.kv.is_contiguous():
        raise ValueError(f"{what}: the cache must be a contiguous bf16 or float8_e4m3fn tensor")
    if cache.is_fp8:
        sc = cache.kv_scale
        if (sc is None or sc.dtype != torch.float32 or not sc.is_contiguous() or sc.device != cache.kv.device
                or tuple(sc.shape) != tuple(cache.kv.shape[:-1])):
            raise ValueError(f"{what}: an FP8 cache needs contiguous f32 kv_scale of shape "
                             f"{tuple(cache.kv.shape[:-1])}")
    if new < 0 or min(cache.lens) < 0 or max(cache.lens) + new > cache.max_len:
        raise ValueError(f"{what}: {max(cache.lens)} + {new} rows exceed the cache's max_len {cache.max_len}")


def rope_append_reference(qkv: torch.Tensor, cache: KVCache, layer: int) -> torch.Tensor:
    """fp32 math of ``rope_reference_`` at position ``lens[b]`` of every sequence; on an FP8 cache the
    rows are then quantized with ``quantize_kv_rows``."""
    B, Hq, Hkv = cache.batch, cache.n_heads, cache.n_kv_heads
    cos, sin = rope_tables(cache.max_len, HEAD_DIM, cache.cfg.rope_theta, qkv.device)
    pos = torch.tensor(cache.lens, device=qkv.device, dtype=torch.long)
    c, s = cos[pos][:, None, :], sin[pos][:, None, :]
    x = qkv[:, : (Hq + Hkv) * HEAD_DIM].view(B, Hq + Hkv, HEAD_DIM).float()
    x1, x2 = x[..., :64], x[..., 64:]
    y = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).to(qkv.dtype)
    v = qkv[:, (Hq + Hkv) * HEAD_DIM:].view(B, Hkv, HEAD_DIM)
    bi = torch.arange(B, device=qkv.device)
    if cache.is_fp8:  # the rotated k is rounded to bf16 (above) and then quantized, v as it comes
        for j, rows in enumerate((y[:, Hq:], v)):
            codes, scale = quantize_kv_rows(rows)
            cache.kv[layer, j].view(torch.uint8)[bi, :, pos] = codes.view(torch.uint8)
            cache.kv_scale[layer, j][bi, :, pos] = scale
    else:
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
    if cache.is_fp8:
        ksc, vsc = cache.k_scale(layer), cache.v_scale(layer)
        _lib.call("th_decode_rope_append_fp8", qkv.data_ptr(), cache.lens_dev.data_ptr(), cos.data_ptr(),
                  sin.data_ptr(), q.data_ptr(), kc.data_ptr(), vc.data_ptr(), ksc.data_ptr(), vsc.data_ptr(),
                  cache.batch, Hq, Hkv, HEAD_DIM, cache.max_len, kc.stride(0), kc.stride(1), ksc.stride(0),
                  ksc.stride(1), _lib.stream_ptr(qkv.device))
        return q
    _lib.call("th_decode_rope_append", qkv.data_ptr(), cache.lens_dev.data_ptr(), cos.data_ptr(),
              sin.data_ptr(), q.data_ptr(), kc.data_ptr(), vc.data_ptr(), cache.batch, Hq, Hkv, HEAD_DIM,
              cache.max_len, kc.stride(0), kc.stride(1), _lib.stream_ptr(qkv.device))
    return q


def decode_attention_reference(q: torch.Tensor, cache: KVCache, layer: int, new: int = 0) -> torch.Tensor:
    """fp32 softmax(q k^T / sqrt(128)) v over the first ``lens[b] + new`` cache rows of every sequence
    (``codes.float() * scale`` on an FP8 cache)."""
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
        if cache.is_fp8:
            k = k * cache.k_scale(layer)[b, :, :n, None]
            v = v * cache.v_scale(layer)[b, :, :n, None]
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
        if cache.is_fp8:
            ksc, vsc = cache.k_scale(layer), cache.v_scale(layer)
            _lib.call("th_decode_attn_fp8_dev", q.data_ptr(), kc.data_ptr(), vc.data_ptr(), ksc.data_ptr(),
                      vsc.data_ptr(), cache.lens_dev.data_ptr(), o.data_ptr(), ws.data_ptr(), cache.batch, Hq, Hkv,
                      HEAD_DIM, cache.max_len, kc.stride(0), kc.stride(1), ksc.stride(0), ksc.stride(1), cap, want,
                      min_keys, int(new), 1.0 / math.sqrt(HEAD_DIM), _lib.stream_ptr(q.device))
            return o
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
    if cache.is_fp8:
        ksc, vsc = cache.k_scale(layer), cache.v_scale(layer)
        _lib.call("th_decode_attn_fp8", q.data_ptr(), kc.data_ptr(), vc.data_ptr(), ksc.data_ptr(), vsc.data_ptr(),
                  cache.lens_dev.data_ptr(), o.data_ptr(), ws.data_ptr(), cache.batch, Hq, Hkv, HEAD_DIM,
                  cache.max_len, kc.stride(0), kc.stride(1), ksc.stride(0), ksc.stride(1), nsplit, chunk, int(new),
                  1.0 / math.sqrt(HEAD_DIM), _lib.stream_ptr(q.device))
        return o
    _lib.call("th_decode_attn", q.data_ptr(), kc.data_ptr(), vc.data_ptr(), cache.lens_dev.data_ptr(),
              o.data_ptr(), ws.data_ptr(), cache.batch, Hq, Hkv, HEAD_DIM, cache.max_len, kc.stride(0),
              kc.stride(1), nsplit, chunk, int(new), 1.0 / math.sqrt(HEAD_DIM), _lib.stream_ptr(q.device))
    return o
