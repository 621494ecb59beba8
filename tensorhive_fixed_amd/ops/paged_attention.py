"""Paged KV cache: RoPE + append and single-token GQA attention through a per-sequence page table.

Pool layout: one bf16 tensor per model, ``pool [n_layers, 2, n_pages, Hkv, PAGE, 128]`` (K = index 0,
V = 1) with ``PAGE = 64`` rows: every ``(page, kv_head)`` is one contiguous 16 KB run of 256-byte rows,
which is what ``csrc/paged_attn.hip`` streams.  Logical row ``r`` of sequence ``b`` is row ``r % PAGE``
of page ``table[b][r // PAGE]``.  ``table`` (host, a list of lists) and ``table_dev [B, max_pages]``
(int32 on the device, ``max_pages = ceil(max_len / PAGE)``) hold the same ids; device entries at or
past a sequence's pages are stale and never read.  ``lens`` / ``lens_dev``, ``set_lens``, ``advance``,
``advance_host`` and ``workspace`` keep ``KVCache``'s contract.

Allocation is host side.  ``free_pages`` is a plain list popped from its end; ``reserve(b, rows)``
gives sequence ``b`` pages for at least ``rows`` rows and uploads its table row only when a page was
added; ``release(b)`` returns them.  ``share_prefix(src, dst, rows)`` points the empty sequence ``dst``
at ``src``'s first ``rows / PAGE`` pages (whole pages only, so an append never lands in a shared page)
and sets its length to ``rows``; pages are reference-counted and freed by their last owner.

``paged_rope_append`` / ``paged_decode_attention`` have the shapes and meaning of ``rope_append`` /
``decode_attention`` (``ops/decode_attention.py``), which forward here for a cache with ``is_paged``.
GPU tensors run the gfx950 kernels (a missing entry point raises); CPU tensors run the fp32
references below: the rows gathered through the table, then the math of the dense references, so a
paged and a dense cache with the same content give the same bits on the CPU.

Chunk steps (a block of new tokens per sequence, for a subset of the sequences: the prompt suffixes behind
a shared prefix) are in ``ops/paged_chunk_attention.py``; ``seq_view`` and ``advance_seqs`` below serve them.

Cascade decode (opt-in): with ``cache.cascade_rows = P`` (whole pages that every sequence shares, checked by the
setter and again by every call; ``common_prefix_rows()`` is the most it can be) ``decode_attention`` forwards
to ``ops/paged_cascade_attention.py``, which reads the shared pages once per KV head for the whole batch, on MFMAs,
and only the rows behind them per sequence.  The default 0 keeps ``paged_decode_attention`` and its bits.

Not supported (each raises ``ValueError``): an FP8 pool, block steps (``extend_attention``), appending into
a page that is still shared (no copy-on-write), and the device-geometry form a captured graph needs.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .decode_attention import HEAD_DIM, pick_nsplit
from .rope import rope_tables

PAGE = 64


def pages_for(rows: int) -> int:
    return -(-int(rows) // PAGE)


def paged_cache_bytes(cfg, n_pages: int) -> int:
    """Bytes of the pool of ``PagedKVCache(cfg, ..., n_pages=n_pages)``."""
    return cfg.n_layers * 2 * n_pages * cfg.n_kv_heads * PAGE * HEAD_DIM * 2


class PagedKVCache:
    """The K/V rows of every layer for ``batch`` sequences of at most ``max_len`` tokens, in ``n_pages``
    pages of ``PAGE`` rows shared by the sequences."""

    is_paged = True
    is_fp8 = False

    def __init__(self, cfg, batch: int, max_len: int, n_pages: int, device="cpu"):
        if cfg.head_dim != HEAD_DIM:
            raise ValueError(f"PagedKVCache: head_dim {cfg.head_dim} is not supported (128 only)")
        if cfg.n_heads % cfg.n_kv_heads or cfg.n_heads // cfg.n_kv_heads not in (1, 2, 4, 8):
            raise ValueError("PagedKVCache: n_heads must be 1, 2, 4 or 8 times n_kv_heads")
        if batch <= 0 or max_len <= 0 or n_pages <= 0:
            raise ValueError("PagedKVCache: batch, max_len and n_pages must be positive")
        if max_len > cfg.max_seq_len:
            raise ValueError(f"PagedKVCache: max_len {max_len} exceeds the model's max_seq_len {cfg.max_seq_len}")
        self.cfg = cfg
        self.batch, self.max_len, self.n_pages = batch, max_len, n_pages
        self.max_pages = pages_for(max_len)
        self.n_heads, self.n_kv_heads = cfg.n_heads, cfg.n_kv_heads
        self.device = torch.device(device)
        self.pool = torch.zeros((cfg.n_layers, 2, n_pages, cfg.n_kv_heads, PAGE, HEAD_DIM),
                                device=self.device, dtype=torch.bfloat16)
        self.table: list[list[int]] = [[] for _ in range(batch)]
        self.table_dev = torch.zeros((batch, self.max_pages), device=self.device, dtype=torch.int32)
        self.free_pages: list[int] = list(range(n_pages - 1, -1, -1))  # popped from the end: 0, 1, 2, ...
        self._refs = [0] * n_pages
        self.lens: list[int] = [0] * batch
        self.lens_dev = torch.zeros(batch, device=self.device, dtype=torch.int32)
        self._ws: torch.Tensor | None = None
        self._scatter: tuple | None = None  # fill's index tensors, dropped when the table changes
        self._view: tuple | None = None  # seq_view's gathered rows, dropped when a table row or a length changes
        self._cascade_rows = 0

    # ------------------------------------------------------------------ allocation (host)
    def _upload(self, b: int) -> None:
        self.table_dev[b, : len(self.table[b])] = torch.tensor(self.table[b], dtype=torch.int32)
        self._scatter = self._view = None

    def reserve(self, b: int, rows: int) -> None:
        """Pages for at least ``rows`` rows of sequence ``b``; raises, with nothing changed, when the pool
        is short or ``rows > max_len``."""
        need = pages_for(rows) - len(self.table[b])
        if rows > self.max_len:
            raise ValueError(f"PagedKVCache.reserve: {rows} rows exceed max_len {self.max_len}")
        if need > len(self.free_pages):
            raise ValueError(f"PagedKVCache.reserve: sequence {b} needs {need} more pages for {rows} rows, "
                             f"{len(self.free_pages)} of {self.n_pages} are free")
        if need <= 0:
            return
        for _ in range(need):
            p = self.free_pages.pop()
            self._refs[p] = 1
            self.table[b].append(p)
        self._upload(b)

    def release(self, b: int) -> None:
        """Give sequence ``b``'s pages back (a shared page only when ``b`` was its last owner) and set
        its length to 0."""
        for p in self.table[b]:
            self._refs[p] -= 1
            if self._refs[p] == 0:
                self.free_pages.append(p)
        self.table[b] = []
        self._scatter = self._view = None
        self.lens[b] = 0
        self.lens_dev[b] = 0

    def share_prefix(self, src: int, dst: int, rows: int) -> None:
        """Point the empty sequence ``dst`` at the pages of ``src``'s first ``rows`` rows (a multiple of
        ``PAGE``, at most ``lens[src]``) and set ``lens[dst] = rows``."""
        if rows % PAGE or rows < 0:
            raise ValueError(f"PagedKVCache.share_prefix: {rows} rows are not whole pages of {PAGE}")
        if rows > self.lens[src]:
            raise ValueError(f"PagedKVCache.share_prefix: sequence {src} holds {self.lens[src]} rows, not {rows}")
        if src == dst or self.table[dst] or self.lens[dst]:
            raise ValueError(f"PagedKVCache.share_prefix: sequence {dst} is not empty")
        self.table[dst] = self.table[src][: rows // PAGE]
        for p in self.table[dst]:
            self._refs[p] += 1
        self._upload(dst)
        self.lens[dst] = rows
        self.lens_dev[dst] = rows

    def owned_rows(self, b: int) -> int:
        return len(self.table[b]) * PAGE

    def common_prefix_rows(self) -> int:
        """Rows of the largest whole-page prefix whose pool pages every sequence's table names (host tables
        only): ``P`` after ``share_prefix(0, b, P)`` for all ``b``, 0 for sequences that share nothing."""
        n = 0
        for ids in zip(*self.table):
            if any(p != ids[0] for p in ids):
                break
            n += 1
        return n * PAGE

    def check_shared_rows(self, rows: int, what: str = "PagedKVCache") -> None:
        """Raise ``ValueError`` unless the first ``rows`` rows are whole pages that every sequence holds
        (``rows <= min(lens)``) and shares (the host tables agree on their first ``rows / PAGE`` entries)."""
        rows = int(rows)
        if rows <= 0 or rows % PAGE:
            raise ValueError(f"{what}: {rows} shared rows are not a positive number of whole pages of {PAGE}")
        if rows > min(self.lens):
            raise ValueError(f"{what}: {rows} shared rows exceed the shortest sequence ({min(self.lens)} rows)")
        n = rows // PAGE
        if any(t[:n] != self.table[0][:n] for t in self.table):
            raise ValueError(f"{what}: the sequences' tables differ inside their first {n} pages; "
                             f"common_prefix_rows() is {self.common_prefix_rows()}")

    @property
    def cascade_rows(self) -> int:
        """Rows that ``decode_attention`` reads once for the whole batch (``ops/paged_cascade_attention.py``);
        0, the default, keeps the per-sequence kernel."""
        return self._cascade_rows

    @cascade_rows.setter
    def cascade_rows(self, rows: int) -> None:
        if int(rows) != 0:
            self.check_shared_rows(rows, "PagedKVCache.cascade_rows")
        self._cascade_rows = int(rows)

    # ------------------------------------------------------------------ rows
    def k(self, layer: int) -> torch.Tensor:
        return self.pool[layer, 0]

    def v(self, layer: int) -> torch.Tensor:
        return self.pool[layer, 1]

    def _row_index(self, rows_of) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """(sequence, logical row, page, slot) index tensors of rows ``0..rows_of(b)-1`` of every sequence."""
        bs, rs, ps = [], [], []
        for b in range(self.batch):
            n = rows_of(b)
            bs += [b] * n
            rs += range(n)
            ps += [self.table[b][r // PAGE] for r in range(n)]
        r = torch.tensor(rs, dtype=torch.long, device=self.device)
        return (torch.tensor(bs, dtype=torch.long, device=self.device), r,
                torch.tensor(ps, dtype=torch.long, device=self.device), r % PAGE)

    def fill(self, layer: int, k: torch.Tensor, v: torch.Tensor) -> None:
        """Store bf16 ``k`` / ``v [B, Hkv, S, 128]`` (any strides) at rows ``0..S-1`` of ``layer``, scattered
        into the pages the sequences own (``reserve`` first); rows past a sequence's pages, the padding
        of a shorter prompt, are not stored.  Does not touch the lengths."""
        S = k.shape[2]
        want = (self.batch, self.n_kv_heads, S, HEAD_DIM)
        if tuple(k.shape) != want or tuple(v.shape) != want or S > self.max_len:
            raise ValueError(f"PagedKVCache.fill: expected k and v of shape [{self.batch}, {self.n_kv_heads}, "
                             f"S <= {self.max_len}, {HEAD_DIM}], got {tuple(k.shape)} and {tuple(v.shape)}")
        if k.dtype != torch.bfloat16 or v.dtype != torch.bfloat16:
            raise ValueError(f"PagedKVCache.fill: needs bf16 rows, got {k.dtype} and {v.dtype}")
        if self._scatter is None or self._scatter[0] != S:
            self._scatter = (S, self._row_index(lambda b: min(S, self.owned_rows(b))))
        bi, ri, pi, si = self._scatter[1]
        self.pool[layer, 0][pi, :, si] = k[bi, :, ri]
        self.pool[layer, 1][pi, :, si] = v[bi, :, ri]

    def gather(self, layer: int, b: int, n: int) -> tuple[torch.Tensor, torch.Tensor]:
        """Rows ``0..n-1`` of sequence ``b`` -> contiguous ``k``, ``v [Hkv, n, 128]``."""
        r = torch.arange(n, device=self.device)
        pi = torch.tensor(self.table[b], dtype=torch.long, device=self.device)[r // PAGE]
        return tuple(self.pool[layer, j][pi, :, r % PAGE].transpose(0, 1).contiguous() for j in (0, 1))

    # ------------------------------------------------------------------ lengths (KVCache's contract)
    def set_lens(self, lens) -> None:
        lens = [int(n) for n in lens]
        if len(lens) != self.batch or min(lens) < 0 or max(lens) > self.max_len:
            raise ValueError(f"PagedKVCache: lengths {lens} do not fit batch {self.batch} x max_len {self.max_len}")
        if any(n > self.owned_rows(b) for b, n in enumerate(lens)):
            raise ValueError(f"PagedKVCache: lengths {lens} exceed the rows the sequences own "
                             f"({[self.owned_rows(b) for b in range(self.batch)]}): reserve() first")
        self.lens = lens
        self.lens_dev.copy_(torch.tensor(lens, dtype=torch.int32))
        self._view = None

    def advance(self, n: int = 1) -> None:
        if max(self.lens) + n > self.max_len:
            raise ValueError(f"PagedKVCache: {max(self.lens)} + {n} rows exceed max_len {self.max_len}")
        self.lens = [x + n for x in self.lens]
        self.lens_dev += n
        self._view = None

    def seq_view(self, seqs) -> tuple[torch.Tensor, torch.Tensor]:
        """``(lens_dev[seqs], table_dev[seqs])``, contiguous: what a kernel that serves only the sequences
        ``seqs`` takes as its lengths and its table.  Gathered once and kept until a length or a table row
        changes, so the layers of a model step share it; all sequences in order get the tensors themselves."""
        key = tuple(seqs)
        if key == tuple(range(self.batch)):
            return self.lens_dev, self.table_dev
        if self._view is None or self._view[0] != key:
            idx = torch.tensor(key, dtype=torch.long, device=self.device)
            self._view = (key, self.lens_dev[idx].contiguous(), self.table_dev[idx].contiguous())
        return self._view[1], self._view[2]

    def advance_seqs(self, seqs, new, new_dev: torch.Tensor | None = None) -> None:
        """Move the lengths of the sequences ``seqs`` only, by ``new[i]`` rows each, on host and device."""
        if any(self.lens[s] + n > min(self.max_len, self.owned_rows(s)) for s, n in zip(seqs, new) if n):
            raise ValueError(f"PagedKVCache: lengths {[self.lens[s] for s in seqs]} + {list(new)} exceed max_len "
                             f"{self.max_len} or the rows the sequences own")
        for s, n in zip(seqs, new):
            self.lens[s] += n
        if new_dev is None:
            new_dev = torch.tensor(list(new), dtype=torch.int32, device=self.device)
        self.lens_dev.index_add_(0, torch.tensor(list(seqs), dtype=torch.long, device=self.device), new_dev)
        self._view = None

    def advance_host(self, n: int = 1) -> None:
        if max(self.lens) + n > self.max_len:
            raise ValueError(f"PagedKVCache: {max(self.lens)} + {n} rows exceed max_len {self.max_len}")
        self.lens = [x + n for x in self.lens]

    def workspace(self, floats: int) -> torch.Tensor:
        if self._ws is None or self._ws.numel() < floats:
            self._ws = torch.empty(floats, device=self.device, dtype=torch.float32)
        return self._ws


def _check(x: torch.Tensor, cache: PagedKVCache, cols: int, layer: int, new: int, what: str) -> None:
    if not 0 <= layer < cache.pool.shape[0]:
        raise ValueError(f"{what}: no layer {layer} in the cache")
    if x.dtype != torch.bfloat16 or not x.is_contiguous() or x.device != cache.pool.device:
        raise ValueError(f"{what}: needs a contiguous bf16 tensor on the cache's device")
    if x.dim() != 2 or tuple(x.shape) != (cache.batch, cols):
        raise ValueError(f"{what}: expected shape {(cache.batch, cols)}, got {tuple(x.shape)}")
    if cache.pool.dtype != torch.bfloat16 or not cache.pool.is_contiguous():
        raise ValueError(f"{what}: the pool must be a contiguous bf16 tensor")
    if (cache.table_dev.dtype != torch.int32 or not cache.table_dev.is_contiguous()
            or tuple(cache.table_dev.shape) != (cache.batch, cache.max_pages)):
        raise ValueError(f"{what}: table_dev must be contiguous int32 [{cache.batch}, {cache.max_pages}]")
    if new < 0 or min(cache.lens) < 0 or max(cache.lens) + new > cache.max_len:
        raise ValueError(f"{what}: {max(cache.lens)} + {new} rows exceed the cache's max_len {cache.max_len}")
    if any(n + new > cache.owned_rows(b) for b, n in enumerate(cache.lens)):
        raise ValueError(f"{what}: a sequence has fewer pages than its {new} + lens rows: reserve() first")


def paged_rope_append_reference(qkv: torch.Tensor, cache: PagedKVCache, layer: int) -> torch.Tensor:
    """The math of ``rope_append_reference`` at position ``lens[b]``, written through the table."""
    B, Hq, Hkv = cache.batch, cache.n_heads, cache.n_kv_heads
    cos, sin = rope_tables(cache.max_len, HEAD_DIM, cache.cfg.rope_theta, qkv.device)
    pos = torch.tensor(cache.lens, device=qkv.device, dtype=torch.long)
    c, s = cos[pos][:, None, :], sin[pos][:, None, :]
    x = qkv[:, : (Hq + Hkv) * HEAD_DIM].view(B, Hq + Hkv, HEAD_DIM).float()
    x1, x2 = x[..., :64], x[..., 64:]
    y = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).to(qkv.dtype)
    v = qkv[:, (Hq + Hkv) * HEAD_DIM:].view(B, Hkv, HEAD_DIM)
    page = torch.tensor([cache.table[b][n // PAGE] for b, n in enumerate(cache.lens)], device=qkv.device)
    cache.k(layer)[page, :, pos % PAGE] = y[:, Hq:]
    cache.v(layer)[page, :, pos % PAGE] = v
    return y[:, :Hq].reshape(B, Hq * HEAD_DIM).contiguous()


def paged_rope_append(qkv: torch.Tensor, cache: PagedKVCache, layer: int) -> torch.Tensor:
    """``rope_append`` on a paged cache: reserves the page of row ``lens[b]`` for every sequence, rotates
    q / k of ``qkv [B, (Hq+2*Hkv)*128]`` there, stores k / v and returns the rotated q ``[B, Hq*128]``."""
    Hq, Hkv = cache.n_heads, cache.n_kv_heads
    for b, n in enumerate(cache.lens):
        cache.reserve(b, n + 1)
    _check(qkv, cache, (Hq + 2 * Hkv) * HEAD_DIM, layer, 1, "paged_rope_append")
    if not qkv.is_cuda:
        return paged_rope_append_reference(qkv, cache, layer)
    cos, sin = rope_tables(cache.max_len, HEAD_DIM, cache.cfg.rope_theta, qkv.device)
    q = torch.empty((cache.batch, Hq * HEAD_DIM), device=qkv.device, dtype=qkv.dtype)
    kp, vp = cache.k(layer), cache.v(layer)
    _lib.call("th_paged_rope_append", qkv.data_ptr(), cache.lens_dev.data_ptr(), cache.table_dev.data_ptr(),
              cos.data_ptr(), sin.data_ptr(), q.data_ptr(), kp.data_ptr(), vp.data_ptr(), cache.batch, Hq, Hkv,
              HEAD_DIM, cache.max_len, cache.n_pages, cache.max_pages, cache.table_dev.stride(0), kp.stride(0),
              kp.stride(1), _lib.stream_ptr(qkv.device))
    return q


def paged_decode_attention_reference(q: torch.Tensor, cache: PagedKVCache, layer: int, new: int = 0) -> torch.Tensor:
    """The math of ``decode_attention_reference`` on the first ``lens[b] + new`` rows, gathered."""
    B, Hq, Hkv = cache.batch, cache.n_heads, cache.n_kv_heads
    rep = Hq // Hkv
    out = torch.zeros((B, Hq, HEAD_DIM), device=q.device, dtype=torch.float32)
    qf = q.view(B, Hkv, rep, HEAD_DIM).float()
    for b in range(B):
        n = cache.lens[b] + new
        if n == 0:
            continue
        k, v = (x.float() for x in cache.gather(layer, b, n))  # dead rows and other pages are never touched
        s = qf[b] @ k.transpose(-1, -2) / math.sqrt(HEAD_DIM)
        out[b] = (s.softmax(-1) @ v).reshape(Hq, HEAD_DIM)
    return out.reshape(B, Hq * HEAD_DIM).to(q.dtype)


def split_pages(longest: int, nsplit: int) -> int:
    """Pages per split: splits cover whole pages, the same count for every sequence."""
    return max(1, -(-pages_for(longest) // nsplit))


def paged_decode_attention(q: torch.Tensor, cache: PagedKVCache, layer: int, nsplit: int | None = None,
                           new: int = 0) -> torch.Tensor:
    """``q [B, Hq*128]`` against the first ``lens[b] + new`` rows of ``layer`` -> ``o [B, Hq*128]``.
    ``nsplit`` overrides ``pick_nsplit`` (tests)."""
    Hq, Hkv = cache.n_heads, cache.n_kv_heads
    _check(q, cache, Hq * HEAD_DIM, layer, new, "paged_decode_attention")
    if nsplit is not None and not 1 <= int(nsplit) <= 1024:
        raise ValueError("paged_decode_attention: nsplit must be in [1, 1024]")
    if not q.is_cuda:
        return paged_decode_attention_reference(q, cache, layer, new)
    longest = max(cache.lens) + new
    if nsplit is None:
        cus = torch.cuda.get_device_properties(q.device).multi_processor_count
        nsplit = pick_nsplit(cache.batch, Hkv, longest, cus)
    nsplit = int(nsplit)
    o = torch.empty_like(q)
    ws = cache.workspace(cache.batch * Hq * nsplit * (HEAD_DIM + 2))
    kp, vp = cache.k(layer), cache.v(layer)
    _lib.call("th_paged_decode_attn", q.data_ptr(), kp.data_ptr(), vp.data_ptr(), cache.table_dev.data_ptr(),
              cache.lens_dev.data_ptr(), o.data_ptr(), ws.data_ptr(), cache.batch, Hq, Hkv, HEAD_DIM,
              cache.max_len, cache.n_pages, cache.max_pages, cache.table_dev.stride(0), kp.stride(0),
              kp.stride(1), nsplit, split_pages(longest, nsplit), int(new), 1.0 / math.sqrt(HEAD_DIM),
              _lib.stream_ptr(q.device))
    return o
