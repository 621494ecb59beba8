"""Builders and references of the KV-cache geometry tests (``tests/test_decode_geometry.py`` on the CPU,
``tests/gpu/test_decode_geometry_gpu.py`` on the kernels): one sequence per length in one launch, on a
layer that is not layer 0, for the bf16 cache, the FP8 cache and the block kernel; and the closed form
of the marked-row caches that reach row offsets a 1024-row cache never forms.

Nothing here calls code under test except ``KVCache`` (a container) and the CPU quantizer
``quantize_kv_rows``, which ``tests/test_decode_kv_fp8.py`` checks on its own."""
import math

import torch

from tensorhive_fixed_amd.ops.decode_attention import KVCache, quantize_kv_rows
from tests import decode_kv_fp8_oracles as ko
from tests import decode_oracles as do
from tests import extend_oracles as eo

FP8 = torch.float8_e4m3fn
HEADS = [(2, 2), (4, 2), (4, 1), (8, 1)]  # rep 1, 2, 4, 8; rep 2 on two KV heads
# chunks of 520 / 174 / 75 keys (block: 264 + T in 1 / 3 / 7 parts): multiples of no key tile, so every
# tail from 1 to the chunk length occurs at every split start
NSPLITS = [1, 3, 7]
BLOCKS = [1, 3, 8]
SWEEP_LONGEST = 520  # past two 256-key trips of the FP8 kernel
BLOCK_LONGEST = 264  # past two 128-key steps of the block kernel
_POOL = 4099  # rows of randn per (K / V, KV head); a prime above every max_len here


def permutation(lo: int, hi: int, longest_at: int, seed: int) -> list[int]:
    """A seeded permutation of ``lo..hi`` with ``hi`` moved to index ``longest_at``."""
    vals = (torch.randperm(hi - lo + 1, generator=torch.Generator().manual_seed(seed)) + lo).tolist()
    i = vals.index(hi)
    vals[i], vals[longest_at] = vals[longest_at], vals[i]
    return vals


# The device-geometry kernels reduce the lengths with `for (i = lane; i < B; i += 64)`: the longest
# sequence at index 0 is found by lane 0 in the first trip, at index 300 by lane 44 in the fifth.
SWEEP_LENS = {"longest@0": permutation(1, SWEEP_LONGEST, 0, seed=0),
              "longest@300": permutation(1, SWEEP_LONGEST, 300, seed=1)}
BLOCK_LENS = permutation(0, BLOCK_LONGEST, 100, seed=2)


def _rows(Hkv: int, live: list[int], max_len: int, seed: int):
    """bf16 ``[2, B, Hkv, max_len, 128]`` and the generator: row j of sequence b is row
    ``(j + 37 b) mod 4099`` of a randn pool per (K / V, KV head), so the rows of a sequence are distinct and
    two sequences differ at every position; the caller marks the rows at and past ``live[b]`` dead."""
    g = torch.Generator().manual_seed(seed)
    pool = torch.randn(2, Hkv, _POOL, 128, generator=g).to(torch.bfloat16)
    idx = (torch.arange(max_len)[None, :] + 37 * torch.arange(len(live))[:, None]) % _POOL
    dead = torch.arange(max_len)[None, :] >= torch.tensor(live)[:, None]  # [B, max_len]
    return pool, idx, dead, g


def _cache(Hq, Hkv, lens, block, device, layers, layer, fp8, seed):
    B, max_len = len(lens), max(lens) + block + 8
    pool, idx, dead, g = _rows(Hkv, [n + block for n in lens], max_len, seed)
    cfg = do.attn_cfg(Hq, Hkv, n_layers=layers, max_seq_len=max_len)
    cache = KVCache(cfg, B, max_len, device, dtype=FP8 if fp8 else torch.bfloat16)
    if fp8:  # quantization is per row, so it commutes with the gather
        codes, scale = quantize_kv_rows(pool)
        codes = codes.view(torch.uint8)[:, :, idx].permute(0, 2, 1, 3, 4).contiguous()
        scale = scale[:, :, idx].permute(0, 2, 1, 3).contiguous()
        codes.masked_fill_(dead[None, :, None, :, None], ko.NAN_CODE)
        scale.masked_fill_(dead[None, :, None, :], float("nan"))
        cache.kv.view(torch.uint8).fill_(ko.NAN_CODE)
        cache.kv_scale.fill_(float("nan"))
        cache.kv.view(torch.uint8)[layer].copy_(codes)
        cache.kv_scale[layer].copy_(scale)
    else:
        rows = pool[:, :, idx].permute(0, 2, 1, 3, 4).contiguous()
        rows.masked_fill_(dead[None, :, None, :, None], float("nan"))
        cache.kv.fill_(float("nan"))
        cache.kv[layer].copy_(rows)
    cache.set_lens(lens)
    return cache, g


def sweep_cache(Hq: int, Hkv: int, lens: list[int], device, layers: int = 2, layer: int = 1, fp8: bool = False,
                seed: int = 0):
    """(cache, q, ref): a ``KVCache`` of ``max_len = max(lens) + 8`` whose layer ``layer`` holds randn bf16
    rows (``fp8``: their quantization by ``quantize_kv_rows``) with NaN (the NaN code and a NaN scale) at
    and past every ``lens[b]``, every other layer NaN everywhere; randn bf16 q ``[B, Hq*128]``; and the
    fp64 attention over the live rows of ``layer`` (over ``codes * scale`` for ``fp8``)."""
    cache, g = _cache(Hq, Hkv, lens, 0, device, layers, layer, fp8, seed)
    q = torch.randn(len(lens), Hq * 128, generator=g).to(torch.bfloat16).to(device)
    ref = ko.attention_fp64_fp8(q, cache, layer) if fp8 else do.attention_fp64(q, cache, layer)
    return cache, q, ref


def sweep_block_cache(Hq: int, Hkv: int, lens: list[int], T: int, device, layers: int = 2, layer: int = 1,
                      seed: int = 0):
    """(cache, q, ref) for a block of ``T``: as ``sweep_cache`` (bf16) with old lengths ``lens``, the rows
    at and past ``lens[b] + T`` NaN, q ``[B, T, Hq*128]`` and ``extend_fp64`` at ``layer``."""
    cache, g = _cache(Hq, Hkv, lens, T, device, layers, layer, False, seed)
    q = torch.randn(len(lens), T, Hq * 128, generator=g).to(torch.bfloat16).to(device)
    return cache, q, eo.extend_fp64(q, cache, layer)


def dead_rows_are_nan(cache: KVCache, layer: int, block: int = 0) -> bool:
    """Whether the cache is what the builders claim: layer ``layer`` finite below ``lens[b] + block`` and NaN
    (NaN code, NaN scale) from there on, every other layer NaN everywhere."""
    S = cache.max_len
    dead = (torch.arange(S)[None, :] >= (torch.tensor(cache.lens) + block)[:, None])[None, :, None, :]  # [1, B, 1, S]
    ok = True
    for ly in range(cache.kv.shape[0]):
        want = dead if ly == layer else torch.ones_like(dead)
        if cache.is_fp8:
            codes = cache.kv.view(torch.uint8)[ly].cpu()
            isnan = (codes & 0x7F) == 0x7F
            snan = cache.kv_scale[ly].cpu().isnan()
            ok = ok and bool((snan == want.expand_as(snan)).all())
        else:
            isnan = cache.kv[ly].cpu().isnan()
        ok = ok and bool((isnan == want[..., None].expand_as(isnan)).all())
    return ok


def host_geometry(lens, new: int, nsplit: int) -> tuple[int, int]:
    """``(nsplit, chunk)`` as ``decode_attention`` and ``extend_attention`` pass them for a split count."""
    return nsplit, max(1, -(-(max(lens) + new) // nsplit))


# ------------------------------------------------------------------------------------ marked-row caches
MARKED_K = 1.625  # q = ones: the score of a marked key is 128 * 1.625 / sqrt(128) = 18.38


def marked_keys(n: int, mid: int | None = None) -> list[int]:
    """The first and last of ``n`` rows and the two around ``mid`` (default: the middle)."""
    mid = n // 2 if mid is None else mid
    return [0, mid - 1, mid, n - 1]


def marked_closed_form(k_marked: torch.Tensor, v_marked: torch.Tensor, n_keys: int) -> torch.Tensor:
    """fp64 attention of q = ones over ``n_keys`` keys of which ``k_marked / v_marked [M, 128]`` are the
    only rows that are not zero: ``sum e^{s_j} v_j / ((n_keys - M) + sum e^{s_j})`` -> ``[128]``."""
    s = k_marked.double().sum(-1) / math.sqrt(128)
    w = s.exp()
    return (w[:, None] * v_marked.double()).sum(0) / ((n_keys - len(w)) + w.sum())


def marked_rows(n_marked: int, seed: int = 0):
    """(k, v) bf16 ``[n_marked, 128]``: every K row ``1.625 * ones``, every V row its own randn."""
    g = torch.Generator().manual_seed(seed)
    k = torch.full((n_marked, 128), MARKED_K).to(torch.bfloat16)
    return k, torch.randn(n_marked, 128, generator=g).to(torch.bfloat16)
