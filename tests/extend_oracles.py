"""Shapes, builders and the fp64 oracle shared by the block-decode (extend attention) tests."""
import math

import torch

from tensorhive_fixed_amd.ops.decode_attention import KVCache
from tests import decode_oracles as do

SMAX = do.SMAX
HEADS = do.HEADS + [(2, 1)]  # rep 1, 2, 4, 4, 8 and the tiny config's rep 2 on one KV head
BLOCKS = [1, 2, 3, 5, 8]
# key-tile sizes of csrc/extend_attn.hip: one MFMA tile, a wave's step (two tiles), the workgroup's step
KEY_TILES = [16, 32, 128]


def block_lens(T: int) -> list[list[int]]:
    """Old lengths for a block of ``T``: an empty cache, one row, tile neighbours, a ragged batch that
    fills the cache, and for every key-tile size ``boundary - t`` for t = 0..T (the block straddles it)."""
    out = [[0], [1], [63, 64, 65], [1, 200, SMAX - T], [257, 256, 255]]
    for tile in KEY_TILES:
        out.append([tile - t for t in range(T + 1)])
    return out


def nan_dead_block_cache(Hq: int, Hkv: int, lens: list[int], T: int, device, seed: int = 0):
    """(cache, q): randn bf16 K/V with NaN in every row at or past ``lens[b] + T`` (the block's rows are
    live), cache lengths ``lens``, randn bf16 q ``[B, T, Hq*128]``."""
    g = torch.Generator().manual_seed(seed)
    cache = KVCache(do.attn_cfg(Hq, Hkv), len(lens), SMAX, device)
    kv = torch.randn(cache.kv.shape, generator=g).to(torch.bfloat16)
    for b, n in enumerate(lens):
        kv[:, :, b, :, n + T:] = float("nan")
    cache.kv.copy_(kv)
    cache.set_lens(lens)
    q = torch.randn(len(lens), T, Hq * 128, generator=g).to(torch.bfloat16).to(device)
    return cache, q


def extend_fp64(q: torch.Tensor, cache: KVCache, layer: int = 0) -> torch.Tensor:
    """fp64 softmax attention of query row (b, t) over its own ``lens[b] + t + 1`` rows ->
    ``[B, T, Hq*128]`` float64 (CPU)."""
    B, T, Hq, Hkv = cache.batch, q.shape[1], cache.n_heads, cache.n_kv_heads
    rep = Hq // Hkv
    out = torch.zeros(B, T, Hq, 128, dtype=torch.float64)
    qd = q.detach().cpu().double().view(B, T, Hkv, rep, 128)
    kv = cache.kv[layer].detach().cpu()  # one layer: the others may be large
    for b in range(B):
        for t in range(T):
            n = cache.lens[b] + t + 1
            k, v = kv[0, b, :, :n].double(), kv[1, b, :, :n].double()
            s = qd[b, t] @ k.transpose(-1, -2) / math.sqrt(128)
            out[b, t] = (s.softmax(-1) @ v).reshape(Hq, 128)
    return out.reshape(B, T, Hq * 128)


def assert_block_close(o: torch.Tensor, ref: torch.Tensor, Hq: int) -> None:
    """``assert_attention_close`` on the whole output and ``assert_rows_close`` on every (b, t, head) row."""
    B, T = ref.shape[:2]
    do.assert_attention_close(o.reshape(B * T, -1), ref.reshape(B * T, -1))
    do.assert_rows_close(o.reshape(B * T, -1), ref.reshape(B * T, -1), Hq)
