"""Shapes and the fp64 oracle shared by the decode-attention tests (CPU reference and GPU kernels)."""
import math

import torch

from tensorhive_fixed_amd.models.llama3 import LlamaConfig
from tensorhive_fixed_amd.ops.decode_attention import KVCache

SMAX = 1024
HEADS = [(2, 2), (4, 1), (8, 2), (8, 1)]  # rep 1, 4, 4, 8
KV_LENS = [[1], [63, 64, 65], [1, 200, 1024], [257, 256, 255]]
NSPLITS = [1, 3, 8, None]  # 3 does not divide the lengths, 8 leaves splits empty, None = automatic


def attn_cfg(Hq: int, Hkv: int, n_layers: int = 1, max_seq_len: int = SMAX) -> LlamaConfig:
    return LlamaConfig(vocab_size=64, dim=Hq * 128, n_layers=n_layers, n_heads=Hq, n_kv_heads=Hkv,
                       ffn_dim=128, max_seq_len=max_seq_len)


def nan_dead_cache(Hq: int, Hkv: int, lens: list[int], device, seed: int = 0):
    """(cache, q): randn bf16 K/V with every row at or past ``lens[b]`` set to NaN, randn bf16 q."""
    g = torch.Generator().manual_seed(seed)
    cache = KVCache(attn_cfg(Hq, Hkv), len(lens), SMAX, device)
    kv = torch.randn(cache.kv.shape, generator=g).to(torch.bfloat16)
    for b, n in enumerate(lens):
        kv[:, :, b, :, n:] = float("nan")
    cache.kv.copy_(kv)
    cache.set_lens(lens)
    q = torch.randn(len(lens), Hq * 128, generator=g).to(torch.bfloat16).to(device)
    return cache, q


def attention_fp64(q: torch.Tensor, cache: KVCache, layer: int = 0) -> torch.Tensor:
    """fp64 softmax attention of the bf16 inputs over the live rows -> [B, Hq*128] float64 (CPU)."""
    B, Hq, Hkv = cache.batch, cache.n_heads, cache.n_kv_heads
    rep = Hq // Hkv
    out = torch.zeros(B, Hq, 128, dtype=torch.float64)
    qd = q.detach().cpu().double().view(B, Hkv, rep, 128)
    kv = cache.kv.detach().cpu()
    for b in range(B):
        n = cache.lens[b]
        k, v = kv[layer, 0, b, :, :n].double(), kv[layer, 1, b, :, :n].double()
        s = qd[b] @ k.transpose(-1, -2) / math.sqrt(128)
        out[b] = (s.softmax(-1) @ v).reshape(Hq, 128)
    return out.reshape(B, Hq * 128)


def assert_attention_close(o: torch.Tensor, ref: torch.Tensor) -> None:
    """The flash forward's bounds on the same input distribution (tests/gpu/test_flash_attn_gpu.py)."""
    o = o.detach().cpu().double()
    assert torch.isfinite(o).all(), "non-finite output"
    err = (o - ref).abs().max().item()
    rel = ((o - ref).norm() / ref.norm()).item()
    print(f"max abs err {err:.3e}  rel Frobenius err {rel:.3e}")
    assert err < 2e-2, f"max abs err {err}"
    assert rel < 1e-2, f"relative Frobenius err {rel}"
