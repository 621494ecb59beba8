"""Shapes and the fp64 oracle shared by the decode-attention tests (CPU reference and GPU kernels)."""
import math

import torch

from tensorhive_fixed_amd.models.llama3 import LlamaConfig
from tensorhive_fixed_amd.ops.decode_attention import KVCache

SMAX = 1024
HEADS = [(2, 2), (4, 2), (4, 1), (8, 2), (8, 1)]  # rep 1, 2, 4, 4, 8
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


PROFILE_LENS = [1024, 700, 257]
HEAD_GAINS = (1.0, 0.8, 0.6, 0.4)  # a of q head h is HEAD_GAINS[h % 4]: one workgroup's heads disagree on the max


def profile_dead_cache(Hq: int, Hkv: int, lens: list[int], profile: str, device, seed: int = 0):
    """``nan_dead_cache`` with a score profile of ``tests/attention_oracles.py`` along the key axis of
    every sequence (over its own length) and a per-head gain on q: the log2-domain score of (head h,
    key j) is the randn score plus ``HEAD_GAINS[h % 4] * b_j``."""
    from tests import attention_oracles as ao

    g = torch.Generator().manual_seed(seed)
    cache = KVCache(attn_cfg(Hq, Hkv), len(lens), SMAX, device)
    kv = torch.randn(cache.kv.shape, generator=g, dtype=torch.float64)
    e = ao.bias_direction()
    for b, n in enumerate(lens):
        kv[0, 0, b, :, :n] += ao.key_bias(profile, n)[:, None] * e / (16 * ao.C_LOG2)
        kv[:, :, b, :, n:] = float("nan")
    cache.kv.copy_(kv.to(torch.bfloat16))
    cache.set_lens(lens)
    q = torch.randn(len(lens), Hq, 128, generator=g, dtype=torch.float64)
    q += torch.tensor([HEAD_GAINS[h % 4] for h in range(Hq)], dtype=torch.float64)[None, :, None] * e
    return cache, q.reshape(len(lens), Hq * 128).to(torch.bfloat16).to(device)


def assert_rows_close(o: torch.Tensor, ref: torch.Tensor, Hq: int) -> tuple[float, float]:
    """The bounds of ``assert_attention_close`` on every (sequence, q head) row by itself; returns
    the worst row's max-abs and relative error."""
    o = o.detach().cpu().double().view(ref.shape[0], Hq, 128)
    ref = ref.view(ref.shape[0], Hq, 128)
    assert torch.isfinite(o).all(), "non-finite output"
    err = (o - ref).abs().amax(-1)
    rel = (o - ref).norm(dim=-1) / ref.norm(dim=-1)
    print(f"worst row: max abs err {err.max().item():.3e}  rel err {rel.max().item():.3e}")
    b, h = divmod(int(err.argmax()), Hq)
    assert err.max().item() < 2e-2, f"sequence {b} head {h}: max abs err {err.max().item()}"
    b, h = divmod(int(rel.argmax()), Hq)
    assert rel.max().item() < 1e-2, f"sequence {b} head {h}: relative err {rel.max().item()}"
    return err.max().item(), rel.max().item()


def attention_fp64(q: torch.Tensor, cache: KVCache, layer: int = 0) -> torch.Tensor:
    """fp64 softmax attention of the bf16 inputs over the live rows -> [B, Hq*128] float64 (CPU)."""
    B, Hq, Hkv = cache.batch, cache.n_heads, cache.n_kv_heads
    rep = Hq // Hkv
    out = torch.zeros(B, Hq, 128, dtype=torch.float64)
    qd = q.detach().cpu().double().view(B, Hkv, rep, 128)
    kv = cache.kv[layer].detach().cpu()  # one layer: the others may be large
    for b in range(B):
        n = cache.lens[b]
        k, v = kv[0, b, :, :n].double(), kv[1, b, :, :n].double()
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
