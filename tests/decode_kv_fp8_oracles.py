"""Caches and the fp64 oracle of the FP8 KV-cache tests (CPU reference and GPU kernels).  Nothing here
calls code under test except the CPU quantizer ``quantize_kv_rows``, which ``tests/test_decode_kv_fp8.py``
checks on its own."""
import math

import torch

from tensorhive_fixed_amd.ops.decode_attention import KVCache, quantize_kv_rows
from tests import decode_oracles as do

FP8 = torch.float8_e4m3fn
NAN_CODE = 0x7F


def fp8_cache(cfg, batch: int, max_len: int, device) -> KVCache:
    return KVCache(cfg, batch, max_len, device, dtype=FP8)


def _quantized(src: KVCache, device) -> KVCache:
    """An FP8 cache holding the CPU quantization of ``src``'s live bf16 rows; dead rows hold the NaN
    code in every byte and a NaN scale."""
    kv = src.kv.detach().cpu()
    codes = torch.full(kv.shape, NAN_CODE, dtype=torch.uint8)
    scale = torch.full(kv.shape[:-1], float("nan"), dtype=torch.float32)
    for b, n in enumerate(src.lens):
        c, s = quantize_kv_rows(kv[:, :, b, :, :n].contiguous())
        codes[:, :, b, :, :n] = c.view(torch.uint8)
        scale[:, :, b, :, :n] = s
    cache = fp8_cache(src.cfg, src.batch, src.max_len, device)
    cache.kv.view(torch.uint8).copy_(codes)
    cache.kv_scale.copy_(scale)
    cache.set_lens(src.lens)
    return cache


def quantized_nan_dead_cache(Hq: int, Hkv: int, lens: list[int], device, seed: int = 0):
    """(FP8 cache, q) with the values of ``decode_oracles.nan_dead_cache``."""
    src, q = do.nan_dead_cache(Hq, Hkv, lens, "cpu", seed)
    return _quantized(src, device), q.to(device)


def quantized_profile_dead_cache(Hq: int, Hkv: int, lens: list[int], profile: str, device, seed: int = 0):
    """(FP8 cache, q) with the values of ``decode_oracles.profile_dead_cache``."""
    src, q = do.profile_dead_cache(Hq, Hkv, lens, profile, "cpu", seed)
    return _quantized(src, device), q.to(device)


def dequantized_fp64(cache: KVCache, layer: int = 0):
    """(k, v) ``[B, Hkv, Smax, 128]`` float64 on the CPU: ``codes.double() * scale.double()``."""
    kv = cache.kv.detach().cpu()[layer].double() * cache.kv_scale.detach().cpu()[layer].double()[..., None]
    return kv[0], kv[1]


def attention_fp64_fp8(q: torch.Tensor, cache: KVCache, layer: int = 0) -> torch.Tensor:
    """fp64 softmax attention over ``codes.double() * scale.double()`` of the live rows ->
    ``[B, Hq*128]`` float64 (CPU)."""
    B, Hq, Hkv = cache.batch, cache.n_heads, cache.n_kv_heads
    rep = Hq // Hkv
    out = torch.zeros(B, Hq, 128, dtype=torch.float64)
    qd = q.detach().cpu().double().view(B, Hkv, rep, 128)
    kv, sc = cache.kv[layer].detach().cpu(), cache.kv_scale[layer].detach().cpu()
    for b in range(B):  # the live rows only, one sequence at a time: a cache may be large
        n = cache.lens[b]
        kd, vd = (kv[j, b, :, :n].double() * sc[j, b, :, :n].double()[..., None] for j in range(2))
        s = qd[b] @ kd.transpose(-1, -2) / math.sqrt(128)
        out[b] = (s.softmax(-1) @ vd).reshape(Hq, 128)
    return out.reshape(B, Hq * 128)


def attention_f32_kernel_order(q: torch.Tensor, cache: KVCache, layer: int = 0) -> torch.Tensor:
    """An f32 emulation of the kernel's order of scaling on the CPU: the codes dotted with q first, the
    sum times ``kscale[key]``, and ``p * vscale[key]`` before the product with the V codes; bf16 out."""
    B, Hq, Hkv = cache.batch, cache.n_heads, cache.n_kv_heads
    rep = Hq // Hkv
    out = torch.zeros(B, Hq, 128, dtype=torch.float32)
    qf = q.detach().cpu().float().view(B, Hkv, rep, 128) * (1.0 / math.sqrt(128))
    kv, sc = cache.kv.detach().cpu()[layer], cache.kv_scale.detach().cpu()[layer]
    for b in range(B):
        n = cache.lens[b]
        kc, vc = kv[0, b, :, :n].float(), kv[1, b, :, :n].float()
        s = (qf[b] @ kc.transpose(-1, -2)) * sc[0, b, :, None, :n]
        s = s - s.amax(-1, keepdim=True)
        p = s.exp()
        l = p.sum(-1, keepdim=True)
        out[b] = (((p * sc[1, b, :, None, :n]) @ vc) / l).reshape(Hq, 128)
    return out.reshape(B, Hq * 128).to(torch.bfloat16)
