"""Small-batch linear for decode steps on FP8 weights: ``y = (x @ wq.T) * scale`` with at most 16 rows of ``x``.

``quantize_weight_fp8(w)`` turns a contiguous bf16 ``w [N, K]`` into ``(wq, scale)``: ``wq`` is OCP FP8
(``torch.float8_e4m3fn``) in the same ``[out, in]`` layout and ``scale`` is one f32 per output row,
``absmax(w[n]) / 448`` (1.0 for a row of zeros).  The quotient is clamped to +-448 before the cast:
torch's cast to e4m3fn does not saturate (465 becomes NaN) and a quotient may round a hair above 448.
The rule never produces a NaN code.  Activations, accumulation and the KV cache stay as they are.

``decode_linear_fp8(x, wq, scale, out_dtype)`` and ``decode_gate_up_swiglu_fp8(x, w13q, scale13)`` are
the FP8-weight forms of ``ops/decode_linear.py``: ``x [M, K]`` contiguous bf16, f32 accumulation, the
scale applied once per output as one f32 multiplication of the finished sum (``silu(g * sg) * (u * su)``
for the packed gate|up weight).  ``supported_fp8(M, N, K)`` is the shape rule of both, the one of
``decode_linear.supported``.

GPU tensors run ``csrc/decode_linear_fp8.hip``, which streams ``wq`` from HBM once, half the bytes of
the bf16 kernel (a missing entry point raises, there is no fallback); CPU tensors run the fp32
references below.
"""
from __future__ import annotations

import torch
import torch.nn.functional as Fn

from . import _lib
from .decode_linear import K_MULTIPLE, MAX_ROWS, N_MULTIPLE, supported

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0
_MODE = {torch.bfloat16: 0, torch.float32: 1}
_MODE_SWIGLU = 2
# fewest workgroups a launch keeps when a workgroup takes two tiles of output columns: two tiles won from 192
# workgroups on (qkv, gate|up, LM head) and lost at 128 (down: 23.4 against 17.0 us at M = 8)
# (profiles/decode_fp8/README.md)
MIN_WORKGROUPS_FP8 = 192


def supported_fp8(M: int, N: int, K: int) -> bool:
    return supported(M, N, K)


def pick_tiles_fp8(ncols: int) -> int:
    """Tiles of 16 output columns per workgroup, 1 or 2: a policy of its own for the FP8 kernel, whose
    x traffic per weight byte is twice the bf16 kernel's (profiles/decode_fp8/README.md)."""
    return 2 if -(-ncols // 32) >= MIN_WORKGROUPS_FP8 else 1


def quantize_weight_fp8(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """bf16 ``w [N, K]`` -> (``wq`` e4m3fn ``[N, K]``, ``scale`` f32 ``[N]``); module docstring.  Runs
    on ``w``'s device; the bytes are those of the CPU run (tests/gpu/test_decode_linear_fp8_gpu.py)."""
    if w.dtype != torch.bfloat16 or w.dim() != 2 or not w.is_contiguous():
        raise ValueError(f"quantize_weight_fp8: needs a contiguous bf16 [N, K] weight, got {w.dtype} "
                         f"{tuple(w.shape)} with strides {w.stride()}")
    wf = w.float()
    amax = wf.abs().amax(dim=1)
    # a tensor divisor: by a Python scalar the GPU multiplies by the rounded reciprocal, which is not the
    # correctly rounded quotient the CPU gives
    scale = amax / torch.full_like(amax, FP8_MAX)
    scale = torch.where(scale > 0, scale, torch.ones_like(scale))
    wq = (wf / scale[:, None]).clamp(-FP8_MAX, FP8_MAX).to(FP8)
    return wq, scale


def _check(x: torch.Tensor, wq: torch.Tensor, scale: torch.Tensor, what: str) -> None:
    if x.dtype != torch.bfloat16 or wq.dtype != FP8 or scale.dtype != torch.float32:
        raise ValueError(f"{what}: needs bf16 x, float8_e4m3fn wq and f32 scale, got {x.dtype}, {wq.dtype} and "
                         f"{scale.dtype}")
    if x.dim() != 2 or wq.dim() != 2 or scale.dim() != 1:
        raise ValueError(f"{what}: needs x [M, K], wq [N, K] and scale [N], got {tuple(x.shape)}, "
                         f"{tuple(wq.shape)} and {tuple(scale.shape)}")
    if not x.is_contiguous() or not wq.is_contiguous() or not scale.is_contiguous():
        raise ValueError(f"{what}: x, wq and scale must be contiguous (strides {x.stride()}, {wq.stride()} and "
                         f"{scale.stride()})")
    if x.data_ptr() % 16 or wq.data_ptr() % 16 or scale.data_ptr() % 4:
        raise ValueError(f"{what}: x and wq must start on a 16-byte boundary, scale on a 4-byte one")
    if x.device != wq.device or x.device != scale.device:
        raise ValueError(f"{what}: x is on {x.device}, wq on {wq.device}, scale on {scale.device}")
    if x.shape[1] != wq.shape[1]:
        raise ValueError(f"{what}: x has K = {x.shape[1]}, wq has K = {wq.shape[1]}")
    if scale.shape[0] != wq.shape[0]:
        raise ValueError(f"{what}: wq has {wq.shape[0]} rows, scale has {scale.shape[0]} entries")
    M, N, K = x.shape[0], wq.shape[0], x.shape[1]
    if not supported_fp8(M, N, K):
        raise ValueError(f"{what}: M = {M}, N = {N}, K = {K} is not supported (1 <= M <= {MAX_ROWS}, "
                         f"K a multiple of {K_MULTIPLE}, N a multiple of {N_MULTIPLE})")


def _tiles(tiles, ncols: int, what: str) -> int:
    if tiles is None:
        return pick_tiles_fp8(ncols)
    if tiles not in (1, 2):
        raise ValueError(f"{what}: tiles must be 1 or 2, got {tiles}")
    return int(tiles)


def decode_linear_fp8_reference(x: torch.Tensor, wq: torch.Tensor, scale: torch.Tensor,
                                out_dtype=torch.bfloat16) -> torch.Tensor:
    return ((x.float() @ wq.float().t()) * scale).to(out_dtype)


def decode_gate_up_swiglu_fp8_reference(x: torch.Tensor, w13q: torch.Tensor, scale13: torch.Tensor) -> torch.Tensor:
    """``silu(g * sg) * (u * su)`` from the f32 products, rounded to bf16 once."""
    g, u = ((x.float() @ w13q.float().t()) * scale13).chunk(2, dim=-1)
    return (Fn.silu(g) * u).to(x.dtype)


def decode_linear_fp8(x: torch.Tensor, wq: torch.Tensor, scale: torch.Tensor, out_dtype=torch.bfloat16,
                      tiles: int | None = None) -> torch.Tensor:
    """``(x [M, K] @ wq [N, K].T) * scale [N] -> [M, N]`` in ``out_dtype`` (bf16 or f32).  ``tiles``
    overrides ``pick_tiles_fp8`` (tests, measurements)."""
    if out_dtype not in _MODE:
        raise ValueError(f"decode_linear_fp8: out_dtype must be bfloat16 or float32, got {out_dtype}")
    _check(x, wq, scale, "decode_linear_fp8")
    M, K = x.shape
    N = wq.shape[0]
    tiles = _tiles(tiles, N, "decode_linear_fp8")
    if not x.is_cuda:
        return decode_linear_fp8_reference(x, wq, scale, out_dtype)
    y = torch.empty((M, N), device=x.device, dtype=out_dtype)
    _lib.call("th_decode_linear_fp8", x.data_ptr(), wq.data_ptr(), scale.data_ptr(), y.data_ptr(), M, N, K,
              _MODE[out_dtype], tiles, _lib.stream_ptr(x.device))
    return y


def decode_gate_up_swiglu_fp8(x: torch.Tensor, w13q: torch.Tensor, scale13: torch.Tensor,
                              tiles: int | None = None) -> torch.Tensor:
    """``silu((x @ w13q[:F].T) * scale13[:F]) * ((x @ w13q[F:].T) * scale13[F:])`` as bf16 ``[M, F]``."""
    _check(x, w13q, scale13, "decode_gate_up_swiglu_fp8")  # 2F a multiple of 16, as in decode_gate_up_swiglu
    M, K = x.shape
    F2 = w13q.shape[0]
    tiles = _tiles(tiles, F2 // 2, "decode_gate_up_swiglu_fp8")
    if not x.is_cuda:
        return decode_gate_up_swiglu_fp8_reference(x, w13q, scale13)
    y = torch.empty((M, F2 // 2), device=x.device, dtype=x.dtype)
    _lib.call("th_decode_linear_fp8", x.data_ptr(), w13q.data_ptr(), scale13.data_ptr(), y.data_ptr(), M, F2, K,
              _MODE_SWIGLU, tiles, _lib.stream_ptr(x.device))
    return y
