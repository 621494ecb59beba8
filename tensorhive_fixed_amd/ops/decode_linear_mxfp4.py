"""Small-batch linear for decode steps on OCP MXFP4 weights: ``y = x @ dequant(codes, scales).T`` with at
most 16 rows of ``x``.

``quantize_weight_mxfp4(w)`` turns a contiguous bf16 ``w [N, K]`` (the shape rule of
``decode_linear.supported``) into ``(codes, scales)`` in the public OCP layout, so weights quantized
elsewhere load as they are:

* ``codes`` uint8 ``[N, K/2]``: element ``2j`` in the low nibble of byte ``j``, ``2j+1`` in the high one.  A
  code is sign(1) | E2M1(3) with the magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6.
* ``scales`` uint8 ``[N, K/32]``, E8M0: block ``j`` of a row is scaled by ``2^(scales[n, j] - 127)``.

The block exponent ``X`` is the smallest with ``amax / 2^X <= 6`` (nothing clips), from ``torch.frexp`` in
integers: ``amax = m 2^ex`` with ``m`` in [0.5, 1) gives ``ex - 3`` if ``m <= 0.75`` else ``ex - 2``.  The stored
byte ``X + 127`` is clamped to [2, 252], so every dequantized magnitude is zero or a normal bf16 and the
byte shifted left by 23 is a normal f32; an all-zero block gets 127.  Elements round to the nearest E2M1
value, ties to the even code.  Every step is a comparison, an integer operation or a multiplication by an
exact power of two built from its bits, so the CPU and the GPU give the same bytes (a scalar divisor or
``pow`` would not, see ``decode_linear_fp8``).  ``dequantize_mxfp4`` is exact: ``code * 2^e`` is a bf16.

``decode_linear_mxfp4(x, codes, scales, out_dtype)`` and ``decode_gate_up_swiglu_mxfp4(x, codes13,
scales13)`` are the MXFP4 forms of ``ops/decode_linear_fp8.py``: ``x [M, K]`` contiguous bf16, f32
accumulation.  GPU tensors run ``csrc/decode_linear_mxfp4.hip``, which streams 0.53125 bytes per weight
from HBM once (a missing entry point raises, there is no fallback); CPU tensors run the fp32 references
below on the dequantized weight.
"""
from __future__ import annotations

import torch
import torch.nn.functional as Fn

from . import _lib
from .decode_linear import K_MULTIPLE, MAX_ROWS, N_MULTIPLE, supported

BLOCK = 32
E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
SCALE_BYTE_MIN, SCALE_BYTE_MAX, SCALE_BYTE_ZERO = 2, 252, 127
_MODE = {torch.bfloat16: 0, torch.float32: 1}
_MODE_SWIGLU = 2
TILES = (1, 2, 4)
# fewest workgroups a launch keeps when a workgroup takes more tiles of output columns.  At M = 16: four
# tiles won on the LM head (85.4 against 105.3 / 161.1 us at 2 / 1) and gate|up (224 workgroups: 20.6 against
# 23.8 / 28.4), two on qkv (192 workgroups: 9.7 against 12.6 at 1 and 13.1 at 4, which leaves 96), one on
# the down projection (256 workgroups: 21.5 against 28.1 / 38.1) (profiles/decode_mxfp4/README.md)
MIN_WORKGROUPS_MXFP4 = 192


def supported_mxfp4(M: int, N: int, K: int) -> bool:
    return supported(M, N, K)


def pick_tiles_mxfp4(ncols: int) -> int:
    """Tiles of 16 output columns per workgroup: the most of 4, 2, 1 that leaves ``MIN_WORKGROUPS_MXFP4``
    workgroups (profiles/decode_mxfp4/README.md)."""
    for t in (4, 2):
        if -(-ncols // (16 * t)) >= MIN_WORKGROUPS_MXFP4:
            return t
    return 1


def _pow2(byte: torch.Tensor) -> torch.Tensor:
    """``2^(byte - 127)`` as f32 from its bits; ``byte`` an integer tensor within [1, 254]."""
    return (byte.to(torch.int32) << 23).view(torch.float32)


def quantize_weight_mxfp4(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """bf16 ``w [N, K]`` -> (``codes`` uint8 ``[N, K/2]``, ``scales`` uint8 ``[N, K/32]``); module docstring."""
    if w.dtype != torch.bfloat16 or w.dim() != 2 or not w.is_contiguous():
        raise ValueError(f"quantize_weight_mxfp4: needs a contiguous bf16 [N, K] weight, got {w.dtype} "
                         f"{tuple(w.shape)} with strides {w.stride()}")
    N, K = w.shape
    if not supported(1, N, K):
        raise ValueError(f"quantize_weight_mxfp4: N = {N}, K = {K} is not supported (K a multiple of {K_MULTIPLE}, "
                         f"N a multiple of {N_MULTIPLE})")
    wf = w.float().view(N, K // BLOCK, BLOCK)
    amax = wf.abs().amax(dim=-1)
    m, ex = torch.frexp(amax)
    byte = (ex - torch.where(m <= 0.75, 3, 2) + 127).clamp(SCALE_BYTE_MIN, SCALE_BYTE_MAX)
    byte = torch.where(amax == 0, torch.full_like(byte, SCALE_BYTE_ZERO), byte)
    a = wf.abs() * _pow2(254 - byte)[..., None]  # |w| / 2^X, exact
    # nearest E2M1 magnitude; the midpoints 0.75, 1.75 and 3.5 go up and 0.25, 1.25, 2.5 and 5 down, to the even code
    mag = ((a > 0.25).to(torch.uint8) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) + (a >= 3.5) + (a > 5.0))
    c = (mag | (torch.signbit(wf).to(torch.uint8) << 3)).view(N, K // 2, 2)
    return (c[..., 0] | (c[..., 1] << 4)).contiguous(), byte.to(torch.uint8)


def dequantize_mxfp4(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """(``codes [N, K/2]``, ``scales [N, K/32]``) -> the bf16 ``[N, K]`` they stand for, exactly."""
    if codes.dtype != torch.uint8 or scales.dtype != torch.uint8 or codes.dim() != 2 or scales.dim() != 2:
        raise ValueError(f"dequantize_mxfp4: needs uint8 codes [N, K/2] and scales [N, K/32], got {codes.dtype} "
                         f"{tuple(codes.shape)} and {scales.dtype} {tuple(scales.shape)}")
    N, K = codes.shape[0], 2 * codes.shape[1]
    if scales.shape != (N, K // BLOCK) or K % BLOCK:
        raise ValueError(f"dequantize_mxfp4: codes {tuple(codes.shape)} need scales [{N}, {K // BLOCK}], got "
                         f"{tuple(scales.shape)}")
    lut = torch.tensor(E2M1 + tuple(-v for v in E2M1), device=codes.device)
    v = lut[torch.stack((codes & 15, codes >> 4), dim=-1).long()].view(N, K // BLOCK, BLOCK)
    return (v * _pow2(scales)[..., None]).view(N, K).to(torch.bfloat16)


def _check(x: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor, what: str) -> None:
    if x.dtype != torch.bfloat16 or codes.dtype != torch.uint8 or scales.dtype != torch.uint8:
        raise ValueError(f"{what}: needs bf16 x and uint8 codes and scales, got {x.dtype}, {codes.dtype} and "
                         f"{scales.dtype}")
    if x.dim() != 2 or codes.dim() != 2 or scales.dim() != 2:
        raise ValueError(f"{what}: needs x [M, K], codes [N, K/2] and scales [N, K/32], got {tuple(x.shape)}, "
                         f"{tuple(codes.shape)} and {tuple(scales.shape)}")
    if not x.is_contiguous() or not codes.is_contiguous() or not scales.is_contiguous():
        raise ValueError(f"{what}: x, codes and scales must be contiguous (strides {x.stride()}, {codes.stride()} "
                         f"and {scales.stride()})")
    if x.data_ptr() % 16 or codes.data_ptr() % 16 or scales.data_ptr() % 2:
        raise ValueError(f"{what}: x and codes must start on a 16-byte boundary, scales on a 2-byte one")
    if x.device != codes.device or x.device != scales.device:
        raise ValueError(f"{what}: x is on {x.device}, codes on {codes.device}, scales on {scales.device}")
    M, K = x.shape
    N = codes.shape[0]
    if codes.shape[1] * 2 != K or scales.shape != (N, K // BLOCK):
        raise ValueError(f"{what}: x has K = {K}: codes must be [N, {K // 2}] and scales [N, {K // BLOCK}], got "
                         f"{tuple(codes.shape)} and {tuple(scales.shape)}")
    if not supported_mxfp4(M, N, K):
        raise ValueError(f"{what}: M = {M}, N = {N}, K = {K} is not supported (1 <= M <= {MAX_ROWS}, "
                         f"K a multiple of {K_MULTIPLE}, N a multiple of {N_MULTIPLE})")


def _tiles(tiles, ncols: int, what: str) -> int:
    if tiles is None:
        return pick_tiles_mxfp4(ncols)
    if tiles not in TILES:
        raise ValueError(f"{what}: tiles must be 1, 2 or 4, got {tiles}")
    return int(tiles)


def decode_linear_mxfp4_reference(x: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor,
                                  out_dtype=torch.bfloat16) -> torch.Tensor:
    return (x.float() @ dequantize_mxfp4(codes, scales).float().t()).to(out_dtype)


def decode_gate_up_swiglu_mxfp4_reference(x: torch.Tensor, codes13: torch.Tensor, scales13: torch.Tensor) -> torch.Tensor:
    """``silu(g) * u`` from the f32 products, rounded to bf16 once."""
    g, u = (x.float() @ dequantize_mxfp4(codes13, scales13).float().t()).chunk(2, dim=-1)
    return (Fn.silu(g) * u).to(x.dtype)


def decode_linear_mxfp4(x: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor, out_dtype=torch.bfloat16,
                        tiles: int | None = None) -> torch.Tensor:
    """``x [M, K] @ dequant(codes, scales) [N, K].T -> [M, N]`` in ``out_dtype`` (bf16 or f32).  ``tiles``
    overrides ``pick_tiles_mxfp4`` (tests, measurements)."""
    if out_dtype not in _MODE:
        raise ValueError(f"decode_linear_mxfp4: out_dtype must be bfloat16 or float32, got {out_dtype}")
    _check(x, codes, scales, "decode_linear_mxfp4")
    M, K = x.shape
    N = codes.shape[0]
    tiles = _tiles(tiles, N, "decode_linear_mxfp4")
    if not x.is_cuda:
        return decode_linear_mxfp4_reference(x, codes, scales, out_dtype)
    y = torch.empty((M, N), device=x.device, dtype=out_dtype)
    _lib.call("th_decode_linear_mxfp4", x.data_ptr(), codes.data_ptr(), scales.data_ptr(), y.data_ptr(), M, N, K,
              _MODE[out_dtype], tiles, _lib.stream_ptr(x.device))
    return y


def decode_gate_up_swiglu_mxfp4(x: torch.Tensor, codes13: torch.Tensor, scales13: torch.Tensor,
                                tiles: int | None = None) -> torch.Tensor:
    """``silu(x @ W[:F].T) * (x @ W[F:].T)`` as bf16 ``[M, F]`` for the packed gate|up weight ``W [2F, K]``."""
    _check(x, codes13, scales13, "decode_gate_up_swiglu_mxfp4")  # 2F a multiple of 16, as in decode_gate_up_swiglu
    M, K = x.shape
    F2 = codes13.shape[0]
    tiles = _tiles(tiles, F2 // 2, "decode_gate_up_swiglu_mxfp4")
    if not x.is_cuda:
        return decode_gate_up_swiglu_mxfp4_reference(x, codes13, scales13)
    y = torch.empty((M, F2 // 2), device=x.device, dtype=x.dtype)
    _lib.call("th_decode_linear_mxfp4", x.data_ptr(), codes13.data_ptr(), scales13.data_ptr(), y.data_ptr(), M, F2, K,
              _MODE_SWIGLU, tiles, _lib.stream_ptr(x.device))
    return y
