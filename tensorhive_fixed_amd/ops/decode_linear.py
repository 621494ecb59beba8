"""Small-batch linear for decode steps: ``y = x @ w.T`` with at most 16 rows of ``x``.

``decode_linear(x, w, out_dtype)`` takes ``x [M, K]`` and ``w [N, K]`` (the ``[out, in]`` layout of
every ``nn.Parameter`` of the model), both contiguous bf16, and returns ``y [M, N]`` accumulated in
f32 and written as bf16 or, for the LM head, as f32 straight from the accumulator.
``decode_gate_up_swiglu(x, w13)`` takes the packed gate|up weight ``[2F, K]`` of ``ops/swiglu.py``
(gate rows first) and returns ``silu(g) * u`` as bf16 ``[M, F]``; ``g`` and ``u`` stay in f32 and are
never stored.  ``supported(M, N, K)`` is the shape rule of both: 1 <= M <= 16, K a multiple of 256,
N a multiple of 16 (N = 2F for the SwiGLU form, so F a multiple of 8).

GPU tensors run ``csrc/decode_linear.hip``, which streams ``w`` from HBM once (a missing entry point
raises, there is no ``torch.mm`` fallback here: the caller decides with ``supported``); CPU tensors
run the fp32 reference below, which the CPU tests exercise.
"""
from __future__ import annotations

import torch
import torch.nn.functional as Fn

from . import _lib

MAX_ROWS = 16
K_MULTIPLE = 256
N_MULTIPLE = 16
_MODE = {torch.bfloat16: 0, torch.float32: 1}
_MODE_SWIGLU = 2
# fewest workgroups a launch keeps when a workgroup takes two tiles of output columns: 3/4 of the 256 CUs
MIN_WORKGROUPS = 192
# (N, K) whose GEMM stays on hipBLASLt in the model: the Llama-3-8B down projection does not clear the bar
# at M = 8 reliably (24.6-24.9 us against 24.2-24.8, profiles/decode_linear/README.md); the kernel supports it
HIPBLASLT_FASTER = {(4096, 14336)}


def supported(M: int, N: int, K: int) -> bool:
    return 1 <= M <= MAX_ROWS and K >= K_MULTIPLE and K % K_MULTIPLE == 0 and N >= N_MULTIPLE and N % N_MULTIPLE == 0


def preferred(M: int, N: int, K: int) -> bool:
    """What the model's decode step dispatches on: supported, and not measured slower than hipBLASLt."""
    return supported(M, N, K) and (N, K) not in HIPBLASLT_FASTER


def pick_tiles(ncols: int) -> int:
    """Tiles of 16 output columns per workgroup, 1 or 2.  The tiles of a workgroup share its x
    fragments, so two halve the L2 traffic of x (the kernel's time grows with M through it); fewer
    workgroups than ``MIN_WORKGROUPS`` cost more than that saves.  Measured:
    profiles/decode_linear/README.md."""
    return 2 if -(-ncols // 32) >= MIN_WORKGROUPS else 1


def _check(x: torch.Tensor, w: torch.Tensor, what: str) -> None:
    if x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16:
        raise ValueError(f"{what}: needs bf16 x and w, got {x.dtype} and {w.dtype}")
    if x.dim() != 2 or w.dim() != 2:
        raise ValueError(f"{what}: needs x [M, K] and w [N, K], got {tuple(x.shape)} and {tuple(w.shape)}")
    if not x.is_contiguous() or not w.is_contiguous():
        raise ValueError(f"{what}: x and w must be contiguous (strides {x.stride()} and {w.stride()})")
    if x.data_ptr() % 16 or w.data_ptr() % 16:
        raise ValueError(f"{what}: x and w must start on a 16-byte boundary")
    if x.device != w.device:
        raise ValueError(f"{what}: x is on {x.device}, w on {w.device}")
    if x.shape[1] != w.shape[1]:
        raise ValueError(f"{what}: x has K = {x.shape[1]}, w has K = {w.shape[1]}")
    M, N, K = x.shape[0], w.shape[0], x.shape[1]
    if not supported(M, N, K):
        raise ValueError(f"{what}: M = {M}, N = {N}, K = {K} is not supported (1 <= M <= {MAX_ROWS}, "
                         f"K a multiple of {K_MULTIPLE}, N a multiple of {N_MULTIPLE})")


def _tiles(tiles, ncols: int, what: str) -> int:
    if tiles is None:
        return pick_tiles(ncols)
    if tiles not in (1, 2):
        raise ValueError(f"{what}: tiles must be 1 or 2, got {tiles}")
    return int(tiles)


def decode_linear_reference(x: torch.Tensor, w: torch.Tensor, out_dtype=torch.bfloat16) -> torch.Tensor:
    return (x.float() @ w.float().t()).to(out_dtype)


def decode_gate_up_swiglu_reference(x: torch.Tensor, w13: torch.Tensor) -> torch.Tensor:
    """``silu(g) * u`` from the f32 products, rounded to bf16 once."""
    g, u = (x.float() @ w13.float().t()).chunk(2, dim=-1)
    return (Fn.silu(g) * u).to(x.dtype)


def decode_linear(x: torch.Tensor, w: torch.Tensor, out_dtype=torch.bfloat16, tiles: int | None = None) -> torch.Tensor:
    """``x [M, K] @ w [N, K].T -> [M, N]`` in ``out_dtype`` (bf16 or f32).  ``tiles`` overrides
    ``pick_tiles`` (tests, measurements)."""
    if out_dtype not in _MODE:
        raise ValueError(f"decode_linear: out_dtype must be bfloat16 or float32, got {out_dtype}")
    _check(x, w, "decode_linear")
    M, K = x.shape
    N = w.shape[0]
    tiles = _tiles(tiles, N, "decode_linear")
    if not x.is_cuda:
        return decode_linear_reference(x, w, out_dtype)
    y = torch.empty((M, N), device=x.device, dtype=out_dtype)
    _lib.call("th_decode_linear", x.data_ptr(), w.data_ptr(), y.data_ptr(), M, N, K, _MODE[out_dtype], tiles,
              _lib.stream_ptr(x.device))
    return y


def decode_gate_up_swiglu(x: torch.Tensor, w13: torch.Tensor, tiles: int | None = None) -> torch.Tensor:
    """``silu(x @ w13[:F].T) * (x @ w13[F:].T)`` as bf16 ``[M, F]`` for the packed ``w13 [2F, K]``."""
    _check(x, w13, "decode_gate_up_swiglu")  # 2F a multiple of 16: two halves of whole 16-byte output runs
    M, K = x.shape
    F2 = w13.shape[0]
    tiles = _tiles(tiles, F2 // 2, "decode_gate_up_swiglu")
    if not x.is_cuda:
        return decode_gate_up_swiglu_reference(x, w13)
    y = torch.empty((M, F2 // 2), device=x.device, dtype=x.dtype)
    _lib.call("th_decode_linear", x.data_ptr(), w13.data_ptr(), y.data_ptr(), M, F2, K, _MODE_SWIGLU, tiles,
              _lib.stream_ptr(x.device))
    return y
