"""fp64 oracles, inputs and shapes shared by the CPU and GPU tests of ``ops/decode_linear.py``.

Nothing here calls the op: the oracles are ``x . w^T`` and ``silu(g) * u`` in float64, each with the
``mag`` that ``tests/kernel_oracles.assert_rounded_close`` scales its fp32 term by.
"""
from __future__ import annotations

import math

import torch

BF = torch.bfloat16

# (M, N, K); for the SwiGLU form N is 2F
SHAPES = [
    (1, 16, 256),       # smallest everything; a single k-tile: one k-step per wave
    (3, 48, 768),       # odd M; odd tile counts in both dims; 3 k-steps per wave
    (8, 272, 512),      # N is no multiple of any workgroup tile above 16
    (16, 32, 14336),    # full M; the longest K of the workload: the refill loop, the longest chain
    (5, 4800, 256),     # more output tiles than CUs: the grid's tail
    (2, 32, 2048),      # 8 k-steps per wave: exactly one full tile at 1 weight tile, the refill loop is skipped
    (7, 32, 2816),      # 11 k-steps per wave: full tiles and then the tail at every tile count
]
# tiles of 16 output columns per workgroup: both template instances of every form, and the wrapper's
# own choice
TILES = [1, 2, None]
WAVES = 4


def inputs(M: int, N: int, K: int, device="cpu", seed: int = 0):
    """``x ~ N(0, 1)`` and ``w ~ 0.05 N(0, 1)``, rounded to bf16; the same values on every device."""
    g = torch.Generator().manual_seed(1000 * seed + M + 17 * N + 31 * K)
    x = torch.randn(M, K, generator=g).to(BF)
    w = (0.05 * torch.randn(N, K, generator=g)).to(BF)
    return x.to(device), w.to(device)


def linear_oracle(x: torch.Tensor, w: torch.Tensor):
    xd, wd = x.double(), w.double()
    return xd @ wd.t(), xd.abs() @ wd.abs().t()


def swiglu_oracle(x: torch.Tensor, w13: torch.Tensor):
    """ref = silu(g) u;  mag = 1.1 |u| mag_g + |silu(g)| mag_u + |ref|  (1.1 bounds |silu'|)."""
    gu, mag = linear_oracle(x, w13)
    g, u = gu.chunk(2, dim=-1)
    mg, mu = mag.chunk(2, dim=-1)
    sg = g * torch.sigmoid(g)
    ref = sg * u
    return ref, 1.1 * u.abs() * mg + sg.abs() * mu + ref.abs()


def chain_length(K: int) -> int:
    """Longest chain of dependent f32 additions behind one output of ``csrc/decode_linear.hip``: each
    of the 4 waves of a workgroup owns at most ceil(K / 64 / 4) k-steps; per k-step each of its two
    accumulators takes one MFMA, counted as its 32 products added one after the other (the order
    inside the instruction is not documented, serial is the longest it can be); then one addition
    joins the two accumulators and 3 merge the waves."""
    return 32 * math.ceil(K // 64 / WAVES) + WAVES


def fp32_term(K: int, out_dtype) -> float | None:
    """``None`` (the default coefficient of ``mag`` stands) while the chain is within the default's
    256 (bf16 outputs) or 16 (f32 outputs) fp32 ulps, else chain length x 2^-24."""
    chain = chain_length(K)
    return None if chain <= (256 if out_dtype == BF else 16) else chain * 2.0 ** -24
