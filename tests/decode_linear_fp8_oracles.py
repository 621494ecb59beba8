"""fp64 oracles, inputs and shapes shared by the CPU and GPU tests of ``ops/decode_linear_fp8.py``.

Nothing here calls the op under test: the oracles are ``(x . wq^T) * scale`` and ``silu(g) * u`` of the
scaled halves in float64, each with the ``mag`` that ``tests/kernel_oracles.assert_rounded_close``
scales its fp32 term by.  The inputs are those of ``tests/decode_linear_oracles.py`` with ``w``
quantized on the CPU (``quantize_weight_fp8`` is checked on its own in ``tests/test_decode_linear_fp8.py``).
"""
from __future__ import annotations

import math

import torch

from tests import decode_linear_oracles as dlo

BF = torch.bfloat16

# (M, N, K); for the SwiGLU form N is 2F.  The kernel's k-step is 128 wide, each of its 4 waves owns
# K / 128 / 4 k-steps (rounded either way), and keeps U = 8, 4 or 2 of them in flight at 1, 2 or 4
# weight tiles per workgroup (linear forms: 1 or 2; SwiGLU form: 2 or 4).
SHAPES = list(dlo.SHAPES) + [
    # dlo.SHAPES on this kernel: K = 256 gives waves 0 and 2 no k-step at all and waves 1 and 3 one
    # (tail only); K = 512 one each; K = 768 one or two; K = 2048 4 per wave: exactly one full tile at
    # U = 4, two at U = 2, tail only at U = 8; K = 2816 5 or 6 per wave: tail only at U = 8, a full tile
    # then a tail at U = 4, full tiles (and a tail on the waves with 5) at U = 2; K = 14336 28 per wave:
    # the refill loop at every U, with a tail at U = 8, the longest chain
    (2, 32, 4096),      # 8 k-steps per wave: exactly one full tile at U = 8 (the refill loop is skipped), 2 at U = 4
    (7, 32, 5632),      # 11 k-steps per wave: full tiles and then a tail at every U
    (4, 48, 8192),      # 16 k-steps per wave: the refill loop runs at every U and there is no tail at any
]
TILES = dlo.TILES
WAVES = 4
K_STEP = 128


def quantize_cpu(w: torch.Tensor):
    from tensorhive_fixed_amd.ops.decode_linear_fp8 import quantize_weight_fp8

    return quantize_weight_fp8(w.cpu().contiguous())


def inputs(M: int, N: int, K: int, device="cpu", seed: int = 0):
    """``x``, ``wq``, ``scale``: ``decode_linear_oracles.inputs`` with ``w`` quantized on the CPU; the
    same values on every device."""
    x, w = dlo.inputs(M, N, K, "cpu", seed)
    wq, scale = quantize_cpu(w)
    return x.to(device), wq.to(device), scale.to(device)


def linear_oracle(x: torch.Tensor, wq: torch.Tensor, scale: torch.Tensor):
    xd, wd, sd = x.double(), wq.double(), scale.double()
    return (xd @ wd.t()) * sd, (xd.abs() @ wd.abs().t()) * sd


def swiglu_oracle(x: torch.Tensor, w13q: torch.Tensor, scale13: torch.Tensor):
    """ref = silu(g) u;  mag = 1.1 |u| mag_g + |silu(g)| mag_u + |ref|  (1.1 bounds |silu'|), as
    ``decode_linear_oracles.swiglu_oracle``, from the scaled products."""
    gu, mag = linear_oracle(x, w13q, scale13)
    g, u = gu.chunk(2, dim=-1)
    mg, mu = mag.chunk(2, dim=-1)
    sg = g * torch.sigmoid(g)
    ref = sg * u
    return ref, 1.1 * u.abs() * mg + sg.abs() * mu + ref.abs()


def chain_length_fp8(K: int) -> int:
    """Longest chain of dependent f32 roundings behind one output of ``csrc/decode_linear_fp8.hip``:
    each of the 4 waves owns at most ceil(K / 128 / 4) k-steps; per k-step each of its two
    accumulators takes two MFMAs, each counted as its 32 products added one after the other; then one
    addition joins the two accumulators and 3 merge the waves; plus 1 for the multiplication by the
    scale."""
    return 64 * math.ceil(K // K_STEP / WAVES) + WAVES + 1


def fp32_term(K: int, out_dtype) -> float | None:
    """``None`` (the default coefficient of ``mag`` stands) while the chain is within the default's
    256 (bf16 outputs) or 16 (f32 outputs) fp32 ulps, else chain length x 2^-24."""
    chain = chain_length_fp8(K)
    return None if chain <= (256 if out_dtype == BF else 16) else chain * 2.0 ** -24
