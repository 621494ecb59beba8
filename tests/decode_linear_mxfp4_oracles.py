"""Inputs, shapes and the chain length shared by the CPU and GPU tests of ``ops/decode_linear_mxfp4.py``.
The fp64 oracles are those of ``tests/decode_linear_oracles.py`` on the dequantized weight.  The inputs are its
inputs with every 32-block of ``w`` times its own power of two from 2^-8..2^8 (a scale taken from the next
block or row shows), quantized on the CPU (the quantizer has its own test)."""
from __future__ import annotations

import functools
import math

import torch

from tests import decode_linear_oracles as dlo

BF = torch.bfloat16

# (M, N, K); for the SwiGLU form N is 2F.  The kernel's k-step is 256 wide, wave w of 4 owns the k-steps
# [S w / 4, S (w + 1) / 4) of S = K / 256, and keeps U = 4, 4, 2 or 1 of them in flight at 1, 2, 4 or 8
# weight tiles per workgroup (linear forms: 1, 2, 4; SwiGLU form: 2, 4, 8).  k-steps per wave:
#   K = 256: 0, 0, 0, 1 (three waves with none); 512: 0, 1, 0, 1; 768: 0, 1, 1, 1: tail only for U > 1;
#   2048: 2 each: exactly one full tile at U = 2, tail only at U = 4;  2816: 2, 3, 3, 3: full + tail at U = 2;
#   4096: 4 each: exactly one full tile at U = 4 (the refill loop is skipped), two at U = 2;
#   5632: 5, 6, 5, 6: a full tile then a tail at U = 4, full tiles with and without a tail at U = 2;
#   8192: 8 each: the refill loop runs at every U and no U leaves a tail;
#   14336: 14 each: three full tiles and a tail of 2 at U = 4, the longest chain.  U = 1 never has a tail.
SHAPES = list(dlo.SHAPES) + [(2, 32, 4096), (7, 32, 5632), (4, 48, 8192)]
TILES = [1, 2, 4, None]  # every template instance of every form, and the wrapper's own choice


@functools.lru_cache(maxsize=None)
def case(M: int, N: int, K: int):
    """CPU ``x``, ``codes``, ``scales``, the dequantized bf16 weight and both fp64 oracles, computed once."""
    from tensorhive_fixed_amd.ops.decode_linear_mxfp4 import dequantize_mxfp4, quantize_weight_mxfp4

    x, w = dlo.inputs(M, N, K)
    g = torch.Generator().manual_seed(N + K)
    e = torch.randint(-8, 9, (N, K // 32, 1), generator=g)
    w = torch.ldexp(w.float().view(N, K // 32, 32), e).view(N, K).to(BF)
    codes, scales = quantize_weight_mxfp4(w)
    deq = dequantize_mxfp4(codes, scales)
    return x, codes, scales, w, deq, dlo.linear_oracle(x, deq), dlo.swiglu_oracle(x, deq)


def fp32_term(K: int, out_dtype) -> float | None:
    """Longest chain of dependent f32 additions behind one output of ``csrc/decode_linear_mxfp4.hip``: a
    wave owns at most ceil(K / 256 / 4) k-steps; per k-step each of its two accumulators takes four MFMAs,
    each counted as its 32 products added one after the other; then one addition joins the two and 3 merge
    the waves.  ``None`` (the default coefficient stands) while that is within the default's 256 (bf16
    outputs) or 16 (f32 outputs) fp32 ulps, else chain length x 2^-24."""
    chain = 128 * math.ceil(K // 256 / 4) + 4
    return None if chain <= (256 if out_dtype == BF else 16) else chain * 2.0 ** -24
