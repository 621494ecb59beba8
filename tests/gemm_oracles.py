"""Oracles of the weight-gradient GEMM ``C (+)= Aᵀ B`` (``ops/csrc/gemm_tn.hip``): operands whose f32 sums are
exact, so the output is defined bit for bit; rounded operands with an fp64 reference for the element-wise
rounding bound of ``tests/kernel_oracles.py``; an index probe; and the kernel's arithmetic in fp32 with hooks
that plant faults.  Tensors may live on either device; nothing here imports ``tensorhive_fixed_amd.ops``.

Exactness: ``a`` and ``b`` hold integers in [-8, 8] (exact in bf16), column ``m`` of ``a`` and column ``n`` of
``b`` scaled by powers of two, ``c`` integers in [-300, 300] rounded to bf16 on the same grid.  Output (m, n)
then lives on the grid ``sa[m] sb[n]``: every product, every partial sum in any order and the sum with ``c`` is
an integer multiple of the grid step, below ``(64 K + 300)`` steps.  Below 2^24 steps all of them are f32 values,
so f32 arithmetic commits no rounding whatever the order (or the MFMA's internal one), the slab and the reduce
included, and the bf16 output is ``RNE_bf16(sum + c)``: one rounding, no tolerance.
"""
from __future__ import annotations

import torch

TILE, KTILE = 256, 64
COL_SCALES = (2.0 ** -6, 1.0, 2.0 ** 5)
ROW_SCALES = (1.0, 8.0, 1.0 / 64)  # of tests/gpu/test_streaming_paths_gpu.py, here per operand column
EXACT_LIMIT = 2 ** 24

# (K, splitk) of the GPU file's loop lengths: 1, 2, 3, 5, 16 and 64 k-tiles per workgroup
K_SPLITS = [(64, 1), (128, 2), (192, 3), (512, 8), (128, 1), (192, 1), (384, 2), (768, 4), (320, 1), (4096, 1),
            (4096, 4), (8192, 8)]
# output geometries (M, N) of the GPU file: 1 tile; 3 x 2 tiles; 2 x 5 tiles
GEOMETRIES = [(256, 256), (768, 512), (512, 1280)]
# every (K, M, N) the GPU file launches on exact operands
GPU_SHAPES = sorted({(k, 768, 512) for k, _ in K_SPLITS} | {(k, 256, 256) for k in (64, 128, 192, 320)} |
                    {(384, m, n) for m, n in GEOMETRIES})


def _cycle(values, n, phase, device):
    return torch.tensor(values, dtype=torch.float64, device=device)[(torch.arange(n, device=device) + phase) % 3]


def grid_steps(K: int, M: int, N: int, col_scales: bool = True, device="cpu"):
    """(sa [M], sb [N]) column scales of :func:`exact_operands` (all ones without ``col_scales``)."""
    if not col_scales:
        return (torch.ones(M, dtype=torch.float64, device=device), torch.ones(N, dtype=torch.float64, device=device))
    return _cycle(COL_SCALES, M, 0, device), _cycle(COL_SCALES, N, 1, device)


def exact_units(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor | None, sa: torch.Tensor, sb: torch.Tensor):
    """max over outputs of ``|a|ᵀ|b| + |c|`` in units of the element's grid step ``sa[m] sb[n]``."""
    mag = a.double().abs().t() @ b.double().abs()
    if c is not None:
        mag = mag + c.double().abs()
    return float((mag / (sa[:, None] * sb[None, :])).max())


def exact_operands(K: int, M: int, N: int, seed: int, col_scales: bool = True, device="cpu"):
    """bf16 ``a [K, M]``, ``b [K, N]``, ``c [M, N]`` whose product and sum f32 forms exactly (module docstring)."""
    g = torch.Generator().manual_seed(seed)
    sa, sb = grid_steps(K, M, N, col_scales, device)
    ai = torch.randint(-8, 9, (K, M), generator=g).to(device).double()
    bi = torch.randint(-8, 9, (K, N), generator=g).to(device).double()
    ci = torch.randint(-300, 301, (M, N), generator=g).to(device).double().to(torch.bfloat16).double()  # even > 256
    a = (ai * sa[None, :]).to(torch.bfloat16)
    b = (bi * sb[None, :]).to(torch.bfloat16)
    c = (ci * sa[:, None] * sb[None, :]).to(torch.bfloat16)
    assert torch.equal(a.double(), ai * sa[None, :]) and torch.equal(b.double(), bi * sb[None, :])
    assert torch.equal(c.double(), ci * sa[:, None] * sb[None, :])
    units = exact_units(a, b, c, sa, sb)
    assert units < EXACT_LIMIT, f"exact_operands({K}, {M}, {N}): {units} grid steps, f32 holds {EXACT_LIMIT}"
    return a, b, c


def expected_bits(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor | None) -> torch.Tensor:
    """The fp64 product (+ ``c``) rounded once to bf16."""
    s = a.double().t() @ b.double()
    if c is not None:
        s = s + c.double()
    return s.to(torch.bfloat16)


def _confinement(idx: torch.Tensor) -> str:
    rows, cols = idx[:, 0], idx[:, 1]
    tiles = torch.unique(torch.stack([rows // TILE, cols // TILE], 1), dim=0)
    parts = []
    if len(tiles) == 1:
        parts.append(f"one tile ({int(tiles[0, 0])}, {int(tiles[0, 1])})")
    if len(torch.unique(rows)) == 1:
        parts.append(f"one row ({int(rows[0])})")
    if len(torch.unique(cols // 16)) == 1:
        parts.append(f"one 16-column block (columns {int(cols[0]) // 16 * 16}..+15)")
    return ("confined to " + ", ".join(parts)) if parts else \
        f"spread over {len(tiles)} tiles, {len(torch.unique(rows))} rows"


def assert_bit_exact(got: torch.Tensor, expected: torch.Tensor, name: str) -> None:
    """``got == expected`` by value in every element (+0 equals -0), NaN exactly where ``expected`` has NaN."""
    assert got.dtype == expected.dtype == torch.bfloat16, f"{name}: dtypes {got.dtype}, {expected.dtype}"
    assert tuple(got.shape) == tuple(expected.shape), f"{name}: shape {tuple(got.shape)} vs {tuple(expected.shape)}"
    g, e = got.detach().float(), expected.detach().to(got.device).float()
    gn, en = torch.isnan(g), torch.isnan(e)
    wrong = (gn != en) | (~gn & ~en & (g != e))
    nbad = int(wrong.sum())
    if not nbad:
        return
    idx = wrong.nonzero().cpu()
    r, c = int(idx[0, 0]), int(idx[0, 1])
    raise AssertionError(
        f"{name}: {nbad} of {g.numel()} elements differ; first at ({r}, {c}): tile ({r // TILE}, {c // TILE}), "
        f"16 x 16 block ({r % TILE // 16}, {c % TILE // 16}) of it, element ({r % 16}, {c % 16}) of that: "
        f"got {g[r, c].item()!r} expected {e[r, c].item()!r}; {_confinement(idx)}")


def rounded_operands(K: int, M: int, N: int, seed: int, device="cpu"):
    """bf16 ``randn`` operands, column j of ``a`` and of ``b`` scaled by 1, 8 or 1/64, so one output tile spans
    several binades; ``c`` is of the size of the product (``sqrt(K)`` times both column scales)."""
    g = torch.Generator().manual_seed(seed)
    sa, sb = _cycle(ROW_SCALES, M, 0, "cpu").float(), _cycle(ROW_SCALES, N, 1, "cpu").float()
    a = (torch.randn(K, M, generator=g) * sa[None, :]).to(torch.bfloat16)
    b = (torch.randn(K, N, generator=g) * sb[None, :]).to(torch.bfloat16)
    c = (torch.randn(M, N, generator=g) * (K ** 0.5) * sa[:, None] * sb[None, :]).to(torch.bfloat16)
    return a.to(device), b.to(device), c.to(device)


def gemm_oracle(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor | None = None):
    """``(ref, mag)`` in fp64 for ``kernel_oracles.assert_rounded_close``: mag = |a|ᵀ|b| + |c|."""
    ad, bd = a.double(), b.double()
    ref, mag = ad.t() @ bd, ad.abs().t() @ bd.abs()
    if c is not None:
        ref, mag = ref + c.double(), mag + c.double().abs()
    return ref, mag


def fp32_term(K: int, splitk: int) -> float:
    """Coefficient of ``mag`` for the TN GEMM under ``assert_rounded_close``.  bf16 products are exact in f32.
    A workgroup adds K / splitk of them per output, each addition (inside an MFMA or between MFMAs, rounded
    or truncated) off by at most one ulp = 2^-23 of a partial sum that never exceeds ``mag``; the reduce adds
    ``splitk`` partials and the epilogue adds C once, one ulp each."""
    return (K / splitk + splitk + 1) * 2.0 ** -23


def truncate_bf16(x: torch.Tensor) -> torch.Tensor:
    """f32 -> bf16 by dropping the low 16 bits (the planted conversion fault)."""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def emulate(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor | None, beta: bool, splitk: int, *,
            drop_k_row: tuple[int, int, int] | None = None, beta_off_tile: tuple[int, int] | None = None,
            round_partials: bool = False, dup_k_tile: tuple[int, int, int] | None = None,
            truncate: bool = False) -> torch.Tensor:
    """The kernel's arithmetic in fp32: one f32 sum per K-split, the sums added in split order starting from
    zero, C added in f32 (``beta``), one rounding to bf16.  The keywords plant faults:
    ``drop_k_row = (tm, tn, k)`` leaves k-row ``k`` out of output tile (tm, tn); ``beta_off_tile = (tm, tn)``
    ignores C on that tile; ``round_partials`` rounds every split's sum to bf16 before it is added;
    ``dup_k_tile = (tm, tn, kt)`` adds the 64 rows of k-tile ``kt`` twice into tile (tm, tn); ``truncate``
    converts by truncation."""
    K, M = a.shape
    N = b.shape[1]
    assert K % (KTILE * splitk) == 0, (K, splitk)
    kper = K // splitk
    af, bf = a.float(), b.float()
    total = torch.zeros(M, N, dtype=torch.float32, device=a.device)
    for s in range(splitk):
        k0, k1 = s * kper, (s + 1) * kper
        part = af[k0:k1].t() @ bf[k0:k1]
        if drop_k_row is not None and k0 <= drop_k_row[2] < k1:
            tm, tn, k = drop_k_row
            rows, cols = slice(tm * TILE, (tm + 1) * TILE), slice(tn * TILE, (tn + 1) * TILE)
            am = af[k0:k1, rows].clone()
            am[k - k0] = 0
            part[rows, cols] = am.t() @ bf[k0:k1, cols]
        if dup_k_tile is not None and k0 <= dup_k_tile[2] * KTILE < k1:
            tm, tn, kt = dup_k_tile
            rows, cols = slice(tm * TILE, (tm + 1) * TILE), slice(tn * TILE, (tn + 1) * TILE)
            ks = slice(kt * KTILE, (kt + 1) * KTILE)
            part[rows, cols] += af[ks, rows].t() @ bf[ks, cols]
        if round_partials:
            part = part.to(torch.bfloat16).float()
        total = total + part
    if beta:
        cf = c.float().clone()
        if beta_off_tile is not None:
            tm, tn = beta_off_tile
            cf[tm * TILE:(tm + 1) * TILE, tn * TILE:(tn + 1) * TILE] = 0
        total = total + cf
    return truncate_bf16(total) if truncate else total.to(torch.bfloat16)


def swap_tiles(out: torch.Tensor, t0: tuple[int, int], t1: tuple[int, int]) -> torch.Tensor:
    """Planted fault: output tiles ``t0`` and ``t1`` exchanged."""
    o = out.clone()
    r0, c0 = slice(t0[0] * TILE, (t0[0] + 1) * TILE), slice(t0[1] * TILE, (t0[1] + 1) * TILE)
    r1, c1 = slice(t1[0] * TILE, (t1[0] + 1) * TILE), slice(t1[1] * TILE, (t1[1] + 1) * TILE)
    o[r0, c0], o[r1, c1] = out[r1, c1], out[r0, c0]
    return o


def swap_col_blocks(out: torch.Tensor, tile: tuple[int, int], j0: int, j1: int) -> torch.Tensor:
    """Planted fault: 16-column blocks ``j0`` and ``j1`` of one tile exchanged."""
    o = out.clone()
    rows = slice(tile[0] * TILE, (tile[0] + 1) * TILE)
    base = tile[1] * TILE
    o[rows, base + 16 * j0:base + 16 * j0 + 16] = out[rows, base + 16 * j1:base + 16 * j1 + 16]
    o[rows, base + 16 * j1:base + 16 * j1 + 16] = out[rows, base + 16 * j0:base + 16 * j0 + 16]
    return o


def probe_operands(K: int, M: int, N: int, device="cpu"):
    """``a`` with exactly one 1.0 per column, at k = (37 m + 11) % K, and ``b`` bf16 ``randn``; output row m is
    then b[(37 m + 11) % K] bit for bit (returned third), so a slip in the k, m or n index map shows as a
    wrong row and not as a rounding error."""
    g = torch.Generator().manual_seed(K * 31 + M + N)
    k_of_m = (37 * torch.arange(M) + 11) % K
    a = torch.zeros(K, M, dtype=torch.bfloat16)
    a[k_of_m, torch.arange(M)] = 1.0
    b = torch.randn(K, N, generator=g).to(torch.bfloat16)
    return a.to(device), b.to(device), b[k_of_m].to(device)
