"""The weight-gradient GEMM (``ops/csrc/gemm_tn.hip``) bit for bit on operands whose f32 sums are exact
(``tests/gemm_oracles.py``): every loop length, split factor, whole / split / mixed grid, XCD band height and
tile count that takes another path, on the smallest outputs that reach it (1, 3 x 2 and 2 x 5 tiles, so the
XCD remap sees a count above 8 that is no multiple of 8 and bands of 2 and 8 rows end short).  Each launch goes
through ``th_gemm_tn`` with explicit ``splitk`` / ``full`` / band, a slab prefilled with NaN where the reduce
reads and a sentinel behind it, and is repeated to show the same bits.  Rounded operands go through the
element-wise rounding bound; views, special values, the host checks and the wrapper's choices follow.
``pytest -s`` prints the worst ``err / bound`` per group when the module finishes.
"""
import functools

import pytest
import torch

from tests import gemm_oracles as go
from tests import kernel_oracles as ko
from tests.kernel_oracles import assert_rounded_close

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")
SLAB_SENTINEL = -24601.0
C_SENTINEL = -19456.0  # exact in bf16
TAIL = 4096
HB = 64  # flags bit 6: the hb schedule


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from tensorhive_fixed_amd.ops import _lib
    _lib.load(build_if_missing=True)
    assert _lib.library_path().exists()
    yield
    rows = sorted((k, v) for k, v in ko.WORST.items() if k.startswith("gpu gemm_tn "))
    print("\nworst err/bound per case group")
    for k, v in rows:
        print(f"  {k[12:]:<28s} {v:.3f}")


def _tiles(M, N):
    return (M // go.TILE) * (N // go.TILE)


def _launch(a, b, out, accumulate, splitk, full, band=0):
    """One ``th_gemm_tn`` launch into ``out`` with a guarded slab; returns after the device has finished."""
    from tensorhive_fixed_amd.ops import _lib
    K, M = a.shape
    N = b.shape[1]
    needed = (_tiles(M, N) - full) * splitk * go.TILE * go.TILE
    slab = torch.empty(needed + TAIL, device=DEV, dtype=torch.float32)
    slab[:needed] = NAN  # a piece that leaves part of what the reduce reads unwritten shows as NaN
    slab[needed:] = SLAB_SENTINEL
    _lib.call("th_gemm_tn", a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0),
              M, N, K, int(accumulate), splitk, full, slab.data_ptr(), needed, HB | (band << 8),
              _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert bool((slab[needed:] == SLAB_SENTINEL).all()), "the launch wrote behind ws_floats"


def _run(a, b, prefill, accumulate, splitk, full, band=0):
    """Two identical launches (out = the prefill when accumulating, NaN otherwise); the bits must agree."""
    outs = []
    for _ in range(2):
        out = prefill.clone() if accumulate else torch.full_like(prefill, NAN)
        _launch(a, b, out, accumulate, splitk, full, band)
        outs.append(out)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "two identical launches differ"
    return outs[0]


@functools.lru_cache(maxsize=None)
def _exact(K, M, N):
    """Exact operands and their fp64 expectations, once per (geometry, K)."""
    a, b, c = go.exact_operands(K, M, N, seed=K + M + N, device=DEV)
    return a, b, c, {False: go.expected_bits(a, b, None), True: go.expected_bits(a, b, c)}


@functools.lru_cache(maxsize=None)
def _rounded(K, M, N):
    a, b, c = go.rounded_operands(K, M, N, seed=K + M + N, device=DEV)
    return a, b, c, {False: go.gemm_oracle(a, b), True: go.gemm_oracle(a, b, c)}


def _check_case(M, N, K, splitk, full, band, accumulate):
    a, b, c, want = _exact(K, M, N)
    name = f"{M}x{N}x{K} splitk {splitk} full {full} band {band} acc {accumulate}"
    go.assert_bit_exact(_run(a, b, c, accumulate, splitk, full, band), want[accumulate], name)
    out = _run(torch.zeros_like(a), b, c, accumulate, splitk, full, band)
    if accumulate:  # 0 + c = c in f32, and c is a bf16 value (no -0 among the integers)
        assert torch.equal(out.view(torch.int16), c.view(torch.int16)), name + ": a = 0 changed the prefill"
    else:
        assert bool((out.float() == 0).all()), name + ": a = 0 left a nonzero output"


# --------------------------------------------------------------------- loop lengths and split factors
LOOPS = [(768, 512, K, s, 0 if s > 1 else 6) for K, s in go.K_SPLITS] + \
        [(256, 256, K, s, 0 if s > 1 else 1) for K, s in ((64, 1), (128, 2), (192, 3), (320, 1))]


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("M,N,K,splitk,full", LOOPS)
def test_every_loop_length_and_split_factor(M, N, K, splitk, full, accumulate):
    _check_case(M, N, K, splitk, full, 0, accumulate)


# ------------------------------------------------------------------------- whole / mixed / split grids
BANDS = (0, 1, 2, 3, 15)
GRIDS = [(768, 512, f) for f in (0, 1, 3, 5)] + [(512, 1280, f) for f in (0, 2, 7, 9)]


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("M,N,full", GRIDS)
def test_mixed_grid_boundaries_and_bands(M, N, full, band, accumulate):
    _check_case(M, N, 384, 2, full, band, accumulate)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("M,N", go.GEOMETRIES)
def test_whole_tiles_per_band(M, N, band, accumulate):
    _check_case(M, N, 384, 1, _tiles(M, N), band, accumulate)


# ------------------------------------------------------------------------------------------ index probe
PROBES = [(256, 256, 1, 1), (256, 256, 2, 0), (768, 512, 1, 6), (768, 512, 2, 0), (768, 512, 2, 3),
          (512, 1280, 1, 10), (512, 1280, 2, 0), (512, 1280, 2, 7)]


@pytest.mark.parametrize("band", [0, 2])
@pytest.mark.parametrize("M,N,splitk,full", PROBES)
def test_index_probe_rows_are_rows_of_b(M, N, splitk, full, band):
    a, b, want = go.probe_operands(384, M, N, device=DEV)
    out = _run(a, b, torch.empty(M, N, device=DEV, dtype=BF), False, splitk, full, band)
    go.assert_bit_exact(out, want, f"probe {M}x{N} splitk {splitk} full {full} band {band}")


# ------------------------------------------------------------------------------------- rounded operands
ROUNDED = [("whole", 64, 1, 6), ("whole", 192, 1, 6), ("whole", 512, 1, 6), ("split", 192, 3, 0),
           ("split", 512, 8, 0), ("mixed", 512, 2, 3), ("mixed", 192, 3, 5)]


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("group,K,splitk,full", ROUNDED)
def test_rounded_operands_stay_inside_the_rounding_bound(group, K, splitk, full, accumulate):
    M, N = 768, 512
    a, b, c, refmag = _rounded(K, M, N)
    out = _run(a, b, c, accumulate, splitk, full, 2)
    # bf16 products are exact in f32; a workgroup adds K / splitk of them per output, the reduce adds splitk
    # partials, the epilogue adds C once, and each f32 addition -- rounded, or truncated inside the MFMA -- is
    # off by at most one ulp (2^-23) of a partial sum that never exceeds mag: (K / splitk + splitk + 1) 2^-23
    assert_rounded_close(out, *refmag[accumulate], f"gpu gemm_tn {group}" + (" +C" if accumulate else ""),
                         fp32_term=go.fp32_term(K, splitk))


# --------------------------------------------------------------------------------------- views and guards
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("splitk,full", [(1, 6), (2, 0), (2, 3)])
def test_views_are_respected_and_their_surroundings_untouched(splitk, full, accumulate):
    M, N, K = 768, 512, 384
    a0, b0, c0, want = _exact(K, M, N)
    A = torch.full((K + 64, M + 24), NAN, device=DEV, dtype=BF)
    B = torch.full((K + 64, N + 8), NAN, device=DEV, dtype=BF)
    C = torch.full((M + 2, N + 16), C_SENTINEL, device=DEV, dtype=BF)
    a, b, out = A[:K, 8:8 + M], B[:K, 8:8 + N], C[1:1 + M, 8:8 + N]
    a.copy_(a0)
    b.copy_(b0)
    out.copy_(c0 if accumulate else torch.full_like(c0, NAN))
    assert a.stride(0) == M + 24 and b.stride(0) == N + 8 and out.stride(0) == N + 16
    _launch(a, b, out, accumulate, splitk, full, 2)
    assert not bool(torch.isnan(out.float()).any()), "an operand element outside the view reached the output"
    go.assert_bit_exact(out.contiguous(), want[accumulate], f"views splitk {splitk} full {full}")
    outside = torch.ones_like(C, dtype=torch.bool)
    outside[1:1 + M, 8:8 + N] = False
    assert bool((C[outside] == C_SENTINEL).all()), "the launch wrote outside the out view"
    assert int(outside.sum()) == (M + 2) * (N + 16) - M * N


# ----------------------------------------------------------------------------------------- special values
@pytest.mark.parametrize("splitk,full", [(1, 6), (2, 0), (2, 3)])
def test_inf_and_nan_stay_in_their_rows(splitk, full):
    M, N, K = 768, 512, 384
    a0, b, c, want = _exact(K, M, N)
    (k1, m1), (k2, m2) = (70, 5), (300, 600)  # tile rows 0 and 2, the first and the second K half
    a = a0.clone()
    a[k1, m1], a[k2, m2] = float("inf"), NAN
    clean = _run(a0, b, c, True, splitk, full)
    out = _run(a, b, c, True, splitk, full)
    go.assert_bit_exact(out, go.expected_bits(a, b, c), f"special values splitk {splitk} full {full}")
    row1, bk = out[m1].float(), b[k1].float()
    assert bool(torch.isnan(row1[bk == 0]).all()) and int((bk == 0).sum()) > 0  # inf * 0
    assert torch.equal(row1[bk != 0], torch.sign(bk[bk != 0]) * float("inf"))
    assert bool(torch.isnan(out[m2].float()).all())
    others = torch.ones(M, dtype=torch.bool, device=DEV)
    others[[m1, m2]] = False
    assert torch.equal(out[others].view(torch.int16), clean[others].view(torch.int16))
    go.assert_bit_exact(clean, want[True], "clean run")


# -------------------------------------------------------------------------------------------- host checks
HOST_M, HOST_N, HOST_K = 768, 512, 384  # six tiles, all split two ways by default
HOST_NEEDED = 6 * 2 * go.TILE * go.TILE
HOST_CASES = {
    "M=128": dict(M=128),
    "N=384": dict(N=384),
    "K=96": dict(K=96, splitk=1, full=6),
    "K=192 splitk=2": dict(K=192),
    "lda=M-8": dict(lda=HOST_M - 8),
    "lda=M+4": dict(lda=HOST_M + 4),
    "pointer 8 bytes off": dict(a_off=8),
    "full=-1": dict(full=-1),
    "full=tiles+1": dict(full=7),
    "splitk=1 full<tiles": dict(splitk=1, full=5),
    "no workspace": dict(ws=False),
    "ws_floats one short": dict(ws_floats=HOST_NEEDED - 1),
    "flags without bit 6": dict(flags=2 << 8),
    "lda=2^24": dict(lda=1 << 24),
}


@pytest.mark.parametrize("case", list(HOST_CASES))
def test_host_checks_reject_before_any_launch(case):
    """Every one of these is refused by ``th_gemm_tn``'s argument checks, which come before the launch
    (csrc/gemm_tn.hip): the call raises the bad-shape error, and neither ``out`` nor the slab changes."""
    from tensorhive_fixed_amd.ops import _lib
    a, b, c, _ = _exact(HOST_K, HOST_M, HOST_N)
    out = c.clone()
    slab = torch.full((HOST_NEEDED + TAIL,), SLAB_SENTINEL, device=DEV, dtype=torch.float32)
    p = dict(a_off=0, lda=HOST_M, ldb=HOST_N, ldc=HOST_N, M=HOST_M, N=HOST_N, K=HOST_K, splitk=2, full=0, ws=True,
             ws_floats=HOST_NEEDED, flags=HB)
    p.update(HOST_CASES[case])
    with pytest.raises(RuntimeError, match="bad shape"):
        _lib.call("th_gemm_tn", a.data_ptr() + p["a_off"], p["lda"], b.data_ptr(), p["ldb"], out.data_ptr(), p["ldc"],
                  p["M"], p["N"], p["K"], 1, p["splitk"], p["full"], slab.data_ptr() if p["ws"] else None,
                  p["ws_floats"], p["flags"], _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), c.view(torch.int16))
    assert bool((slab == SLAB_SENTINEL).all())


# ------------------------------------------------------------------------------------------- the wrapper
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("pingpong", [9, 10])
@pytest.mark.parametrize("M,N,full10", [(768, 512, 4), (512, 1280, 8)])
def test_wrapper_mixed_and_split_launches_are_bit_exact(M, N, full10, pingpong, accumulate):
    """Under a budget of 4 CUs a forced 2-way split keeps the whole rounds of 4 tiles: 4 of 6 and 8 of 10
    whole tiles in mode 10, none in mode 9."""
    from tensorhive_fixed_amd.ops.gemm_tn import cu_budget, gemm_tn_, tn_full_for
    a, b, c, want = _exact(384, M, N)
    out = c.clone() if accumulate else torch.full_like(c, NAN)
    with cu_budget(4):
        assert tn_full_for(M, N, 2) == full10
        gemm_tn_(a, b, out, accumulate=accumulate, splitk=2, pingpong=pingpong)
    torch.cuda.synchronize()
    go.assert_bit_exact(out, want[accumulate], f"wrapper {M}x{N} mode {pingpong}")


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("kind", ["M=128", "out column-major"])
def test_wrapper_fallback_stays_inside_the_rounding_bound(kind, accumulate):
    """Calls the kernel does not tile go to ``torch``.  (``M = 128`` is an output below one tile: the default
    mode-10 call used to fail in the planner's cost model, which divides by the tile count.)"""
    from tensorhive_fixed_amd.ops.gemm_tn import gemm_tn_
    M, N, K = (128, 256, 192) if kind == "M=128" else (256, 256, 192)
    a, b, c = go.rounded_operands(K, M, N, seed=7, device=DEV)
    out = torch.empty(M, N, device=DEV, dtype=BF) if kind == "M=128" else torch.empty(N, M, device=DEV, dtype=BF).t()
    out.copy_(c)
    assert kind == "M=128" or out.stride(1) != 1
    gemm_tn_(a, b, out, accumulate=accumulate)
    torch.cuda.synchronize()
    # one f32 sum of K products plus C, as fp32_term states for splitk = 1
    assert_rounded_close(out, *go.gemm_oracle(a, b, c if accumulate else None),
                         "gpu gemm_tn fallback" + (" +C" if accumulate else ""), fp32_term=go.fp32_term(K, 1))
