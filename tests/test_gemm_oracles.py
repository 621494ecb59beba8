"""CPU checks of ``tests/gemm_oracles.py``: the exactness condition on every shape the GPU file launches, the
wrapper's CPU path and the fp32 emulation under both rules, and seven planted faults that the bit-exact rule
must catch (five of them also by the element-wise rounding bound on rounded operands) -- plus the record of
what the earlier whole-output rule ``max|err| <= 0.02 max|ref| + 1e-2`` lets through."""
import pytest
import torch

from tensorhive_fixed_amd.ops.gemm_tn import gemm_tn_
from tests import gemm_oracles as go
from tests.kernel_oracles import assert_rounded_close

BF = torch.bfloat16
K_ALL, M, N = 1536, 256, 512  # 64 * lcm(1, 2, 3, 8) k-rows; two output tiles
SPLITS = (1, 2, 3, 8)


@pytest.fixture(scope="module")
def exact():
    a, b, c = go.exact_operands(K_ALL, M, N, seed=1)
    return a, b, c, {False: go.expected_bits(a, b, None), True: go.expected_bits(a, b, c)}


@pytest.fixture(scope="module")
def rounded():
    a, b, c = go.rounded_operands(K_ALL, M, N, seed=2)
    return a, b, c, {False: go.gemm_oracle(a, b), True: go.gemm_oracle(a, b, c)}


@pytest.mark.parametrize("accumulate", [False, True])
def test_cpu_path_is_bit_exact_and_rounded_close(exact, rounded, accumulate):
    a, b, c, want = exact
    out = c.clone()
    gemm_tn_(a, b, out, accumulate=accumulate)
    go.assert_bit_exact(out, want[accumulate], "cpu path")
    a, b, c, refmag = rounded
    out = c.clone()
    gemm_tn_(a, b, out, accumulate=accumulate)
    assert_rounded_close(out, *refmag[accumulate], "cpu path", fp32_term=go.fp32_term(K_ALL, 1))


@pytest.mark.parametrize("splitk", SPLITS)
@pytest.mark.parametrize("accumulate", [False, True])
def test_emulation_is_bit_exact_and_rounded_close(exact, rounded, accumulate, splitk):
    a, b, c, want = exact
    go.assert_bit_exact(go.emulate(a, b, c, accumulate, splitk), want[accumulate], f"emulate splitk {splitk}")
    a, b, c, refmag = rounded
    assert_rounded_close(go.emulate(a, b, c, accumulate, splitk), *refmag[accumulate], f"emulate splitk {splitk}",
                         fp32_term=go.fp32_term(K_ALL, splitk))


@pytest.mark.parametrize("K,Mg,Ng", go.GPU_SHAPES)
def test_exactness_condition_on_every_gpu_shape(K, Mg, Ng):
    """``exact_operands`` asserts the condition itself; here the margin is stated too: 64 K + 300 grid steps."""
    a, b, c = go.exact_operands(K, Mg, Ng, seed=K + Mg)
    units = go.exact_units(a, b, c, *go.grid_steps(K, Mg, Ng))
    assert units <= 64 * K + 300 < go.EXACT_LIMIT
    for t in (a, b, c):
        assert t.dtype == BF and bool(torch.isfinite(t.float()).all())
    assert len(torch.unique(torch.frexp(a.float().abs().max(0).values)[1])) == 3  # three binades of columns


def test_exact_operands_cover_ties_and_rounding():
    """The bit-exact rule only bites where bf16 has to round: count the ties and the inexact outputs."""
    a, b, c = go.exact_operands(4096, 256, 256, seed=3)
    s = a.double().t() @ b.double() + c.double()
    r = s.to(BF).double()
    inexact = r != s
    ulp = 2.0 ** (torch.frexp(s.abs())[1] - 8).double()  # bf16 spacing in the binade of s
    ties = inexact & ((r - s).abs() * 2 == ulp)
    assert int(inexact.sum()) > 10000 and int(ties.sum()) > 1000
    assert int((go.expected_bits(a, b, None).double() != r).sum()) > 60000  # a lost C moves nearly everything


@pytest.mark.parametrize("K", [64, 192, 4096, 8192])
def test_f32_sums_are_exact_in_both_orders(K):
    a, b, _ = go.exact_operands(K, 256, 256, seed=K)
    want = a.double().t() @ b.double()
    af, bf = a.float(), b.float()
    for order in (range(K), range(K - 1, -1, -1)):
        acc = torch.zeros(256, 256)
        for k in order:  # strictly sequential f32 accumulation
            acc.addcmul_(af[k][:, None], bf[k][None, :])
        assert torch.equal(acc.double(), want)
    assert torch.equal((af.t() @ bf).double(), want)
    assert torch.equal((af.flip(0).t() @ bf.flip(0)).double(), want)


# ------------------------------------------------------------------------------------- planted faults
KF = 384  # two splits of three k-tiles; <= 512 for the rounding bound


def _faulty(fault, a, b, c, splitk):
    """Output of the emulation with planted fault 1-7 (accumulating: C matters to faults 2 and 4)."""
    kw = {1: dict(drop_k_row=(0, 1, 200)), 2: dict(beta_off_tile=(0, 1)), 4: dict(round_partials=True),
          6: dict(dup_k_tile=(0, 0, 4)), 7: dict(truncate=True)}.get(fault, {})
    out = go.emulate(a, b, c, True, splitk, **kw)
    if fault == 3:
        out = go.swap_tiles(out, (0, 0), (0, 1))
    if fault == 5:
        out = go.swap_col_blocks(out, (0, 1), 2, 9)
    return out


@pytest.mark.parametrize("splitk", [1, 2])
@pytest.mark.parametrize("fault", [1, 2, 3, 4, 5, 6, 7])
def test_bit_exact_rule_catches_every_planted_fault(fault, splitk):
    a, b, c = go.exact_operands(KF, M, N, seed=4)
    want = go.expected_bits(a, b, c)
    go.assert_bit_exact(go.emulate(a, b, c, True, splitk), want, "clean")
    with pytest.raises(AssertionError, match="elements differ") as e:
        go.assert_bit_exact(_faulty(fault, a, b, c, splitk), want, f"fault {fault}")
    if fault in (1, 2, 6):
        assert "confined to one tile" in str(e.value)
    if fault == 5:
        assert "confined to one tile (0, 1)" in str(e.value) and "16 x 16 block (0, 2)" in str(e.value)


@pytest.mark.parametrize("splitk", [1, 2])
@pytest.mark.parametrize("fault", [1, 2, 3, 5, 6])
def test_rounding_bound_catches_structural_faults(fault, splitk):
    a, b, c = go.rounded_operands(KF, M, N, seed=5)
    ref, mag = go.gemm_oracle(a, b, c)
    term = go.fp32_term(KF, splitk)
    assert_rounded_close(go.emulate(a, b, c, True, splitk), ref, mag, "clean", fp32_term=term)
    with pytest.raises(AssertionError, match="outside the rounding bound"):
        assert_rounded_close(_faulty(fault, a, b, c, splitk), ref, mag, f"fault {fault}", fp32_term=term)


def test_bit_exact_report_and_special_values():
    e = torch.zeros(512, 512, dtype=BF)
    g = e.clone()
    g[300, 17:40] = 1.0
    with pytest.raises(AssertionError, match=r"23 of 262144 .*first at \(300, 17\): tile \(1, 0\), 16 x 16 block "
                                             r"\(2, 1\) of it, element \(12, 1\).*one tile \(1, 0\), one row \(300\)"):
        go.assert_bit_exact(g, e, "row")
    go.assert_bit_exact(-e, e, "signed zero")  # by value
    e[5, 5], e[6, 6] = float("nan"), float("inf")
    go.assert_bit_exact(e.clone(), e, "nan and inf in place")
    for bad in (0.0, float("inf")):
        g = e.clone()
        g[5, 5] = bad
        with pytest.raises(AssertionError):
            go.assert_bit_exact(g, e, "nan lost")
    g = e.clone()
    g[6, 6] = -float("inf")
    with pytest.raises(AssertionError):
        go.assert_bit_exact(g, e, "inf sign")


def test_probe_rows_are_rows_of_b():
    for K, Mp, Np in ((64, 256, 256), (384, 768, 512)):
        a, b, want = go.probe_operands(K, Mp, Np)
        assert torch.equal(a.float().sum(0), torch.ones(Mp)) and int((a != 0).sum()) == Mp
        go.assert_bit_exact(go.emulate(a, b, None, False, 1), want, "probe")
        assert torch.equal(want[5], b[(37 * 5 + 11) % K])
        with pytest.raises(AssertionError):  # a k-row map off by one row
            go.assert_bit_exact(go.emulate(a.roll(1, 0), b, None, False, 1), want, "probe shifted")


def test_old_whole_output_rule_misses_a_lost_c():
    """The gap, as a test of the earlier rule and not of the kernel: at (M, N, K) = (768, 512, 4096), the only
    split-K accumulate case of ``test_gemm_tn_matches_fp32`` before the prefill was scaled, C ignored on one
    tile (fault 2) passes ``max|err| <= 0.02 max|ref| + 1e-2``; the element-wise bound does not let it pass,
    and neither does the old rule once the prefill is of the product's size."""
    Mo, No, Ko = 768, 512, 4096
    g = torch.Generator().manual_seed(Mo * 7 + No + Ko)
    a = torch.randn(Ko, Mo, generator=g).to(BF)
    b = torch.randn(Ko, No, generator=g).to(BF)
    c = torch.randn(Mo, No, generator=g).to(BF)
    ref = a.float().t() @ b.float() + c.float()
    out = go.emulate(a, b, c, True, 2, beta_off_tile=(1, 1))
    err = (out.float() - ref).abs().max().item()
    tol = 0.02 * ref.abs().max().item() + 1e-2
    print(f"old rule, C lost on one tile: err {err:.3f} tolerance {tol:.3f}")
    assert 1.0 < err <= tol
    with pytest.raises(AssertionError):
        assert_rounded_close(out, *go.gemm_oracle(a, b, c), "fault 2", fp32_term=go.fp32_term(Ko, 2))
    c = (c.float() * Ko ** 0.5).to(BF)
    ref = a.float().t() @ b.float() + c.float()
    out = go.emulate(a, b, c, True, 2, beta_off_tile=(1, 1))
    assert (out.float() - ref).abs().max().item() > 0.02 * ref.abs().max().item() + 1e-2
