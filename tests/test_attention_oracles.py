"""The fp64 attention oracles of ``tests/attention_oracles.py`` against autograd, and the conditions
that qualify the score profiles as inputs of ``tests/gpu/test_attention_profiles_gpu.py``: which
profiles move the running max late, how large the scores get, and that the scaled operand's second
bf16 rounding alone stays within 4x the format baseline (the GPU bound is twice that).
"""
import pytest
import torch

from tests import attention_oracles as ao

CASES = [(S, Hq, Hkv, p, causal) for _, S, Hq, Hkv in ao.SHAPES for p in ao.PROFILES for causal in (True, False)]


def _id(c):
    return f"S{c[0]}-h{c[1]}x{c[2]}-{c[3]}-{'causal' if c[4] else 'full'}"


# ------------------------------------------------------------------------------- closed form <-> autograd
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("S,Hq,Hkv,profile", [(70, 4, 1, "randn"), (40, 4, 2, "ramp_up"), (33, 2, 2, "large")])
def test_closed_form_backward_equals_fp64_autograd(S, Hq, Hkv, profile, causal):
    q, k, v, do = ao.profile_inputs(S, Hq, Hkv, profile, seed=3)
    x = [t.double().requires_grad_(True) for t in (q, k, v)]
    rep = Hq // Hkv
    Q = x[0].transpose(0, 1)
    K, V = (t.transpose(0, 1).repeat_interleave(rep, 0) for t in x[1:])
    s = Q @ K.transpose(1, 2) * ao.SCALE
    if causal:
        s = s.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
    o = (torch.softmax(s, -1) @ V).transpose(0, 1)
    o.backward(do.double())
    ex = ao.exact(q, k, v, do, causal)
    for name, ref in (("o", o.detach()), ("lse", torch.logsumexp(s, -1).detach()), ("dq", x[0].grad),
                      ("dk", x[1].grad), ("dv", x[2].grad)):
        err = (ex[name] - ref).abs().max().item()
        assert err <= 1e-10, f"{name}: {err}"


def test_profile_bias_adds_a_times_b_to_the_log2_score():
    """Without the randn part the score is a_i * b_j exactly, up to the bf16 rounding of the biased k."""
    S = 256
    for p in ao.KEY_PROFILES:
        q, k, _, _ = ao.profile_inputs(S, 1, 1, p, seed=0, sigma=0.0)
        want = ao.row_gain(p, S)[:, None] * ao.key_bias(p, S)[None, :]
        got = ao.scores_log2(q, k, causal=False)[0]
        assert (got - want).abs().max().item() <= 2.0 ** -8 * want.abs().max().item() + 1e-12, p


def test_format_baseline_rounds_only_where_the_format_forces_it():
    """Outputs are bf16 values, lse is untouched, and the errors are a few bf16 steps of the outputs."""
    c = ao.case(256, 4, 1, "randn", True)
    base = ao.format_baseline(c["q"], c["k"], c["v"], c["do"], True)
    assert torch.equal(base["lse"], c["exact"]["lse"])
    for n in ao.TENSORS:
        assert torch.equal(base[n], base[n].to(ao.BF).double())
        peak = c["exact"][n].abs().max().item()
        assert 2.0 ** -10 * peak <= c["E_b"][n] <= 2.0 ** -5 * peak, (n, c["E_b"][n], peak)


# ------------------------------------------------------------------------------------- late rescales
def test_late_rescales_counts_a_hand_made_walk():
    """Tile maxima 0, 9, 13, 18: visits 1 (9 > 8) and 3 (18 - 9 > 8) fire, visit 2 (13 - 9) does not."""
    s = torch.full((32, 256), -30.0, dtype=torch.float64)
    for t, top in enumerate((0.0, 9.0, 13.0, 18.0)):
        s[:, 64 * t + 5] = top
    assert ao.late_rescales(s, causal=False) == (2, 3)
    # one row of the block is enough: visit 2 fires for row 7 and every row takes its running max
    # (13), so visit 3 (18 - 13) no longer does
    s[7, 64 * 2 + 9] = 17.5
    assert ao.late_rescales(s, causal=False) == (2, 3)
    s[:, 64 * 3 + 5] = 22.0
    assert ao.late_rescales(s, causal=False) == (3, 3)
    s[7, 64 * 2 + 9] = -30.0
    s[:, 64 * 3 + 5] = 17.0  # exactly the threshold above 9: deferred
    assert ao.late_rescales(s, causal=False) == (1, 3)
    # causal: 64 rows = two blocks that see one and one tile -> no visit after tile 0
    assert ao.late_rescales(torch.zeros(64, 64, dtype=torch.float64), causal=True) == (0, 0)
    assert ao.late_rescales(torch.zeros(256, 256, dtype=torch.float64), causal=True) == (0, 12)


@pytest.mark.parametrize("S,Hq,Hkv", [(256, 4, 1), (320, 2, 2)])
def test_only_the_moving_profiles_rescale_after_the_first_tile(S, Hq, Hkv):
    for p in ao.PROFILES:
        c = ao.case(S, Hq, Hkv, p, True)
        fired, visits = ao.late_rescales(c["s_log2"][0], causal=True)
        print(f"S={S} {p}: {fired} of {visits} visits after tile 0 rescale")
        if p in ao.STILL:
            assert fired == 0, (p, fired)
        if p in ao.MOVING:
            assert fired >= 4, (p, fired)


# ------------------------------------------------------------------ what justifies the GPU margins
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_profiles_qualify_for_the_gpu_margin(c):
    S, Hq, Hkv, profile, causal = c
    k = ao.case(*c)
    s = k["s_log2"]
    peak = s[torch.isfinite(s)].abs().max().item()
    ratios = {n: k["E_m"][n] / k["E_b"][n] for n in ao.TENSORS}
    print(f"max |score| {peak:.1f} log2 units;  E_m / E_b " + "  ".join(f"{n} {r:.2f}" for n, r in ratios.items()))
    assert all(k["E_b"][n] > 0 for n in ao.TENSORS) and k["E_b"]["lse"] == 0.0
    if profile == "large":
        assert peak > 50
        return
    assert peak <= 26, peak
    for n, r in ratios.items():
        assert r <= 4, f"{n}: operand rounding alone is {r:.2f} x the format baseline"


def test_large_scores_break_the_k_side_rowsum():
    """The dK|dV kernels' P (K-side operand rounding, Q-side lse) does not sum to 1; the miss grows
    with |score|: a few 1e-3 for randn, a few 1e-2 at +-58 log2 units."""
    small = ao.case(256, 4, 1, "randn", True)["model_rowsum_k"]
    large = ao.case(256, 4, 1, "large", True)["model_rowsum_k"]
    d_small, d_large = (small - 1).abs().max().item(), (large - 1).abs().max().item()
    print(f"max |rowsum(P) - 1|: randn {d_small:.4f}  large {d_large:.4f}")
    assert d_small < 0.01 < 0.03 < d_large < 0.2


def test_lse_tolerance_is_raised_only_where_the_operand_model_needs_it():
    """``2e-3 + 2**-9 * |score|_max`` is not met by the operand model itself on causal rows of ``large``
    that see few keys (the rounding error of a score scales with sum |q_d k_d|, not with the score), so
    the tolerance takes the model's own per-row error where that is larger -- and nowhere else."""
    worst = {}
    for c in CASES:
        k = ao.case(*c)
        first_form = k["lse_tol_plain"]
        smax = (first_form - 2e-3) * 2.0 ** 9
        err = (k["model_lse"] - k["exact"]["lse"]).abs()
        worst[c] = (err / first_form).max().item()
        assert bool((k["lse_tol"] >= first_form).all())
        raised = k["lse_tol"] > first_form
        assert torch.equal(k["lse_tol"][raised], 2e-3 + err[raised])
        assert bool((err[raised] > 2.0 ** -9 * smax[raised]).all())
    assert worst[(256, 4, 1, "large", True)] > 2, worst[(256, 4, 1, "large", True)]
    # the rounding bound proper: |d score| <= 2**-9 * scale * sum_d |q_d k_d| and lse is 1-Lipschitz in max norm
    k = ao.case(256, 4, 1, "large", True)
    q, kk = k["q"].double().transpose(0, 1), k["k"].double().transpose(0, 1)
    absdot = ao.SCALE * (q.abs() @ kk.abs().transpose(1, 2).repeat_interleave(4, 0))
    absdot = absdot.masked_fill(~torch.isfinite(k["s_log2"]), 0.0).amax(-1)
    assert bool(((k["model_lse"] - k["exact"]["lse"]).abs() <= 2.0 ** -9 * absdot * (1 + 1e-3)).all())


def test_block_max_abs_localises_one_bad_block():
    ref = torch.zeros(200, 3, ao.D, dtype=torch.float64)
    got = ref.clone()
    got[199, 1, 5] = 0.25
    got[32, 2, 0] = -0.5
    e = ao.block_max_abs(got, ref)
    assert e.shape == (7, 3) and e[6, 1] == 0.25 and e[1, 2] == 0.5 and e.sum() == 0.75


# ------------------------------------------------------------------------------------- tail lengths
TAIL_CASES = [(S, p, causal) for S in ao.TAIL_LENGTHS for p in ao.TAIL_PROFILES for causal in (True, False)]


@pytest.mark.parametrize("S,profile,causal", TAIL_CASES,
                         ids=[f"S{S}-{p}-{'causal' if c else 'full'}" for S, p, c in TAIL_CASES])
def test_tail_lengths_qualify_for_the_gpu_margin(S, profile, causal):
    """Every (length, profile, mask) of tests/gpu/test_flash_tails_gpu.py, at the seed of TAIL_SEEDS."""
    c = ao.tail_case(S, profile, causal)
    print("E_m / E_b " + "  ".join(f"{n} {c['E_m'][n] / c['E_b'][n]:.2f}" for n in ao.TENSORS if c["E_b"][n] > 0))
    assert ao.tail_misses(c, S, profile, causal) == []
    walks = [ao.late_rescales(c["s_log2"][h], causal) for h in range(ao.TAIL_HEADS[0])]
    if profile == "randn":
        assert all(fired == 0 for fired, _ in walks), walks
    elif ao.ramp_must_rescale(S):
        assert all(fired >= 1 for fired, _ in walks), walks
    else:  # one tile, or S = 65: the ramp cannot rise by the threshold past tile 0
        assert all(fired == 0 for fired, _ in walks), walks


def test_tail_seeds_are_the_first_that_qualify():
    for p in ao.TAIL_PROFILES:
        assert ao.TAIL_SEEDS[p] == {S: ao.first_tail_seed(S, p) for S in ao.TAIL_LENGTHS}, p
    assert [S for S in ao.TAIL_LENGTHS if S > ao.TILE_KEYS and not ao.ramp_must_rescale(S)] == [65]


def test_one_row_is_exact_and_its_cancellation_bounds_hold_for_an_f32_walk():
    """S = 1: o = v, dq = dk = 0 exactly; dP and delta summed in f32 in two different orders differ by less
    than the bound on |dS| that ``single_row_bounds`` starts from."""
    for p in ao.TAIL_PROFILES:
        c = ao.tail_case(1, p, True)
        q, k, v, do = (c[n] for n in ("q", "k", "v", "do"))
        assert torch.equal(c["exact"]["o"], v.double().repeat_interleave(2, 1))
        assert c["exact"]["dq"].abs().max() == 0 and c["exact"]["dk"].abs().max() == 0
        if p == "randn":
            assert 7e-3 < c["E_b"]["dv"] < 9e-3, c["E_b"]["dv"]  # half a bf16 step of |dO| in [2, 4)
        dq_b, dk_b = ao.single_row_bounds(q, k, v, do)
        assert dq_b.shape == (1, 4, ao.D) and dk_b.shape == (1, 2, ao.D) and bool((dq_b > 0).all())
        prod = (do.float() * v.float().repeat_interleave(2, 1))[0]  # [Hq, D]
        fwd, rev = torch.zeros(4), torch.zeros(4)
        for d in range(ao.D):
            fwd, rev = fwd + prod[:, d], rev + prod[:, ao.D - 1 - d]
        ds_bound = 2 * ao.D * 2.0 ** -24 * prod.double().abs().sum(-1)
        assert bool(((fwd - rev).double().abs() <= ds_bound).all())
        want = ds_bound[:, None] * ao.SCALE * k.double().repeat_interleave(2, 1)[0].abs() * (1 + 2.0 ** -8)
        assert torch.allclose(dq_b[0], want, rtol=1e-12, atol=0)


def test_rope_grad_map_is_the_rotary_backward_before_one_rounding():
    """``grad_map=rope_backward(S)``: exact dq / dk are those of the plain solve turned by rope_oracle's
    angles (sign -1), dv and o are untouched, and the baseline rounds the rotated value once."""
    from tests import kernel_oracles as ko

    S, causal = 33, True
    c = ao.tail_case(S, "randn", causal)
    q, k, v, do = (c[n] for n in ("q", "k", "v", "do"))
    turn = ao.rope_backward(S)
    ex = ao.exact(q, k, v, do, causal, grad_map=turn)
    packed = torch.cat([c["exact"]["dq"].reshape(S, -1), c["exact"]["dk"].reshape(S, -1)], 1)
    want, _ = ko.rope_oracle(packed, S, 6, ao.D, ao.ROPE_THETA, -1.0)
    got = torch.cat([ex["dq"].reshape(S, -1), ex["dk"].reshape(S, -1)], 1)
    assert (got - want).abs().max().item() <= 1e-12
    assert torch.equal(ex["dv"], c["exact"]["dv"]) and torch.equal(ex["o"], c["exact"]["o"])
    base = ao.format_baseline(q, k, v, do, causal, grad_map=turn)
    for n in ("dq", "dk"):  # one rounding, of the rotated value: a bf16 within half a step of it
        assert torch.equal(base[n], base[n].to(ao.BF).double())
        assert 0 < (base[n] - ex[n]).abs().max().item() <= 2.0 ** -5 * ex[n].abs().max().item()
    assert torch.equal(base["dv"], ao.format_baseline(q, k, v, do, causal)["dv"])
