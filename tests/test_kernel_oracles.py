"""The fp64 oracles of ``tests/kernel_oracles.py`` against the CPU fallbacks of the op wrappers, under
the same assertion the GPU tests use -- and proof that this assertion notices small corruptions.

The corruptions: one element moved two bf16 steps, one 8-element chunk of a row zeroed, two adjacent
rows swapped, and the per-column operand rolled by one column (RMSNorm's weight vector; for the ops
without a weight the analogous slip: SwiGLU's up-projection columns, the cross-entropy target column).
"""
import types

import pytest
import torch

from tests import kernel_oracles as ko
from tests.kernel_oracles import assert_rounded_close

BF = torch.bfloat16
SCALES = [1.0, 8.0, 1.0 / 64]


def _bf(*shape, scale=1.0):
    return (torch.randn(*shape) * scale).to(BF)


def _weight(D):
    return (1 + 0.1 * torch.randn(D)).to(BF)


# ------------------------------------------------------------------------------ oracle <-> fallback
@pytest.mark.parametrize("scale", SCALES)
def test_rmsnorm_fallback_matches_oracle(scale):
    from tensorhive_fixed_amd.ops import rmsnorm as R
    torch.manual_seed(0)
    T, D, eps = 7, 136, 1e-5
    x, w = _bf(T, D, scale=scale).requires_grad_(True), _weight(D).requires_grad_(True)
    dy, dres = _bf(T, D), _bf(T, D, scale=scale)
    fwd = ko.rmsnorm_fwd_oracle(x.detach(), w.detach(), eps)
    _, y_raw, rstd = R._fwd(x.detach(), w.detach(), eps)
    assert_rounded_close(rstd, *fwd["rstd"], "cpu rmsnorm rstd")
    assert_rounded_close(y_raw, *fwd["y"], "cpu rmsnorm y")

    y = R.rmsnorm(x, w, eps)
    assert torch.equal(y, y_raw)
    y.backward(dy)
    bwd = ko.rmsnorm_bwd_oracle(dy, x.detach(), w.detach(), eps)
    assert_rounded_close(x.grad, *bwd["dx"], "cpu rmsnorm dx")
    assert_rounded_close(w.grad, *bwd["dw"], "cpu rmsnorm dw")

    x.grad = w.grad = None
    h, xr = R.rmsnorm_fork(x, w, eps)
    assert torch.equal(h, y_raw) and torch.equal(xr, x)
    torch.autograd.backward([h, xr], [dy, dres])
    bwd = ko.rmsnorm_bwd_oracle(dy, x.detach(), w.detach(), eps, dres=dres)
    assert_rounded_close(x.grad, *bwd["dx"], "cpu rmsnorm_fork dx")
    assert_rounded_close(w.grad, *bwd["dw"], "cpu rmsnorm_fork dw")


@pytest.mark.parametrize("scale", SCALES)
def test_rmsnorm_add_fork_fallback_matches_oracle(scale):
    from tensorhive_fixed_amd.ops.rmsnorm import rmsnorm_add_fork
    torch.manual_seed(1)
    T, D, eps = 5, 72, 1e-5
    y, r = _bf(T, D, scale=scale).requires_grad_(True), _bf(T, D).requires_grad_(True)
    w = _weight(D).requires_grad_(True)
    dh, dx = _bf(T, D), _bf(T, D)
    h, xsum = rmsnorm_add_fork(y, r, w, eps)
    fwd = ko.rmsnorm_fwd_oracle(y.detach(), w.detach(), eps, addend=r.detach())
    assert torch.equal(xsum, (y.detach().float() + r.detach().float()).to(BF))
    assert torch.equal(xsum, fwd["xsum"][0].to(BF))
    assert_rounded_close(h, *fwd["y"], "cpu rmsnorm_add_fork y")
    torch.autograd.backward([h, xsum], [dh, dx])
    bwd = ko.rmsnorm_bwd_oracle(dh, xsum.detach(), w.detach(), eps, dres=dx)
    assert_rounded_close(y.grad, *bwd["dx"], "cpu rmsnorm_add_fork dy")
    assert torch.equal(y.grad, r.grad)
    assert_rounded_close(w.grad, *bwd["dw"], "cpu rmsnorm_add_fork dw")


def test_rmsnorm_dw_accumulates_into_flat_gradient_on_cpu():
    from tensorhive_fixed_amd.ops.rmsnorm import rmsnorm
    torch.manual_seed(2)
    T, D, eps = 9, 40, 1e-5
    x, w, dy = _bf(T, D), _weight(D).requires_grad_(True), _bf(T, D)
    prev = _bf(D)
    w.main_grad = prev.clone()
    w.th_store = types.SimpleNamespace(accumulating=True, mark_ready=lambda p: None)
    rmsnorm(x, w, eps).backward(dy)
    bwd = ko.rmsnorm_bwd_oracle(dy, x, w.detach(), eps, dw_prev=prev)
    assert_rounded_close(w.main_grad, *bwd["dw"], "cpu rmsnorm dw accumulate")


@pytest.mark.parametrize("scale", SCALES)
def test_swiglu_fallback_matches_oracle(scale):
    from tensorhive_fixed_amd.ops.swiglu import swiglu
    torch.manual_seed(3)
    T, F = 9, 24
    gu = _bf(T, 2 * F, scale=scale)
    gu[0, :4] = torch.tensor([40.0, -40.0, 0.0, -1.28], dtype=BF)  # saturated, zero, and the dg cancellation
    gu.requires_grad_(True)
    d = _bf(T, F)
    out = swiglu(gu)
    assert_rounded_close(out, *ko.swiglu_fwd_oracle(gu.detach()), "cpu swiglu out")
    out.backward(d)
    assert_rounded_close(gu.grad, *ko.swiglu_bwd_oracle(d, gu.detach()), "cpu swiglu dgu")


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("Dh", [16, 64])
def test_rope_fallback_matches_oracle(Dh, sign):
    from tensorhive_fixed_amd.ops.rope import rope_inplace
    torch.manual_seed(4)
    B, S, Hq, Hkv, theta = 2, 11, 2, 1, 500000.0
    x = _bf(B * S, (Hq + 2 * Hkv) * Dh)
    got = rope_inplace(x.clone(), S, Hq + Hkv, Dh, theta, sign)
    ref, mag = ko.rope_oracle(x, S, Hq + Hkv, Dh, theta, sign)
    assert_rounded_close(got, ref, mag, "cpu rope")
    assert torch.equal(got[:, (Hq + Hkv) * Dh:], x[:, (Hq + Hkv) * Dh:])
    assert torch.equal(got[0], x[0]) and torch.equal(got[S], x[S])  # position 0 of each batch: angle 0


def _ce_case():
    torch.manual_seed(5)
    R, V = 8, 45
    logits = _bf(R, V, scale=3.0)
    logits[1] += 80
    logits[2, 7] += 60
    logits[3] = 1.5
    tgt = torch.tensor([0, V - 1, 7, 3, -100, -1, V, V + 3])
    return logits, tgt


def test_ce_rows_fallback_matches_oracle():
    from tensorhive_fixed_amd.ops.cross_entropy import ce_rows_
    logits, tgt = _ce_case()
    R, V = logits.shape
    for gs in (0.5, 0.0):
        o = ko.ce_oracle(logits, tgt, gs)
        lg = logits.clone()
        loss = ce_rows_(lg, tgt, gs)
        assert_rounded_close(loss, *o["loss"], "cpu ce loss")
        assert_rounded_close(lg, *o["dlogits"], "cpu ce dlogits")
        assert not loss[4:].any() and not lg[4:].any()  # ignore index, -1, V, V + 3
    # a row-strided chunk: the first V columns of a wider buffer, padding untouched
    buf = _bf(R, V + 5)
    buf[:, :V] = logits
    before = buf.clone()
    loss = ce_rows_(buf[:, :V], tgt, 0.5)
    o = ko.ce_oracle(logits, tgt, 0.5)
    assert_rounded_close(loss, *o["loss"], "cpu ce loss")
    assert_rounded_close(buf[:, :V], *o["dlogits"], "cpu ce dlogits")
    assert torch.equal(buf[:, V:], before[:, V:])


@pytest.mark.parametrize("gdtype", [BF, torch.float32])
@pytest.mark.parametrize("step", [1, 2, 1000])
def test_adamw_fallback_matches_oracle(gdtype, step):
    from tensorhive_fixed_amd.ops.adamw import adamw_flat_, grad_sumsq_
    torch.manual_seed(6)
    n = 64
    g = (torch.randn(n) * 0.3).to(gdtype)
    ns = torch.zeros(1)
    grad_sumsq_(g, ns)
    assert_rounded_close(ns, *ko.sumsq_oracle(g), "cpu sumsq")
    prev = torch.tensor([3.25])
    acc = prev.clone()
    grad_sumsq_(g, acc, accumulate=True)
    assert_rounded_close(acc, *ko.sumsq_oracle(g, prev), "cpu sumsq accumulate")
    for norm_sq, clip, wd in ((None, 1.0, 0.1), (ns, 0.0, 0.0), (ns, 1.0, 0.1), (ns, 1e6, 0.1)):
        master = torch.randn(n)
        m, v = torch.randn(n) * 0.1, (torch.randn(n) * 0.1).pow(2)
        p = torch.zeros(n, dtype=BF)
        hp = dict(lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=wd, step=step, grad_scale=0.5,
                  norm_sq=norm_sq, clip=clip)
        o = ko.adamw_oracle(master, m, v, g, **hp)
        adamw_flat_(p, master, m, v, g, **hp)
        for name, got in (("master", master), ("m", m), ("v", v), ("p", p)):
            assert_rounded_close(got, *o[name], f"cpu adamw {name}")
        assert torch.equal(p, master.to(BF))


def test_adamw_oracle_clip_branches():
    """The clip factor: absent without a norm or with clip = 0, 1 under a large clip, clip / norm otherwise."""
    torch.manual_seed(7)
    n = 16
    master, m, v = torch.randn(n), torch.zeros(n), torch.zeros(n)
    g = torch.randn(n)
    ns = g.pow(2).sum().reshape(1)
    hp = dict(lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.0, step=1)
    plain = ko.adamw_oracle(master, m, v, g, **hp)["m"][0]
    assert torch.equal(ko.adamw_oracle(master, m, v, g, norm_sq=ns, clip=0.0, **hp)["m"][0], plain)
    assert torch.equal(ko.adamw_oracle(master, m, v, g, norm_sq=ns, clip=1e6, **hp)["m"][0], plain)
    clipped = ko.adamw_oracle(master, m, v, g, norm_sq=ns, clip=1.0, **hp)["m"][0]
    assert torch.allclose(clipped, plain / ns.double().sqrt(), rtol=1e-5)


@pytest.mark.parametrize("accumulate", [False, True])
def test_embedding_fallback_matches_oracle(accumulate):
    from tensorhive_fixed_amd.ops.embedding import embedding
    torch.manual_seed(8)
    V, D = 12, 16
    tok = torch.tensor([[0, 5, 5, 5], [11, 3, 5, 3]])
    w = _bf(V, D).requires_grad_(True)
    dy = _bf(2, 4, D)
    prev = _bf(V, D) if accumulate else None
    if accumulate:
        w.main_grad = prev.clone()
        w.th_store = types.SimpleNamespace(accumulating=True, mark_ready=lambda p: None)
    embedding(tok, w).backward(dy)
    got = w.main_grad if accumulate else w.grad
    ref, mag = ko.embedding_bwd_oracle(tok.reshape(-1), dy.reshape(-1, D), V, prev)
    assert_rounded_close(got, ref, mag, "cpu embedding gw")
    absent = [i for i in range(V) if i not in (0, 3, 5, 11)]
    assert torch.equal(got[absent], prev[absent] if accumulate else torch.zeros(len(absent), D, dtype=BF))


def test_sort_tokens_keeps_equal_ids_in_position_order():
    from tensorhive_fixed_amd.ops.embedding import sort_tokens
    torch.manual_seed(9)
    ids = torch.randint(0, 7, (300,))
    s, perm = sort_tokens(ids)
    assert torch.equal(ids[perm], s) and bool((s[1:] >= s[:-1]).all())
    same = s[1:] == s[:-1]
    assert bool((perm[1:][same] > perm[:-1][same]).all())


# ------------------------------------------------------------------------------- the assertion bites
def _bump_two_bf16_steps(t, idx):
    out = t.clone()
    bits = out.view(torch.int16)
    bits[idx] += 2  # the magnitude grows by two bf16 steps, whatever the sign
    return out


def _zero_chunk(t, row, col):
    out = t.clone()
    out[row, col: col + 8] = 0
    return out


def _swap_rows(t, row):
    out = t.clone()
    out[[row, row + 1]] = out[[row + 1, row]]
    return out


def _biggest(ref):
    flat = int(ref.abs().reshape(-1).argmax())
    return flat // ref.shape[1], flat % ref.shape[1]


def _rmsnorm_fwd_case():
    from tensorhive_fixed_amd.ops.rmsnorm import rmsnorm_reference
    torch.manual_seed(10)
    x, w = _bf(6, 136), _weight(136)
    ref, mag = ko.rmsnorm_fwd_oracle(x, w, 1e-5)["y"]
    good = rmsnorm_reference(x, w, 1e-5)
    return good, ref, mag, rmsnorm_reference(x, torch.roll(w, 1), 1e-5)


def _swiglu_bwd_case():
    from tensorhive_fixed_amd.ops.swiglu import swiglu
    torch.manual_seed(11)
    gu, d = _bf(6, 2 * 72), _bf(6, 72)
    ref, mag = ko.swiglu_bwd_oracle(d, gu)

    def run(inp):
        inp = inp.clone().requires_grad_(True)
        swiglu(inp).backward(d)
        return inp.grad

    rolled = gu.clone()
    rolled[:, 72:] = torch.roll(gu[:, 72:], 1, dims=1)  # the up-projection columns slipped by one
    return run(gu), ref, mag, run(rolled)


def _ce_dlogits_case():
    from tensorhive_fixed_amd.ops.cross_entropy import ce_rows_
    torch.manual_seed(12)
    R, V = 6, 1003
    logits = _bf(R, V, scale=3.0)
    tgt = torch.randint(1, V - 1, (R,))
    ref, mag = ko.ce_oracle(logits, tgt, 0.5)["dlogits"]
    good, rolled = logits.clone(), logits.clone()
    ce_rows_(good, tgt, 0.5)
    ce_rows_(rolled, tgt + 1, 0.5)  # the one-hot column slipped by one
    return good, ref, mag, rolled


@pytest.mark.parametrize("case", [_rmsnorm_fwd_case, _swiglu_bwd_case, _ce_dlogits_case])
def test_assertion_rejects_small_corruptions(case):
    good, ref, mag, rolled = case()
    name = case.__name__
    assert assert_rounded_close(good, ref, mag, name) <= 1.0
    r, c = _biggest(ref)
    corrupted = {
        "two bf16 steps": _bump_two_bf16_steps(good, (r, c)),
        "chunk zeroed": _zero_chunk(good, r, (c // 8) * 8),
        "rows swapped": _swap_rows(good, 2),
        "operand rolled": rolled,
    }
    for what, bad in corrupted.items():
        with pytest.raises(AssertionError, match="outside the rounding bound"):
            assert_rounded_close(bad, ref, mag, f"{name} {what}")


def test_assertion_rejects_nan_and_reports_the_worst_element():
    ref = torch.tensor([[1.0, 2.0], [3.0, 4.0]], dtype=torch.float64)
    got = ref.float()
    assert assert_rounded_close(got, ref, ref.abs(), "exact f32") == 0.0
    bad = got.clone()
    bad[1, 0] = float("nan")
    with pytest.raises(AssertionError, match=r"1 of 4 elements.*worst at \(1, 0\)"):
        assert_rounded_close(bad, ref, ref.abs(), "nan f32")
    bad = got.clone()
    bad[0, 1] += 2.0 ** -18
    with pytest.raises(AssertionError, match=r"worst at \(0, 1\)"):
        assert_rounded_close(bad, ref, ref.abs(), "off f32")
