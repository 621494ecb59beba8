"""Loop, tail and accumulate paths of the streaming kernels (RMSNorm, SwiGLU, RoPE, cross-entropy, AdamW
and its norm, embedding backward, transpose) against the fp64 oracles of ``tests/kernel_oracles.py``,
element by element under ``assert_rounded_close``; what is exactly defined is compared bit for bit.

Every shape is the smallest that still reaches its path: more rows than the launch cap so a workgroup
loops (RMSNorm backward 512, SwiGLU 4096 rows), more work than one grid pass (RoPE 524,288 chunks, AdamW
and the norm 4,194,304 elements), rows with a vector body and a scalar tail (cross-entropy), every
``MAXV`` instantiation and the first shape each rejects.  Inputs mix the scales 1, 8 and 1/64 row by row
so one case spans several binades.  All tests run in one process; ``pytest -s`` prints the worst
``err / bound`` per kernel output when the module finishes.
"""
import pytest
import torch

from tests import kernel_oracles as ko
from tests.kernel_oracles import assert_rounded_close

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
EPS = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from tensorhive_fixed_amd.ops import _lib
    _lib.load(build_if_missing=True)
    assert _lib.library_path().exists()
    yield
    rows = sorted((k, v) for k, v in ko.WORST.items() if k.startswith("gpu "))
    print("\nworst err/bound per kernel output")
    for k, v in rows:
        print(f"  {k[4:]:<28s} {v:.3f}")


def _call(name, *args):
    from tensorhive_fixed_amd.ops import _lib
    _lib.call(name, *args, _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()


def _scales(n, phase=0):
    return torch.tensor([1.0, 8.0, 1.0 / 64], device=DEV)[(torch.arange(n, device=DEV) + phase) % 3]


def _rows(T, D, phase=0):
    """bf16 [T, D] normal values, row t scaled by 1, 8 or 1/64."""
    return (torch.randn(T, D, device=DEV) * _scales(T, phase)[:, None]).to(BF)


def _weight(D):
    return (1 + 0.1 * torch.randn(D, device=DEV)).to(BF)


def _check(got, refmag, name, **kw):
    return assert_rounded_close(got, refmag[0], refmag[1], "gpu " + name, **kw)


# ----------------------------------------------------------------------------------------- RMSNorm
# D: one lane (8), a partial pass (136), each MAXV instantiation's last and next-first width
# (4096 | 4104, 8192 | 8200) and the widest supported (16384).  T: one row, and more rows than 512.
RMS_FWD = [(3, D) for D in (8, 136, 4096, 4104, 8192, 8200, 16384)] + [(T, 136) for T in (1, 513, 1100)]


@pytest.mark.parametrize("T,D", RMS_FWD)
def test_rmsnorm_forward_fork_add_fork(T, D):
    from tensorhive_fixed_amd.ops import rmsnorm as R
    torch.manual_seed(100 + D + T)
    x, r, w = _rows(T, D), _rows(T, D, 1), _weight(D)
    o = ko.rmsnorm_fwd_oracle(x, w, EPS)
    _, y, rstd = R._fwd(x, w, EPS)
    _check(y, o["y"], "rmsnorm y")
    _check(rstd, o["rstd"], "rmsnorm rstd")
    h, xr = R.rmsnorm_fork(x, w, EPS)
    assert torch.equal(h, y) and xr.data_ptr() == x.data_ptr()

    o = ko.rmsnorm_fwd_oracle(x, w, EPS, addend=r)
    xsum, h, rstd = R._fwd_add(x, r, w, EPS)
    assert torch.equal(xsum, (x.float() + r.float()).to(BF))
    assert torch.equal(xsum, o["xsum"][0].to(BF))
    _check(h, o["y"], "rmsnorm_add y")
    _check(rstd, o["rstd"], "rmsnorm_add rstd")
    h2, x2 = R.rmsnorm_add_fork(x, r, w, EPS)
    assert torch.equal(h2, h) and torch.equal(x2, xsum)


# 512 workgroups: T 513 and 520 give 1-2 rows per workgroup, T 1100 gives 2-3 (uneven both times)
RMS_BWD = [(T, D) for T in (513, 1100) for D in (136, 4096)] + [(520, 8200)]


@pytest.mark.parametrize("with_dres", [False, True])
@pytest.mark.parametrize("T,D", RMS_BWD)
def test_rmsnorm_backward_row_loop(T, D, with_dres):
    from tensorhive_fixed_amd.ops import rmsnorm as R
    torch.manual_seed(200 + D + T)
    x, dy, w = _rows(T, D), _rows(T, D, 1), _weight(D)
    dres = _rows(T, D, 2) if with_dres else None
    x2, _, rstd = R._fwd(x, w, EPS)
    dx, dw = R._bwd(x2, w, rstd, dy, dres, x.shape)
    o = ko.rmsnorm_bwd_oracle(dy, x, w, EPS, dres=dres)
    _check(dx, o["dx"], "rmsnorm dx+dres" if with_dres else "rmsnorm dx")
    _check(dw, o["dw"], "rmsnorm dw")
    dx2, dw2 = R._bwd(x2, w, rstd, dy, dres, x.shape)
    assert torch.equal(dx2, dx) and torch.equal(dw2, dw)  # no atomics: same bits


@pytest.mark.parametrize("T,D,nblk", [(1100, 136, 512), (513, 4096, 512), (40, 4104, 7)])
def test_rmsnorm_dw_accumulates_into_prefilled_vector(T, D, nblk):
    from tensorhive_fixed_amd.ops import rmsnorm as R
    torch.manual_seed(300 + D)
    x, dy, w = _rows(T, D), _rows(T, D, 1), _weight(D)
    _, _, rstd = R._fwd(x, w, EPS)
    prev = (torch.randn(D, device=DEV) * 4).to(BF)
    dw, dx = prev.clone(), torch.empty_like(x)
    ws = torch.empty(nblk * D, device=DEV, dtype=torch.float32)
    _call("th_rmsnorm_bwd", dy.data_ptr(), x.data_ptr(), w.data_ptr(), rstd.data_ptr(), dx.data_ptr(), dw.data_ptr(),
          ws.data_ptr(), nblk, T, D, 1, None)
    o = ko.rmsnorm_bwd_oracle(dy, x, w, EPS, dw_prev=prev)
    _check(dx, o["dx"], "rmsnorm dx")
    _check(dw, o["dw"], "rmsnorm dw accumulate")


def test_rmsnorm_rejects_rows_wider_than_16384():
    T, D = 3, 16392
    torch.manual_seed(4)
    x, r, w = _rows(T, D), _rows(T, D, 1), _weight(D)
    y, xsum, dx = (torch.full((T, D), 3.0, device=DEV, dtype=BF) for _ in range(3))
    rstd = torch.full((T,), 3.0, device=DEV)
    dw = torch.full((D,), 3.0, device=DEV, dtype=BF)
    ws = torch.full((T * D,), 3.0, device=DEV)
    with pytest.raises(RuntimeError, match="bad shape"):
        _call("th_rmsnorm_fwd", x.data_ptr(), w.data_ptr(), y.data_ptr(), rstd.data_ptr(), T, D, EPS)
    with pytest.raises(RuntimeError, match="bad shape"):
        _call("th_rmsnorm_add_fwd", x.data_ptr(), r.data_ptr(), w.data_ptr(), xsum.data_ptr(), y.data_ptr(),
              rstd.data_ptr(), T, D, EPS)
    with pytest.raises(RuntimeError, match="bad shape"):
        _call("th_rmsnorm_bwd", r.data_ptr(), x.data_ptr(), w.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
              dw.data_ptr(), ws.data_ptr(), T, T, D, 0, None)
    torch.cuda.synchronize()
    for out in (y, xsum, dx, rstd, dw, ws):
        assert bool((out == 3.0).all())


# ------------------------------------------------------------------------------------------ SwiGLU
def _gate_up(T, F):
    gu = _rows(T, 2 * F)
    gu[:, 0] = torch.tensor([40.0, -40.0, 0.0], device=DEV).to(BF)[torch.arange(T, device=DEV) % 3]  # gate column 0
    gu[T - 1, F - 1] = 40.0
    gu[T - 1, F - 2] = -40.0
    return gu


@pytest.mark.parametrize("T,F", [(4133, 72), (8200, 8)])  # more rows than the 4096 workgroups: 1-2 and 2-3 each
def test_swiglu_row_loop(T, F):
    from tensorhive_fixed_amd.ops.swiglu import swiglu
    torch.manual_seed(400 + F)
    gu = _gate_up(T, F).requires_grad_(True)
    d = _rows(T, F, 1)
    out = swiglu(gu)
    _check(out, ko.swiglu_fwd_oracle(gu.detach()), "swiglu out")
    out.backward(d)
    _check(gu.grad, ko.swiglu_bwd_oracle(d, gu.detach()), "swiglu dgu")


@pytest.mark.parametrize("T,F", [(136, 64), (4104, 128)])  # a token tile cut at 8 rows, several feature tiles
def test_swiglu_bwd_transposed_against_oracle(T, F):
    torch.manual_seed(500 + F)
    gu, d = _gate_up(T, F), _rows(T, F, 1)
    dgu = torch.empty_like(gu)
    dguT = torch.empty(2 * F, T, device=DEV, dtype=BF)
    _call("th_swiglu_bwd_t", d.data_ptr(), gu.data_ptr(), dgu.data_ptr(), dguT.data_ptr(), T, F)
    _check(dgu, ko.swiglu_bwd_oracle(d, gu), "swiglu_t dgu")
    assert torch.equal(dguT, dgu.t())


# -------------------------------------------------------------------------------------------- RoPE
# the last case is 13200 * 5 * 8 = 528,000 chunks against 2048 * 256 = 524,288 lanes: a second grid pass
@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("Dh,Hq,Hkv,B,S", [(16, 4, 2, 2, 24), (64, 4, 1, 2, 40), (128, 2, 1, 2, 24), (128, 4, 1, 2, 6600)])
def test_rope_against_fp64_angles(Dh, Hq, Hkv, B, S, sign):
    from tensorhive_fixed_amd.ops.rope import rope_inplace
    torch.manual_seed(600 + Dh)
    theta, nrot = 500000.0, Hq + Hkv
    x = _rows(B * S, (Hq + 2 * Hkv) * Dh)
    x[S:2 * S] = x[:S]  # batch 2 repeats batch 1: its positions start again at 0, so must its output
    got = rope_inplace(x.clone(), S, nrot, Dh, theta, sign)
    torch.cuda.synchronize()
    _check(got, ko.rope_oracle(x, S, nrot, Dh, theta, sign), f"rope sign {sign:+.0f}")
    assert torch.equal(got[:, nrot * Dh:], x[:, nrot * Dh:])  # v heads
    assert torch.equal(got[S:2 * S], got[:S])
    assert torch.equal(got[S], x[S])  # angle 0


# ----------------------------------------------------------------------------------- cross-entropy
IGNORE = -100


def _ce_rows(V, ld):
    """Four row kinds x six targets in a [24, ld] buffer whose columns V.. are padding."""
    kinds, R = 4, 24
    buf = (torch.randn(R, ld, device=DEV) * 3).to(BF)
    k = torch.arange(R, device=DEV) % kinds
    lg = buf[:, :V]
    lg[k == 1] += 80                      # all logits shifted by +80
    spike = lg[k == 2]
    spike[:, V - 1] = spike.float().max() + 60   # one logit 60 above the rest
    lg[k == 2] = spike
    lg[k == 3] = 1.5                      # all logits equal
    tgt = torch.tensor([0, V - 1, IGNORE, -1, V, V + 3], device=DEV)[torch.arange(R, device=DEV) // kinds]
    return buf, tgt


# scalar path in two passes of 512 lanes | vector body + 3-column tail in a strided chunk | vector loop longer
# than one pass (625 vectors) | one vector | one column
@pytest.mark.parametrize("V,ld", [(1003, 1003), (1003, 1008), (5000, 5000), (8, 8), (1, 1)])
def test_cross_entropy_row_layouts(V, ld):
    from tensorhive_fixed_amd.ops.cross_entropy import ce_rows_
    torch.manual_seed(700 + V + ld)
    buf, tgt = _ce_rows(V, ld)
    R = buf.shape[0]
    before = buf.clone()
    o = ko.ce_oracle(before[:, :V], tgt, 0.5, IGNORE)
    loss = torch.full((R,), 7.0, device=DEV)
    lse = torch.full((R,), 7.0, device=DEV)
    _call("th_ce_fwd_bwd", buf.data_ptr(), ld, tgt.data_ptr(), loss.data_ptr(), lse.data_ptr(), R, V, 0.5, IGNORE)
    _check(loss, o["loss"], "ce loss")
    _check(lse, o["lse"], "ce lse")
    _check(buf[:, :V], o["dlogits"], "ce dlogits")
    assert torch.equal(buf[:, V:], before[:, V:])  # padding columns
    invalid = (tgt == IGNORE) | (tgt < 0) | (tgt >= V)
    assert int(invalid.sum()) == 16
    assert not bool(loss[invalid].any()) and not bool(buf[:, :V][invalid].any())

    buf0 = before.clone()
    loss0 = ce_rows_(buf0[:, :V], tgt, 0.0, IGNORE)  # grad_scale 0: the loss stays, the gradient vanishes
    torch.cuda.synchronize()
    _check(loss0, o["loss"], "ce loss")
    assert not bool(buf0[:, :V].any()) and torch.equal(buf0[:, V:], before[:, V:])


# ---------------------------------------------------------------------------------- AdamW and norm
GRID_PASS = 2048 * 256 * 8  # elements one pass of the capped grid covers
HP = dict(lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-8, grad_scale=0.5)


def _flat(n, phase=0):
    return torch.randn(n, device=DEV) * _scales(n, phase)


# one vector | one pass + one vector | two passes + a partial third
@pytest.mark.parametrize("gdtype", [BF, torch.float32], ids=["bf16grad", "f32grad"])
@pytest.mark.parametrize("n", [8, GRID_PASS + 8, 2 * GRID_PASS + 8 * 1001])
def test_adamw_and_norm_grid_stride(n, gdtype):
    from tensorhive_fixed_amd.ops.adamw import adamw_flat_, grad_sumsq_
    torch.manual_seed(800 + n % 1000)
    g = (_flat(n) * 0.05).to(gdtype)
    ns = torch.full((1,), -1.0, device=DEV)
    grad_sumsq_(g, ns)
    _check(ns, ko.sumsq_oracle(g), "sumsq")
    prev = torch.tensor([2.5], device=DEV) * float(ns)
    acc = prev.clone()
    grad_sumsq_(g, acc, accumulate=True)
    _check(acc, ko.sumsq_oracle(g, prev), "sumsq accumulate")

    norm = float(ns.sqrt()) * HP["grad_scale"]
    clips = {"no norm": (None, 1.0), "clip 0": (ns, 0.0), "active": (ns, 0.25 * norm), "factor 1": (ns, 1e3 * norm)}
    if n == 8:  # every combination where it costs nothing
        combos = [(s, c, wd) for s in (1, 2, 1000) for c in clips for wd in (0.0, 0.1)]
    else:       # each step, clip configuration and weight decay at least once
        combos = [(1, "no norm", 0.1), (2, "clip 0", 0.0), (1000, "active", 0.1), (2, "factor 1", 0.1)]
    master0 = _flat(n, 1)
    m0 = _flat(n, 2) * 0.05
    v0 = (_flat(n) * 0.05).pow(2)
    for step, cname, wd in combos:
        norm_sq, clip = clips[cname]
        hp = dict(HP, weight_decay=wd, step=step, norm_sq=norm_sq, clip=clip)
        o = ko.adamw_oracle(master0, m0, v0, g, **hp)
        runs = []
        for _ in range(2):
            master, m, v = master0.clone(), m0.clone(), v0.clone()
            p = torch.zeros(n, device=DEV, dtype=BF)
            adamw_flat_(p, master, m, v, g, **hp)
            runs.append((master, m, v, p))
        master, m, v, p = runs[0]
        for name, got in (("master", master), ("m", m), ("v", v), ("p", p)):
            _check(got, o[name], f"adamw {name}")
        assert torch.equal(p, master.to(BF))
        assert all(torch.equal(a, b) for a, b in zip(*runs))
        del runs, o


# --------------------------------------------------------------------------------------- embedding
EMB_V = 300


def _tokens(pattern):
    if pattern == "one":
        return torch.tensor([7], device=DEV)
    if pattern == "distinct":
        return torch.randperm(EMB_V, device=DEV)[:200]
    if pattern == "run128":
        return torch.full((128,), 5, device=DEV)
    # ids 0 and V - 1 once each (the first and last sorted position), runs of 1 and longer runs between
    mid = torch.cat([torch.randint(1, 12, (250,), device=DEV), torch.tensor([100, 200], device=DEV)])
    ids = torch.cat([mid, torch.tensor([0, EMB_V - 1], device=DEV)])
    return ids[torch.randperm(ids.numel(), device=DEV)]


@pytest.mark.parametrize("pattern", ["one", "distinct", "run128", "mixed"])
@pytest.mark.parametrize("D", [8, 512, 4104])  # 4104: the MAXV = 4 instantiation
def test_embedding_backward_runs(D, pattern):
    from tensorhive_fixed_amd.ops.embedding import embedding, sort_tokens
    torch.manual_seed(900 + D)
    tok = _tokens(pattern)
    T = tok.numel()
    s, perm = sort_tokens(tok)
    assert torch.equal(tok[perm], s)
    same = s[1:] == s[:-1]
    assert bool((perm[1:][same] > perm[:-1][same]).all())  # ascending inside each run: a fixed summation order

    w = torch.randn(EMB_V, D, device=DEV).to(BF).requires_grad_(True)
    dy = _rows(T, D)
    embedding(tok, w).backward(dy)
    ref, mag = ko.embedding_bwd_oracle(tok, dy, EMB_V)
    _check(w.grad, (ref, mag), "embedding gw")
    first = w.grad.clone()
    w.grad = None
    embedding(tok, w).backward(dy)
    assert torch.equal(first, w.grad)

    prev = (torch.randn(EMB_V, D, device=DEV) * 2).to(BF)
    gw = prev.clone()
    _call("th_embedding_bwd", s.data_ptr(), perm.data_ptr(), dy.data_ptr(), gw.data_ptr(), T, D, 1)
    _check(gw, ko.embedding_bwd_oracle(tok, dy, EMB_V, prev), "embedding gw accumulate")
    absent = torch.ones(EMB_V, dtype=torch.bool, device=DEV)
    absent[tok] = False
    assert torch.equal(gw[absent], prev[absent])


def test_embedding_rejects_rows_wider_than_8192():
    from tensorhive_fixed_amd.ops.embedding import sort_tokens
    T, D, V = 4, 8200, 6
    tok = torch.tensor([1, 3, 3, 0], device=DEV)
    s, perm = sort_tokens(tok)
    dy = _rows(T, D)
    gw = torch.full((V, D), 3.0, device=DEV, dtype=BF)
    with pytest.raises(RuntimeError, match="bad shape"):
        _call("th_embedding_bwd", s.data_ptr(), perm.data_ptr(), dy.data_ptr(), gw.data_ptr(), T, D, 0)
    torch.cuda.synchronize()
    assert bool((gw == 3.0).all())


# --------------------------------------------------------------------------------------- transpose
# tiles 1: 128 x 64, 2: 128 x 128, 3: 64 x 128; each on one 8 x 8 corner, on both orientations of a shape that
# cuts the others' edges, and on a shape spanning several tiles with both edges cut
@pytest.mark.parametrize("R,C", [(8, 8), (136, 72), (72, 136), (200, 264)])
@pytest.mark.parametrize("tile", [1, 2, 3])
def test_transpose_every_tile_on_every_edge(tile, R, C):
    from tensorhive_fixed_amd.ops.transpose import transpose
    torch.manual_seed(1000 + R)
    x = torch.randn(R, C, device=DEV).to(BF)
    out = transpose(x, tile=tile)
    torch.cuda.synchronize()
    assert out.shape == (C, R) and torch.equal(out, x.t().contiguous())
    base = torch.randn(R, C + 24, device=DEV).to(BF)
    view = base[:, 8:8 + C]  # 16-byte aligned column slice of a wider buffer
    out = transpose(view, tile=tile)
    torch.cuda.synchronize()
    assert torch.equal(out, view.t().contiguous())
