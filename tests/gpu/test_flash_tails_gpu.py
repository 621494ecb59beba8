"""The flash attention kernels' geometry: every length tail, strided layouts, isolation, the 32-bit switch.

* ``ao.TAIL_LENGTHS`` (1 ... 263: one short of and one past the 32-row wave block, the 64-key tile, the
  128-row workgroup and the 256-key fused dK|dV block) against the fp64 oracle per 32-row block per head,
  with the criterion of ``test_attention_profiles_gpu.py``; batch entry 1 carries the other profile, so
  the tail of entry 0 abuts live rows of entry 1;
* the rotary backward folded into the dQ / dK epilogues against fp64 at tails;
* the C entry points on padded layouts (``ld``, ``bs``, ``ldo``, ``bso`` beyond dense, NaN in every input
  pad, a sentinel in every output pad): bit-equal to the dense run, no sentinel touched;
* a NaN batch entry or KV group cannot disturb another, and two runs agree bit for bit;
* the switch to register-staged tiles where ``S * ld * 2`` reaches 2^31, from both sides.

``TH_ATTN_ACCURACY_JSON=<file>`` makes a run add its figures there under ``"tails"``.
"""
import functools
import json
import os

import pytest
import torch

from tests import attention_oracles as ao
from tests.gpu.test_attention_profiles_gpu import MARGIN_BASELINE, _batch_profiles
from tests.gpu.test_attention_profiles_gpu import _check_blocks as _profile_blocks
from tests.gpu.test_attention_profiles_gpu import _key as _profile_key
from tests.gpu.test_flash_attn_gpu import KF_DEFAULT, PROD_FLAGS, PROD_IDS

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = ao.D
B = 2
HQ, HKV = ao.TAIL_HEADS
KH = 1 << 19
FWD_VARIANTS = [None, 11]  # the default (15, LDS-DMA tiles) and its register-staged twin
FWD_IDS = ["fwd", "fwd_regstage"]
SENT16, SENT32 = 0x5A5A, 0x5A5A5A5A  # bf16 2.4e16, f32 1.5e16: neither is a value any kernel here writes
_RECORD: dict = {"flash": {}, "lse": {}, "rope": {}}


@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    path = os.environ.get("TH_ATTN_ACCURACY_JSON")
    if path:
        whole = {}
        if os.path.exists(path):
            with open(path) as f:
                whole = json.load(f)
        whole["tails"] = _RECORD
        with open(path, "w") as f:
            json.dump(whole, f, indent=1, sort_keys=True)


def _mask_id(causal):
    return "causal" if causal else "full"


def _profiles(profile: str) -> list[str]:
    """Batch entry 0 carries the case's profile, entry 1 the other one of ``ao.TAIL_PROFILES``."""
    i = ao.TAIL_PROFILES.index(profile)
    return [ao.TAIL_PROFILES[(i + b) % len(ao.TAIL_PROFILES)] for b in range(B)]


@functools.lru_cache(maxsize=None)
def _inputs(S, profile, causal):
    cases = [ao.tail_case(S, p, causal) for p in _profiles(profile)]
    qkv = torch.cat([torch.cat([c[n].reshape(S, -1) for n in ("q", "k", "v")], 1) for c in cases]).to(DEV)
    dout = torch.cat([c["do"].reshape(S, -1) for c in cases]).to(DEV)
    return cases, qkv.contiguous(), dout.contiguous()


@functools.lru_cache(maxsize=None)
def _forward(S, profile, causal, variant):
    from tensorhive_fixed_amd.ops.attention import flash_fwd

    _, qkv, _ = _inputs(S, profile, causal)
    return flash_fwd(qkv, B, S, HQ, HKV, D, causal=causal, variant=variant)


@functools.lru_cache(maxsize=None)
def _backward(S, profile, causal, flags, rope=False):
    """The backward on the default forward's o and lse, as in training."""
    from tensorhive_fixed_amd.ops.attention import flash_bwd
    from tensorhive_fixed_amd.ops.rope import rope_tables

    _, qkv, dout = _inputs(S, profile, causal)
    o, lse = _forward(S, profile, causal, None)
    tabs = rope_tables(S, D, ao.ROPE_THETA, qkv.device) if rope else None
    return flash_bwd(dout, qkv, o, lse, B, S, HQ, HKV, D, causal=causal, flags=flags, rope=tabs)


def _check_blocks(name, got, exact, unit, where, record):
    """``got`` [S, H, D] of one batch entry against the exact result, per 32-row block per head."""
    assert torch.isfinite(got).all(), f"{name} {where}: non-finite"
    limit = MARGIN_BASELINE * unit
    err = ao.block_max_abs(got.cpu(), exact)
    blk, head = divmod(int(err.argmax()), err.shape[1])
    worst = err.max().item()
    print(f"{name} {where}: worst block rows {32 * blk}-{32 * blk + 31} head {head} err {worst:.4g} = "
          f"{worst / unit:.2f} x E_b ({unit:.4g}), limit {limit:.4g}")
    record[name] = worst / unit
    return [] if worst <= limit else [f"{name} {where}: rows {32 * blk}-{32 * blk + 31} head {head}: err {worst:.4g} "
                                      f"> {limit:.4g} ({worst / unit:.2f} x E_b)"]


def _check_within(name, got, bound, where):
    """S = 1: |got| against an elementwise bound (the exact value is 0)."""
    over = got.cpu().double().abs() - bound
    print(f"{name} {where}: max |{name}| {got.float().abs().max().item():.3g}, smallest slack {-over.max().item():.3g}")
    return [] if over.max().item() <= 0 else [f"{name} {where}: |{name}| exceeds the f32 cancellation bound by "
                                               f"{over.max().item():.3g}"]


def _bf16_ulp(x: torch.Tensor) -> torch.Tensor:
    return torch.exp2(torch.floor(torch.log2(x.double().abs().clamp_min(2.0 ** -126))) - 7)


def _grads(dqkv, b, S):
    rows = dqkv[b * S:(b + 1) * S]
    return {"dq": rows[:, :HQ * D].reshape(S, HQ, D), "dk": rows[:, HQ * D:(HQ + HKV) * D].reshape(S, HKV, D),
            "dv": rows[:, (HQ + HKV) * D:].reshape(S, HKV, D)}


# ------------------------------------------------------------------------ 1. tail lengths against fp64
@pytest.mark.parametrize("variant", FWD_VARIANTS, ids=FWD_IDS)
@pytest.mark.parametrize("causal", [True, False], ids=_mask_id)
@pytest.mark.parametrize("profile", ao.TAIL_PROFILES)
@pytest.mark.parametrize("S", ao.TAIL_LENGTHS, ids=lambda s: f"S{s}")
def test_tail_forward_per_block(S, profile, causal, variant):
    cases, _, _ = _inputs(S, profile, causal)
    o, lse = _forward(S, profile, causal, variant)
    assert torch.isfinite(lse).all()
    fid = FWD_IDS[FWD_VARIANTS.index(variant)]
    bad = []
    for b, (p, c) in enumerate(zip(_profiles(profile), cases)):
        key = f"S{S}|{p}|{_mask_id(causal)}|{fid}|b{b}"
        got = o.view(B, S, HQ, D)[b]
        if S == 1:  # o = v exactly: a bf16 value, so the kernel may be one step of it off and no more
            want = c["exact"]["o"]
            miss = ((got.cpu().double() - want).abs() / _bf16_ulp(want)).max().item()
            print(f"o batch {b} ({p}): worst |o - v| {miss:.2f} bf16 steps of v")
            if not miss <= 1:
                bad.append(f"o batch {b} ({p}): {miss:.2f} bf16 steps from the v row")
        else:
            bad += _check_blocks("o", got, c["exact"]["o"], c["E_b"]["o"], f"batch {b} ({p})",
                                 _RECORD["flash"].setdefault(key, {}))
        err = (lse[b].cpu().double() - c["exact"]["lse"]).abs()
        rel = err / c["lse_tol"]
        h, r = divmod(int(rel.argmax()), S)
        print(f"lse batch {b} ({p}): worst err {err.max().item():.3e}; worst err/tolerance {rel.max().item():.2f} "
              f"at head {h} row {r}")
        _RECORD["lse"][key] = [err.max().item(), rel.max().item()]
        if rel.max().item() > 1:
            bad.append(f"lse batch {b} ({p}) head {h} row {r}: err {err[h, r].item():.3e} > "
                       f"{c['lse_tol'][h, r].item():.3e}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("causal", [True, False], ids=_mask_id)
@pytest.mark.parametrize("profile", ao.PROFILES)
@pytest.mark.parametrize("Bs,S,Hq,Hkv", ao.SHAPES)
def test_register_staged_forward_at_the_profile_shapes(Bs, S, Hq, Hkv, profile, causal):
    """Forward variant 11 on the whole matrix of ``test_attention_profiles_gpu.test_flash_forward_per_block``,
    by its criterion (``large``: the operand model's margin)."""
    from tensorhive_fixed_amd.ops.attention import flash_fwd

    profiles = _batch_profiles(Bs, profile)
    cases = [ao.case(S, Hq, Hkv, p, causal) for p in profiles]
    qkv = torch.cat([torch.cat([c[n].reshape(S, -1) for n in ("q", "k", "v")], 1) for c in cases]).to(DEV)
    o, lse = flash_fwd(qkv.contiguous(), Bs, S, Hq, Hkv, D, causal=causal, variant=11)
    assert torch.isfinite(lse).all()
    bad = []
    for b, (p, c) in enumerate(zip(profiles, cases)):
        key = _profile_key(Bs, S, Hq, Hkv, p, causal, "fwd_regstage") + (f"|b{b}" if Bs > 1 else "")
        bad += _profile_blocks("o", o.view(Bs, S, Hq, D)[b], c, p, f"batch {b} ({p})", key)
        rel = ((lse[b].cpu().double() - c["exact"]["lse"]).abs() / c["lse_tol"]).max().item()
        print(f"lse batch {b} ({p}): worst err/tolerance {rel:.2f}")
        if rel > 1:
            bad.append(f"lse batch {b} ({p}): {rel:.2f} x its tolerance")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("bwd_flags", PROD_FLAGS, ids=PROD_IDS)
@pytest.mark.parametrize("causal", [True, False], ids=_mask_id)
@pytest.mark.parametrize("profile", ao.TAIL_PROFILES)
@pytest.mark.parametrize("S", ao.TAIL_LENGTHS, ids=lambda s: f"S{s}")
def test_tail_backward_per_block(S, profile, causal, bwd_flags):
    cases, _, _ = _inputs(S, profile, causal)
    dqkv = _backward(S, profile, causal, bwd_flags)
    flag_id = PROD_IDS[PROD_FLAGS.index(bwd_flags)]
    if bwd_flags == KF_DEFAULT and S % 64:
        # flash_bwd_impl clears bit 4 before it chooses any kernel: the same launches as kh, whose
        # oracle comparison is the kh case of this test
        assert torch.equal(dqkv, _backward(S, profile, causal, KH))
        return
    bad = []
    for b, (p, c) in enumerate(zip(_profiles(profile), cases)):
        key = f"S{S}|{p}|{_mask_id(causal)}|{flag_id}|b{b}"
        where = f"batch {b} ({p}) {flag_id}"
        got = _grads(dqkv, b, S)
        rec = _RECORD["flash"].setdefault(key, {})
        if S == 1:
            dq_b, dk_b = ao.single_row_bounds(c["q"], c["k"], c["v"], c["do"])
            bad += _check_within("dq", got["dq"], dq_b, where) + _check_within("dk", got["dk"], dk_b, where)
            bad += _check_blocks("dv", got["dv"], c["exact"]["dv"], c["E_b"]["dv"], where, rec)
            continue
        for name in ("dq", "dk", "dv"):
            bad += _check_blocks(name, got[name], c["exact"][name], c["E_b"][name], where, rec)
    assert not bad, "\n".join(bad)


# --------------------------------------------------- 2. rotary backward in the epilogues, against fp64
@pytest.mark.parametrize("bwd_flags", [KF_DEFAULT, KH], ids=["kf_default", "kh"])
@pytest.mark.parametrize("causal", [True, False], ids=_mask_id)
@pytest.mark.parametrize("S", [1, 33, 65, 129, 257], ids=lambda s: f"S{s}")
def test_rotary_backward_in_the_epilogues_per_block(S, causal, bwd_flags):
    """dq and dk of ``flash_bwd(..., rope=tables)``: the exact gradients turned back in fp64, held to the
    format baseline that rounds once, after the rotation; dv is the un-fused call's, bit for bit."""
    profile = "randn"
    cases, _, _ = _inputs(S, profile, causal)
    dqkv = _backward(S, profile, causal, bwd_flags, rope=True)
    plain = _backward(S, profile, causal, bwd_flags)
    assert torch.equal(dqkv[:, (HQ + HKV) * D:], plain[:, (HQ + HKV) * D:])
    flag_id = "kf_default" if bwd_flags == KF_DEFAULT else "kh"
    bad = []
    for b, (p, c) in enumerate(zip(_profiles(profile), cases)):
        where = f"batch {b} ({p}) {flag_id} rope"
        got = _grads(dqkv, b, S)
        if S == 1:  # position 0: the rotation is the identity, dq = dk = 0
            dq_b, dk_b = ao.single_row_bounds(c["q"], c["k"], c["v"], c["do"])
            bad += _check_within("dq", got["dq"], dq_b, where) + _check_within("dk", got["dk"], dk_b, where)
            continue
        rc = ao.tail_rope_case(S, p, causal)
        rec = _RECORD["rope"].setdefault(f"S{S}|{p}|{_mask_id(causal)}|{flag_id}|b{b}", {})
        for name in ("dq", "dk"):
            bad += _check_blocks(name, got[name], rc["exact"][name], rc["E_b"][name], where, rec)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------- 3. strided layouts, memory discipline
def _sentinel(n, dtype):
    if dtype == torch.bfloat16:
        return torch.full((n,), SENT16, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    return torch.full((n,), SENT32, dtype=torch.int32, device=DEV).view(torch.float32)


def _untouched(buf, live):
    """Every element of ``buf`` outside the boolean mask ``live`` still holds the sentinel."""
    raw = buf.view(torch.int16 if buf.dtype == torch.bfloat16 else torch.int32).reshape(-1)
    return bool((raw[~live.reshape(-1)] == (SENT16 if buf.dtype == torch.bfloat16 else SENT32)).all())


class _Layout:
    """Packed qkv / dqkv with row stride ``ld`` and ``guard`` rows after each batch entry, o / dO
    likewise with ``ldo``; lse and delta with ``slack`` floats past their ends."""

    def __init__(self, Bn, S, Hq, Hkv, pad, pado, guard, slack):
        self.B, self.S, self.Hq, self.Hkv = Bn, S, Hq, Hkv
        self.row, self.orow = (Hq + 2 * Hkv) * D, Hq * D
        self.ld, self.ldo, self.rows = self.row + pad, self.orow + pado, S + guard
        self.bs, self.bso = self.rows * self.ld, self.rows * self.ldo
        self.nl = Bn * Hq * S
        self.slack = slack

    def place(self, dense, width, stride, fill):
        """``dense`` [B * S, width] into a fresh [B, rows, stride] buffer filled with ``fill``."""
        buf = fill(self.B * self.rows * stride, dense.dtype).view(self.B, self.rows, stride)
        buf[:, :self.S, :width] = dense.view(self.B, self.S, width)
        return buf

    def live(self, width, stride):
        m = torch.zeros(self.B, self.rows, stride, dtype=torch.bool, device=DEV)
        m[:, :self.S, :width] = True
        return m

    def take(self, buf, width):
        return buf[:, :self.S, :width].reshape(self.B * self.S, width)

    def forward(self, qkv, causal, flags):
        from tensorhive_fixed_amd.ops import _lib

        o = _sentinel(self.B * self.bso, torch.bfloat16).view(self.B, self.rows, self.ldo)
        lse = _sentinel(self.nl + self.slack, torch.float32)
        q = qkv.data_ptr()
        k = q + self.Hq * D * 2
        v = k + self.Hkv * D * 2
        _lib.call("th_flash_attn_fwd", q, k, v, o.data_ptr(), lse.data_ptr(), self.B, self.S, self.Hq, self.Hkv, D,
                  int(causal), self.ld, self.bs, self.ldo, self.bso, ao.SCALE, flags, _lib.stream_ptr(qkv.device))
        return o, lse

    def backward(self, qkv, dout, o, lse, causal, flags, rope=None):
        from tensorhive_fixed_amd.ops import _lib

        dqkv = _sentinel(self.B * self.bs, torch.bfloat16).view(self.B, self.rows, self.ld)
        delta = _sentinel(2 * self.nl + self.slack, torch.float32)
        q = qkv.data_ptr()
        k = q + self.Hq * D * 2
        v = k + self.Hkv * D * 2
        dq = dqkv.data_ptr()
        dk = dq + self.Hq * D * 2
        dv = dk + self.Hkv * D * 2
        head = (q, k, v, o.data_ptr(), dout.data_ptr(), lse.data_ptr(), delta.data_ptr())
        geom = (self.B, self.S, self.Hq, self.Hkv, D, int(causal), self.ld, self.bs, self.ldo, self.bso, ao.SCALE)
        if rope is not None:
            _lib.call("th_flash_attn_bwd_rope", *head, dq, dk, dv, *geom, rope[0].data_ptr(), rope[1].data_ptr(),
                      flags, _lib.stream_ptr(qkv.device))
        else:
            _lib.call("th_flash_attn_bwd", *head, None, dq, dk, dv, *geom, flags, _lib.stream_ptr(qkv.device))
        return dqkv, delta


def _nan(n, dtype):
    return torch.full((n,), float("nan"), dtype=dtype, device=DEV)


def _randn_inputs(Bn, S, Hq, Hkv, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(Bn * S, (Hq + 2 * Hkv) * D, generator=g).to(torch.bfloat16).to(DEV)
    dout = torch.randn(Bn * S, Hq * D, generator=g).to(torch.bfloat16).to(DEV)
    return qkv, dout


@pytest.mark.parametrize("causal", [True, False], ids=_mask_id)
@pytest.mark.parametrize("S", [33, 129, 200, 257], ids=lambda s: f"S{s}")
def test_padded_layouts_equal_the_dense_run_and_touch_no_pad(S, causal):
    """NaN in every input pad column and guard row, a sentinel in every output pad, guard row and tail:
    the live regions equal the dense run's bit for bit (same kernels, same values; the block maps do not
    depend on strides) and every sentinel survives."""
    qkv, dout = _randn_inputs(B, S, HQ, HKV, seed=S)
    dense = _Layout(B, S, HQ, HKV, 0, 0, 0, 0)
    padded = _Layout(B, S, HQ, HKV, pad=8 * 3, pado=8 * 2, guard=2, slack=64)
    qkv_p = padded.place(qkv, padded.row, padded.ld, _nan)
    dout_p = padded.place(dout, padded.orow, padded.ldo, _nan)
    live_o, live_g = padded.live(padded.orow, padded.ldo), padded.live(padded.row, padded.ld)
    live_l = torch.arange(padded.nl + padded.slack, device=DEV) < padded.nl
    live_d = torch.arange(2 * padded.nl + padded.slack, device=DEV) < 2 * padded.nl
    for fid, fflags in zip(FWD_IDS, (0, 16 + 11)):
        o_d, lse_d = dense.forward(qkv.view(B, S, -1), causal, fflags)
        o_p, lse_p = padded.forward(qkv_p, causal, fflags)
        assert torch.isfinite(o_d).all() and torch.isfinite(lse_d).all(), fid
        assert torch.equal(padded.take(o_p, padded.orow), dense.take(o_d, dense.orow)), fid
        assert torch.equal(lse_p[:padded.nl], lse_d), fid
        assert _untouched(o_p, live_o) and _untouched(lse_p, live_l), fid
    o_d, lse_d = dense.forward(qkv.view(B, S, -1), causal, 0)
    o_p, lse_p = padded.forward(qkv_p, causal, 0)
    for flag_id, flags in zip(PROD_IDS, PROD_FLAGS):
        g_d, delta_d = dense.backward(qkv.view(B, S, -1), dout.view(B, S, -1), o_d, lse_d, causal, flags)
        g_p, delta_p = padded.backward(qkv_p, dout_p, o_p, lse_p, causal, flags)
        assert torch.isfinite(g_d).all(), flag_id
        assert torch.equal(padded.take(g_p, padded.row), dense.take(g_d, dense.row)), flag_id
        assert torch.equal(delta_p[:padded.nl], delta_d[:padded.nl]), flag_id
        assert _untouched(g_p, live_g), flag_id
        # the second half of delta (-lse * log2 e) is written by the default path only; its slack by none
        assert _untouched(delta_p, live_d), flag_id


# -------------------------------------------------------------------- 4. isolation, reproducibility
def _run_all(qkv, dout, S, causal):
    """o, lse of both forwards and dqkv of every production backward (on the default forward)."""
    from tensorhive_fixed_amd.ops.attention import flash_bwd, flash_fwd

    out = {}
    for fid, variant in zip(FWD_IDS, (15, 11)):
        out[fid] = flash_fwd(qkv, B, S, HQ, HKV, D, causal=causal, variant=variant)
    o, lse = out["fwd"]
    for flag_id, flags in zip(PROD_IDS, PROD_FLAGS):
        out[flag_id] = flash_bwd(dout, qkv, o, lse, B, S, HQ, HKV, D, causal=causal, flags=flags)
    return out


@pytest.mark.parametrize("causal", [True, False], ids=_mask_id)
@pytest.mark.parametrize("S", [129, 257], ids=lambda s: f"S{s}")
def test_a_nan_batch_entry_or_kv_group_disturbs_no_other(S, causal):
    qkv, dout = _randn_inputs(B, S, HQ, HKV, seed=100 + S)
    clean = _run_all(qkv, dout, S, causal)
    assert all(torch.isfinite(t).all() for v in clean.values() for t in (v if isinstance(v, tuple) else (v,)))
    nan = float("nan")
    # batch entry 1: q, k, v, dO
    qkv_b, dout_b = qkv.clone(), dout.clone()
    qkv_b[S:], dout_b[S:] = nan, nan
    got = _run_all(qkv_b, dout_b, S, causal)
    for fid in FWD_IDS:
        assert torch.equal(got[fid][0][:S], clean[fid][0][:S]), fid
        assert torch.equal(got[fid][1][0], clean[fid][1][0]), fid
    for flag_id in PROD_IDS:
        assert torch.equal(got[flag_id][:S], clean[flag_id][:S]), flag_id
    # KV group 1 of both entries: q heads 2-3, k head 1, v head 1, dO heads 2-3
    G = HQ // HKV
    qcols = slice(G * D, 2 * G * D)
    qkv_g, dout_g = qkv.clone(), dout.clone()
    qkv_g[:, qcols] = nan
    qkv_g[:, (HQ + 1) * D:(HQ + 2) * D] = nan
    qkv_g[:, (HQ + HKV + 1) * D:] = nan
    dout_g[:, qcols] = nan
    got = _run_all(qkv_g, dout_g, S, causal)
    for fid in FWD_IDS:
        assert torch.equal(got[fid][0][:, :G * D], clean[fid][0][:, :G * D]), fid
        assert torch.equal(got[fid][1][:, :G], clean[fid][1][:, :G]), fid
    group0 = torch.cat([torch.arange(0, G * D), torch.arange(HQ * D, (HQ + 1) * D),
                        torch.arange((HQ + HKV) * D, (HQ + HKV + 1) * D)]).to(DEV)
    for flag_id in PROD_IDS:
        assert torch.equal(got[flag_id][:, group0], clean[flag_id][:, group0]), flag_id


@pytest.mark.parametrize("causal", [True, False], ids=_mask_id)
@pytest.mark.parametrize("S", [129, 257], ids=lambda s: f"S{s}")
def test_two_runs_agree_bit_for_bit(S, causal):
    qkv, dout = _randn_inputs(B, S, HQ, HKV, seed=200 + S)
    first, second = _run_all(qkv, dout, S, causal), _run_all(qkv, dout, S, causal)
    for name in FWD_IDS:
        assert torch.equal(first[name][0], second[name][0]) and torch.equal(first[name][1], second[name][1]), name
    for name in PROD_IDS:
        assert torch.equal(first[name], second[name]), name


# ------------------------------------------------------------------------ 5. the 32-bit offset switch
SW_S, SW_HQ, SW_HKV = 129, 2, 1
LD_BELOW = ((1 << 31) // (2 * SW_S)) // 8 * 8  # the largest multiple of 8 with S * ld * 2 < 2^31
LD_ABOVE = LD_BELOW + 8


def _switch_case(ld):
    free = torch.cuda.mem_get_info()[0]
    if free < 8 << 30:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB free on the device, 8 GiB needed")
    qkv, dout = _randn_inputs(1, SW_S, SW_HQ, SW_HKV, seed=7)
    wide = _Layout(1, SW_S, SW_HQ, SW_HKV, pad=ld - (SW_HQ + 2 * SW_HKV) * D, pado=0, guard=0, slack=0)
    assert wide.ld == ld and ld % 8 == 0
    # only the live row slices are written, and nothing else is read
    qkv_w = wide.place(qkv, wide.row, wide.ld, lambda n, dt: torch.empty(n, dtype=dt, device=DEV))
    return qkv, dout, wide, qkv_w


def test_ldsdma_kernels_just_below_the_32_bit_boundary():
    from tensorhive_fixed_amd.ops.attention import flash_bwd, flash_fwd

    assert SW_S * LD_BELOW * 2 < 1 << 31 <= SW_S * (LD_BELOW + 8) * 2
    qkv, dout, wide, qkv_w = _switch_case(LD_BELOW)
    o_d, lse_d = flash_fwd(qkv, 1, SW_S, SW_HQ, SW_HKV, D)
    g_d = flash_bwd(dout, qkv, o_d, lse_d, 1, SW_S, SW_HQ, SW_HKV, D, flags=KH)
    o_w, lse_w = wide.forward(qkv_w, True, 0)
    g_w, _ = wide.backward(qkv_w, dout.view(1, SW_S, -1), o_w, lse_w, True, KH)
    fwd_same = torch.equal(o_w.view(SW_S, -1), o_d) and torch.equal(lse_w.view_as(lse_d), lse_d)
    bwd_same = torch.equal(wide.take(g_w, wide.row), g_d)
    del qkv_w, g_w
    torch.cuda.empty_cache()
    assert fwd_same and bwd_same, (fwd_same, bwd_same)


def test_register_staged_kernels_take_over_at_the_32_bit_boundary():
    from tensorhive_fixed_amd.ops.attention import flash_bwd, flash_fwd
    from tensorhive_fixed_amd.ops.rope import rope_tables

    assert SW_S * LD_ABOVE * 2 >= 1 << 31
    qkv, dout, wide, qkv_w = _switch_case(LD_ABOVE)
    o_d, lse_d = flash_fwd(qkv, 1, SW_S, SW_HQ, SW_HKV, D, variant=11)
    g_d = flash_bwd(dout, qkv, o_d, lse_d, 1, SW_S, SW_HQ, SW_HKV, D, flags=32)
    o_w, lse_w = wide.forward(qkv_w, True, 0)
    g_w, _ = wide.backward(qkv_w, dout.view(1, SW_S, -1), o_w, lse_w, True, KH)
    fwd_same = torch.equal(o_w.view(SW_S, -1), o_d) and torch.equal(lse_w.view_as(lse_d), lse_d)
    bwd_same = torch.equal(wide.take(g_w, wide.row), g_d)
    try:
        with pytest.raises(RuntimeError, match="bad shape"):  # rope tables with overflowing offsets
            wide.backward(qkv_w, dout.view(1, SW_S, -1), o_w, lse_w, True, KH,
                          rope=rope_tables(SW_S, D, ao.ROPE_THETA, qkv.device))
    finally:
        del qkv_w, g_w
        torch.cuda.empty_cache()
    assert fwd_same and bwd_same, (fwd_same, bwd_same)
