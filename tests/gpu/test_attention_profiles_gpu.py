"""The attention kernels on score profiles that move the running max (tests/attention_oracles.py):
flash forward, dQ and the dK|dV kernels of every production flag set against the exact fp64 result,
per 32-row block per head, within a multiple of what the bf16 format alone costs; the split-KV decode
kernel on the same key profiles, per (sequence, q head) row.

``TH_ATTN_ACCURACY_JSON=<file>`` makes a run leave its figures there
(scripts/attention_accuracy_table.py renders profiles/attention_accuracy/README.md from them).
"""
import functools
import json
import os

import pytest
import torch

from tests import attention_oracles as ao
from tests import decode_oracles as do
from tests.gpu.test_flash_attn_gpu import PROD_FLAGS, PROD_IDS

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = ao.D
MARGIN_BASELINE = 8.0  # x E_b: 4 (operand rounding, CPU-checked) x 2 (f32 accumulation order, the kernel's own lse)
MARGIN_MODEL = 2.0  # x E_m, ``large`` only
_RECORD: dict = {"flash": {}, "lse": {}, "rowsum_large": {}, "decode": {}}


@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    path = os.environ.get("TH_ATTN_ACCURACY_JSON")
    if path:
        with open(path, "w") as f:
            json.dump(_RECORD, f, indent=1, sort_keys=True)


def _batch_profiles(B: int, profile: str) -> list[str]:
    """Batch entry 0 carries the case's profile, entry 1 one from the other regime of the list."""
    i = ao.PROFILES.index(profile)
    return [ao.PROFILES[(i + 3 * b) % len(ao.PROFILES)] for b in range(B)]


@functools.lru_cache(maxsize=None)
def _forward(B, S, Hq, Hkv, profile, causal):
    """Packed qkv and dO on the device, the kernel's forward, and the fp64 cases of the batch entries."""
    from tensorhive_fixed_amd.ops.attention import flash_fwd

    cases = [ao.case(S, Hq, Hkv, p, causal) for p in _batch_profiles(B, profile)]
    qkv = torch.cat([torch.cat([c[n].reshape(S, -1) for n in ("q", "k", "v")], 1) for c in cases]).to(DEV)
    dout = torch.cat([c["do"].reshape(S, -1) for c in cases]).to(DEV)
    o, lse = flash_fwd(qkv.contiguous(), B, S, Hq, Hkv, D, causal=causal)
    return cases, qkv.contiguous(), dout.contiguous(), o, lse


def _check_blocks(name, got, case, profile, where, key):
    """``got`` [S, H, D] of one batch entry against the exact result, per 32-row block per head."""
    assert torch.isfinite(got).all(), f"{name} {where}: non-finite"
    large = profile == "large"
    unit = case["E_m"][name] if large else case["E_b"][name]
    limit = (MARGIN_MODEL if large else MARGIN_BASELINE) * unit
    err = ao.block_max_abs(got.cpu(), case["exact"][name])
    blk, head = divmod(int(err.argmax()), err.shape[1])
    worst = err.max().item()
    ratio = worst / unit
    print(f"{name} {where}: worst block rows {32 * blk}-{32 * blk + 31} head {head} err {worst:.4g} = "
          f"{ratio:.2f} x {'E_m' if large else 'E_b'} ({unit:.4g}), limit {limit:.4g}")
    _RECORD["flash"].setdefault(key, {})[name] = ratio
    return [] if worst <= limit else [f"{name} {where}: rows {32 * blk}-{32 * blk + 31} head {head}: err {worst:.4g} "
                                      f"> {limit:.4g} ({ratio:.2f} x {'E_m' if large else 'E_b'})"]


def _key(B, S, Hq, Hkv, profile, causal, flag_id):
    return f"{profile}|B{B} S{S} {Hq}/{Hkv}|{'causal' if causal else 'full'}|{flag_id}"


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("profile", ao.PROFILES)
@pytest.mark.parametrize("B,S,Hq,Hkv", ao.SHAPES)
def test_flash_forward_per_block(B, S, Hq, Hkv, profile, causal):
    cases, _, _, o, lse = _forward(B, S, Hq, Hkv, profile, causal)
    assert torch.isfinite(lse).all()
    bad = []
    for b, (p, c) in enumerate(zip(_batch_profiles(B, profile), cases)):
        key = _key(B, S, Hq, Hkv, p, causal, "fwd") + (f"|b{b}" if B > 1 else "")
        bad += _check_blocks("o", o.view(B, S, Hq, D)[b], c, p, f"batch {b} ({p})", key)
        err = (lse[b].cpu().double() - c["exact"]["lse"]).abs()
        rel = err / c["lse_tol"]
        h, r = divmod(int(rel.argmax()), S)
        plain = (err / c["lse_tol_plain"]).max().item()  # against 2e-3 + 2**-9 |score|_max alone
        print(f"lse batch {b} ({p}): worst err {err.max().item():.3e}; worst err/tolerance {rel.max().item():.2f} "
              f"at head {h} row {r}; err/(2e-3 + 2**-9 |score|_max) {plain:.2f}")
        _RECORD["lse"][key] = [err.max().item(), rel.max().item(), plain]
        if rel.max().item() > 1:
            bad.append(f"lse batch {b} ({p}) head {h} row {r}: err {err[h, r].item():.3e} > {c['lse_tol'][h, r].item():.3e}")
        if p == "large":
            # what the K-side-scaled dK|dV kernels exponentiate: K-side scores minus the kernel's own lse
            rowsum = torch.exp(c["s_k"] - lse[b].cpu().double()[..., None]).sum(-1)
            dev = (rowsum - 1).abs().max().item()
            print(f"large batch {b}: max |rowsum(P) - 1| with K-side rounding and the kernel's lse: {dev:.4f}")
            _RECORD["rowsum_large"][key] = dev
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("bwd_flags", PROD_FLAGS, ids=PROD_IDS)
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("profile", ao.PROFILES)
@pytest.mark.parametrize("B,S,Hq,Hkv", ao.SHAPES)
def test_flash_backward_per_block(B, S, Hq, Hkv, profile, causal, bwd_flags):
    """The backward gets its own forward's o and lse, as in training."""
    from tensorhive_fixed_amd.ops.attention import flash_bwd

    cases, qkv, dout, o, lse = _forward(B, S, Hq, Hkv, profile, causal)
    dqkv = flash_bwd(dout, qkv, o, lse, B, S, Hq, Hkv, D, causal=causal, flags=bwd_flags)
    flag_id = PROD_IDS[PROD_FLAGS.index(bwd_flags)]
    cols = {"dq": (0, Hq), "dk": (Hq, Hkv), "dv": (Hq + Hkv, Hkv)}
    bad = []
    for b, (p, c) in enumerate(zip(_batch_profiles(B, profile), cases)):
        key = _key(B, S, Hq, Hkv, p, causal, flag_id) + (f"|b{b}" if B > 1 else "")
        for name, (h0, nh) in cols.items():
            got = dqkv[b * S:(b + 1) * S, h0 * D:(h0 + nh) * D].reshape(S, nh, D)
            bad += _check_blocks(name, got, c, p, f"batch {b} ({p}) {flag_id}", key)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------- decode
@functools.lru_cache(maxsize=None)
def _decode_case(Hq, Hkv, profile):
    cache, q = do.profile_dead_cache(Hq, Hkv, do.PROFILE_LENS, profile, DEV)
    return cache, q, do.attention_fp64(q, cache)


@pytest.mark.parametrize("nsplit", do.NSPLITS, ids=lambda n: f"nsplit{n}")
@pytest.mark.parametrize("profile", ao.KEY_PROFILES)
@pytest.mark.parametrize("Hq,Hkv", [(8, 2), (8, 1)])
def test_decode_attention_profiles_per_row(Hq, Hkv, profile, nsplit):
    from tensorhive_fixed_amd.ops.decode_attention import decode_attention

    cache, q, ref = _decode_case(Hq, Hkv, profile)
    err, rel = do.assert_rows_close(decode_attention(q, cache, 0, nsplit=nsplit), ref, Hq)
    _RECORD["decode"][f"{profile}|{Hq}/{Hkv}|nsplit {nsplit}"] = [err, rel]


@pytest.mark.parametrize("nsplit", [3, None])
def test_decode_attention_ramp_up_is_bit_reproducible(nsplit):
    from tensorhive_fixed_amd.ops.decode_attention import decode_attention

    cache, q, _ = _decode_case(8, 2, "ramp_up")
    assert torch.equal(decode_attention(q, cache, 0, nsplit=nsplit), decode_attention(q, cache, 0, nsplit=nsplit))
