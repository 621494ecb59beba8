"""The geometry builders of ``tests/decode_geometry_oracles.py`` and the CPU fp32 references on them: the
builders put NaN where they claim to, the permutations are what the GPU tests rely on, the project's
CPU references pass the per-row bounds on the sweep inputs at layer 1 (so a GPU failure on them is the
kernel's), the split geometry the device derives is the host's, and the closed form of the marked-row
caches agrees with the fp64 oracle on a miniature."""
import functools

import pytest
import torch

from tests import decode_geometry_oracles as dg
from tests import decode_kv_fp8_oracles as ko
from tests import decode_oracles as do
from tests import extend_oracles as eo

PERM = "longest@300"


@functools.lru_cache(maxsize=None)
def _sweep(Hq, Hkv, fp8):
    return dg.sweep_cache(Hq, Hkv, dg.SWEEP_LENS[PERM], "cpu", fp8=fp8)


def test_permutations():
    for name, lens in dg.SWEEP_LENS.items():
        assert sorted(lens) == list(range(1, dg.SWEEP_LONGEST + 1)), name
    assert dg.SWEEP_LENS["longest@0"][0] == dg.SWEEP_LONGEST
    assert dg.SWEEP_LENS["longest@300"].index(dg.SWEEP_LONGEST) == 300  # past the first trip of 64 lanes
    assert sorted(dg.BLOCK_LENS) == list(range(dg.BLOCK_LONGEST + 1))
    # chunks that are a multiple of no key tile (64 / 128 / 256 keys, 16 / 32 for the block kernel)
    for ns in dg.NSPLITS:
        assert dg.host_geometry(dg.SWEEP_LENS[PERM], 0, ns)[1] % 16
        for T in dg.BLOCKS:
            assert dg.host_geometry(dg.BLOCK_LENS, T, ns)[1] % 16 or ns == 1


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_sweep_cache_has_nan_where_it_claims(fp8):
    cache, q, ref = _sweep(4, 2, fp8)
    assert cache.kv.shape[0] == 2 and cache.max_len == dg.SWEEP_LONGEST + 8 and cache.batch == dg.SWEEP_LONGEST
    assert cache.lens == dg.SWEEP_LENS[PERM]
    assert dg.dead_rows_are_nan(cache, 1)
    assert torch.isfinite(ref).all() and ref.shape == (cache.batch, 4 * 128) and q.dtype == torch.bfloat16
    # two sequences differ at every live position, and the rows of a sequence are distinct
    k = cache.kv[1, 0].view(torch.uint8 if fp8 else torch.int16)
    a, b = dg.SWEEP_LENS[PERM].index(400), dg.SWEEP_LENS[PERM].index(399)
    assert bool((k[a, :, :399] != k[b, :, :399]).any(-1).all())
    assert len({bytes(r.numpy().tobytes()) for r in k[a, 0, :400]}) == 400
    # a cache that breaks the claim is seen
    cache.kv.view(torch.uint8)[1, 0, a, 0, 400] = 0
    assert not dg.dead_rows_are_nan(cache, 1)
    cache.kv.view(torch.uint8)[1, 0, a, 0, 400] = 0xFF if not fp8 else ko.NAN_CODE
    _sweep.cache_clear()


def test_block_cache_has_nan_where_it_claims():
    cache, q, ref = dg.sweep_block_cache(4, 2, dg.BLOCK_LENS, 3, "cpu")
    assert cache.max_len == dg.BLOCK_LONGEST + 3 + 8 and cache.lens == dg.BLOCK_LENS
    assert dg.dead_rows_are_nan(cache, 1, block=3) and not dg.dead_rows_are_nan(cache, 1, block=2)
    assert torch.isfinite(ref).all() and ref.shape == (dg.BLOCK_LONGEST + 1, 3, 4 * 128)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("Hq,Hkv", dg.HEADS)
def test_decode_reference_on_the_sweep(Hq, Hkv, fp8):
    from tensorhive_fixed_amd.ops.decode_attention import decode_attention, decode_attention_reference

    cache, q, ref = _sweep(Hq, Hkv, fp8)
    o = decode_attention_reference(q, cache, 1)
    do.assert_rows_close(o, ref, Hq)
    assert torch.equal(decode_attention(q, cache, 1, nsplit=3), o)  # CPU tensors run the reference


@pytest.mark.parametrize("T", dg.BLOCKS, ids=lambda t: f"T{t}")
@pytest.mark.parametrize("Hq,Hkv", dg.HEADS)
def test_extend_reference_on_the_sweep(Hq, Hkv, T):
    from tensorhive_fixed_amd.ops.extend_attention import extend_attention_reference

    cache, q, ref = dg.sweep_block_cache(Hq, Hkv, dg.BLOCK_LENS, T, "cpu")
    eo.assert_block_close(extend_attention_reference(q, cache, 1), ref, Hq)


def test_a_reference_on_the_wrong_layer_or_length_fails():
    """The bounds see one wrong sequence among 520: layer 0 is NaN, and one key fewer at length 300 is outside."""
    from tensorhive_fixed_amd.ops.decode_attention import decode_attention_reference

    cache, q, ref = _sweep(4, 2, False)
    with pytest.raises(AssertionError):
        do.assert_rows_close(decode_attention_reference(q, cache, 0), ref, 4)
    o = decode_attention_reference(q, cache, 1)
    b = dg.SWEEP_LENS[PERM].index(300)
    cache.lens[b] = 299
    try:
        o[b] = decode_attention_reference(q, cache, 1)[b]
    finally:
        cache.lens[b] = 300
    do.assert_attention_close(o, ref)  # the global bound alone does not notice
    with pytest.raises(AssertionError, match=f"sequence {b} "):
        do.assert_rows_close(o, ref, 4)


@pytest.mark.parametrize("name", list(dg.SWEEP_LENS))
def test_device_split_geometry_is_the_host_rule(name):
    from tensorhive_fixed_amd.ops.decode_attention import (MIN_KEYS_PER_SPLIT, device_split_geometry,
                                                           pick_nsplit)

    lens, max_len = dg.SWEEP_LENS[name], dg.SWEEP_LONGEST + 8
    for ns in (3, 7):
        assert device_split_geometry(lens, 0, ns, max_len, min_keys=1, cap=ns) == dg.host_geometry(lens, 0, ns)
    for Hkv in (1, 2):
        for cus in (256, 4096):  # 4096: a `want` above 1 at this batch
            want = -(-cus // (len(lens) * Hkv))
            ns = pick_nsplit(len(lens), Hkv, max(lens), cus)
            cap = pick_nsplit(len(lens), Hkv, max_len, cus)
            assert device_split_geometry(lens, 0, want, max_len, MIN_KEYS_PER_SPLIT, cap) == \
                dg.host_geometry(lens, 0, ns)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_marked_closed_form_against_fp64_on_a_miniature(fp8):
    """The construction of the 2^24-row tests at 4096 rows: zeros, four marked keys, NaN past the length."""
    from tensorhive_fixed_amd.ops.decode_attention import KVCache

    S, n = 4096, 4096 - 3
    cache = KVCache(do.attn_cfg(1, 1, max_seq_len=S), 1, S, "cpu", dtype=dg.FP8 if fp8 else torch.bfloat16)
    keys = dg.marked_keys(n)
    k, v = dg.marked_rows(4)
    fill = torch.zeros(1, 1, S, 128, dtype=torch.bfloat16)
    kk, vv = fill.clone(), fill.clone()
    kk[0, 0, keys], vv[0, 0, keys] = k, v
    cache.fill(0, kk, vv)
    if fp8:
        cache.kv.view(torch.uint8)[:, :, :, :, n:] = ko.NAN_CODE
        cache.kv_scale[:, :, :, :, n:] = float("nan")
        km = cache.kv[0, 0, 0, 0, keys].double() * cache.kv_scale[0, 0, 0, 0, keys].double()[:, None]
        vm = cache.kv[0, 1, 0, 0, keys].double() * cache.kv_scale[0, 1, 0, 0, keys].double()[:, None]
    else:
        cache.kv[:, :, :, :, n:] = float("nan")
        km, vm = k, v
    cache.set_lens([n])
    q = torch.ones(1, 128, dtype=torch.bfloat16)
    ref = ko.attention_fp64_fp8(q, cache) if fp8 else do.attention_fp64(q, cache)
    closed = dg.marked_closed_form(km, vm, n)
    assert (closed - ref[0]).abs().max().item() < 1e-12
    # each marked row carries about a quarter of the output: one read from a zero row is far outside the bound
    w = 1.0 / (4 + (n - 4) / torch.tensor(128 * dg.MARKED_K / 128 ** 0.5).exp().item())
    assert 0.2 < w < 0.25
    wrong = dg.marked_closed_form(km[:3], vm[:3], n)
    with pytest.raises(AssertionError):
        do.assert_rows_close(wrong[None, :].float(), ref, 1)
