"""The gfx950 block-decode kernels (csrc/extend_attn.hip) on the GPU: ``extend_attention`` against an fp64
softmax per query row with NaN in every dead cache row, rows with no live key in a split, causality as
isolation, T = 1 against ``decode_attention``, bit reproducibility, score profiles, and
``rope_append_block`` bit for bit against T single appends."""
import functools

import pytest
import torch

from tests import decode_oracles as do
from tests import extend_oracles as eo

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from tensorhive_fixed_amd.ops import _lib
    _lib.load(build_if_missing=True)
    assert hasattr(_lib.load(), "th_extend_attn") and hasattr(_lib.load(), "th_decode_rope_append_block")


@functools.lru_cache(maxsize=None)
def _case(Hq, Hkv, lens, T):
    """Inputs and their fp64 reference, computed once per shape and shared by the split counts."""
    cache, q = eo.nan_dead_block_cache(Hq, Hkv, list(lens), T, DEV)
    return cache, q, eo.extend_fp64(q, cache)


def _extend(q, cache, nsplit=None):
    from tensorhive_fixed_amd.ops.extend_attention import extend_attention

    return extend_attention(q, cache, 0, nsplit=nsplit)


@pytest.mark.parametrize("nsplit", do.NSPLITS, ids=lambda n: f"nsplit{n}")
@pytest.mark.parametrize("li", range(len(eo.block_lens(1))), ids=lambda i: f"lens{i}")
@pytest.mark.parametrize("T", eo.BLOCKS, ids=lambda t: f"T{t}")
@pytest.mark.parametrize("Hq,Hkv", eo.HEADS)
def test_extend_attention_against_fp64(Hq, Hkv, T, li, nsplit):
    cache, q, ref = _case(Hq, Hkv, tuple(eo.block_lens(T)[li]), T)
    eo.assert_block_close(_extend(q, cache, nsplit), ref, Hq)


@pytest.mark.parametrize("lens,nsplit", [((13,), 3), ((5, 900), 8)], ids=["13-nsplit3", "5-900-nsplit8"])
def test_rows_without_a_live_key_in_a_split(lens, nsplit):
    """[13] + 8 in 3 chunks of 7: the last split starts at key 14, which query row 0 (keys 0..13) never
    sees; [5, 900]: every split but the first is empty for the short sequence."""
    cache, q, ref = _case(8, 2, lens, 8)
    eo.assert_block_close(_extend(q, cache, nsplit), ref, 8)


@pytest.mark.parametrize("T", [2, 5, 8])
def test_causality_as_isolation(T):
    """NaN in K and V of the block's last row changes no bit of the query rows before it."""
    cache, q, _ = _case(8, 2, (63, 200, 1024 - T), T)
    a = _extend(q, cache, 3)
    kv = cache.kv.clone()
    try:
        for b, n in enumerate(cache.lens):
            cache.kv[:, :, b, :, n + T - 1] = float("nan")
        b_ = _extend(q, cache, 3)
    finally:
        cache.kv.copy_(kv)
    assert torch.isfinite(b_[:, : T - 1].float()).all()
    assert torch.equal(a[:, : T - 1], b_[:, : T - 1])


@pytest.mark.parametrize("Hq,Hkv", eo.HEADS)
def test_single_token_block_against_decode_attention(Hq, Hkv):
    from tensorhive_fixed_amd.ops.decode_attention import decode_attention

    cache, q, ref = _case(Hq, Hkv, (1, 200, 1023), 1)
    eo.assert_block_close(_extend(q, cache), ref, Hq)
    single = decode_attention(q.view(3, -1), cache, 0, new=1)
    eo.assert_block_close(single.view(3, 1, -1), ref, Hq)


@pytest.mark.parametrize("nsplit", [3, None])
def test_extend_attention_is_bit_reproducible(nsplit):
    cache, q, _ = _case(8, 2, (1, 200, 1016), 8)
    a = _extend(q, cache, nsplit)
    assert torch.equal(a, _extend(q, cache, nsplit))
    kv = cache.kv.clone()
    try:  # a batch entry whose live rows are NaN leaves the others alone
        cache.kv[:, :, 1] = float("nan")
        b = _extend(q, cache, nsplit)
    finally:
        cache.kv.copy_(kv)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize("profile", ["rising_spikes", "ramp_up"])
def test_extend_attention_on_score_profiles(profile):
    """Scores that keep moving the running max; the T rows of a block carry different gains."""
    Hq, Hkv, T = 8, 2, 4
    cache, q1 = do.profile_dead_cache(Hq, Hkv, do.PROFILE_LENS, profile, DEV)
    cache.set_lens([n - T for n in do.PROFILE_LENS])  # the last T live rows are the block
    gains = torch.tensor([1.0, 0.75, 0.5, 0.25], device=DEV, dtype=torch.bfloat16)
    q = (q1[:, None, :] * gains[None, :, None]).contiguous()
    ref = eo.extend_fp64(q, cache)
    for nsplit in (1, 3, None):
        eo.assert_block_close(_extend(q, cache, nsplit), ref, Hq)


@pytest.mark.parametrize("T", [1, 3, 8])
def test_rope_append_block_matches_single_appends(T):
    from tensorhive_fixed_amd.ops.decode_attention import KVCache, rope_append
    from tensorhive_fixed_amd.ops.extend_attention import rope_append_block

    Hq, Hkv = 8, 2
    pos = [0, 77, do.SMAX - T]
    cfg = do.attn_cfg(Hq, Hkv, n_layers=2)
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(3, T, (Hq + 2 * Hkv) * 128, generator=g).to(torch.bfloat16).to(DEV)
    caches = []
    for _ in range(2):
        c = KVCache(cfg, 3, do.SMAX, DEV)
        c.kv.fill_(-7.0)  # a sentinel: any other row written shows
        c.set_lens(pos)
        caches.append(c)
    blk, one = caches
    q_blk = rope_append_block(qkv, blk, 1)
    q_one = []
    for t in range(T):
        q_one.append(rope_append(qkv[:, t].contiguous(), one, 1))
        one.advance(1)
    assert blk.lens == pos  # the block append does not move the lengths
    assert torch.equal(q_blk, torch.stack(q_one, dim=1))
    assert torch.equal(blk.kv, one.kv)
    written = (blk.kv != -7.0).any(-1).sum().item()
    assert written <= 2 * 3 * Hkv * T and written > 0
