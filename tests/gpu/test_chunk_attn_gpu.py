"""The chunked-prefill kernels (csrc/chunk_attn.hip) on the GPU: ``chunk_attention`` against fp64 per
(b, t, head) row at the query-tile and key-tile boundaries with ragged old and new lengths, causality and
isolation bit for bit, agreement with the block kernel, ``rope_append_chunk`` against single appends, and
``Llama.prefill_chunk`` / ``generate(prefill_chunk=N)`` on the tiny model."""
import pytest
import torch

from tensorhive_fixed_amd.ops.chunk_attention import KEY_TILE, QUERY_TILE, chunk_attention, rope_append_chunk
from tensorhive_fixed_amd.ops.decode_attention import KVCache, rope_append
from tensorhive_fixed_amd.ops.extend_attention import extend_attention
from tests import extend_oracles as eo
from tests import test_speculate as ts
from tests.decode_oracles import attn_cfg

pytestmark = pytest.mark.gpu

DEV = "cuda"
SMAX = eo.SMAX
HEADS = [(2, 2), (4, 2), (4, 1), (8, 1)]  # rep 1, 2, 4, 8
ULP = 2.0 ** -8


def tile_tokens(Hq, Hkv):
    return QUERY_TILE // (Hq // Hkv)


def old_lens(T):
    return [[0, 1, 63], [64, 65, 200], [KEY_TILE - 1, KEY_TILE, SMAX - T]]


def new_lens(T, case):
    return [[T, min(1, T), T - 1], [0, T, min(1, T)], [T - 1, T, T]][case]


def chunk_cache(Hq, Hkv, lens, new, T, poison=float("nan")):
    """``nan_dead_block_cache`` with every cache row at or past ``lens[b] + new[b]`` and every q row
    ``t >= new[b]`` poisoned as well."""
    cache, q = eo.nan_dead_block_cache(Hq, Hkv, lens, T, DEV)
    for b, (n, k) in enumerate(zip(lens, new)):
        cache.kv[:, :, b, :, n + k:] = poison
        q[b, k:] = poison
    return cache, q


def assert_live_rows_close(o, ref, new, Hq):
    live = torch.cat([o[b, :k] for b, k in enumerate(new)])
    eo.assert_block_close(live[None], torch.cat([ref[b, :k] for b, k in enumerate(new)])[None], Hq)
    for b, k in enumerate(new):
        assert not o[b, k:].any(), f"sequence {b}: rows past new_lens are not exactly zero"


@pytest.mark.parametrize("case", [0, 1, 2])
@pytest.mark.parametrize("tile_off", [None, -1, 0, 1], ids=["T1", "tile-1", "tile", "tile+1"])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_chunk_attention_against_fp64(Hq, Hkv, tile_off, case):
    T = 1 if tile_off is None else tile_tokens(Hq, Hkv) + tile_off
    lens, new = old_lens(T)[case], new_lens(T, case)
    cache, q = chunk_cache(Hq, Hkv, lens, new, T)
    o = chunk_attention(q, cache, 0, new)
    assert_live_rows_close(o.cpu(), eo.extend_fp64(q, cache), new, Hq)


@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_a_later_row_changes_no_bit_of_the_rows_before_it(Hq, Hkv):
    T = tile_tokens(Hq, Hkv) + 1
    lens, new = [0, KEY_TILE - 1, 200], [T, T - 1, 2]
    cache, q = chunk_cache(Hq, Hkv, lens, new, T, poison=0.0)
    before = chunk_attention(q, cache, 0, new)
    for b, (n, k) in enumerate(zip(lens, new)):
        cache.kv[:, :, b, :, n + k - 1] = 3.0e4  # K and V of the last live row: large, finite
    after = chunk_attention(q, cache, 0, new)
    for b, k in enumerate(new):
        assert torch.equal(before[b, : k - 1], after[b, : k - 1]), f"sequence {b}"

@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_a_nan_sequence_leaves_the_others_alone_and_runs_repeat(Hq, Hkv):
    T = tile_tokens(Hq, Hkv) + 1
    lens, new = [70, 5, 300], [T, T, T - 1]
    cache, q = chunk_cache(Hq, Hkv, lens, new, T)
    clean = chunk_attention(q, cache, 0, new)
    assert torch.equal(clean, chunk_attention(q, cache, 0, new))
    cache.kv[:, :, 1] = float("nan")
    q[1] = float("nan")
    dirty = chunk_attention(q, cache, 0, new)
    assert torch.equal(clean[0], dirty[0]) and torch.equal(clean[2], dirty[2])


@pytest.mark.parametrize("T", [1, 5, 8])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_agrees_with_the_block_kernel(Hq, Hkv, T):
    cache, q = eo.nan_dead_block_cache(Hq, Hkv, [0, KEY_TILE - 3, SMAX - T], T, DEV)
    o = chunk_attention(q, cache, 0, [T] * 3)
    eo.assert_block_close(o.cpu(), extend_attention(q, cache, 0).cpu().double(), Hq)


@pytest.mark.parametrize("T", [1, 9, 130])
def test_rope_append_chunk_has_the_bits_of_single_appends(T):
    Hq, Hkv, lens = 4, 2, [0, 37, SMAX - T]
    new = [T, T // 2, max(T - 1, 1)]
    cfg = attn_cfg(Hq, Hkv, n_layers=2)
    qkv = torch.randn(3, T, (Hq + 2 * Hkv) * 128, generator=torch.Generator().manual_seed(T)).bfloat16().to(DEV)
    cache, ref = KVCache(cfg, 3, SMAX, DEV), KVCache(cfg, 3, SMAX, DEV)
    for c in (cache, ref):
        c.kv.fill_(-7.0)  # the sentinel
        c.set_lens(lens)
    q = rope_append_chunk(qkv, cache, 1, new)
    assert cache.lens == lens
    q_ref = []
    for t in range(T):
        q_ref.append(rope_append(qkv[:, t].contiguous(), ref, 1))
        ref.advance(1)
    q_ref = torch.stack(q_ref, dim=1)
    assert (cache.kv[0] == -7.0).all(), "the other layer was written"
    for b, (n, k) in enumerate(zip(lens, new)):
        assert torch.equal(q[b, :k], q_ref[b, :k]) and not q[b, k:].any()
        assert torch.equal(cache.kv[1, :, b, :, n: n + k], ref.kv[1, :, b, :, n: n + k])
        assert (cache.kv[1, :, b, :, :n] == -7.0).all() and (cache.kv[1, :, b, :, n + k:] == -7.0).all()


@pytest.mark.parametrize("new", [[16, 16], [9, 16]])
def test_prefill_chunk_logits_no_worse_than_the_full_forward(new):
    from tests.gpu import test_speculate_gpu as tg

    _, gpu, tokens = tg._pair()
    ref, full = tg._references()
    cache, _ = tg._prefilled(gpu, tokens.to(DEV), tg.LENS)
    chunk = torch.stack([tokens[b, n: n + 16] for b, n in enumerate(tg.LENS)]).to(DEV)
    got = torch.mm(gpu.prefill_chunk(chunk, new, cache), gpu.lm_head.t()).float().cpu()
    assert cache.lens == [n + k for n, k in zip(tg.LENS, new)] == cache.lens_dev.tolist()
    rows = [n + k - 1 for n, k in zip(tg.LENS, new)]
    e_new = max((got[b] - ref[b, r]).abs().max().item() for b, r in enumerate(rows))
    e_full = max((full[b, r] - ref[b, r]).abs().max().item() for b, r in enumerate(rows))
    peak = max(ref[b, r].abs().max().item() for b, r in enumerate(rows))
    print(f"new {new}  e_new {e_new:.5f}  e_full {e_full:.5f}  max|logit| {peak:.4f}")
    assert e_new <= 2 * e_full + ULP * peak


def test_generate_with_prefill_chunk_matches_plain_generate():
    from tests.gpu import test_speculate_gpu as tg

    _, gpu, _ = tg._pair()
    tokens, lens = ts.prompts("random")
    plain = gpu.generate(tokens.to(DEV), lens, max_new_tokens=ts.NEW)
    assert torch.equal(gpu.generate(tokens.to(DEV), lens, max_new_tokens=ts.NEW, prefill_chunk=8), plain)
