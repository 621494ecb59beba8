"""``chunk_attention`` split over the keys (``th_chunk_attn_split``) on the GPU: against fp64 with splits
that are empty, end inside the new block or lie past a row's limit, over a workspace full of NaN; its bits
against the unsplit launch, a second run and a NaN neighbour; and the call the rule itself splits."""
import pytest
import torch

from tensorhive_fixed_amd.ops.chunk_attention import QUERY_TILE, chunk_attention, pick_chunk_nsplit
from tensorhive_fixed_amd.ops.decode_attention import KVCache
from tests import extend_oracles as eo
from tests.decode_oracles import attn_cfg
from tests.gpu.test_chunk_attn_gpu import (DEV, HEADS, assert_live_rows_close, chunk_cache, new_lens, old_lens,
                                           tile_tokens)

pytestmark = pytest.mark.gpu


def poison_workspace(cache, Hkv, T, rep, nsplit):
    cache.workspace(cache.batch * Hkv * -(-T * rep // QUERY_TILE) * nsplit * QUERY_TILE * 130).fill_(float("nan"))


@pytest.mark.parametrize("case", [0, 1, 2])
@pytest.mark.parametrize("nsplit", [2, 3, 7])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_split_chunk_attention_against_fp64(Hq, Hkv, nsplit, case):
    T = tile_tokens(Hq, Hkv) + 1  # two query tiles, the second holds one token
    lens, new = old_lens(T)[case], new_lens(T, case)
    cache, q = chunk_cache(Hq, Hkv, lens, new, T)
    poison_workspace(cache, Hkv, T, Hq // Hkv, nsplit)
    o = chunk_attention(q, cache, 0, new, nsplit=nsplit)
    assert_live_rows_close(o.cpu(), eo.extend_fp64(q, cache), new, Hq)


@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_split_bits(Hq, Hkv):
    T = tile_tokens(Hq, Hkv) + 1
    lens, new = [70, 5, 300], [T, T, T - 1]
    cache, q = chunk_cache(Hq, Hkv, lens, new, T)
    assert torch.equal(chunk_attention(q, cache, 0, new, nsplit=1), chunk_attention(q, cache, 0, new))
    clean = chunk_attention(q, cache, 0, new, nsplit=3)
    assert torch.equal(clean, chunk_attention(q, cache, 0, new, nsplit=3))
    cache.kv[:, :, 1] = float("nan")
    q[1] = float("nan")
    dirty = chunk_attention(q, cache, 0, new, nsplit=3)
    assert torch.equal(clean[0], dirty[0]) and torch.equal(clean[2], dirty[2])


def test_the_rule_splits_a_short_chunk_on_a_long_cache():
    Hq, Hkv, T, old, smax = 4, 1, 40, 2100, 2304
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    assert pick_chunk_nsplit(1, Hkv, Hq // Hkv, T, old + T, cus) >= 2
    g = torch.Generator().manual_seed(0)
    cache = KVCache(attn_cfg(Hq, Hkv, max_seq_len=smax), 1, smax, DEV)
    kv = torch.randn(cache.kv.shape, generator=g).bfloat16()
    kv[:, :, :, :, old + T:] = float("nan")
    cache.kv.copy_(kv)
    cache.set_lens([old])
    q = torch.randn(1, T, Hq * 128, generator=g).bfloat16().to(DEV)
    poison_workspace(cache, Hkv, T, Hq // Hkv, 16)
    o = chunk_attention(q, cache, 0, [T])
    eo.assert_block_close(o.cpu(), eo.extend_fp64(q, cache), Hq)
