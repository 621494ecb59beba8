"""Cascade decode on a paged KV cache (ops/paged_cascade_attention.py) on the CPU: ``generate(cascade=True)`` against
plain ``generate``, ``common_prefix_rows`` and the op's refusals."""
import pytest
import torch

from tensorhive_fixed_amd.models.llama3 import Llama
from tensorhive_fixed_amd.ops.paged_attention import PagedKVCache
from tensorhive_fixed_amd.ops.paged_cascade_attention import paged_cascade_decode_attention
from tests.test_paged_chunk import CFG, SMAX, prefix_prompts


@pytest.mark.parametrize("N", [70, 10])
def test_generate_with_cascade_returns_the_plain_ids(N):
    model, (tok, lens) = Llama(CFG, device="cpu", seed=3), prefix_prompts()
    plain = model.generate(tok, lens, max_new_tokens=6)
    assert torch.equal(model.generate(tok, lens, max_new_tokens=6, paged_kv=True, shared_prefix=N, cascade=True), plain)


@pytest.mark.parametrize("kw", [{}, {"paged_kv": True}])
def test_generate_refuses_cascade_without_a_shared_prefix(kw):
    model, (tok, lens) = Llama(CFG, device="cpu", seed=3), prefix_prompts()
    with pytest.raises(ValueError, match="cascade"):
        model.generate(tok, lens, max_new_tokens=4, cascade=True, **kw)


def shared_cache():
    """Three sequences on the two pages of sequence 0, two of them with pages of their own behind."""
    cache = PagedKVCache(CFG, 3, SMAX, 8)
    assert cache.common_prefix_rows() == 0
    cache.reserve(0, 130)
    assert cache.common_prefix_rows() == 0  # the others hold nothing
    cache.set_lens([130, 0, 0])
    for b in (1, 2):
        cache.share_prefix(0, b, 128)
    return cache


def test_common_prefix_rows():
    cache = shared_cache()
    assert cache.common_prefix_rows() == 128 and cache.cascade_rows == 0
    cache.reserve(1, 200)
    cache.reserve(2, 129)
    assert cache.common_prefix_rows() == 128
    cache.cascade_rows = 128
    assert cache.cascade_rows == 128
    cache.release(2)
    assert cache.common_prefix_rows() == 0


@pytest.mark.parametrize("bad", ["part_page", "zero", "past_min_len", "table"])
def test_op_refusals_change_nothing(bad):
    cache = shared_cache()
    cache.reserve(1, 200)
    cache.set_lens([130, 200, 128])
    rows = {"part_page": 96, "zero": 0, "past_min_len": 192, "table": 128}[bad]
    if bad == "table":  # sequence 1 on a copy of the second page: same rows, another page
        cache.table[1][1] = cache.free_pages[-1]
    q = torch.ones(3, CFG.n_heads * 128, dtype=torch.bfloat16)
    state = (list(cache.lens), [list(t) for t in cache.table], cache.lens_dev.clone(), cache.table_dev.clone())
    with pytest.raises(ValueError, match="paged_cascade_decode_attention"):
        paged_cascade_decode_attention(q, cache, 0, rows)
    with pytest.raises(ValueError, match="cascade_rows"):
        cache.cascade_rows = rows or 64 + 1
    assert (cache.lens, cache.table, cache.cascade_rows) == (*state[:2], 0)
    assert torch.equal(cache.lens_dev, state[2]) and torch.equal(cache.table_dev, state[3])
    if bad != "table":
        assert paged_cascade_decode_attention(q, cache, 0, 128).shape == q.shape  # the good call beside it
