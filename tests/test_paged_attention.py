"""The paged KV cache (ops/paged_attention.py) on the CPU: the page allocator, prefix sharing, the
tiny model on a paged cache against the dense cache bit for bit, and what the feature refuses."""
import pytest
import torch

from tensorhive_fixed_amd.models.llama3 import Llama, LlamaConfig
from tensorhive_fixed_amd.ops.decode_attention import KVCache
from tensorhive_fixed_amd.ops.paged_attention import PAGE, PagedKVCache

CFG = LlamaConfig.tiny()


def _cache(n_pages=5, batch=3, max_len=256):
    return PagedKVCache(CFG, batch, max_len, n_pages)


def test_reserve_release_and_reuse():
    c = _cache()
    c.free_pages = [1, 4, 0, 3, 2]  # popped from the end
    c.reserve(0, 65)
    c.reserve(1, 1)
    assert c.table[:2] == [[2, 3], [0]] and c.table_dev[0, :2].tolist() == [2, 3]
    c.reserve(0, 128)  # already owned: nothing moves
    assert c.table[0] == [2, 3] and c.free_pages == [1, 4]
    c.set_lens([100, 1, 0])
    c.release(0)
    assert c.lens == [0, 1, 0] and c.lens_dev.tolist() == [0, 1, 0] and c.free_pages == [1, 4, 2, 3]
    c.reserve(2, 256)
    assert c.table[2] == [3, 2, 4, 1] and c.free_pages == []


def test_exhaustion_raises_and_changes_nothing():
    c = _cache()
    c.reserve(0, 200)
    state = ([list(t) for t in c.table], list(c.free_pages), c.table_dev.clone())
    for b, rows in ((1, 129), (0, 257)):  # 3 pages with 1 free; more rows than max_len
        with pytest.raises(ValueError, match="reserve"):
            c.reserve(b, rows)
    assert (c.table, c.free_pages) == state[:2] and torch.equal(c.table_dev, state[2])
    with pytest.raises(ValueError, match="reserve"):
        c.set_lens([0, 65, 0])  # rows nobody reserved


def test_share_prefix_counts_references():
    c = _cache()
    c.reserve(0, 130)
    c.set_lens([130, 0, 0])
    c.reserve(2, 1)
    for dst, rows in ((1, 100), (1, 192), (2, 64), (0, 64)):  # not whole pages, past lens[src], not empty (twice)
        with pytest.raises(ValueError, match="share_prefix"):
            c.share_prefix(0, dst, rows)
    c.share_prefix(0, 1, 128)
    assert c.table[1] == c.table[0][:2] and c.lens[1] == 128 and c.table_dev[1, :2].tolist() == c.table[0][:2]
    c.reserve(1, 129)  # the next append lands in a page of its own
    assert c.table[1][2] not in c.table[0]
    shared = c.table[0][:2]
    c.release(0)
    assert not set(shared) & set(c.free_pages) and len(c.free_pages) == 1  # only its unshared third page
    c.release(1)
    assert set(shared) <= set(c.free_pages) and len(c.free_pages) == 4


def _tokens():
    return torch.randint(0, CFG.vocab_size, (2, 64), generator=torch.Generator().manual_seed(11))


def test_decode_steps_on_a_paged_cache_match_the_dense_cache_bit_for_bit():
    model, tokens, lens = Llama(CFG, device="cpu", seed=3), _tokens(), [5, 17]
    dense = KVCache(CFG, 2, 64, "cpu")
    paged = PagedKVCache(CFG, 2, 64, 4)
    paged.free_pages = [2, 0, 3, 1]
    prompt = torch.zeros_like(tokens)
    for b, n in enumerate(lens):
        prompt[b, :n] = tokens[b, :n]
    assert torch.equal(model.prefill(prompt, lens, dense), model.prefill(prompt, lens, paged))
    assert paged.table == [[1], [3]]
    for i in range(6):
        step = torch.stack([tokens[b, n + i] for b, n in enumerate(lens)])
        assert torch.equal(model.decode_step(step, dense), model.decode_step(step, paged))
    assert paged.lens == dense.lens == [11, 23] and paged.lens_dev.tolist() == [11, 23]


def test_generate_with_a_paged_cache_returns_the_plain_ids():
    model, tokens = Llama(CFG, device="cpu", seed=3), _tokens()
    plain = model.generate(tokens[:, :60], [5, 60], max_new_tokens=8)  # the longer one crosses a page
    assert torch.equal(model.generate(tokens[:, :60], [5, 60], max_new_tokens=8, paged_kv=True), plain)


@pytest.mark.parametrize("kw", [{"graph": True}, {"kv_fp8": True}, {"speculate": 2}, {"prefill_chunk": 8}],
                         ids=lambda kw: next(iter(kw)))
def test_generate_refuses_paged_kv_with(kw):
    model = Llama(CFG, device="cpu", seed=3)
    with pytest.raises(ValueError, match="paged"):
        model.generate(_tokens()[:, :8], max_new_tokens=4, paged_kv=True, **kw)


@pytest.mark.parametrize("what", ["decode_graph", "extend_step", "prefill_chunk"])
def test_block_chunk_and_captured_steps_refuse_a_paged_cache(what):
    model, cache = Llama(CFG, device="cpu", seed=3), PagedKVCache(CFG, 2, 64, 2)
    tok = _tokens()[:, :4]
    call = {"decode_graph": lambda: model.decode_graph(cache), "extend_step": lambda: model.extend_step(tok, cache),
            "prefill_chunk": lambda: model.prefill_chunk(tok, [4, 4], cache)}[what]
    with pytest.raises(ValueError, match="paged"):
        call()
    assert cache.lens == [0, 0] and cache.table == [[], []] and PAGE == 64
