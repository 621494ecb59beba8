"""Chunked prefill on the CPU (fp32 references, tiny model): the argument checks of ``rope_append_chunk`` /
``chunk_attention``, ``Llama.prefill_chunk`` against ``prefill`` and against ``decode_step``s, and
``generate(prefill_chunk=N)`` against the one-shot run.  The model and prompts are those of
tests/test_speculate.py, whose seed leaves no near-tie between the top two logits."""
import pytest
import torch

from tensorhive_fixed_amd.ops.chunk_attention import chunk_attention, rope_append_chunk
from tensorhive_fixed_amd.ops.decode_attention import KVCache
from tests import test_speculate as ts
from tests.decode_oracles import attn_cfg

ULP = 2.0 ** -8


def _logits(m, h):
    return torch.mm(h, m.lm_head.t()).float()


def test_argument_checks():
    cache = KVCache(attn_cfg(4, 2), 2, 16)
    cache.set_lens([3, 10])
    q = torch.zeros(2, 5, 4 * 128, dtype=torch.bfloat16)
    qkv = torch.zeros(2, 5, 8 * 128, dtype=torch.bfloat16)
    for fn, x in ((rope_append_chunk, qkv), (chunk_attention, q)):
        assert fn(x, cache, 0, [5, 0]).shape == (2, 5, 4 * 128)
        for bad, new in ((x.float(), [1, 1]), (x[:, :, :128], [1, 1]), (x[0], [1, 1]), (x.transpose(0, 1), [1, 1]),
                         (x, [6, 1]), (x, [-1, 1]), (x, [1]), (x, [1, 7])):  # 10 + 7 rows > max_len 16
            with pytest.raises(ValueError, match=fn.__name__):
                fn(bad, cache, 0, new)
        with pytest.raises(ValueError, match="layer"):
            fn(x, cache, 1, [1, 1])
        with pytest.raises(ValueError, match="new_dev"):
            fn(x, cache, 0, [1, 1], torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="chunk"):
        chunk_attention(q, KVCache(attn_cfg(4, 2), 2, 16, dtype=torch.float8_e4m3fn), 0, [1, 1])
    with pytest.raises(ValueError, match="rep"):
        chunk_attention(torch.zeros(1, 2, 3 * 128, dtype=torch.bfloat16), KVCache(attn_cfg(3, 1), 1, 16), 0, [1])


def test_prefill_in_chunks_of_7_matches_prefill():
    m = ts.model()
    tokens, lens = ts.prompts("pattern_long")  # 37 and 49 tokens: ragged, and the last chunk is short
    ref_cache, cache = KVCache(m.cfg, 2, 64), KVCache(m.cfg, 2, 64)
    ref = _logits(m, m.prefill(tokens, lens, ref_cache))
    h = m._prefill_prompts(tokens, lens, max(lens), cache, 7)
    assert cache.lens == lens and cache.lens_dev.tolist() == lens
    assert (_logits(m, h) - ref).abs().max().item() <= ULP * ref.abs().max().item()
    for b, n in enumerate(lens):  # the same rows, up to the order of the fp32 sums before the bf16 rounding
        assert torch.allclose(cache.kv[:, :, b, :, :n].float(), ref_cache.kv[:, :, b, :, :n].float(), atol=2 ** -6)
        assert not cache.kv[:, :, b, :, n:].any()  # padding rows wrote nothing


def test_prefill_chunk_continues_a_cache_like_decode_steps():
    m = ts.model()
    tokens, lens = ts.prompts("random")
    more = torch.randint(0, m.cfg.vocab_size, (2, 9), generator=torch.Generator().manual_seed(3))
    new = [9, 4]
    ref_cache, cache = KVCache(m.cfg, 2, 32), KVCache(m.cfg, 2, 32)
    m.prefill(tokens, lens, ref_cache)
    m.prefill(tokens, lens, cache)
    got = _logits(m, m.prefill_chunk(more, new, cache))
    assert cache.lens == [5 + 9, 17 + 4]
    for b, n in enumerate(new):  # single steps of one sequence at a time: the other one rides along and is reset
        for t in range(n):
            before = list(ref_cache.lens)
            step = m.decode_step(more[:, t].contiguous(), ref_cache)
            ref_cache.set_lens([x + (i == b) for i, x in enumerate(before)])
        assert (got[b] - step[b]).abs().max().item() <= ULP * step[b].abs().max().item()
    with pytest.raises(ValueError, match="prefill_chunk"):
        m.prefill_chunk(more, [10, 1], cache)
    with pytest.raises(ValueError, match="prefill_chunk"):
        m.prefill_chunk(more[0], [1], cache)


def test_generate_with_prefill_chunk():
    m = ts.model()
    tokens, lens = ts.prompts("random")
    ref = ts.plain("random")[0]
    assert torch.equal(m.generate(tokens, lens, max_new_tokens=ts.NEW, prefill_chunk=5), ref)
    assert torch.equal(m.generate(tokens, lens, max_new_tokens=ts.NEW, prefill_chunk=5, speculate=3), ref)
    with pytest.raises(ValueError, match="prefill_chunk"):
        m.generate(tokens, lens, max_new_tokens=2, prefill_chunk=5, kv_fp8=True)
    with pytest.raises(ValueError, match="prefill_chunk"):
        m.generate(tokens, lens, max_new_tokens=2, prefill_chunk=0)
