"""Chunk steps on a paged KV cache (ops/paged_chunk_attention.py) on the CPU: the ops and the tiny model bit for
bit against the dense cache, ``generate(shared_prefix=N)`` against plain ``generate``, and the refusals."""
import pytest
import torch

from tensorhive_fixed_amd.models.llama3 import Llama, LlamaConfig
from tensorhive_fixed_amd.ops.chunk_attention import chunk_attention, rope_append_chunk
from tensorhive_fixed_amd.ops.decode_attention import KVCache
from tensorhive_fixed_amd.ops.paged_attention import PagedKVCache, pages_for
from tensorhive_fixed_amd.ops.paged_chunk_attention import paged_chunk_attention, paged_rope_append_chunk

CFG = LlamaConfig.tiny()
SMAX = 320
QKV = (CFG.n_heads + 2 * CFG.n_kv_heads) * 128


def permuted(cache):
    cache.free_pages = list(range(0, cache.n_pages, 2)) + list(range(1, cache.n_pages, 2))  # no neighbours adjacent
    return cache


def with_rows(pool, cache, layer, b, k, v, first):
    """``pool`` with ``k`` / ``v [Hkv, n, 128]`` at rows ``first ..`` of sequence ``b``, through ``cache``'s table."""
    r = torch.arange(first, first + k.shape[1], device=pool.device)
    page = torch.tensor(cache.table[b], dtype=torch.long, device=pool.device)[r // 64]
    pool[layer, :, page, :, r % 64] = torch.stack([k, v]).permute(2, 0, 1, 3)
    return pool


@pytest.mark.parametrize("T", [1, 9, 70])
@pytest.mark.parametrize("lens", [[0, 37, 63], [64, 65, 200]], ids=lambda v: "-".join(map(str, v)))
def test_ops_through_a_permuted_table_have_the_dense_bits(lens, T):
    new = [T, 0, max(T - 1, 1)]
    g = torch.Generator().manual_seed(T)
    dense = KVCache(CFG, 3, SMAX, "cpu")
    dense.kv.copy_(torch.randn(dense.kv.shape, generator=g))
    paged = permuted(PagedKVCache(CFG, 3, SMAX, sum(pages_for(n + k) for n, k in zip(lens, new)) + 2))
    paged.pool.copy_(torch.randn(paged.pool.shape, generator=g))  # the sentinel
    for b, n in enumerate(lens):
        paged.reserve(b, n)
        with_rows(paged.pool, paged, 1, b, dense.kv[1, 0, b, :, :n], dense.kv[1, 1, b, :, :n], 0)
    for c in (dense, paged):
        c.set_lens(lens)
    qkv = torch.randn(3, T, QKV, generator=g).bfloat16()
    want = paged.pool.clone()
    q = paged_rope_append_chunk(qkv, paged, 1, new)
    assert torch.equal(q, rope_append_chunk(qkv, dense, 1, new)) and paged.lens == lens
    for b, (n, k) in enumerate(zip(lens, new)):
        with_rows(want, paged, 1, b, dense.kv[1, 0, b, :, n: n + k], dense.kv[1, 1, b, :, n: n + k], n)
    assert torch.equal(paged.pool, want)  # the dense rows, and no other row, page or layer
    assert torch.equal(paged_chunk_attention(q, paged, 1, new), chunk_attention(q, dense, 1, new))


def test_tiny_model_prefill_paged_chunk_equals_prefill_chunk():
    model = Llama(CFG, device="cpu", seed=3)
    tok = torch.randint(0, CFG.vocab_size, (2, 160), generator=torch.Generator().manual_seed(11))
    dense, paged = KVCache(CFG, 2, SMAX, "cpu"), permuted(PagedKVCache(CFG, 2, SMAX, 5))
    assert torch.equal(model.prefill_paged_chunk(tok[:, :70].contiguous(), [70, 0], paged)[:1],
                       model.prefill_chunk(tok[:, :70].contiguous(), [70, 0], dense)[:1])
    paged.share_prefix(0, 1, 64)
    dense.kv[:, :, 1, :, :64] = dense.kv[:, :, 0, :, :64]  # what sharing means for the dense cache: a copy
    dense.set_lens([70, 64])
    got = model.prefill_paged_chunk(tok[1:, 64:137].contiguous(), [73], paged, seqs=[1])
    assert torch.equal(got, model.prefill_chunk(tok[:, 64:137].contiguous(), [0, 73], dense)[1:])
    assert paged.lens == dense.lens == [70, 137] == paged.lens_dev.tolist()
    assert paged.table[1][0] == paged.table[0][0] and len(paged.table[1]) == 3 and len(paged.free_pages) == 1


def prefix_prompts(B=3):
    tok = torch.randint(0, CFG.vocab_size, (B, 100), generator=torch.Generator().manual_seed(5))
    tok[:, :71] = tok[:1, :71]  # they differ from token 71 on
    return tok, [75, 100, 90][:B]


@pytest.mark.parametrize("N", [70, 10])
def test_generate_with_a_shared_prefix_returns_the_plain_ids(N):
    model, (tok, lens) = Llama(CFG, device="cpu", seed=3), prefix_prompts()
    plain = model.generate(tok, lens, max_new_tokens=6)
    assert torch.equal(model.generate(tok, lens, max_new_tokens=6, paged_kv=True, shared_prefix=N), plain)


@pytest.mark.parametrize("kw", [{"paged_kv": False}, {"shared_prefix": 0}, {"shared_prefix": 75}, {"shared_prefix": 72},
                                {"graph": True}, {"kv_fp8": True}, {"speculate": 2}, {"prefill_chunk": 8}],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_generate_refuses_shared_prefix_with(kw):
    model, (tok, lens) = Llama(CFG, device="cpu", seed=3), prefix_prompts()
    assert tok[0, 71] != tok[1, 71]
    with pytest.raises(ValueError, match="shared_prefix|paged"):
        model.generate(tok, lens, **{"max_new_tokens": 4, "paged_kv": True, "shared_prefix": 70, **kw})


BAD = {"good": {}, "shared_page": dict(lens=[100, 128]), "pool_short": dict(n_pages=5), "max_len": dict(lens=[128, 312]),
       "new_lens": dict(new=[10, 1]), "seqs_twice": dict(seqs=[1, 1]), "seqs_range": dict(seqs=[0, 2]),
       "dtype": dict(x=torch.float32), "shape": dict(cols=128), "new_dev": dict(new_dev=torch.zeros(2))}


@pytest.mark.parametrize("bad", BAD)
def test_op_refusals_change_nothing(bad):
    kw = {"lens": [128, 128], "new": [9, 9], "seqs": [0, 1], "x": torch.bfloat16, "new_dev": None, "n_pages": 7,
          "cols": QKV, **BAD[bad]}
    paged = PagedKVCache(CFG, 2, SMAX, kw["n_pages"])
    paged.reserve(0, 128)
    paged.set_lens([128, 0])
    paged.share_prefix(0, 1, 128)  # both sequences hold the same two pages
    paged.reserve(1, 320)
    paged.set_lens(kw["lens"])
    state = ([list(t) for t in paged.table], list(paged.free_pages), paged.table_dev.clone(), paged.pool.clone())
    qkv = torch.ones(2, 9, kw["cols"], dtype=kw["x"])
    if bad == "good":  # the call every other case spoils in one place
        assert paged_rope_append_chunk(qkv, paged, 0, kw["new"]).any() and len(paged.table[0]) == 3
        return
    with pytest.raises(ValueError, match="paged_rope_append_chunk"):
        paged_rope_append_chunk(qkv, paged, 0, kw["new"], kw["new_dev"], seqs=kw["seqs"])
    assert (paged.table, paged.free_pages, paged.lens) == (*state[:2], kw["lens"]) and paged.lens_dev.tolist() == kw["lens"]
    assert torch.equal(paged.table_dev, state[2]) and torch.equal(paged.pool, state[3])
