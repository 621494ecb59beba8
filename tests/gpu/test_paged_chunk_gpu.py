"""The paged chunk kernels (csrc/chunk_attn.hip, ops/paged_chunk_attention.py) on the GPU, through permuted page
tables with NaN wherever a sequence owns nothing: the dense kernels' bits, fp64 bounds, the tiny model."""
import functools
import math

import pytest
import torch

from tensorhive_fixed_amd.ops import _lib
from tensorhive_fixed_amd.ops.chunk_attention import chunk_attention, rope_append_chunk
from tensorhive_fixed_amd.ops.decode_attention import KVCache
from tensorhive_fixed_amd.ops.paged_attention import PagedKVCache, pages_for
from tensorhive_fixed_amd.ops.paged_chunk_attention import paged_chunk_attention, paged_rope_append_chunk
from tests import extend_oracles as eo
from tests.decode_oracles import attn_cfg
from tests.gpu import test_speculate_gpu as tg
from tests.gpu.test_chunk_attn_gpu import (DEV, HEADS, SMAX, ULP, assert_live_rows_close, chunk_cache, new_lens,
                                           old_lens, tile_tokens)
from tests.gpu.test_chunk_attn_split_gpu import poison_workspace
from tests.test_paged_chunk import permuted as _permute, with_rows

pytestmark = pytest.mark.gpu
NAN = float("nan")


def paged_from(dense, new, permute=True, spare=3):
    """Layer 0 of ``dense`` in a paged cache: NaN in every unowned page and every row at or past ``lens + new``
    (``dense`` has it there), table entries past a sequence's pages out of range, no two neighbours adjacent."""
    rows = [n + k for n, k in zip(dense.lens, new)]
    cache = PagedKVCache(dense.cfg, dense.batch, SMAX, sum(pages_for(r) for r in rows) + spare, DEV)
    cache.pool.fill_(NAN)
    if permute:
        _permute(cache)
    for b, r in enumerate(rows):
        cache.reserve(b, r)
    cache.fill(0, dense.k(0), dense.v(0))
    cache.set_lens(dense.lens)
    for b in range(dense.batch):
        cache.table_dev[b, len(cache.table[b]):] = cache.n_pages + 7
    return cache


@functools.lru_cache(maxsize=None)
def _case(Hq, Hkv, T, case):
    lens, new = old_lens(T)[case], new_lens(T, case)
    dense, q = chunk_cache(Hq, Hkv, lens, new, T)
    return dense, q, new, eo.extend_fp64(q, dense), paged_from(dense, new)


@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("case", [0, 1, 2])
@pytest.mark.parametrize("tile_off", [None, -1, 1], ids=["T1", "tile-1", "tile+1"])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_paged_chunk_attention_has_the_dense_bits(Hq, Hkv, tile_off, case, nsplit):
    T = 1 if tile_off is None else tile_tokens(Hq, Hkv) + tile_off
    dense, q, new, ref, paged = _case(Hq, Hkv, T, case)
    poison_workspace(paged, Hkv, T, Hq // Hkv, nsplit)
    o = paged_chunk_attention(q, paged, 0, new, nsplit=nsplit)
    assert torch.equal(o, chunk_attention(q, dense, 0, new, nsplit=nsplit))
    assert_live_rows_close(o.cpu(), ref, new, Hq)


@pytest.mark.parametrize("nsplit", [1, 3, None])
def test_placement_is_invisible(nsplit):
    dense, q, new, _, permuted = _case(8, 1, tile_tokens(8, 1) + 1, 2)
    identity = paged_from(dense, new, permute=False)
    assert identity.table[0] == [0, 1] and permuted.table != identity.table
    a = paged_chunk_attention(q, permuted, 0, new, nsplit=nsplit)
    assert torch.equal(a, paged_chunk_attention(q, identity, 0, new, nsplit=nsplit))
    assert torch.equal(a, paged_chunk_attention(q, permuted, 0, new, nsplit=nsplit))


@pytest.mark.parametrize("T", [1, 9, 130])
def test_paged_append_has_the_dense_bits_and_a_bad_table_entry_stores_nothing(T):
    Hq, Hkv, lens = 4, 2, [0, 37, SMAX - T]
    new = [T, T // 2 + 1, max(T - 1, 1)]
    cfg = attn_cfg(Hq, Hkv, n_layers=2)
    g = torch.Generator().manual_seed(T)
    qkv = torch.randn(3, T, (Hq + 2 * Hkv) * 128, generator=g).bfloat16().to(DEV)
    dense = KVCache(cfg, 3, SMAX, DEV)
    dense.set_lens(lens)
    q_ref = rope_append_chunk(qkv, dense, 1, new)
    sentinel = torch.randn((2, 2, 24, Hkv, 64, 128), generator=g).bfloat16().to(DEV)
    pools = []
    for bad in (False, True):
        paged = _permute(PagedKVCache(cfg, 3, SMAX, 24, DEV))
        paged.pool.copy_(sentinel)
        for b, (n, k) in enumerate(zip(lens, new)):
            paged.reserve(b, n + k)
        paged.set_lens(lens)
        if bad:  # the page of sequence 1's first new rows
            paged.table_dev[1, 0] = 24
        assert torch.equal(paged_rope_append_chunk(qkv, paged, 1, new), q_ref) and paged.lens == lens
        pools.append(paged)
    good, bad = pools
    want = sentinel.clone()
    for b, (n, k) in enumerate(zip(lens, new)):
        with_rows(want, good, 1, b, dense.kv[1, 0, b, :, n: n + k], dense.kv[1, 1, b, :, n: n + k], n)
    assert torch.equal(good.pool, want)  # the dense append's rows, and no other row, page or layer
    want[:, :, good.table[1][0]] = sentinel[:, :, good.table[1][0]]  # nothing where the bad entry pointed from
    assert torch.equal(bad.pool, want)


def test_shared_prefix_at_op_level():
    Hq, Hkv, T = 4, 2, 5
    cfg = attn_cfg(Hq, Hkv)
    g = torch.Generator().manual_seed(7)
    cache = _permute(PagedKVCache(cfg, 2, SMAX, 6, DEV))
    cache.pool.fill_(NAN)
    cache.reserve(0, 128)
    prefix = torch.randn(2, 2, Hkv, 128, 128, generator=g).bfloat16().to(DEV)
    cache.fill(0, prefix[0], prefix[1])
    cache.set_lens([128, 0])
    qkv = torch.randn(2, T, (Hq + 2 * Hkv) * 128, generator=g).bfloat16().to(DEV)
    q0 = paged_rope_append_chunk(qkv[:1].contiguous(), cache, 0, [T], seqs=[0])
    before = paged_chunk_attention(q0, cache, 0, [T], seqs=[0])
    cache.share_prefix(0, 1, 128)
    q1 = paged_rope_append_chunk(qkv[1:].contiguous(), cache, 0, [T - 2], seqs=[1])  # a page of its own
    assert cache.table[1][:2] == cache.table[0][:2] and cache.table[1][2] != cache.table[0][2]
    q, new = torch.cat([q0, q1]), [T, T - 2]
    o = paged_chunk_attention(q, cache, 0, new)
    assert torch.equal(o[:1], before)
    gathered = KVCache(cfg, 2, SMAX, "cpu")
    for b, k in enumerate(new):
        gathered.kv[0, :, b, :, : 128 + k] = torch.stack(cache.gather(0, b, 128 + k)).cpu()
    gathered.set_lens([128, 128])
    assert_live_rows_close(o.cpu(), eo.extend_fp64(q, gathered), new, Hq)


@pytest.mark.parametrize("nsplit", [1, 3])
def test_a_poisoned_sequence_stays_in_its_pages(nsplit):
    T = tile_tokens(4, 1) + 1
    dense, q = chunk_cache(4, 1, [70, 5, 300], [T, T, T - 1], T)
    cache = paged_from(dense, [T, T, T - 1])
    clean = paged_chunk_attention(q, cache, 0, [T, T, T - 1], nsplit=nsplit)
    cache.pool[:, :, cache.table[1]] = NAN
    q[1] = NAN
    dirty = paged_chunk_attention(q, cache, 0, [T, T, T - 1], nsplit=nsplit)
    assert torch.equal(clean[[0, 2]], dirty[[0, 2]])


BAD_CALLS = {"head_dim": {"Dh": 64}, "rep6": {"Hq": 6}, "misaligned_head_stride": {"stride_h": 64 * 128 + 4},
             "overlapping_heads": {"stride_h": 64 * 128 - 8}, "overlapping_pages": {"stride_page": 64 * 128 - 8},
             "no_pages": {"n_pages": 0}, "max_pages": {"max_pages": 15}, "table_stride": {"table_stride": 15},
             "nsplit1": {"nsplit": 1}, "nsplit17": {"nsplit": 17}}


def test_entry_point_rejections_launch_nothing():
    dense, q, new, ref, cache = _case(8, 1, tile_tokens(8, 1) + 1, 2)
    T = q.shape[1]
    new_dev = torch.tensor(new, dtype=torch.int32, device=DEV)
    o = torch.full_like(q, 7.0)
    ws = torch.full((3 * 2 * 16 * 128 * 130,), 7.0, device=DEV)
    kp = cache.k(0)
    good = dict(B=3, T=T, Hq=8, Hkv=1, Dh=128, Smax=SMAX, n_pages=cache.n_pages, max_pages=16, table_stride=16,
                stride_page=kp.stride(0), stride_h=kp.stride(1), nsplit=3)

    def call(split, **kw):
        a = {**good, **kw}
        head = (q.data_ptr(), kp.data_ptr(), cache.v(0).data_ptr(), cache.table_dev.data_ptr(), cache.lens_dev.data_ptr(),
                new_dev.data_ptr(), o.data_ptr())
        geo = tuple(a[k] for k in list(good)[:-1])
        tail = (1.0 / math.sqrt(128), _lib.stream_ptr(q.device))
        if split:
            return _lib.load().th_paged_chunk_attn_split(*head, ws.data_ptr(), *geo, a["nsplit"], *tail)
        return _lib.load().th_paged_chunk_attn(*head, *geo, *tail)

    for name, kw in BAD_CALLS.items():
        assert call(True, **kw) < 0, name
        assert "nsplit" in kw or call(False, **kw) < 0, name
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()) and bool((ws == 7.0).all())
    for split in (False, True):
        assert call(split) == 0
        assert_live_rows_close(o.cpu(), ref, new, 8)


@pytest.mark.parametrize("new", [[16, 16], [9, 16]])
def test_prefill_paged_chunk_logits_no_worse_than_the_full_forward(new):
    _, gpu, tokens = tg._pair()
    ref, full = tg._references()
    cache = _permute(PagedKVCache(gpu.cfg, 2, 64, 4, DEV))
    prompt = torch.stack([tokens[b] * (torch.arange(64) < n) for b, n in enumerate(tg.LENS)]).to(DEV)
    gpu.prefill(prompt, tg.LENS, cache)
    chunk = torch.stack([tokens[b, n: n + 16] for b, n in enumerate(tg.LENS)]).to(DEV)
    got = torch.mm(gpu.prefill_paged_chunk(chunk, new, cache), gpu.lm_head.t()).float().cpu()
    assert cache.lens == [n + k for n, k in zip(tg.LENS, new)] == cache.lens_dev.tolist()
    rows = [n + k - 1 for n, k in zip(tg.LENS, new)]
    e_new = max((got[b] - ref[b, r]).abs().max().item() for b, r in enumerate(rows))
    e_full = max((full[b, r] - ref[b, r]).abs().max().item() for b, r in enumerate(rows))
    peak = max(ref[b, r].abs().max().item() for b, r in enumerate(rows))
    print(f"new {new}  e_new {e_new:.5f}  e_full {e_full:.5f}  max|logit| {peak:.4f}")
    assert e_new <= 2 * e_full + ULP * peak


def test_generate_with_a_shared_prefix_on_gpu():
    _, gpu, _ = tg._pair()
    # the plain run prefills on the flash forward, this one on the chunk kernels: equal ids need a prompt pair whose
    # greedy steps have no near-tie under that rounding difference (with 71 common tokens step 4 of sequence 1 has one)
    tok = torch.randint(0, gpu.cfg.vocab_size, (2, 100), generator=torch.Generator().manual_seed(5))
    tok[:, :70] = tok[:1, :70]
    tok, lens = tok.to(DEV), [75, 100]
    plain = gpu.generate(tok, lens, max_new_tokens=8, stream_gemm=True)
    assert torch.equal(gpu.generate(tok, lens, max_new_tokens=8, stream_gemm=True, paged_kv=True, shared_prefix=70), plain)
