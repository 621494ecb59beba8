"""The gfx950 cascade decode kernels (csrc/paged_cascade_attn.hip): sequences that share their first pages against
the fp64 oracle and bounds of the dense kernel's test (tests/decode_oracles.py), NaN in every page and row a
sequence does not own; the rows of one MFMA tile kept apart, bit for bit; the refusals; the tiny model."""
import functools
import math

import pytest
import torch

from tests import decode_oracles as do

pytestmark = pytest.mark.gpu

DEV = "cuda"
ULP = 2.0 ** -8
# (lens, P): B 1 with no suffix; an empty suffix beside one that crosses a page; ...; 40 rows at rep 8 (the third
# row tile partly padding); 72 rows at rep 8 (two row groups)
CASES = [([64], 64), ([128, 129, 193, 1024], 128), ([200, 449, 450], 192), ([1024] * 5, 960), ([65] * 9, 64)]


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from tensorhive_fixed_amd.ops import _lib
    _lib.load(build_if_missing=True)
    assert hasattr(_lib.load(), "th_paged_cascade_decode_attn")


def _shared(dense, lens, P):
    """Layer 0 of ``dense`` in a paged cache whose sequences share the pages of their first ``P`` rows: a permuted
    free list, NaN in every unowned page and dead row, table entries past a sequence's pages out of range."""
    from tensorhive_fixed_amd.ops.paged_attention import PagedKVCache, pages_for

    n_pages = P // 64 + sum(pages_for(n) - P // 64 for n in lens) + 3
    cache = PagedKVCache(dense.cfg, len(lens), do.SMAX, n_pages, DEV)
    cache.pool.fill_(float("nan"))
    cache.free_pages = list(range(0, n_pages, 2)) + list(range(1, n_pages, 2))
    cache.reserve(0, lens[0])
    cache.set_lens([lens[0]] + [0] * (len(lens) - 1))
    for b in range(1, len(lens)):
        cache.share_prefix(0, b, P)
        cache.reserve(b, lens[b])
    cache.fill(0, dense.k(0), dense.v(0))
    cache.set_lens(lens)
    for b in range(len(lens)):
        cache.table_dev[b, len(cache.table[b]):] = n_pages + 7
    return cache


@functools.lru_cache(maxsize=None)
def _case(Hq, Hkv, lens, P):
    """Dense inputs with sequence 0's first ``P`` rows in every sequence, their fp64 reference and the paged cache."""
    dense, q = do.nan_dead_cache(Hq, Hkv, list(lens), DEV)
    dense.kv[:, :, 1:, :, :P] = dense.kv[:, :, :1, :, :P]
    return q, do.attention_fp64(q, dense), _shared(dense, list(lens), P)


@pytest.mark.parametrize("nsplit", [1, None], ids=lambda n: f"nsplit{n}")
@pytest.mark.parametrize("prefix_splits", [1, 3, None], ids=lambda n: f"psplit{n}")
@pytest.mark.parametrize("lens,P", CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else f"P{v}")
@pytest.mark.parametrize("Hq,Hkv", do.HEADS)
def test_cascade_attention_against_fp64(Hq, Hkv, lens, P, prefix_splits, nsplit):
    from tensorhive_fixed_amd.ops.decode_attention import decode_attention
    from tensorhive_fixed_amd.ops.paged_cascade_attention import paged_cascade_decode_attention

    q, ref, cache = _case(Hq, Hkv, tuple(lens), P)
    assert cache.common_prefix_rows() >= P
    do.assert_attention_close(paged_cascade_decode_attention(q, cache, 0, P, nsplit, prefix_splits), ref)
    if prefix_splits is None:  # the public dispatch
        cache.cascade_rows = P
        o = decode_attention(q, cache, 0, nsplit=nsplit)
        cache.cascade_rows = 0
        do.assert_attention_close(o, ref)


@pytest.mark.parametrize("Hq,Hkv", [(8, 2), (8, 1)])
def test_rows_of_a_tile_do_not_mix(Hq, Hkv):
    from tensorhive_fixed_amd.ops.paged_cascade_attention import paged_cascade_decode_attention

    lens, P = [200, 449, 450], 192  # 12 or 24 query rows: all three sequences inside one or two MFMA tiles
    dense, q = do.nan_dead_cache(Hq, Hkv, lens, DEV, seed=4)
    dense.kv[:, :, 1:, :, :P] = dense.kv[:, :, :1, :, :P]
    cache = _shared(dense, lens, P)
    clean = paged_cascade_decode_attention(q, cache, 0, P)
    assert torch.equal(clean, paged_cascade_decode_attention(q, cache, 0, P))  # no atomics: the same bits
    cache.pool[:, :, cache.table[1][P // 64:]] = float("nan")
    q = q.clone()
    q[1] = float("nan")
    o = paged_cascade_decode_attention(q, cache, 0, P)
    assert torch.equal(o[[0, 2]], clean[[0, 2]])


BAD_CALLS = {"head_dim": {"Dh": 64}, "rep3": {"Hq": 6}, "misaligned_head_stride": {"stride_h": 64 * 128 + 4},
             "overlapping_pages": {"stride_page": 2 * 64 * 128 - 8}, "table_stride": {"table_stride": 15},
             "shared0": {"shared_pages": 0}, "shared_large": {"shared_pages": 17}, "psplit0": {"prefix_splits": 0},
             "psplit_large": {"prefix_splits": 1025}, "pchunk0": {"prefix_chunk": 0},
             "pchunk_short": {"prefix_splits": 2, "prefix_chunk": 1}, "nsplit0": {"nsplit": 0},
             "nsplit_large": {"nsplit": 1025}, "chunk_pages0": {"chunk_pages": 0},
             "chunk_pages_large": {"nsplit": 1024, "chunk_pages": 1 << 15}}


def test_refusals_launch_nothing():
    from tensorhive_fixed_amd.ops import _lib
    from tensorhive_fixed_amd.ops.paged_cascade_attention import paged_cascade_decode_attention

    q, ref, cache = _case(8, 2, (200, 449, 450), 192)
    o = torch.full_like(q, 7.0)
    ws = torch.full((3 * 8 * 2048 * 130,), 7.0, device=DEV)  # room for every split count below
    own, keep, cache._ws = cache._ws, cache.table[2][1], ws
    try:
        for rows in (96, 256):  # not whole pages; past min(lens) = 200
            with pytest.raises(ValueError, match="shared rows"):
                paged_cascade_decode_attention(q, cache, 0, rows)
        cache.table[2][1] = cache.table[2][3]
        with pytest.raises(ValueError, match="tables differ"):
            paged_cascade_decode_attention(q, cache, 0, 192)
    finally:
        cache._ws, cache.table[2][1] = own, keep
    kp = cache.k(0)
    good = dict(B=3, Hq=8, Hkv=2, Dh=128, Smax=do.SMAX, n_pages=cache.n_pages, max_pages=16, table_stride=16,
                stride_page=kp.stride(0), stride_h=kp.stride(1), shared_pages=3, prefix_splits=2, prefix_chunk=2,
                nsplit=2, chunk_pages=3)

    def call(**kw):
        a = {**good, **kw}
        return _lib.load().th_paged_cascade_decode_attn(
            q.data_ptr(), kp.data_ptr(), cache.v(0).data_ptr(), cache.table_dev.data_ptr(), cache.lens_dev.data_ptr(),
            o.data_ptr(), ws.data_ptr(), *(a[k] for k in good), 0, 1.0 / math.sqrt(128), _lib.stream_ptr(q.device))

    for name, kw in BAD_CALLS.items():
        assert call(**kw) < 0, name
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()) and bool((ws == 7.0).all())
    assert call() == 0
    do.assert_attention_close(o, ref)


def test_tiny_model_decodes_behind_a_shared_prefix():
    from tensorhive_fixed_amd.models.llama3 import Llama, LlamaConfig
    from tensorhive_fixed_amd.ops.paged_attention import PagedKVCache

    cfg = LlamaConfig.tiny()
    cpu = Llama(cfg, device="cpu", seed=3)
    gpu = Llama(cfg, device=DEV, seed=0)
    gpu.load_state_dict(cpu.state_dict())
    tokens = torch.randint(0, cfg.vocab_size, (2, 104), generator=torch.Generator().manual_seed(11))
    tokens[1, :70] = tokens[0, :70]  # one whole page of them is shared
    tok, P, lens, steps = tokens.to(DEV), 64, [69, 81], 20
    cache = PagedKVCache(cfg, 2, 128, 4, DEV)
    cache.free_pages = [2, 0, 3, 1]
    gpu.prefill_paged_chunk(tok[:1, :P].contiguous(), [P], cache, seqs=[0])
    cache.share_prefix(0, 1, P)
    h = gpu.prefill_paged_chunk(tok[:, P: max(lens)].contiguous(), [n - P for n in lens], cache)
    cache.cascade_rows = P
    out = [torch.mm(h, gpu.lm_head.t()).float()]
    for i in range(steps):
        out.append(gpu.decode_step(torch.stack([tok[b, n + i] for b, n in enumerate(lens)]), cache, stream_gemm=True))
    inc = torch.stack(out, dim=1).cpu()
    assert cache.lens == [n + steps for n in lens] and cache.common_prefix_rows() == P
    ref = cpu.logits(tokens).float()
    full = gpu.logits(tok).float().cpu()
    rows = [slice(n - 1, n + steps) for n in lens]
    e_new = max((inc[b] - ref[b, r]).abs().max().item() for b, r in enumerate(rows))
    e_full = max((full[b, r] - ref[b, r]).abs().max().item() for b, r in enumerate(rows))
    peak = max(ref[b, r].abs().max().item() for b, r in enumerate(rows))
    print(f"e_new {e_new:.5f}  e_full {e_full:.5f}  max|logit| {peak:.4f}")
    assert e_new <= 2 * e_full + ULP * peak
    prompt = tok[:, :100].contiguous()
    ids = gpu.generate(prompt, [75, 100], max_new_tokens=8, stream_gemm=True, paged_kv=True, shared_prefix=70,
                       cascade=True)
    assert tuple(ids.shape) == (2, 8)
