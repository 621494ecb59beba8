"""The gfx950 paged-cache kernels (csrc/paged_attn.hip): attention through a permuted page table against
the fp64 oracle and bounds of the dense kernel's test (tests/decode_oracles.py), with NaN in every page
and row a sequence does not own; placement, sharing and isolation bit for bit; the append against the
dense append; the entry point's rejections; the tiny model on a paged cache."""
import functools
import math

import pytest
import torch

from tests import decode_oracles as do

pytestmark = pytest.mark.gpu

DEV = "cuda"
ULP = 2.0 ** -8
LENS = do.KV_LENS + [[1, 64, 65], [127, 128, 129], [255, 256, 257]]  # around a page, a wave's 2nd page, a step


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from tensorhive_fixed_amd.ops import _lib
    _lib.load(build_if_missing=True)
    assert hasattr(_lib.load(), "th_paged_decode_attn") and hasattr(_lib.load(), "th_paged_rope_append")


def _paged(dense, lens, permute=True, spare=3):
    """The live rows of layer 0 of ``dense`` in a paged cache: NaN in every unowned page and dead row, table
    entries past a sequence's pages out of range, and (``permute``) no two logical neighbours adjacent."""
    from tensorhive_fixed_amd.ops.paged_attention import PagedKVCache, pages_for

    n_pages = sum(pages_for(n) for n in lens) + spare
    cache = PagedKVCache(dense.cfg, len(lens), do.SMAX, n_pages, DEV)
    cache.pool.fill_(float("nan"))
    if permute:  # reversed and interleaved: pops give n-1, n-3, ..., then the other parity
        cache.free_pages = list(range(0, n_pages, 2)) + list(range(1, n_pages, 2))
    for b, n in enumerate(lens):
        cache.reserve(b, n)
    cache.fill(0, dense.k(0), dense.v(0))  # dense's dead rows are NaN already
    cache.set_lens(lens)
    for b in range(len(lens)):
        cache.table_dev[b, len(cache.table[b]):] = n_pages + 7
    return cache


@functools.lru_cache(maxsize=None)
def _case(Hq, Hkv, lens):
    """Dense inputs, their fp64 reference and the permuted paged cache, once per shape."""
    dense, q = do.nan_dead_cache(Hq, Hkv, list(lens), DEV)
    return dense, q, do.attention_fp64(q, dense), _paged(dense, list(lens))


@pytest.mark.parametrize("nsplit", do.NSPLITS, ids=lambda n: f"nsplit{n}")
@pytest.mark.parametrize("lens", LENS, ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("Hq,Hkv", do.HEADS)
def test_paged_attention_against_fp64(Hq, Hkv, lens, nsplit):
    from tensorhive_fixed_amd.ops.decode_attention import decode_attention

    _, q, ref, paged = _case(Hq, Hkv, tuple(lens))
    do.assert_attention_close(decode_attention(q, paged, 0, nsplit=nsplit), ref)  # the public dispatch


@pytest.mark.parametrize("nsplit", [1, 3, None])
def test_placement_is_invisible(nsplit):
    from tensorhive_fixed_amd.ops.paged_attention import paged_decode_attention

    dense, q, _, permuted = _case(8, 2, (1, 200, 1024))
    identity = _paged(dense, [1, 200, 1024], permute=False)
    assert identity.table[2] == list(range(5, 21)) and permuted.table != identity.table
    a = paged_decode_attention(q, permuted, 0, nsplit=nsplit)
    assert torch.equal(a, paged_decode_attention(q, identity, 0, nsplit=nsplit))
    assert torch.equal(a, paged_decode_attention(q, permuted, 0, nsplit=nsplit))


def _fp64_of_gathered(q, cache):
    from tensorhive_fixed_amd.ops.decode_attention import KVCache

    dense = KVCache(cache.cfg, cache.batch, do.SMAX, "cpu")
    for b, n in enumerate(cache.lens):
        k, v = cache.gather(0, b, n)
        dense.kv[0, 0, b, :, :n], dense.kv[0, 1, b, :, :n] = k.cpu(), v.cpu()
    dense.set_lens(cache.lens)
    return do.attention_fp64(q, dense)


def test_shared_prefix():
    from tensorhive_fixed_amd.ops.paged_attention import paged_decode_attention

    dense, q = do.nan_dead_cache(4, 2, [200, 0], DEV, seed=2)
    cache = _paged(dense, [200, 0], spare=4)
    before = paged_decode_attention(q, cache, 0)
    cache.share_prefix(0, 1, 128)
    cache.reserve(1, 131)
    own = torch.randn(2, 3, 2, 128, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16).to(DEV)
    cache.pool[0, :, cache.table[1][2], :, :3] = own.transpose(1, 2)  # rows 128..130 of sequence 1 only
    cache.set_lens([200, 131])
    o = paged_decode_attention(q, cache, 0)
    assert torch.equal(cache.gather(0, 1, 128)[0], cache.gather(0, 0, 128)[0])
    do.assert_rows_close(o, _fp64_of_gathered(q, cache), 4)
    assert torch.equal(o[0], before[0])


def test_paged_rope_append_matches_the_dense_append():
    from tensorhive_fixed_amd.ops.decode_attention import KVCache, rope_append
    from tensorhive_fixed_amd.ops.paged_attention import PagedKVCache

    Hq, Hkv, pos = 8, 2, [0, 63, 64, do.SMAX - 1]
    cfg = do.attn_cfg(Hq, Hkv, n_layers=2)
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(4, (Hq + 2 * Hkv) * 128, generator=g).to(torch.bfloat16).to(DEV)
    dense = KVCache(cfg, 4, do.SMAX, DEV)
    dense.set_lens(pos)
    paged = PagedKVCache(cfg, 4, do.SMAX, 22, DEV)
    paged.pool.copy_(torch.randn(paged.pool.shape, generator=g))  # the sentinel
    paged.free_pages = list(range(0, 22, 2)) + list(range(1, 22, 2))
    for b, p in enumerate(pos):
        paged.reserve(b, p)  # the page of row pos[b] itself is left to the append where it is a new one
    paged.set_lens(pos)
    before = paged.pool.clone()
    assert torch.equal(rope_append(qkv, paged, 1), rope_append(qkv, dense, 1))
    touched = torch.zeros(before.shape, dtype=torch.bool, device=DEV)
    for b, p in enumerate(pos):
        touched[1, :, paged.table[b][p // 64], :, p % 64] = True
        for j in (0, 1):
            assert torch.equal(paged.gather(1, b, p + 1)[j][:, p], dense.kv[1, j, b, :, p])
    assert torch.equal(paged.pool[~touched], before[~touched])  # no other row, no other layer


def test_a_poisoned_sequence_stays_in_its_pages():
    from tensorhive_fixed_amd.ops.paged_attention import paged_decode_attention

    dense, q = do.nan_dead_cache(8, 2, [130, 257, 64], DEV, seed=4)
    cache = _paged(dense, [130, 257, 64])
    clean = paged_decode_attention(q, cache, 0)
    cache.pool[:, :, cache.table[1]] = float("nan")
    q = q.clone()
    q[1] = float("nan")
    o = paged_decode_attention(q, cache, 0)
    assert torch.equal(o[[0, 2]], clean[[0, 2]])


BAD_CALLS = {"head_dim": {"Dh": 64}, "rep3": {"Hq": 6}, "misaligned_head_stride": {"stride_h": 64 * 128 + 4},
             "overlapping_pages": {"stride_page": 2 * 64 * 128 - 8}, "nsplit0": {"nsplit": 0},
             "nsplit_large": {"nsplit": 1025}, "chunk_pages0": {"chunk_pages": 0},
             "chunk_pages_large": {"nsplit": 1024, "chunk_pages": 1 << 15}, "table_stride": {"table_stride": 15}}


def test_entry_point_rejections_launch_nothing():
    from tensorhive_fixed_amd.ops import _lib

    _, q, ref, cache = _case(8, 2, (1, 200, 1024))
    o = torch.full_like(q, 7.0)
    ws = torch.full((3 * 8 * 1024 * 130,), 7.0, device=DEV)  # room for every nsplit below
    kp = cache.k(0)
    good = dict(B=3, Hq=8, Hkv=2, Dh=128, Smax=do.SMAX, n_pages=cache.n_pages, max_pages=16, table_stride=16,
                stride_page=kp.stride(0), stride_h=kp.stride(1), nsplit=2, chunk_pages=8)

    def call(**kw):
        a = {**good, **kw}
        return _lib.load().th_paged_decode_attn(
            q.data_ptr(), kp.data_ptr(), cache.v(0).data_ptr(), cache.table_dev.data_ptr(), cache.lens_dev.data_ptr(),
            o.data_ptr(), ws.data_ptr(), a["B"], a["Hq"], a["Hkv"], a["Dh"], a["Smax"], a["n_pages"], a["max_pages"],
            a["table_stride"], a["stride_page"], a["stride_h"], a["nsplit"], a["chunk_pages"], 0,
            1.0 / math.sqrt(128), _lib.stream_ptr(q.device))

    for name, kw in BAD_CALLS.items():
        assert call(**kw) < 0, name
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()) and bool((ws == 7.0).all())
    assert call() == 0
    do.assert_attention_close(o, ref)


@functools.lru_cache(maxsize=None)
def _tiny_pair():
    from tensorhive_fixed_amd.models.llama3 import Llama, LlamaConfig

    cfg = LlamaConfig.tiny()
    cpu = Llama(cfg, device="cpu", seed=3)
    gpu = Llama(cfg, device=DEV, seed=0)
    gpu.load_state_dict(cpu.state_dict())
    tokens = torch.randint(0, cfg.vocab_size, (2, 64), generator=torch.Generator().manual_seed(11))
    return cpu, gpu, tokens


def _teacher_forced(model, tokens, lens, steps, cache):
    prompt = torch.zeros_like(tokens)
    for b, n in enumerate(lens):
        prompt[b, :n] = tokens[b, :n]
    out = [torch.mm(model.prefill(prompt, lens, cache), model.lm_head.t()).float()]
    for i in range(steps):
        step = torch.stack([tokens[b, n + i] for b, n in enumerate(lens)])
        out.append(model.decode_step(step, cache, stream_gemm=True))
    return torch.stack(out, dim=1).cpu()


def test_tiny_model_decodes_on_a_paged_cache():
    from tensorhive_fixed_amd.ops.decode_attention import KVCache
    from tensorhive_fixed_amd.ops.paged_attention import PagedKVCache

    cpu, gpu, tokens = _tiny_pair()
    lens, steps = [5, 17], 20
    paged = PagedKVCache(gpu.cfg, 2, 64, 4, DEV)
    paged.free_pages = [2, 0, 3, 1]
    inc = _teacher_forced(gpu, tokens.to(DEV), lens, steps, paged)
    dense = _teacher_forced(gpu, tokens.to(DEV), lens, steps, KVCache(gpu.cfg, 2, 64, DEV))
    assert torch.equal(inc.argmax(-1), dense.argmax(-1))
    ref = cpu.logits(tokens).float()
    full = gpu.logits(tokens.to(DEV)).float().cpu()
    rows = [slice(n - 1, n + steps) for n in lens]
    e_new = max((inc[b] - ref[b, r]).abs().max().item() for b, r in enumerate(rows))
    e_full = max((full[b, r] - ref[b, r]).abs().max().item() for b, r in enumerate(rows))
    peak = max(ref[b, r].abs().max().item() for b, r in enumerate(rows))
    print(f"e_new {e_new:.5f}  e_full {e_full:.5f}  max|logit| {peak:.4f}")
    assert e_new <= 2 * e_full + ULP * peak


def test_generate_with_a_paged_cache_on_gpu():
    _, gpu, tokens = _tiny_pair()
    prompt = tokens[:, :60].to(DEV)
    plain = gpu.generate(prompt, [5, 60], max_new_tokens=8, stream_gemm=True)
    assert torch.equal(gpu.generate(prompt, [5, 60], max_new_tokens=8, stream_gemm=True, paged_kv=True), plain)
