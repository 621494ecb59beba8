"""Decode attention with its split geometry derived on the device (th_decode_attn_dev) against the
host rule, bit for bit, and the decode step captured into a graph against the eager step."""
import functools

import pytest
import torch

from tests import decode_oracles as do

pytestmark = pytest.mark.gpu

DEV = "cuda"
ULP = 2.0 ** -8  # as tests/gpu/test_decode_attn_gpu.py


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from tensorhive_fixed_amd.ops import _lib
    _lib.load(build_if_missing=True)
    assert hasattr(_lib.load(), "th_decode_attn_dev")


@functools.lru_cache(maxsize=None)
def _case(Hq, Hkv, lens):
    cache, q = do.nan_dead_cache(Hq, Hkv, list(lens), DEV)
    return cache, q, do.attention_fp64(q, cache)


@pytest.mark.parametrize("nsplit", [None, 3, 8], ids=lambda n: f"nsplit{n}")
@pytest.mark.parametrize("lens", do.KV_LENS, ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("Hq,Hkv", do.HEADS)
def test_device_geometry_has_the_bits_of_the_host_rule(Hq, Hkv, lens, nsplit):
    from tensorhive_fixed_amd.ops.decode_attention import decode_attention

    cache, q, ref = _case(Hq, Hkv, tuple(lens))
    host = decode_attention(q, cache, 0, nsplit=nsplit)
    dev = decode_attention(q, cache, 0, nsplit=nsplit, device_geometry=True)
    assert torch.equal(dev, host)
    do.assert_attention_close(dev, ref)


@pytest.mark.parametrize("longest", [256, 512])
@pytest.mark.parametrize("Hq,Hkv", do.HEADS)
def test_new_token_lands_on_a_split_boundary(Hq, Hkv, longest):
    """``new=1`` with ``longest`` exactly 256 / 512: ``longest // 256`` steps to 1 / 2 with this very key."""
    from tensorhive_fixed_amd.ops.decode_attention import decode_attention

    lens = [longest - 1, 100, longest - 2]
    cache, q = do.nan_dead_cache(Hq, Hkv, [n + 1 for n in lens], DEV, seed=longest)  # rows < lens[b] + 1 live
    ref = do.attention_fp64(q, cache)
    cache.set_lens(lens)
    host = decode_attention(q, cache, 0, new=1)
    dev = decode_attention(q, cache, 0, new=1, device_geometry=True)
    assert torch.equal(dev, host)
    do.assert_attention_close(dev, ref)
    for nsplit in (3, 8):
        assert torch.equal(decode_attention(q, cache, 0, nsplit=nsplit, new=1, device_geometry=True),
                           decode_attention(q, cache, 0, nsplit=nsplit, new=1))


@functools.lru_cache(maxsize=None)
def _tiny():
    from tensorhive_fixed_amd.models.llama3 import Llama, LlamaConfig

    cfg = LlamaConfig.tiny()
    model = Llama(cfg, device=DEV, seed=0)
    model.load_state_dict(Llama(cfg, device="cpu", seed=3).state_dict())  # the weights of test_decode_attn_gpu
    tokens = torch.randint(0, cfg.vocab_size, (2, 512), generator=torch.Generator().manual_seed(11)).to(DEV)
    return model, tokens


def _prefill(model, tokens, lens, cache):
    S = -(-max(lens) // 64) * 64
    prompt = torch.zeros((tokens.shape[0], S), device=DEV, dtype=tokens.dtype)
    for b, n in enumerate(lens):
        prompt[b, :n] = tokens[b, :n]
    model.prefill(prompt, lens, cache)


def _next(tokens, lens, i):
    return torch.stack([tokens[b, n + i] for b, n in enumerate(lens)])


def _assert_same(got, ref, exact, what):
    if exact:
        assert torch.equal(got, ref), what
    else:
        err = (got - ref).abs().max().item()
        assert err <= ULP * ref.abs().max().item(), (what, err)


@pytest.mark.parametrize("stream_gemm", [True, False], ids=["stream", "hipblaslt"])
def test_replayed_steps_equal_eager_steps(stream_gemm):
    """B 2, prompts of 505 and 300 in a cache of 512: ``longest`` runs 506..512, so the last step goes
    from one live split to two under a grid fixed at two.  With ``stream_gemm`` every GEMM of the tiny
    model is the project's own kernel and the logits must have the same bits; on hipBLASLt the bound is
    the one of ``test_generate_on_gpu``."""
    from tensorhive_fixed_amd.ops.decode_attention import KVCache
    from tensorhive_fixed_amd.ops.decode_linear import preferred

    model, tokens = _tiny()
    c = model.cfg
    if stream_gemm:
        kv = c.n_kv_heads * c.head_dim
        for N, K in ((c.dim + 2 * kv, c.dim), (c.dim, c.dim), (2 * c.ffn_dim, c.dim), (c.dim, c.ffn_dim),
                     (c.vocab_size, c.dim)):
            assert preferred(2, N, K), (N, K)
    lens, steps = [505, 300], 7
    eager, replayed = KVCache(c, 2, 512, DEV), KVCache(c, 2, 512, DEV)
    _prefill(model, tokens, lens, eager)
    _prefill(model, tokens, lens, replayed)
    graph = model.decode_graph(replayed, stream_gemm=stream_gemm)
    assert replayed.lens == lens and replayed.lens_dev.tolist() == lens  # the warm-up moved nothing
    for i in range(steps):
        nxt = _next(tokens, lens, i)
        ref = model.decode_step(nxt, eager, stream_gemm=stream_gemm)
        _assert_same(graph.step(nxt), ref, stream_gemm, f"step {i}")
    assert replayed.lens == [n + steps for n in lens] and replayed.lens_dev.tolist() == replayed.lens
    with pytest.raises(ValueError):
        graph.step(nxt)
    assert replayed.lens_dev.tolist() == replayed.lens == [n + steps for n in lens]

    # the same graph object after another prefill into its cache, against a fresh cache
    lens2 = [20, 64]
    tokens2 = tokens.flip(1)
    _prefill(model, tokens2, lens2, replayed)
    fresh = KVCache(c, 2, 512, DEV)
    _prefill(model, tokens2, lens2, fresh)
    for i in range(3):
        nxt = _next(tokens2, lens2, i)
        ref = model.decode_step(nxt, fresh, stream_gemm=stream_gemm)
        _assert_same(graph.step(nxt), ref, stream_gemm, f"reuse step {i}")
    assert replayed.lens == [n + 3 for n in lens2] and replayed.lens_dev.tolist() == replayed.lens


def test_generate_with_graph_equals_eager():
    model, _ = _tiny()
    lens = [5, 17]  # the prompts of test_generate_on_gpu
    tokens = torch.randint(0, model.cfg.vocab_size, (2, 64), generator=torch.Generator().manual_seed(11))
    prompt = tokens[:, :17].to(DEV)
    ids, logits = model.generate(prompt, lens, max_new_tokens=8, return_logits=True, stream_gemm=True)
    gids, glogits = model.generate(prompt, lens, max_new_tokens=8, return_logits=True, stream_gemm=True,
                                   graph=True)
    assert torch.equal(gids, ids) and torch.equal(glogits, logits)
    kw = dict(max_new_tokens=8, temperature=0.8, top_k=20, stream_gemm=True)
    a = model.generate(prompt, lens, generator=torch.Generator(device=DEV).manual_seed(4), **kw)
    b = model.generate(prompt, lens, generator=torch.Generator(device=DEV).manual_seed(4), graph=True, **kw)
    assert torch.equal(a, b)
