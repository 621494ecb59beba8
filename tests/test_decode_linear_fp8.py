"""``ops/decode_linear_fp8.py`` on the CPU: the quantizer's rule, the exactness of e4m3 in bf16, the fp32
references against the fp64 oracles of ``tests/decode_linear_fp8_oracles.py``, every rejection, and
``fp8`` through ``decode_step``, ``generate`` and the generate workload."""
import functools
import json

import pytest
import torch

from tensorhive_fixed_amd.models.llama3 import Llama, LlamaConfig
from tensorhive_fixed_amd.ops.decode_attention import KVCache
from tensorhive_fixed_amd.ops.decode_linear_fp8 import (decode_gate_up_swiglu_fp8, decode_linear_fp8,
                                                        quantize_weight_fp8, supported_fp8)
from tests import decode_linear_fp8_oracles as fo
from tests import decode_linear_oracles as dlo
from tests.kernel_oracles import assert_rounded_close

BF = torch.bfloat16
FP8 = torch.float8_e4m3fn
NAN_CODES = (0x7F, 0xFF)


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    x, wq, scale = fo.inputs(M, N, K)
    return x, wq, scale, fo.linear_oracle(x, wq, scale), fo.swiglu_oracle(x, wq, scale)


# ------------------------------------------------------------------------------------------ quantizer
def _codes(wq):
    return wq.view(torch.uint8)


def test_quantizer_rule_on_the_test_inputs():
    worst = 0.0
    for M, N, K in dlo.SHAPES:
        _, w = dlo.inputs(M, N, K)
        wq, scale = quantize_weight_fp8(w)
        assert wq.dtype == FP8 and wq.shape == w.shape and wq.is_contiguous()
        assert scale.dtype == torch.float32 and scale.shape == (N,)
        codes = _codes(wq)
        assert not bool(((codes & 0x7F) == 0x7F).any()), "a NaN code"
        assert torch.equal(scale, w.float().abs().amax(1) / 448.0)
        assert bool((wq.float().abs().amax(1) == 448.0).all()), "a row that does not reach |code| = 448"
        # 3 mantissa bits: half an ulp is 2^-4 relative; below the smallest normal 2^-6 the step is 2^-9
        err = (wq.double() * scale.double()[:, None] - w.double()).abs()
        bound = 2.0 ** -4 * w.double().abs() + 2.0 ** -10 * scale.double()[:, None]
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all())
    print(f"worst quantization err / bound {worst:.3f}")


def test_quantizer_zero_row_and_saturation():
    w = torch.zeros(4, 256, dtype=BF)
    w[1, 3] = 1.0
    w[2] = torch.linspace(-3.0, 3.0, 256).to(BF)
    w[3, :2] = torch.tensor([-1e30, 1e-30]).to(BF)
    wq, scale = quantize_weight_fp8(w)
    assert scale[0].item() == 1.0 and bool((_codes(wq)[0] == 0).all())
    assert wq[1, 3].float().item() == 448.0 and scale[1].item() == (torch.tensor(1.0) / 448.0).item()
    assert not bool(((_codes(wq) & 0x7F) == 0x7F).any())
    assert wq[3, 0].float().item() == -448.0 and wq[3, 1].float().item() == 0.0
    # torch's cast alone does not saturate, which is why the rule clamps first
    assert bool(torch.tensor([465.0]).to(FP8).float().isnan().all())
    # an absmax whose quotient lands above 448 in f32 must still give the code of 448, not NaN
    hi = torch.tensor([[3.3895e38] + [0.0] * 255, [1.1755e-38 * 3] + [0.0] * 255]).to(BF)
    q, s = quantize_weight_fp8(hi)
    assert bool((q[:, 0].float() == 448.0).all()) and bool(torch.isfinite(s).all())


def test_quantizer_rejects():
    for bad in (torch.ones(4, 256), torch.ones(256, dtype=BF), torch.ones(256, 4, dtype=BF).t()):
        with pytest.raises(ValueError):
            quantize_weight_fp8(bad)


def test_every_finite_e4m3_code_is_a_bf16_value():
    codes = torch.tensor([c for c in range(256) if c not in NAN_CODES], dtype=torch.uint8)
    assert codes.numel() == 254
    v = codes.view(FP8).float()
    assert bool(torch.isfinite(v).all())
    assert torch.equal(v.to(BF).float(), v)  # bf16 holds it exactly
    assert torch.equal(_codes(v.to(BF).to(FP8)), codes)  # and back to the same code, -0 included
    assert v.abs().max().item() == 448.0 and v[v > 0].min().item() == 2.0 ** -9
    assert bool(torch.tensor(NAN_CODES, dtype=torch.uint8).view(FP8).float().isnan().all())


# ------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("M,N,K", fo.SHAPES, ids=lambda v: str(v))
def test_references_against_fp64(M, N, K):
    x, wq, scale, (ref, mag), (sref, smag) = _case(M, N, K)
    y = decode_linear_fp8(x, wq, scale)
    assert y.dtype == BF and y.shape == (M, N)
    assert_rounded_close(y, ref, mag, "cpu decode_linear_fp8 bf16")
    y32 = decode_linear_fp8(x, wq, scale, out_dtype=torch.float32)
    assert y32.dtype == torch.float32
    assert_rounded_close(y32, ref, mag, "cpu decode_linear_fp8 f32")
    a = decode_gate_up_swiglu_fp8(x, wq, scale)
    assert a.dtype == BF and a.shape == (M, N // 2)
    assert_rounded_close(a, sref, smag, "cpu decode_gate_up_swiglu_fp8")


def test_chain_length_follows_the_kernel_structure():
    assert fo.chain_length_fp8(256) == 64 + 5 and fo.chain_length_fp8(512) == 64 + 5
    assert fo.chain_length_fp8(768) == 128 + 5 and fo.chain_length_fp8(14336) == 64 * 28 + 5
    assert fo.fp32_term(256, BF) is None and fo.fp32_term(256, torch.float32) == 69 * 2.0 ** -24


# ------------------------------------------------------------------------------------------ rejections
def _xws(M=4, N=32, K=256):
    return torch.ones(M, K, dtype=BF), torch.ones(N, K, dtype=BF).to(FP8), torch.ones(N)


@pytest.mark.parametrize("M", [0, 17])
def test_rejects_row_counts(M):
    x, wq, s = _xws(M=M)
    with pytest.raises(ValueError):
        decode_linear_fp8(x, wq, s)
    with pytest.raises(ValueError):
        decode_gate_up_swiglu_fp8(x, wq, s)


def test_rejects_shapes_outside_the_rule():
    for kw in ({"K": 320}, {"K": 128}, {"N": 24}, {"N": 8}):
        with pytest.raises(ValueError):
            decode_linear_fp8(*_xws(**kw))
    x, wq, s = _xws()
    with pytest.raises(ValueError):  # mismatched K
        decode_linear_fp8(_xws(K=512)[0], wq, s)
    with pytest.raises(ValueError):  # not matrices
        decode_linear_fp8(torch.ones(2, 2, 256, dtype=BF), wq, s)
    with pytest.raises(ValueError):  # scale of another length
        decode_linear_fp8(x, wq, torch.ones(16))
    with pytest.raises(ValueError):  # scale not a vector
        decode_linear_fp8(x, wq, torch.ones(32, 1))
    for rows in (33, 40):  # no packed pair at all; 2F = 40 breaks the rule
        with pytest.raises(ValueError):
            decode_gate_up_swiglu_fp8(x, torch.ones(rows, 256, dtype=BF).to(FP8), torch.ones(rows))


def test_rejects_dtypes_and_layouts():
    x, wq, s = _xws()
    with pytest.raises(ValueError):
        decode_linear_fp8(x, wq.to(BF), s)  # bf16 weight
    with pytest.raises(ValueError):
        decode_linear_fp8(x, wq.float().to(torch.float8_e5m2), s)  # the other fp8
    with pytest.raises(ValueError):
        decode_linear_fp8(x, wq.view(torch.uint8), s)  # raw bytes
    with pytest.raises(ValueError):
        decode_linear_fp8(x.float(), wq, s)
    with pytest.raises(ValueError):
        decode_linear_fp8(x, wq, s.double())
    with pytest.raises(ValueError):
        decode_linear_fp8(x, wq, s.to(BF))
    with pytest.raises(ValueError):
        decode_linear_fp8(torch.ones(4, 512, dtype=BF)[:, ::2], wq, s)  # non-contiguous x
    with pytest.raises(ValueError):
        decode_linear_fp8(x, torch.ones(256, 32, dtype=BF).to(FP8).t(), s)  # non-contiguous wq
    with pytest.raises(ValueError):
        decode_gate_up_swiglu_fp8(x, torch.ones(256, 32, dtype=BF).to(FP8).t(), s)
    with pytest.raises(ValueError):
        decode_linear_fp8(x, wq, torch.ones(64)[::2])  # non-contiguous scale
    with pytest.raises(ValueError):
        decode_linear_fp8(x, torch.ones(32 * 256 + 1, dtype=BF).to(FP8)[1:].view(32, 256), s)  # wq off 16 bytes
    for bad in (torch.float16, torch.float64, torch.int32):
        with pytest.raises(ValueError):
            decode_linear_fp8(x, wq, s, out_dtype=bad)
    with pytest.raises(ValueError):
        decode_linear_fp8(x, wq, s, tiles=3)
    with pytest.raises(ValueError):
        decode_gate_up_swiglu_fp8(x, wq, s, tiles=0)


def test_supported_fp8_covers_the_model_configurations():
    for name in ("llama3-8b", "llama3-1b-shape", "tiny"):
        c = LlamaConfig.named(name)
        qkv = (c.n_heads + 2 * c.n_kv_heads) * c.head_dim
        for N, K in [(qkv, c.dim), (c.dim, c.n_heads * c.head_dim), (2 * c.ffn_dim, c.dim), (c.dim, c.ffn_dim),
                     (c.vocab_size, c.dim)]:
            for M in (1, 8, 16):
                assert supported_fp8(M, N, K), (name, M, N, K)
            assert not supported_fp8(17, N, K) and not supported_fp8(0, N, K)
    assert not supported_fp8(8, 4096, 4096 + 128) and not supported_fp8(8, 4096 + 8, 4096)


# ------------------------------------------------------------------------------------------ model
def _tiny_model():
    cfg = LlamaConfig.tiny()
    model = Llama(cfg, device="cpu", seed=3)
    tokens = torch.randint(0, cfg.vocab_size, (2, 48), generator=torch.Generator().manual_seed(11))
    return cfg, model, tokens


def _prefilled(model, tokens, lens):
    cache = KVCache(model.cfg, tokens.shape[0], 64, tokens.device)
    prompt = torch.zeros((tokens.shape[0], max(lens)), dtype=tokens.dtype)
    for b, n in enumerate(lens):
        prompt[b, :n] = tokens[b, :n]
    model.prefill(prompt, lens, cache)
    return cache


def test_decode_step_fp8_needs_quantized_weights():
    cfg, model, tokens = _tiny_model()
    cache = _prefilled(model, tokens, [5, 17])
    with pytest.raises(ValueError, match="quantize_decode_weights"):
        model.decode_step(tokens[:, 20], cache, fp8=True)
    with pytest.raises(ValueError, match="quantize_decode_weights"):
        model.decode_step(tokens[:, 20], cache, stream_gemm=True, fp8=True)  # fp8 takes precedence
    with pytest.raises(ValueError, match="quantize_decode_weights"):
        model.decode_graph(cache, fp8=True)
    assert cache.lens == [5, 17]
    model.quantize_decode_weights()
    y = model.decode_step(tokens[:, 20], cache, fp8=True)
    assert y.dtype == torch.float32 and y.shape == (2, cfg.vocab_size) and cache.lens == [6, 18]
    assert torch.equal(model.decode_graph(cache, fp8=True).step(tokens[:, 21]),
                       model.decode_step(tokens[:, 21], _rewound(cache), fp8=True))


def _rewound(cache):
    cache.set_lens([n - 1 for n in cache.lens])
    return cache


def test_decode_step_fp8_rejects_17_rows():
    cfg, model, tokens = _tiny_model()
    model.quantize_decode_weights()
    B = 17
    toks = tokens[0, :B * 2].view(B, 2)
    cache = _prefilled(model, toks, [1] * B)
    with pytest.raises(ValueError, match="16"):
        model.decode_step(toks[:, 1], cache, fp8=True)
    assert cache.lens == [1] * B
    with pytest.raises(ValueError, match="16"):
        model.generate(toks[:, :1], max_new_tokens=2, fp8=True)


def test_quantized_weights_stay_out_of_the_state_dict():
    cfg, model, _ = _tiny_model()
    keys = list(model.state_dict().keys())
    names = [n for n, _ in model.named_parameters()]
    nbuf = len(list(model.buffers()))
    order = [n for n, _, _ in model.params_in_backward_order()]
    model.quantize_decode_weights()
    assert list(model.state_dict().keys()) == keys
    assert [n for n, _ in model.named_parameters()] == names and len(list(model.buffers())) == nbuf
    assert [n for n, _, _ in model.params_in_backward_order()] == order
    fw = model.fp8_weights
    assert len(fw["layers"]) == cfg.n_layers and set(fw["layers"][0]) == {"wqkv", "wo", "w13", "w2"}
    for (wq, s), w in [(fw["lm_head"], model.lm_head)] + [(fw["layers"][1][n], getattr(model.layers[1], n))
                                                          for n in ("wqkv", "wo", "w13", "w2")]:
        assert wq.dtype == FP8 and wq.shape == w.shape and s.shape == (w.shape[0],)
        assert not isinstance(wq, torch.nn.Parameter)
    # calling it again re-quantizes from the current parameters
    with torch.no_grad():
        model.lm_head.mul_(2.0)
    old = fw["lm_head"][1].clone()
    model.quantize_decode_weights()
    assert torch.equal(model.fp8_weights["lm_head"][1], 2.0 * old)


def test_quantize_decode_weights_rejects_unsupported_shapes():
    cfg = LlamaConfig(vocab_size=520, dim=256, n_layers=1, n_heads=2, n_kv_heads=1, ffn_dim=512, max_seq_len=64)
    model = Llama(cfg, device="cpu")  # the LM head has 520 rows: no multiple of 16
    with pytest.raises(ValueError, match="lm_head"):
        model.quantize_decode_weights()
    assert model.fp8_weights is None


def test_generate_fp8():
    cfg, model, tokens = _tiny_model()
    assert model.fp8_weights is None
    ids, logits = model.generate(tokens[:, :17], [5, 17], max_new_tokens=4, return_logits=True, fp8=True)
    assert model.fp8_weights is not None  # generate quantized on its own
    assert ids.shape == (2, 4) and logits.shape == (2, 4, cfg.vocab_size) and logits.dtype == torch.float32
    assert torch.equal(ids, logits.argmax(-1))
    ids2, logits2 = model.generate(tokens[:, :17], [5, 17], max_new_tokens=4, return_logits=True, fp8=True, graph=True)
    assert torch.equal(ids2, ids) and torch.equal(logits2, logits)
    base = model.generate(tokens[:, :17], [5, 17], max_new_tokens=4, return_logits=True)[1]
    assert torch.equal(base[:, 0], logits[:, 0])  # step 0 comes from the bf16 prefill either way
    assert not torch.equal(base[:, 1:], logits[:, 1:])  # and the steps do run on other weights


def test_generate_workload_fp8(capsys):
    from tensorhive_fixed_amd.workloads import llama3_generate

    assert llama3_generate.main(["--model", "tiny", "--device", "cpu", "--batch", "2", "--prompt-len", "9",
                                 "--max-new-tokens", "4", "--fp8-weights"]) == 0
    done = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert done["event"] == "done" and done["fp8_weights"] is True and done["new_tokens"] == 8
    assert isinstance(done["quantize_ms"], float) and done["quantize_ms"] >= 0
    assert done["stream_gemm"] is False and done["graph"] is False
    assert llama3_generate.main(["--model", "tiny", "--device", "cpu", "--batch", "2", "--prompt-len", "9",
                                 "--max-new-tokens", "2"]) == 0
    done = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert done["fp8_weights"] is False and done["quantize_ms"] is None
