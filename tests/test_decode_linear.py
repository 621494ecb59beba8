"""``ops/decode_linear.py`` on the CPU: its fp32 references against the fp64 oracles, every rejection,
``supported`` over the model configurations, and ``stream_gemm`` through ``decode_step``, ``generate``
and the generate workload."""
import functools
import json
import math

import pytest
import torch

from tensorhive_fixed_amd.models.llama3 import Llama, LlamaConfig
from tensorhive_fixed_amd.ops.decode_attention import KVCache
from tensorhive_fixed_amd.ops.decode_linear import decode_gate_up_swiglu, decode_linear, supported
from tests import decode_linear_oracles as dlo
from tests.kernel_oracles import assert_rounded_close

BF = torch.bfloat16


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    x, w = dlo.inputs(M, N, K)
    return x, w, dlo.linear_oracle(x, w), dlo.swiglu_oracle(x, w)


@pytest.mark.parametrize("M,N,K", dlo.SHAPES, ids=lambda v: str(v))
def test_references_against_fp64(M, N, K):
    x, w, (ref, mag), (sref, smag) = _case(M, N, K)
    y = decode_linear(x, w)
    assert y.dtype == BF and y.shape == (M, N)
    assert_rounded_close(y, ref, mag, "cpu decode_linear bf16")
    y32 = decode_linear(x, w, out_dtype=torch.float32)
    assert y32.dtype == torch.float32
    assert_rounded_close(y32, ref, mag, "cpu decode_linear f32")
    a = decode_gate_up_swiglu(x, w)
    assert a.dtype == BF and a.shape == (M, N // 2)
    assert_rounded_close(a, sref, smag, "cpu decode_gate_up_swiglu")


def _xw(M=4, N=32, K=256, dtype=BF):
    return torch.ones(M, K, dtype=dtype), torch.ones(N, K, dtype=dtype)


@pytest.mark.parametrize("M", [0, 17])
def test_rejects_row_counts(M):
    x, w = _xw(M=M)
    with pytest.raises(ValueError):
        decode_linear(x, w)
    with pytest.raises(ValueError):
        decode_gate_up_swiglu(x, w)


def test_rejects_shapes_outside_the_rule():
    for kw in ({"K": 320}, {"K": 128}, {"N": 24}, {"N": 8}):
        with pytest.raises(ValueError):
            decode_linear(*_xw(**kw))
    with pytest.raises(ValueError):  # mismatched K
        decode_linear(_xw(K=256)[0], _xw(K=512)[1])
    with pytest.raises(ValueError):  # not matrices
        decode_linear(torch.ones(2, 2, 256, dtype=BF), _xw()[1])


def test_rejects_dtypes_and_layouts():
    x, w = _xw()
    with pytest.raises(ValueError):
        decode_linear(x.half(), w.half())
    with pytest.raises(ValueError):
        decode_linear(x.float(), w)
    with pytest.raises(ValueError):
        decode_linear(torch.ones(4, 512, dtype=BF)[:, ::2], w)  # non-contiguous x
    with pytest.raises(ValueError):
        decode_linear(x, torch.ones(256, 32, dtype=BF).t())  # non-contiguous w
    with pytest.raises(ValueError):
        decode_gate_up_swiglu(x, torch.ones(256, 32, dtype=BF).t())
    for bad in (torch.float16, torch.float64, torch.int32):
        with pytest.raises(ValueError):
            decode_linear(x, w, out_dtype=bad)
    with pytest.raises(ValueError):
        decode_linear(x, w, tiles=3)


def test_rejects_odd_rows_in_w13():
    x, _ = _xw()
    for rows in (33, 40):  # no packed pair at all; two halves of 20 rows, and 2F = 40 breaks the rule
        with pytest.raises(ValueError):
            decode_gate_up_swiglu(x, torch.ones(rows, 256, dtype=BF))


def test_supported_covers_the_model_configurations():
    for name in ("llama3-8b", "llama3-1b-shape", "tiny"):
        c = LlamaConfig.named(name)
        qkv = (c.n_heads + 2 * c.n_kv_heads) * c.head_dim
        shapes = [(qkv, c.dim), (c.dim, c.n_heads * c.head_dim), (2 * c.ffn_dim, c.dim), (c.ffn_dim, c.dim),
                  (c.dim, c.ffn_dim), (c.vocab_size, c.dim)]
        for N, K in shapes:
            for M in (1, 8, 16):
                assert supported(M, N, K), (name, M, N, K)
            assert not supported(17, N, K) and not supported(0, N, K)
    assert LlamaConfig.named("llama3-8b").vocab_size == 128256
    assert not supported(8, 4096, 4096 + 64) and not supported(8, 4096 + 8, 4096)


@functools.lru_cache(maxsize=None)
def _tiny():
    cfg = LlamaConfig.tiny()
    model = Llama(cfg, device="cpu", seed=3)
    tokens = torch.randint(0, cfg.vocab_size, (2, 48), generator=torch.Generator().manual_seed(11))
    return cfg, model, tokens


def _teacher_forced(model, tokens, lens, steps, stream_gemm):
    cache = KVCache(model.cfg, tokens.shape[0], 64, tokens.device)
    prompt = torch.zeros((tokens.shape[0], max(lens)), dtype=tokens.dtype)
    for b, n in enumerate(lens):
        prompt[b, :n] = tokens[b, :n]
    model.prefill(prompt, lens, cache)
    out = []
    for i in range(steps):
        nxt = torch.stack([tokens[b, n + i] for b, n in enumerate(lens)])
        out.append(model.decode_step(nxt, cache, stream_gemm=stream_gemm))
    assert cache.lens == [n + steps for n in lens]
    return torch.stack(out, dim=1)


def test_decode_step_stream_gemm_matches_the_default_path():
    cfg, model, tokens = _tiny()
    lens, steps = [5, 17], 4
    base = _teacher_forced(model, tokens, lens, steps, False)
    new = _teacher_forced(model, tokens, lens, steps, True)
    assert new.dtype == torch.float32 and new.shape == (2, steps, cfg.vocab_size)
    err = (new - base).abs().max().item()
    peak = base.abs().max().item()
    bound = 2.0 ** (math.floor(math.log2(peak)) - 7)  # one bf16 step (8 significant bits) at the largest |logit|
    print(f"max |delta| {err:.4g}  bound {bound:.4g}")
    assert err <= bound


def test_decode_step_stream_gemm_falls_back_above_16_rows():
    cfg, model, tokens = _tiny()
    B = 17
    toks = tokens[0, :B * 2].view(B, 2)
    a = _teacher_forced(model, toks, [1] * B, 1, False)
    b = _teacher_forced(model, toks, [1] * B, 1, True)
    assert torch.equal(a, b)  # no supported shape at this batch: the same GEMMs run


def test_generate_stream_gemm():
    cfg, model, tokens = _tiny()
    ids, logits = model.generate(tokens[:, :17], [5, 17], max_new_tokens=4, return_logits=True, stream_gemm=True)
    assert ids.shape == (2, 4) and logits.shape == (2, 4, cfg.vocab_size) and logits.dtype == torch.float32
    assert torch.equal(ids, logits.argmax(-1))


def test_generate_workload_stream_gemm(capsys):
    from tensorhive_fixed_amd.workloads import llama3_generate

    assert llama3_generate.main(["--model", "tiny", "--device", "cpu", "--batch", "2", "--prompt-len", "9",
                                 "--max-new-tokens", "4", "--stream-gemm"]) == 0
    done = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert done["event"] == "done" and done["stream_gemm"] is True and done["new_tokens"] == 8
    assert llama3_generate.main(["--model", "tiny", "--device", "cpu", "--batch", "2", "--prompt-len", "9",
                                 "--max-new-tokens", "2"]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["stream_gemm"] is False
