"""``ops/decode_linear_mxfp4.py`` on the CPU: the quantizer's rule, the references, ``mxfp4`` through the model."""
import json

import pytest
import torch

from tensorhive_fixed_amd.models.llama3 import Llama, LlamaConfig
from tensorhive_fixed_amd.ops.decode_linear_mxfp4 import (decode_gate_up_swiglu_mxfp4, decode_linear_mxfp4,
                                                          dequantize_mxfp4, quantize_weight_mxfp4)
from tests import decode_linear_mxfp4_oracles as mo
from tests.kernel_oracles import assert_rounded_close

BF = torch.bfloat16


def test_every_code_at_every_nibble_under_several_scales_round_trips():
    n, j = torch.arange(16)[:, None], torch.arange(128)[None, :]
    codes = (((j + n) % 16) | (((j + 3 * n + 5) % 16) << 4)).to(torch.uint8)  # every code in both nibbles of every block
    scales = torch.tensor([2, 252, 127, 100, 128, 200, 31, 251], dtype=torch.uint8)[(n + torch.arange(8)[None, :]) % 8]
    w = dequantize_mxfp4(codes, scales)
    assert w.dtype == BF and w.shape == (16, 256) and bool(torch.isfinite(w).all())
    assert w.float().abs().min().item() == 0.0 and w.float().abs()[w != 0].min().item() == 2.0 ** -126
    c2, s2 = quantize_weight_mxfp4(w)
    assert torch.equal(c2, codes) and torch.equal(s2, scales)  # -0 included
    assert torch.equal(dequantize_mxfp4(c2, s2).view(torch.int16), w.view(torch.int16))


def test_ties_block_exponent_and_zero_block():
    w = torch.zeros(16, 256, dtype=BF)
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0])
    w[0, :8], w[0, 8:16] = ties.to(BF), (-ties).to(BF)       # amax 6: X = 0
    w[1, 32:40] = (ties * 2.0 ** -20).to(BF)                  # the same under X = -20, in block 1
    w[2, 0], w[2, 32], w[2, 64] = 48.0, 48.25, 47.75          # 6 * 2^3, a bf16 ulp above it, one below
    codes, scales = quantize_weight_mxfp4(w)
    want = torch.tensor([0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 6.0])
    deq = dequantize_mxfp4(codes, scales).float()
    assert torch.equal(deq[0, :8], want) and torch.equal(deq[0, 8:16], -want)
    assert torch.equal(deq[1, 32:40], want * 2.0 ** -20)
    assert scales[0, 0].item() == 127 and scales[1, 1].item() == 107
    assert scales[2, :3].tolist() == [130, 131, 130]
    assert bool((scales[3:] == 127).all()) and bool((codes[3:] == 0).all())  # all-zero blocks


@pytest.mark.parametrize("M,N,K", mo.SHAPES[:4], ids=lambda v: str(v))
def test_quantization_error_and_references_against_fp64(M, N, K):
    x, codes, scales, w, deq, (ref, mag), (sref, smag) = mo.case(M, N, K)
    assert codes.shape == (N, K // 2) and scales.shape == (N, K // 32) and codes.dtype == scales.dtype == torch.uint8
    step = torch.ldexp(torch.ones(()), scales.int() - 127).double()[..., None]  # 2^X: half the widest gap x scale
    assert bool(((w.double() - deq.double()).abs().view(N, K // 32, 32) <= step).all())
    assert bool((w.float().abs().view(N, K // 32, 32).amax(-1) <= 6 * step[..., 0]).all())  # nothing clips
    assert_rounded_close(decode_linear_mxfp4(x, codes, scales), ref, mag, "cpu decode_linear_mxfp4 bf16")
    assert_rounded_close(decode_linear_mxfp4(x, codes, scales, out_dtype=torch.float32), ref, mag,
                         "cpu decode_linear_mxfp4 f32")
    assert_rounded_close(decode_gate_up_swiglu_mxfp4(x, codes, scales), sref, smag, "cpu decode_gate_up_swiglu_mxfp4")


def test_model_generate_and_refusals(capsys):
    from tensorhive_fixed_amd.workloads import llama3_generate

    cfg = LlamaConfig.tiny()
    model = Llama(cfg, device="cpu", seed=3)
    keys = list(model.state_dict().keys())
    tokens = torch.randint(0, cfg.vocab_size, (2, 17), generator=torch.Generator().manual_seed(11))
    ids, logits = model.generate(tokens, [5, 17], max_new_tokens=4, return_logits=True, mxfp4=True, stream_gemm=True)
    mw = model.mxfp4_weights  # generate quantized on its own; the parameters and the state dict stay
    assert list(model.state_dict().keys()) == keys and model.fp8_weights is None
    assert set(mw["layers"][0]) == {"wqkv", "wo", "w13", "w2"} and mw["lm_head"][0].shape == (cfg.vocab_size, cfg.dim // 2)
    assert torch.equal(ids, logits.argmax(-1)) and logits.dtype == torch.float32
    base = model.generate(tokens, [5, 17], max_new_tokens=4, return_logits=True)[1]
    assert torch.equal(base[:, 0], logits[:, 0]) and not torch.equal(base[:, 1:], logits[:, 1:])
    for kw in ({"graph": True}, {"paged_kv": True}):  # these touch only how attention finds its rows
        got = model.generate(tokens, [5, 17], max_new_tokens=4, return_logits=True, mxfp4=True, **kw)
        assert torch.equal(got[0], ids) and torch.equal(got[1], logits)
    assert model.generate(tokens, [5, 17], max_new_tokens=4, mxfp4=True, kv_fp8=True, graph=True).shape == (2, 4)
    for kw in ({"fp8": True}, {"speculate": 2}):
        with pytest.raises(ValueError, match="mxfp4"):
            model.generate(tokens, [5, 17], max_new_tokens=4, mxfp4=True, **kw)
    with pytest.raises(ValueError, match="16"):
        model.generate(tokens[:1].expand(17, -1).contiguous(), max_new_tokens=2, mxfp4=True)
    argv = ["--model", "tiny", "--device", "cpu", "--batch", "2", "--prompt-len", "9", "--max-new-tokens", "3"]
    assert llama3_generate.main(argv + ["--mxfp4-weights", "--graph"]) == 0
    done = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert done["mxfp4_weights"] is True and done["fp8_weights"] is False and done["quantize_ms"] >= 0
    assert llama3_generate.main(argv) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["mxfp4_weights"] is False
