"""csrc/decode_linear_mxfp4.hip on the GPU: every form and template instance against fp64, tails and isolation,
the entry point's rejections, the quantizer on the device, and ``mxfp4`` through the model."""
import functools

import pytest
import torch

from tests import decode_linear_mxfp4_oracles as mo
from tests.kernel_oracles import assert_rounded_close

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
MODES = {0: BF, 1: torch.float32, 2: BF}


@functools.lru_cache(maxsize=None)
def _dev(M, N, K):
    return tuple(t.to(DEV) for t in mo.case(M, N, K)[:3])


def _run(x, codes, scales, mode, tiles):
    from tensorhive_fixed_amd.ops.decode_linear_mxfp4 import decode_gate_up_swiglu_mxfp4, decode_linear_mxfp4

    if mode == 2:
        return decode_gate_up_swiglu_mxfp4(x, codes, scales, tiles=tiles)
    return decode_linear_mxfp4(x, codes, scales, out_dtype=MODES[mode], tiles=tiles)


@pytest.mark.parametrize("tiles", mo.TILES, ids=lambda t: f"tiles{t}")
@pytest.mark.parametrize("mode", [0, 1, 2], ids=lambda m: f"mode{m}")
@pytest.mark.parametrize("M,N,K", mo.SHAPES, ids=lambda v: str(v))
def test_forms_against_fp64(M, N, K, mode, tiles):
    ref, mag = mo.case(M, N, K)[6 if mode == 2 else 5]
    y = _run(*_dev(M, N, K), mode, tiles)
    assert_rounded_close(y, ref, mag, f"gpu decode_linear_mxfp4 mode {mode}", fp32_term=mo.fp32_term(K, MODES[mode]))


@pytest.mark.parametrize("tiles", [1, 2, 4], ids=lambda t: f"tiles{t}")
@pytest.mark.parametrize("M,N,K", [(1, 16, 256), (3, 48, 768), (8, 272, 512)], ids=lambda v: str(v))
def test_tails_and_isolation(M, N, K, tiles):
    """Heads of over-allocated buffers: NaN in the x rows >= M, and in the rows >= N the largest code under the
    scale byte 255, whose f32 is inf.  A dead row that reaches a live output makes it differ from the clean run."""
    x, codes, scales = _dev(M, N, K)
    xb = torch.full((16, K), float("nan"), device=DEV, dtype=BF)
    cb = torch.full((N + 64, K // 2), 0x77, device=DEV, dtype=torch.uint8)
    sb = torch.full((N + 64, K // 32), 255, device=DEV, dtype=torch.uint8)
    xb[:M], cb[:N], sb[:N] = x, codes, scales
    for mode in MODES:
        clean = _run(x, codes, scales, mode, tiles)
        assert bool(torch.isfinite(clean.float()).all())
        assert torch.equal(_run(xb[:M], cb[:N], sb[:N], mode, tiles), clean)
        assert torch.equal(_run(x, codes, scales, mode, tiles), clean)


def test_entry_point_rejections():
    """Straight through the C ABI: a negative code, no launch, the output untouched."""
    from tensorhive_fixed_amd.ops import _lib

    fn = _lib.load(build_if_missing=True).th_decode_linear_mxfp4
    stream = _lib.stream_ptr(torch.device(DEV))
    x = torch.ones(17, 512, device=DEV, dtype=BF)
    codes = torch.full((32, 256), 0x22, device=DEV, dtype=torch.uint8)  # 1.0 everywhere
    sc = torch.full((32, 16), 126, device=DEV, dtype=torch.uint8)       # times 0.5
    y = torch.full((17, 32), 7.0, device=DEV, dtype=torch.float32)
    bad = [  # (M, N, K, mode, tiles)
           (0, 32, 512, 1, 1), (17, 32, 512, 1, 1), (8, 32, 128, 1, 2), (8, 24, 512, 1, 1), (8, 32, 512, 3, 1),
           (8, 32, 512, -1, 1), (8, 32, 512, 1, 3), (8, 32, 512, 2, 0)]
    for M, N, K, mode, tiles in bad:
        assert fn(x.data_ptr(), codes.data_ptr(), sc.data_ptr(), y.data_ptr(), M, N, K, mode, tiles, stream) < 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert fn(x.data_ptr(), codes.data_ptr(), sc.data_ptr(), y.data_ptr(), 8, 32, 512, 1, 4, stream) == 0  # a good one runs
    torch.cuda.synchronize()
    assert bool((y[:8] == 256.0).all()) and bool((y[8:] == 7.0).all())


def test_quantizer_on_the_device_returns_the_cpu_bytes():
    from tensorhive_fixed_amd.ops.decode_linear_mxfp4 import quantize_weight_mxfp4

    for M, N, K in [(3, 48, 768), (5, 4800, 256)]:
        w = mo.case(M, N, K)[3].clone()
        w[1] = 0
        w[2, :8] = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0]).to(BF) * 2.0 ** 9  # ties under the block's amax
        c_c, s_c = quantize_weight_mxfp4(w)
        c_g, s_g = quantize_weight_mxfp4(w.to(DEV))
        assert c_g.is_cuda and torch.equal(c_g.cpu(), c_c) and torch.equal(s_g.cpu(), s_c)


@functools.lru_cache(maxsize=None)
def _tiny_pair():
    from tensorhive_fixed_amd.models.llama3 import Llama, LlamaConfig

    cfg = LlamaConfig.tiny()
    cpu = Llama(cfg, device="cpu", seed=3)
    gpu = Llama(cfg, device=DEV, seed=0)
    gpu.load_state_dict(cpu.state_dict())
    cpu.quantize_decode_weights_mxfp4()
    gpu.quantize_decode_weights_mxfp4()
    tokens = torch.randint(0, cfg.vocab_size, (2, 64), generator=torch.Generator().manual_seed(11))
    return cpu, gpu, tokens


def _teacher_forced(model, tokens, lens, steps):
    """Incremental logits [B, 1 + steps, vocab]: bf16 prefill, then one ``decode_step(mxfp4=True)`` per position."""
    from tensorhive_fixed_amd.ops.decode_attention import KVCache

    cache = KVCache(model.cfg, tokens.shape[0], 64, tokens.device)
    prompt = torch.zeros_like(tokens)
    for b, n in enumerate(lens):
        prompt[b, :n] = tokens[b, :n]
    out = [torch.mm(model.prefill(prompt, lens, cache), model.lm_head.t()).float()]
    for i in range(steps):
        nxt = torch.stack([tokens[b, n + i] for b, n in enumerate(lens)])
        out.append(model.decode_step(nxt, cache, mxfp4=True).clone())
    return torch.stack(out, dim=1).cpu()


def test_mxfp4_logits_no_worse_than_the_full_forward():
    """GPU kernels against the CPU fp32 path on the same quantized weights and the same flow, under the
    margin of the FP8 tiny-model check: twice what the GPU bf16 forward itself is off the CPU's, plus a
    bf16 ulp of the largest logit."""
    cpu, gpu, tokens = _tiny_pair()
    lens, steps = [5, 17], 20
    bf16_ref = cpu.logits(tokens).float()
    full = gpu.logits(tokens.to(DEV)).float().cpu()
    ref, inc = _teacher_forced(cpu, tokens, lens, steps), _teacher_forced(gpu, tokens.to(DEV), lens, steps)
    rows = [slice(n - 1, n + steps) for n in lens]
    e_new = max((inc[b] - ref[b]).abs().max().item() for b in range(len(lens)))
    e_full = max((full[b, r] - bf16_ref[b, r]).abs().max().item() for b, r in enumerate(rows))
    peak = max(bf16_ref[b, r].abs().max().item() for b, r in enumerate(rows))
    e_quant = max((ref[b] - bf16_ref[b, r]).abs().max().item() for b, r in enumerate(rows))
    print(f"e_new {e_new:.5f}  e_full {e_full:.5f}  e_quant {e_quant:.5f}  max|logit| {peak:.4f}")
    assert e_new <= 2 * e_full + 2.0 ** -8 * peak


def test_generate_mxfp4_graph_equals_eager_and_refusals():
    _, gpu, tokens = _tiny_pair()
    prompt = tokens[:, :17].to(DEV)
    ids, logits = gpu.generate(prompt, [5, 17], max_new_tokens=8, return_logits=True, mxfp4=True)
    assert ids.shape == (2, 8) and torch.equal(ids, logits.argmax(-1))
    ids_g, logits_g = gpu.generate(prompt, [5, 17], max_new_tokens=8, return_logits=True, mxfp4=True, graph=True)
    assert torch.equal(ids_g, ids) and torch.equal(logits_g, logits)
    for kw in ({"fp8": True}, {"speculate": 2}):
        with pytest.raises(ValueError, match="mxfp4"):
            gpu.generate(prompt, [5, 17], max_new_tokens=4, mxfp4=True, **kw)
    with pytest.raises(ValueError, match="16"):
        gpu.generate(prompt[:1].expand(17, -1).contiguous(), max_new_tokens=2, mxfp4=True)
