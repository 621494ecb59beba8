"""The gfx950 FP8-weight streaming linear (csrc/decode_linear_fp8.hip) on the GPU: all three epilogues
against the fp64 oracles of ``tests/decode_linear_fp8_oracles.py`` in every template instance, the exact
decode of every finite e4m3 code at every byte position, memory discipline around x / Wq / scale / y,
row independence, bit reproducibility, the C entry point's rejections, the quantizer on the device,
and ``fp8`` through ``decode_step``, ``decode_graph`` and ``generate``.  ``pytest -s`` prints the worst
``err / bound`` per form when the module finishes."""
import functools

import pytest
import torch

from tests import decode_linear_fp8_oracles as fo
from tests import decode_linear_oracles as dlo
from tests import kernel_oracles as ko
from tests.kernel_oracles import assert_rounded_close

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
FP8 = torch.float8_e4m3fn
ULP = 2.0 ** -8
PAD = 4096  # elements around every slice of the memory-discipline test


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from tensorhive_fixed_amd.ops import _lib
    _lib.load(build_if_missing=True)
    assert hasattr(_lib.load(), "th_decode_linear_fp8")
    yield
    print("\nworst err/bound per form")
    for k, v in sorted(ko.WORST.items()):
        if k.startswith("gpu decode_") and "fp8" in k:
            print(f"  {k[4:]:<32s} {v:.3f}")


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """Inputs and both fp64 references, computed once per shape and shared by every test."""
    x, wq, scale = fo.inputs(M, N, K, DEV)
    return x, wq, scale, fo.linear_oracle(x, wq, scale), fo.swiglu_oracle(x, wq, scale)


def _check_forms(M, N, K, run_linear, run_swiglu):
    """Each form under its bound.  fp32_term: the default coefficient of ``mag`` stands while the
    kernel's longest chain of dependent f32 roundings is within it, else chain length x 2^-24 with the
    chain of ``decode_linear_fp8_oracles.chain_length_fp8`` (two MFMAs of 32 additions per k-step on
    each of two accumulators, their sum, the merge of the 4 waves, the scale)."""
    _, _, _, (ref, mag), (sref, smag) = _case(M, N, K)
    assert_rounded_close(run_linear(BF), ref, mag, "gpu decode_linear_fp8 bf16", fp32_term=fo.fp32_term(K, BF))
    assert_rounded_close(run_linear(torch.float32), ref, mag, "gpu decode_linear_fp8 f32",
                         fp32_term=fo.fp32_term(K, torch.float32))
    assert_rounded_close(run_swiglu(), sref, smag, "gpu decode_gate_up_swiglu_fp8", fp32_term=fo.fp32_term(K, BF))


def _tid(t):
    return f"tiles{t}"


@pytest.mark.parametrize("tiles", fo.TILES, ids=_tid)
@pytest.mark.parametrize("M,N,K", fo.SHAPES, ids=lambda v: str(v))
def test_forms_against_fp64(M, N, K, tiles):
    from tensorhive_fixed_amd.ops.decode_linear_fp8 import decode_gate_up_swiglu_fp8, decode_linear_fp8

    x, wq, scale, _, _ = _case(M, N, K)
    _check_forms(M, N, K, lambda dt: decode_linear_fp8(x, wq, scale, out_dtype=dt, tiles=tiles),
                 lambda: decode_gate_up_swiglu_fp8(x, wq, scale, tiles=tiles))


def _raw(x, wq, scale, y, N, mode, tiles):
    from tensorhive_fixed_amd.ops import _lib
    _lib.call("th_decode_linear_fp8", x.data_ptr(), wq.data_ptr(), scale.data_ptr(), y.data_ptr(), x.shape[0], N,
              x.shape[1], mode, tiles, _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("tiles", [1, 2], ids=_tid)
def test_exact_decode_of_every_code_at_every_byte_position(tiles):
    """One-hot x rows pick single weight bytes: y[m, n] = value(wq[n, 16 j + m]) * scale[n], a single
    product, zeros and one f32 multiplication, so the f32 output is exact.  A fnuz reading, a wrong
    subnormal, sign, byte order within a dword or k-order between the operands all show."""
    N, K = 32, 256
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    codes = ((k + 9 * n) % 256).to(torch.uint8)
    codes[codes == 0x7F] = 0x7E
    codes[codes == 0xFF] = 0xFE
    for pos in range(16):  # every finite code sits at every position of a 16-byte load
        assert torch.unique(codes[:, pos::16]).numel() == 254
    scale = (1.37e-3 * (torch.arange(N) + 1)).float()
    want_all = codes.view(FP8).float() * scale[:, None]  # [N, K], exact in f32 up to the one multiplication
    wq, sc = codes.to(DEV).view(FP8), scale.to(DEV)
    for j in range(16):
        x = torch.zeros(16, K, dtype=BF)
        x[torch.arange(16), 16 * j + torch.arange(16)] = 1.0
        y = torch.full((16, N), float("nan"), device=DEV, dtype=torch.float32)
        _raw(x.to(DEV), wq, sc, y, N, 1, tiles)
        want = want_all[:, 16 * j: 16 * j + 16].t().contiguous()  # [m, n]
        got = y.cpu()
        assert torch.equal(got, want), (j, (got != want).nonzero()[:4].tolist())


def _framed(t, fill):
    """A copy of ``t`` in the middle of a larger buffer filled with ``fill``; returns (buffer, view)."""
    buf = torch.full((t.numel() + 2 * PAD,), fill, device=DEV, dtype=t.dtype)
    view = buf[PAD: PAD + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


@pytest.mark.parametrize("tiles", [1, 2], ids=_tid)
@pytest.mark.parametrize("M,N,K", fo.SHAPES, ids=lambda v: str(v))
def test_memory_discipline(M, N, K, tiles):
    """x, Wq, scale and y are slices in the middle of larger buffers: NaN around x and scale, the NaN
    code 0x7f around Wq, a bit pattern around y.  A padded row of M, or a weight row or scale past a
    partial or dead tile, that is read into a live output shows as NaN; one that is written breaks the
    pattern."""
    x, wq, scale, _, _ = _case(M, N, K)
    _, xs = _framed(x, float("nan"))
    _, ss = _framed(scale, float("nan"))
    _, wb = _framed(wq.view(torch.uint8), 0x7F)
    ws = wb.view(FP8)
    assert xs.data_ptr() % 16 == 0 and ws.data_ptr() % 16 == 0
    outs = {}
    for mode, dt, cols in ((0, BF, N), (1, torch.float32, N), (2, BF, N // 2)):
        sentinel = 0x5A5A if dt == BF else 0x5A5A5A5A
        ibuf = torch.full((M * cols + 2 * PAD,), sentinel, device=DEV, dtype=torch.int16 if dt == BF else torch.int32)
        y = ibuf.view(dt)[PAD: PAD + M * cols].view(M, cols)
        _raw(xs, ws, ss, y, N, mode, tiles)
        assert bool(torch.isfinite(y.float()).all()), f"mode {mode}: non-finite output"
        assert bool((ibuf[:PAD] == sentinel).all()) and bool((ibuf[PAD + M * cols:] == sentinel).all()), \
            f"mode {mode}: written outside y"
        outs[mode] = y.clone()
    _check_forms(M, N, K, lambda dt: outs[0] if dt == BF else outs[1], lambda: outs[2])


@pytest.mark.parametrize("tiles", fo.TILES, ids=_tid)
def test_row_independence(tiles):
    from tensorhive_fixed_amd.ops.decode_linear_fp8 import decode_gate_up_swiglu_fp8, decode_linear_fp8

    x, wq, scale, _, _ = _case(8, 272, 512)
    x2 = x.clone()
    x2[1:] = dlo.inputs(8, 272, 512, DEV, seed=1)[0][1:] * 3
    assert torch.equal(x2[0], x[0]) and not torch.equal(x2[1:], x[1:])
    for dt in (BF, torch.float32):
        a = decode_linear_fp8(x, wq, scale, out_dtype=dt, tiles=tiles)
        b = decode_linear_fp8(x2, wq, scale, out_dtype=dt, tiles=tiles)
        assert torch.equal(a[0], b[0]) and not torch.equal(a[1:], b[1:])
    a = decode_gate_up_swiglu_fp8(x, wq, scale, tiles=tiles)
    b = decode_gate_up_swiglu_fp8(x2, wq, scale, tiles=tiles)
    assert torch.equal(a[0], b[0]) and not torch.equal(a[1:], b[1:])


@pytest.mark.parametrize("tiles", fo.TILES, ids=_tid)
@pytest.mark.parametrize("M,N,K", [(8, 272, 512), (16, 32, 14336)], ids=lambda v: str(v))
def test_bit_reproducible(M, N, K, tiles):
    from tensorhive_fixed_amd.ops.decode_linear_fp8 import decode_gate_up_swiglu_fp8, decode_linear_fp8

    x, wq, scale, _, _ = _case(M, N, K)
    for dt in (BF, torch.float32):
        assert torch.equal(decode_linear_fp8(x, wq, scale, out_dtype=dt, tiles=tiles),
                           decode_linear_fp8(x, wq, scale, out_dtype=dt, tiles=tiles))
    assert torch.equal(decode_gate_up_swiglu_fp8(x, wq, scale, tiles=tiles),
                       decode_gate_up_swiglu_fp8(x, wq, scale, tiles=tiles))


def test_entry_point_rejections():
    """Straight through the C ABI: a negative code, no launch, the output untouched."""
    from tensorhive_fixed_amd.ops import _lib

    fn = _lib.load().th_decode_linear_fp8
    stream = _lib.stream_ptr(torch.device(DEV))
    x = torch.ones(17, 512, device=DEV, dtype=BF)
    wq = torch.ones(32, 512, device=DEV, dtype=BF).to(FP8)
    sc = torch.full((32,), 0.5, device=DEV)
    y = torch.full((17, 32), 7.0, device=DEV, dtype=torch.float32)
    # (M, N, K, mode, tiles): M = 17 and 0, K and N off the rule, an odd half of w13, no such mode / tile count
    bad = [(17, 32, 512, 0, 1), (0, 32, 512, 0, 1), (8, 32, 320, 0, 1), (8, 32, 128, 1, 2), (8, 24, 512, 0, 1),
           (8, 40, 512, 2, 2), (8, 32, 512, 3, 1), (8, 32, 512, 0, 3), (8, 32, 512, 2, 0)]
    for M, N, K, mode, tiles in bad:
        rc = fn(x.data_ptr(), wq.data_ptr(), sc.data_ptr(), y.data_ptr(), M, N, K, mode, tiles, stream)
        assert rc < 0, (M, N, K, mode, tiles, rc)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert fn(x.data_ptr(), wq.data_ptr(), sc.data_ptr(), y.data_ptr(), 8, 32, 512, 1, 2, stream) == 0  # a good one runs
    torch.cuda.synchronize()
    assert bool((y[:8] == 256.0).all()) and bool((y[8:] == 7.0).all())


def test_quantizer_on_the_device_returns_the_cpu_bytes():
    from tensorhive_fixed_amd.ops.decode_linear_fp8 import quantize_weight_fp8

    for M, N, K in [(3, 48, 768), (5, 4800, 256)]:
        _, w = dlo.inputs(M, N, K)
        w = w.clone()
        w[1] = 0  # a row of zeros
        w[2, :16] = torch.tensor([2.0 ** -e for e in range(16)]).to(BF)  # down into the subnormal codes and to zero
        wq_c, s_c = quantize_weight_fp8(w)
        wq_g, s_g = quantize_weight_fp8(w.to(DEV))
        assert wq_g.is_cuda and wq_g.dtype == FP8 and s_g.dtype == torch.float32
        assert torch.equal(s_g.cpu(), s_c)
        assert torch.equal(wq_g.cpu().view(torch.uint8), wq_c.view(torch.uint8))


@functools.lru_cache(maxsize=None)
def _tiny_pair():
    from tensorhive_fixed_amd.models.llama3 import Llama, LlamaConfig

    cfg = LlamaConfig.tiny()
    cpu = Llama(cfg, device="cpu", seed=3)
    gpu = Llama(cfg, device=DEV, seed=0)
    gpu.load_state_dict(cpu.state_dict())
    cpu.quantize_decode_weights()
    gpu.quantize_decode_weights()
    tokens = torch.randint(0, cfg.vocab_size, (2, 64), generator=torch.Generator().manual_seed(11))
    return cpu, gpu, tokens


def _teacher_forced(model, tokens, lens, steps, step):
    """Incremental logits [B, 1 + steps, vocab]: bf16 prefill (prompts zero-padded to 64 columns), then
    ``step(next_tokens, cache)`` per position."""
    from tensorhive_fixed_amd.ops.decode_attention import KVCache

    cache = KVCache(model.cfg, tokens.shape[0], 64, tokens.device)
    prompt = torch.zeros_like(tokens)
    for b, n in enumerate(lens):
        prompt[b, :n] = tokens[b, :n]
    h = model.prefill(prompt, lens, cache)
    out = [torch.mm(h, model.lm_head.t()).float()]
    for i in range(steps):
        nxt = torch.stack([tokens[b, n + i] for b, n in enumerate(lens)])
        out.append(step(nxt, cache).clone())
    return torch.stack(out, dim=1)


def test_fp8_logits_no_worse_than_the_full_forward():
    """GPU kernels against the CPU fp32 path on the same (quantized) weights and the same flow: the
    margin of ``test_stream_gemm_logits_no_worse_than_the_full_forward``.  ``e_quant`` is what the
    quantization itself moves (CPU fp8 flow against the CPU bf16 logits): recorded, not bounded."""
    cpu, gpu, tokens = _tiny_pair()
    lens, steps = [5, 17], 20
    bf16_ref = cpu.logits(tokens).float()
    ref = _teacher_forced(cpu, tokens, lens, steps, lambda t, c: cpu.decode_step(t, c, fp8=True))
    full = gpu.logits(tokens.to(DEV)).float().cpu()
    inc = _teacher_forced(gpu, tokens.to(DEV), lens, steps, lambda t, c: gpu.decode_step(t, c, fp8=True)).cpu()
    rows = [slice(n - 1, n + steps) for n in lens]
    e_new = max((inc[b] - ref[b]).abs().max().item() for b in range(len(lens)))
    e_full = max((full[b, r] - bf16_ref[b, r]).abs().max().item() for b, r in enumerate(rows))
    peak = max(bf16_ref[b, r].abs().max().item() for b, r in enumerate(rows))
    e_quant = max((ref[b] - bf16_ref[b, r]).abs().max().item() for b, r in enumerate(rows))
    print(f"e_new {e_new:.5f}  e_full {e_full:.5f}  e_quant {e_quant:.5f}  max|logit| {peak:.4f}")
    assert e_new <= 2 * e_full + ULP * peak


def test_decode_graph_fp8_replays_the_eager_step():
    from tensorhive_fixed_amd.ops.decode_attention import KVCache

    _, gpu, tokens = _tiny_pair()
    toks = tokens.to(DEV)
    lens = [5, 17]
    eager = _teacher_forced(gpu, toks, lens, 3, lambda t, c: gpu.decode_step(t, c, fp8=True))
    graphs = {}

    def replay(t, cache):
        if id(cache) not in graphs:
            graphs[id(cache)] = gpu.decode_graph(cache, fp8=True)
        return graphs[id(cache)].step(t)

    replayed = _teacher_forced(gpu, toks, lens, 3, replay)
    assert torch.equal(replayed, eager)
    with pytest.raises(ValueError):  # above 16 rows there is nothing to capture
        gpu.decode_graph(KVCache(gpu.cfg, 17, 64, DEV), fp8=True)


def test_generate_fp8_graph_equals_eager():
    _, gpu, tokens = _tiny_pair()
    prompt = tokens[:, :17].to(DEV)
    ids, logits = gpu.generate(prompt, [5, 17], max_new_tokens=8, return_logits=True, fp8=True)
    assert ids.shape == (2, 8) and logits.shape == (2, 8, gpu.cfg.vocab_size) and logits.dtype == torch.float32
    assert torch.equal(ids, logits.argmax(-1))
    ids_g, logits_g = gpu.generate(prompt, [5, 17], max_new_tokens=8, return_logits=True, fp8=True, graph=True)
    assert torch.equal(ids_g, ids) and torch.equal(logits_g, logits)
