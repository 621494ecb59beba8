"""Block decode steps and speculative greedy generation on the GPU (tiny model): teacher-forced
``extend_step`` logits against the CPU fp32-path logits of the same weights under the rule of
``test_incremental_logits_no_worse_than_the_full_forward`` (tests/gpu/test_decode_attn_gpu.py), on the
default, the weight-streaming and the FP8 flow, and ``generate(speculate=3)`` against plain ``generate``.
The model seed is the one tests/test_speculate.py chose on the CPU."""
import functools

import pytest
import torch

from tests import test_speculate as ts

pytestmark = pytest.mark.gpu

DEV = "cuda"
ULP = 2.0 ** -8
LENS = [5, 17]


@functools.lru_cache(maxsize=None)
def _pair():
    from tensorhive_fixed_amd.models.llama3 import Llama

    cpu = ts.model()
    gpu = Llama(cpu.cfg, device=DEV, seed=0)
    gpu.load_state_dict(cpu.state_dict())
    tokens = torch.randint(0, cpu.cfg.vocab_size, (2, 64), generator=torch.Generator().manual_seed(11))
    return cpu, gpu, tokens


def _prefilled(model, tokens, lens):
    from tensorhive_fixed_amd.ops.decode_attention import KVCache

    cache = KVCache(model.cfg, tokens.shape[0], 64, tokens.device)
    prompt = torch.zeros_like(tokens)
    for b, n in enumerate(lens):
        prompt[b, :n] = tokens[b, :n]
    h = model.prefill(prompt, lens, cache)
    return cache, torch.mm(h, model.lm_head.t()).float()


def _teacher_forced_blocks(model, tokens, lens, T, blocks, **kw):
    """Incremental logits [B, 1 + blocks * T, vocab]: the prefill's row, then ``blocks`` extend steps of T."""
    cache, first = _prefilled(model, tokens, lens)
    out = [first[:, None]]
    for i in range(blocks):
        blk = torch.stack([tokens[b, n + i * T: n + (i + 1) * T] for b, n in enumerate(lens)])
        out.append(model.extend_step(blk, cache, **kw))
    assert cache.lens == [n + blocks * T for n in lens]
    return torch.cat(out, dim=1)


def _teacher_forced_single(model, tokens, lens, steps, **kw):
    cache, first = _prefilled(model, tokens, lens)
    out = [first]
    for i in range(steps):
        out.append(model.decode_step(torch.stack([tokens[b, n + i] for b, n in enumerate(lens)]), cache, **kw))
    return torch.stack(out, dim=1)


@functools.lru_cache(maxsize=None)
def _references():
    cpu, gpu, tokens = _pair()
    ref = cpu.logits(tokens).float()  # CPU fp32-path logits of the same weights
    full = gpu.logits(tokens.to(DEV)).float().cpu()
    return ref, full


@pytest.mark.parametrize("stream_gemm", [False, True], ids=["plain", "stream"])
@pytest.mark.parametrize("T", [2, 4, 8])
def test_extend_step_logits_no_worse_than_the_full_forward(T, stream_gemm):
    _, gpu, tokens = _pair()
    blocks = 16 // T
    steps = blocks * T
    ref, full = _references()
    inc = _teacher_forced_blocks(gpu, tokens.to(DEV), LENS, T, blocks, stream_gemm=stream_gemm).cpu()
    rows = [slice(n - 1, n + steps) for n in LENS]
    e_new = max((inc[b] - ref[b, r]).abs().max().item() for b, r in enumerate(rows))
    e_full = max((full[b, r] - ref[b, r]).abs().max().item() for b, r in enumerate(rows))
    peak = max(ref[b, r].abs().max().item() for b, r in enumerate(rows))
    print(f"T {T}  e_new {e_new:.5f}  e_full {e_full:.5f}  max|logit| {peak:.4f}")
    assert e_new <= 2 * e_full + ULP * peak


@pytest.mark.parametrize("T", [2, 4, 8])
def test_extend_step_fp8_against_sequential_fp8_steps(T):
    """The FP8 flow has its own weights, so its reference is the same flow's single-token steps."""
    _, gpu, tokens = _pair()
    blocks = 16 // T
    steps = blocks * T
    ref, full = _references()
    gpu.quantize_decode_weights()
    try:
        seq = _teacher_forced_single(gpu, tokens.to(DEV), LENS, steps, fp8=True).cpu()
        inc = _teacher_forced_blocks(gpu, tokens.to(DEV), LENS, T, blocks, fp8=True).cpu()
    finally:
        gpu.fp8_weights = None
    rows = [slice(n - 1, n + steps) for n in LENS]
    e_new = (inc - seq).abs().max().item()
    e_full = max((full[b, r] - ref[b, r]).abs().max().item() for b, r in enumerate(rows))
    peak = seq.abs().max().item()
    print(f"T {T}  e_new {e_new:.5f}  e_full {e_full:.5f}  max|logit| {peak:.4f}")
    assert e_new <= 2 * e_full + ULP * peak


def test_speculative_generate_matches_plain_generate():
    _, gpu, _ = _pair()
    tokens, lens = ts.prompts("random")
    new = ts.NEW
    ids_p, log_p = gpu.generate(tokens.to(DEV), lens, max_new_tokens=new, return_logits=True)
    stats = {}
    ids_s, log_s = gpu.generate(tokens.to(DEV), lens, max_new_tokens=new, return_logits=True, speculate=3,
                                spec_stats=stats)
    assert ids_s.shape == ids_p.shape and log_s.shape == log_p.shape
    assert torch.equal(ids_s, log_s.argmax(-1))
    assert stats["emitted"] == [new, new] and 1 <= stats["steps"] <= new - 1
    diverged = 0
    for b in range(2):
        neq = (ids_p[b] != ids_s[b]).nonzero()
        if neq.numel() == 0:
            continue
        i = int(neq[0])  # the first divergence: everything before it is equal, by construction
        diverged += 1
        drift = (log_p[b, :i] - log_s[b, :i]).abs().max().item() if i else 0.0
        gap = abs(log_p[b, i, ids_p[b, i]].item() - log_p[b, i, ids_s[b, i]].item())
        print(f"sequence {b} diverges at {i}: gap {gap:.5f}, drift before it {drift:.5f}")
        assert gap <= 2 * drift, f"sequence {b} diverges at {i} with gap {gap} and only {drift} of drift"
    assert diverged <= 1
