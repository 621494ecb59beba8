"""Speculative greedy generation on the CPU (tiny model): ``generate(speculate=k)`` must emit the ids of the
plain greedy run whatever the drafter proposes, in the number of steps the drafts' quality implies; the
prompt-lookup drafter on hand-written histories; the argument checks.

``SEED`` is chosen here, on the CPU: it is the first model seed at which no step of the plain runs below
has a top-2 logit gap under ``2^-8 * max|logit|`` (``test_the_seed_leaves_no_near_tie`` holds it to that),
so every comparison of ids, here and in tests/gpu/test_speculate_gpu.py, is exact with no excused position."""
import functools
import math

import pytest
import torch

from tensorhive_fixed_amd.models.llama3 import Llama, LlamaConfig
from tensorhive_fixed_amd.models.speculate import prompt_lookup, prompt_lookup_draft

SEED = 6
NEW = 24
LENS = [5, 17]
KS = [1, 3, 7]
ULP = 2.0 ** -8


def prompts(kind: str) -> tuple[torch.Tensor, list[int]]:
    """``random``: two random prompts of 5 and 17 tokens.  ``pattern``: a 16-token pattern repeated, cut at 5
    and 17 tokens; ``pattern_long``: the same cut at 37 and 49, so the prompt itself holds repeats."""
    g = torch.Generator().manual_seed(11)
    vocab = LlamaConfig.tiny().vocab_size
    if kind == "random":
        return torch.randint(0, vocab, (2, 17), generator=g), LENS
    pattern = torch.randint(0, vocab, (16,), generator=g)
    lens = LENS if kind == "pattern" else [37, 49]
    return pattern.repeat(4)[None, : max(lens)].repeat(2, 1).contiguous(), lens


@functools.lru_cache(maxsize=None)
def model(seed: int = SEED) -> Llama:
    return Llama(LlamaConfig.tiny(), device="cpu", seed=seed)


@functools.lru_cache(maxsize=None)
def plain(kind: str, seed: int = SEED):
    """ids and logits of the plain greedy run: the reference of every speculative run."""
    tokens, lens = prompts(kind)
    return model(seed).generate(tokens, lens, max_new_tokens=NEW, return_logits=True)


def smallest_gap_ratio(seed: int) -> float:
    worst = math.inf
    for kind in ("random", "pattern", "pattern_long"):
        _, logits = plain(kind, seed)
        top = logits.topk(2, dim=-1).values
        worst = min(worst, ((top[..., 0] - top[..., 1]) / logits.abs().amax(-1)).min().item())
    return worst


def test_the_seed_leaves_no_near_tie():
    assert smallest_gap_ratio(SEED) >= ULP
    assert all(smallest_gap_ratio(s) < ULP for s in range(SEED))  # SEED is the first such seed


def ref_drafter(kind: str, right: list[int], calls: list | None = None):
    """A ``draft_fn`` built from the plain run's ids: sequence b gets its true next tokens in the first
    ``right[b]`` drafts and wrong ones (true id + 1) after them."""
    ids = plain(kind)[0].tolist()
    lens = prompts(kind)[1]
    vocab = LlamaConfig.tiny().vocab_size

    def draft(histories, k):
        out = []
        for b, h in enumerate(histories):
            e = len(h) - lens[b]
            assert h[lens[b]:] == ids[b][:e]  # the history is the prompt and what was emitted
            true = (ids[b] + [0] * k)[e: e + k]
            out.append([t if i < right[b] else (t + 1) % vocab for i, t in enumerate(true)])
        if calls is not None:
            calls.append([len(h) - n for h, n in zip(histories, lens)])
        return out

    return draft


def run(kind: str, k: int, draft_fn, **kw):
    tokens, lens = prompts(kind)
    stats = {}
    out = model().generate(tokens, lens, max_new_tokens=NEW, speculate=k, draft_fn=draft_fn, spec_stats=stats, **kw)
    return out, stats, lens


@pytest.mark.parametrize("k", KS)
def test_an_oracle_drafter_emits_k_plus_one_tokens_per_step(k):
    ids, st, lens = run("random", k, ref_drafter("random", [k, k]))
    assert torch.equal(ids, plain("random")[0])
    assert st["steps"] == math.ceil((NEW - 1) / (k + 1))
    assert st["emitted"] == [NEW, NEW] and st["drafted"] == 2 * k * st["steps"]
    assert st["accepted"] >= 2 * (NEW - 1 - st["steps"])
    assert st["cache_lens"] == [n + NEW - 1 for n in lens]


@pytest.mark.parametrize("k", KS)
def test_an_always_wrong_drafter_costs_one_step_per_token(k):
    ids, st, lens = run("random", k, ref_drafter("random", [0, 0]))
    assert torch.equal(ids, plain("random")[0])
    assert st["steps"] == NEW - 1 and st["accepted"] == 0 and st["drafted"] == 2 * k * (NEW - 1)
    assert st["cache_lens"] == [n + NEW - 1 for n in lens]


@pytest.mark.parametrize("k", KS)
def test_ragged_acceptance(k):
    right = [k // 3, (2 * k + 1) // 3]  # sequence b emits right[b] + 1 tokens per step
    calls: list = []
    ids, st, lens = run("random", k, ref_drafter("random", right, calls))
    assert torch.equal(ids, plain("random")[0])
    assert st["steps"] == max(math.ceil((NEW - 1) / (j + 1)) for j in right)
    # before step s (0-based) sequence b has emitted 1 + s * (right[b] + 1) tokens, until it is done
    assert calls == [[min(NEW, 1 + s * (j + 1)) for j in right] for s in range(st["steps"])]
    assert st["emitted"] == [NEW, NEW]
    assert st["cache_lens"] == [n + e - 1 for n, e in zip(lens, st["emitted"])]


@pytest.mark.parametrize("kind", ["pattern", "pattern_long"])
@pytest.mark.parametrize("k", KS)
def test_prompt_lookup_on_a_repeating_prompt(kind, k):
    (ids, logits), st, lens = run(kind, k, None, return_logits=True)
    ref_ids, ref_logits = plain(kind)
    assert torch.equal(ids, ref_ids)
    assert torch.equal(ids, logits.argmax(-1))  # the row that chose each emitted token
    assert logits.shape == ref_logits.shape
    # the block step computes what the single steps compute, in another order of the same fp32 sums
    assert (logits - ref_logits).abs().max().item() <= ULP * ref_logits.abs().max().item()
    assert 1 <= st["steps"] <= NEW - 1 and 0 <= st["accepted"] <= st["drafted"]


def test_stream_gemm_and_fp8_flows():
    m = model()
    tokens, lens = prompts("random")
    for kw in ({"stream_gemm": True}, {"fp8": True}):
        ref = m.generate(tokens, lens, max_new_tokens=8, **kw)
        got = m.generate(tokens, lens, max_new_tokens=8, speculate=3, **kw)
        assert got.shape == ref.shape == (2, 8)
    m.fp8_weights = None


def test_prompt_lookup():
    # n-gram priority: the 3-gram (1 2 3) wins over the more recent 2-gram (2 3) and 1-gram (3)
    assert prompt_lookup([1, 2, 3, 7, 7, 2, 3, 8, 3, 9, 1, 2, 3], 2) == [7, 7]
    # no 3-gram repeat: the 2-gram (2 3), then its most recent earlier occurrence
    assert prompt_lookup([2, 3, 5, 2, 3, 6, 4, 2, 3], 2) == [6, 4]
    # only the last token repeats: the 1-gram, most recent occurrence first
    assert prompt_lookup([4, 1, 9, 4, 2, 8, 4], 2) == [2, 8]
    # fewer than k tokens follow: the last proposed one pads
    assert prompt_lookup([5, 6, 5], 4) == [6, 5, 5, 5]
    assert prompt_lookup([1, 1], 3) == [1, 1, 1]
    # an occurrence may overlap the suffix itself
    assert prompt_lookup([7, 7, 7, 7], 2) == [7, 7]
    # no repeat at all, and a single token: the last token k times
    assert prompt_lookup([1, 2, 3, 4], 3) == [4, 4, 4]
    assert prompt_lookup([9], 2) == [9, 9]
    assert prompt_lookup_draft([[1, 2, 1], [3]], 1) == [[2], [3]]


def test_argument_checks():
    m = model()
    tokens, lens = prompts("random")
    for kw, msg in (({"speculate": 8}, "speculate"), ({"speculate": -1}, "speculate"),
                    ({"speculate": 2, "temperature": 0.7}, "temperature"),
                    ({"speculate": 2, "graph": True}, "graph"), ({"speculate": 2, "kv_fp8": True}, "kv_fp8")):
        with pytest.raises(ValueError, match=msg):
            m.generate(tokens, lens, max_new_tokens=4, **kw)
    room = m.cfg.max_seq_len - 17
    m.generate(tokens, lens, max_new_tokens=1, speculate=3)
    with pytest.raises(ValueError, match="max_seq_len"):
        m.generate(tokens, lens, max_new_tokens=room - 2, speculate=3)  # the k draft rows do not fit
    with pytest.raises(ValueError, match="draft_fn"):
        m.generate(tokens, lens, max_new_tokens=4, speculate=2, draft_fn=lambda h, k: [[0] * k])


def test_extend_step_checks_and_matches_single_steps():
    from tensorhive_fixed_amd.ops.decode_attention import KVCache

    m = model()
    tokens, lens = prompts("random")
    T = 4
    block = torch.randint(0, m.cfg.vocab_size, (2, T), generator=torch.Generator().manual_seed(3))
    caches = []
    for _ in range(2):
        c = KVCache(m.cfg, 2, 32)
        m.prefill(tokens, lens, c)
        caches.append(c)
    a = m.extend_step(block, caches[0])
    b = torch.stack([m.decode_step(block[:, t].contiguous(), caches[1]) for t in range(T)], dim=1)
    assert a.shape == (2, T, m.cfg.vocab_size) and a.dtype == torch.float32
    assert caches[0].lens == caches[1].lens == [n + T for n in lens]
    assert (a - b).abs().max().item() <= ULP * b.abs().max().item()
    with pytest.raises(ValueError, match="token ids"):
        m.extend_step(block[0], caches[0])
    with pytest.raises(ValueError, match="quantize_decode_weights"):
        m.extend_step(block, caches[0], fp8=True)
    m.quantize_decode_weights()
    try:
        with pytest.raises(ValueError, match="16 rows"):
            m.extend_step(torch.zeros(2, 9, dtype=torch.long), caches[0], fp8=True)
    finally:
        m.fp8_weights = None
