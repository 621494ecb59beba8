"""The gfx950 decode kernels (csrc/decode_attn.hip) and KV-cache generation on the GPU: split-KV
attention against an fp64 softmax with NaN in every dead cache row, bit reproducibility, RoPE +
cache append, incremental logits against the existing full-sequence forward, ``generate``."""
import functools

import pytest
import torch

from tests import decode_oracles as do

pytestmark = pytest.mark.gpu

DEV = "cuda"
ULP = 2.0 ** -8


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from tensorhive_fixed_amd.ops import _lib
    _lib.load(build_if_missing=True)
    assert hasattr(_lib.load(), "th_decode_attn") and hasattr(_lib.load(), "th_decode_rope_append")


@functools.lru_cache(maxsize=None)
def _case(Hq, Hkv, lens):
    """Inputs and their fp64 reference, computed once per shape and shared by the split counts."""
    cache, q = do.nan_dead_cache(Hq, Hkv, list(lens), DEV)
    return cache, q, do.attention_fp64(q, cache)


@pytest.mark.parametrize("nsplit", do.NSPLITS, ids=lambda n: f"nsplit{n}")
@pytest.mark.parametrize("lens", do.KV_LENS, ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("Hq,Hkv", do.HEADS)
def test_decode_attention_against_fp64(Hq, Hkv, lens, nsplit):
    from tensorhive_fixed_amd.ops.decode_attention import decode_attention

    cache, q, ref = _case(Hq, Hkv, tuple(lens))
    do.assert_attention_close(decode_attention(q, cache, 0, nsplit=nsplit), ref)


@pytest.mark.parametrize("nsplit", [3, None])
def test_decode_attention_is_bit_reproducible(nsplit):
    from tensorhive_fixed_amd.ops.decode_attention import decode_attention

    cache, q, _ = _case(8, 2, (1, 200, 1024))
    a = decode_attention(q, cache, 0, nsplit=nsplit)
    b = decode_attention(q, cache, 0, nsplit=nsplit)
    assert torch.equal(a, b)


def test_rope_append():
    from tensorhive_fixed_amd.ops.decode_attention import KVCache, rope_append

    Hq, Hkv = 8, 2
    pos = [0, 77, do.SMAX - 1]
    cfg = do.attn_cfg(Hq, Hkv, n_layers=2)
    g = torch.Generator().manual_seed(5)
    host = KVCache(cfg, 3, do.SMAX, "cpu")
    host.kv.copy_(torch.randn(host.kv.shape, generator=g))
    host.set_lens(pos)
    qkv = torch.randn(3, (Hq + 2 * Hkv) * 128, generator=g).to(torch.bfloat16)
    dev = KVCache(cfg, 3, do.SMAX, DEV)
    dev.kv.copy_(host.kv)
    dev.set_lens(pos)
    before = host.kv.clone()
    q_ref = rope_append(qkv, host, 1)  # the CPU reference
    q = rope_append(qkv.to(DEV), dev, 1)
    got = dev.kv.cpu()
    touched = torch.zeros(before.shape, dtype=torch.bool)
    for b, p in enumerate(pos):
        touched[1, :, b, :, p] = True
        assert torch.equal(got[1, 1, b, :, p], qkv[b, (Hq + Hkv) * 128:].view(Hkv, 128))  # v bit-exact
    assert torch.equal(got[~touched], before[~touched])  # no other row written
    # q and k under the bound of the RoPE kernel's own test (tests/gpu/test_kernels_gpu.py)
    for a, ref in ((q.cpu(), q_ref), (got[1, 0][touched[1, 0]], host.kv[1, 0][touched[1, 0]])):
        err = (a.float() - ref.float()).abs().max().item()
        assert err <= 3e-2 + 1e-2 * ref.float().abs().max().item(), err


@functools.lru_cache(maxsize=None)
def _tiny_pair():
    from tensorhive_fixed_amd.models.llama3 import Llama, LlamaConfig

    cfg = LlamaConfig.tiny()
    cpu = Llama(cfg, device="cpu", seed=3)
    gpu = Llama(cfg, device=DEV, seed=0)
    gpu.load_state_dict(cpu.state_dict())
    tokens = torch.randint(0, cfg.vocab_size, (2, 64), generator=torch.Generator().manual_seed(11))
    return cpu, gpu, tokens


def _teacher_forced(model, tokens, lens, steps):
    """Incremental logits [B, 1 + steps, vocab] (prompts zero-padded to 64 columns for the prefill)."""
    from tensorhive_fixed_amd.ops.decode_attention import KVCache

    cache = KVCache(model.cfg, tokens.shape[0], 64, tokens.device)
    prompt = torch.zeros_like(tokens)
    for b, n in enumerate(lens):
        prompt[b, :n] = tokens[b, :n]
    h = model.prefill(prompt, lens, cache)
    out = [torch.mm(h, model.lm_head.t()).float()]
    for i in range(steps):
        out.append(model.decode_step(torch.stack([tokens[b, n + i] for b, n in enumerate(lens)]), cache))
    return torch.stack(out, dim=1)


def test_incremental_logits_no_worse_than_the_full_forward():
    cpu, gpu, tokens = _tiny_pair()
    lens, steps = [5, 17], 20
    ref = cpu.logits(tokens).float()  # CPU fp32-path logits of the same weights
    full = gpu.logits(tokens.to(DEV)).float().cpu()
    inc = _teacher_forced(gpu, tokens.to(DEV), lens, steps).cpu()
    rows = [slice(n - 1, n + steps) for n in lens]
    e_new = max((inc[b] - ref[b, r]).abs().max().item() for b, r in enumerate(rows))
    e_full = max((full[b, r] - ref[b, r]).abs().max().item() for b, r in enumerate(rows))
    peak = max(ref[b, r].abs().max().item() for b, r in enumerate(rows))
    print(f"e_new {e_new:.5f}  e_full {e_full:.5f}  max|logit| {peak:.4f}")
    assert e_new <= 2 * e_full + ULP * peak


def test_generate_on_gpu():
    from tensorhive_fixed_amd.ops.decode_attention import KVCache

    _, gpu, tokens = _tiny_pair()
    lens = [5, 17]
    prompt = tokens[:, :17].to(DEV)
    ids, logits = gpu.generate(prompt, lens, max_new_tokens=8, return_logits=True)
    assert ids.shape == (2, 8) and logits.shape == (2, 8, gpu.cfg.vocab_size)
    assert int(ids.min()) >= 0 and int(ids.max()) < gpu.cfg.vocab_size
    assert torch.equal(ids, logits.argmax(-1))
    padded = torch.zeros((2, 64), device=DEV, dtype=prompt.dtype)
    for b, n in enumerate(lens):
        padded[b, :n] = prompt[b, :n]
    h = gpu.prefill(padded, lens, KVCache(gpu.cfg, 2, 64, DEV))
    step0 = torch.mm(h, gpu.lm_head.t()).float()
    # the same prompt rows through the same kernels; what lies after a prompt differs (padding here,
    # the longer prompt's tokens in generate) and is masked by causality
    err = (logits[:, 0] - step0).abs().max().item()
    assert err <= ULP * step0.abs().max().item(), err
