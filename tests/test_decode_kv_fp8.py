"""The FP8 (e4m3) KV cache on the CPU: the quantization rule, the cache object, the reference append
and attention against the fp64 oracle of ``tests/decode_kv_fp8_oracles.py``, an f32 emulation of the
kernel's order of scaling under the same bounds, and ``generate(kv_fp8=True)``."""
import functools

import pytest
import torch

from tests import attention_oracles as ao
from tests import decode_kv_fp8_oracles as ko
from tests import decode_oracles as do

BF = torch.bfloat16
FP8 = torch.float8_e4m3fn


def _q(x):
    from tensorhive_fixed_amd.ops.decode_attention import quantize_kv_rows

    return quantize_kv_rows(x)


# ------------------------------------------------------------------------------------------ quantizer
def test_quantizer_zero_row_and_absmax():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 5, 128, generator=g).to(BF)
    x[1, 2] = 0
    x[2, 0, 17] = -9.5  # a row whose absmax is negative
    codes, scale = _q(x)
    assert codes.shape == x.shape and codes.dtype == FP8 and scale.shape == (3, 5) and scale.dtype == torch.float32
    assert scale[1, 2].item() == 1.0 and bool((codes[1, 2].view(torch.uint8) == 0).all())
    assert torch.equal(scale, torch.where(x.float().abs().amax(-1) > 0, x.float().abs().amax(-1) / 448, 1.0))
    assert not bool(((codes.view(torch.uint8) & 0x7F) == 0x7F).any())  # never a NaN code
    # an element equal to the absmax maps to +-448
    at_max = x.float().abs() == x.float().abs().amax(-1, keepdim=True)
    at_max[1, 2] = False
    assert torch.equal(codes.float()[at_max], 448.0 * x.float()[at_max].sign())
    assert codes.float()[2, 0, 17].item() == -448.0


def test_quantizer_never_a_nan_code_on_extreme_rows():
    big = torch.tensor([3.3895e38, -3.3895e38, 1e-38, 0.0] * 32).to(BF)  # bf16 max, a tiny value
    tiny = torch.tensor([9.2e-41] * 128).to(BF)  # a bf16 subnormal row: absmax / 448 is an f32 subnormal
    for row in (big, tiny, -tiny):
        codes, scale = _q(row[None])
        assert bool(torch.isfinite(scale).all()) and bool((scale > 0).all())
        assert not bool(((codes.view(torch.uint8) & 0x7F) == 0x7F).any())
        assert bool(torch.isfinite(codes.float()).all())


def test_quantizer_ladder_reaches_down_through_the_subnormal_codes_to_zero():
    """Row elements 2^-e under an absmax of 1: the quotient is 448 * 2^-e = 1.75 * 2^(8-e), a normal code
    down to e = 14 (the smallest normal exponent is -6), 7 subnormal steps of 2^-9 at e = 15, then
    1.75 steps -> 2 (e = 17), 0.875 -> 1 (e = 18) and 0.44 -> 0 (e = 19).
    e = 16 is 3.5 steps, a tie that the last bit of the f32 quotient decides: 3 or 4 steps."""
    n = 22
    x = torch.zeros(1, 128)
    x[0, :n] = torch.tensor([2.0 ** -e for e in range(n)])
    x[0, n:2 * n] = -x[0, :n]
    codes, scale = _q(x.to(BF))
    assert scale.item() == torch.tensor(1.0) / torch.tensor(448.0)  # absmax 1
    v = codes.float()[0]
    step = 2.0 ** -9
    want = {e: 7.0 * 2.0 ** (6 - e) for e in range(16)}
    want.update({17: 2 * step, 18: step, 19: 0.0, 20: 0.0, 21: 0.0})
    for e, w in want.items():
        assert v[e].item() == w and v[n + e].item() == -w, (e, v[e].item(), w)
    assert v[16].item() in (3 * step, 4 * step) and v[n + 16].item() == -v[16].item()
    assert bool((codes.view(torch.uint8)[0, 2 * n:] == 0).all())
    assert not bool(((codes.view(torch.uint8) & 0x7F) == 0x7F).any())


def test_quantizer_is_idempotent_on_representable_rows():
    """Rows of e4m3 values times a power-of-two scale, the absmax being 448 * scale: the codes come back."""
    g = torch.Generator().manual_seed(1)
    codes = torch.randint(0, 256, (6, 128), generator=g, dtype=torch.uint8)
    codes[(codes & 0x7F) == 0x7F] = 0x3C
    codes[:, 5] = 0x7E  # 448 in every row
    codes[3, 5] = 0xFE  # -448
    for scale in (1.0, 2.0 ** -7, 2.0 ** 5):
        x = (codes.view(FP8).float() * scale).to(BF)  # exact: 4 significant bits, a power-of-two factor
        assert torch.equal(x.float(), codes.view(FP8).float() * scale)
        c2, s2 = _q(x)
        assert bool((s2 == scale).all())
        assert torch.equal(c2.float(), codes.view(FP8).float())  # +-0 aside, the same codes


# ---------------------------------------------------------------------------------------------- cache
def test_kvcache_dtype_and_scale_shape():
    from tensorhive_fixed_amd.ops.decode_attention import KVCache, kv_cache_bytes

    cfg = do.attn_cfg(8, 2, n_layers=3)
    c = KVCache(cfg, 2, 64)
    assert c.kv.dtype == BF and c.kv_scale is None and not c.is_fp8
    c8 = KVCache(cfg, 2, 64, "cpu", dtype=FP8)
    assert c8.kv.dtype == FP8 and c8.kv.shape == (3, 2, 2, 2, 64, 128) and c8.kv.element_size() == 1
    assert c8.kv_scale.dtype == torch.float32 and c8.kv_scale.shape == (3, 2, 2, 2, 64) and c8.is_fp8
    assert kv_cache_bytes(cfg, 2, 64, FP8) == c8.kv.numel() + 4 * c8.kv_scale.numel()
    assert kv_cache_bytes(cfg, 2, 64) == 2 * c.kv.numel()
    for bad in (torch.float16, torch.float32, torch.float8_e5m2, torch.uint8):
        with pytest.raises(ValueError):
            KVCache(cfg, 2, 64, "cpu", dtype=bad)


def test_fill_quantizes_rows_and_copies_on_bf16():
    from tensorhive_fixed_amd.ops.decode_attention import KVCache

    cfg = do.attn_cfg(4, 2, n_layers=2)
    g = torch.Generator().manual_seed(2)
    k = torch.randn(3, 7, 2, 128, generator=g).to(BF).transpose(1, 2)  # [B, Hkv, S, 128], strided
    v = torch.randn(3, 7, 2, 128, generator=g).to(BF).transpose(1, 2)
    c = KVCache(cfg, 3, 16)
    c.fill(1, k, v)
    assert torch.equal(c.k(1)[:, :, :7], k) and torch.equal(c.v(1)[:, :, :7], v)
    assert not bool(c.kv[0].any()) and not bool(c.kv[1, :, :, :, 7:].any())
    c8 = KVCache(cfg, 3, 16, dtype=FP8)
    c8.fill(1, k, v)
    for j, x in enumerate((k, v)):
        codes, scale = _q(x.contiguous())
        assert torch.equal(c8.kv[1, j, :, :, :7].view(torch.uint8), codes.view(torch.uint8))
        assert torch.equal(c8.kv_scale[1, j, :, :, :7], scale)
    assert not bool(c8.kv.view(torch.uint8)[0].any()) and bool((c8.kv_scale[0] == 1).all())
    with pytest.raises(ValueError):
        c8.fill(0, k[:, :1], v[:, :1])
    with pytest.raises(ValueError):
        c8.fill(0, k.float(), v.float())


def test_reference_append_touches_one_row_and_one_scale():
    from tensorhive_fixed_amd.ops.decode_attention import KVCache, rope_append

    Hq, Hkv = 4, 1
    pos = [0, 77, do.SMAX - 1]
    cfg = do.attn_cfg(Hq, Hkv, n_layers=2)
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(3, (Hq + 2 * Hkv) * 128, generator=g).to(BF)
    ref = KVCache(cfg, 3, do.SMAX)
    ref.set_lens(pos)
    q_ref = rope_append(qkv, ref, 1)  # the bf16 reference: the rows before quantization
    c8 = KVCache(cfg, 3, do.SMAX, dtype=FP8)
    c8.kv.view(torch.uint8).fill_(0x5A)
    c8.kv_scale.fill_(-7.0)
    c8.set_lens(pos)
    q = rope_append(qkv, c8, 1)
    assert torch.equal(q, q_ref)
    touched = torch.zeros(c8.kv_scale.shape, dtype=torch.bool)
    for b, p in enumerate(pos):
        touched[1, :, b, :, p] = True
        for j in range(2):
            codes, scale = _q(ref.kv[1, j, b, :, p])
            assert torch.equal(c8.kv[1, j, b, :, p].view(torch.uint8), codes.view(torch.uint8))
            assert torch.equal(c8.kv_scale[1, j, b, :, p], scale)
    assert bool((c8.kv.view(torch.uint8)[~touched] == 0x5A).all()) and bool((c8.kv_scale[~touched] == -7.0).all())


# ------------------------------------------------------------------------------------------ attention
@functools.lru_cache(maxsize=None)
def _case(Hq, Hkv, lens):
    cache, q = ko.quantized_nan_dead_cache(Hq, Hkv, list(lens), "cpu")
    return cache, q, ko.attention_fp64_fp8(q, cache)


@functools.lru_cache(maxsize=None)
def _profile_case(Hq, Hkv, profile):
    cache, q = ko.quantized_profile_dead_cache(Hq, Hkv, do.PROFILE_LENS, profile, "cpu")
    return cache, q, ko.attention_fp64_fp8(q, cache)


def test_oracle_caches_hold_nan_in_dead_rows():
    cache, _, ref = _case(4, 1, (1, 200, 1024))
    codes = cache.kv.view(torch.uint8)
    for b, n in enumerate(cache.lens):
        assert bool((codes[:, :, b, :, n:] == ko.NAN_CODE).all()) and bool(cache.kv_scale[:, :, b, :, n:].isnan().all())
        assert bool(torch.isfinite(cache.kv[:, :, b, :, :n].float()).all())
        assert bool(torch.isfinite(cache.kv_scale[:, :, b, :, :n]).all())
    assert bool(torch.isfinite(ref).all())


@pytest.mark.parametrize("lens", do.KV_LENS, ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("Hq,Hkv", do.HEADS)
def test_reference_attention_against_fp64(Hq, Hkv, lens):
    from tensorhive_fixed_amd.ops.decode_attention import decode_attention

    cache, q, ref = _case(Hq, Hkv, tuple(lens))
    do.assert_attention_close(decode_attention(q, cache, 0), ref)


@pytest.mark.parametrize("lens", do.KV_LENS, ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("Hq,Hkv", do.HEADS)
def test_kernel_order_of_scaling_in_f32_against_fp64(Hq, Hkv, lens):
    """codes dotted, then ``* kscale``; ``p * vscale`` before PV: the bounds hold for that order in f32."""
    cache, q, ref = _case(Hq, Hkv, tuple(lens))
    do.assert_attention_close(ko.attention_f32_kernel_order(q, cache), ref)


@pytest.mark.parametrize("profile", ao.KEY_PROFILES)
def test_kernel_order_of_scaling_in_f32_on_the_profiles(profile):
    cache, q, ref = _profile_case(8, 2, profile)
    do.assert_attention_close(ko.attention_f32_kernel_order(q, cache), ref)


def test_new_rows_count():
    """``new=1`` attends over the row just appended, as on a bf16 cache."""
    from tensorhive_fixed_amd.ops.decode_attention import decode_attention

    cache, q, _ = _case(4, 1, (63, 64, 65))
    want = decode_attention(q, cache, 0)
    cache.set_lens([62, 63, 64])
    try:
        assert torch.equal(decode_attention(q, cache, 0, new=1), want)
    finally:
        cache.set_lens([63, 64, 65])


# ------------------------------------------------------------------------------------------- generate
@functools.lru_cache(maxsize=None)
def _tiny():
    from tensorhive_fixed_amd.models.llama3 import Llama, LlamaConfig

    cfg = LlamaConfig.tiny()
    model = Llama(cfg, device="cpu", seed=3)
    tokens = torch.randint(0, cfg.vocab_size, (2, 64), generator=torch.Generator().manual_seed(11))
    return model, tokens


def _flow(model, prompt, lens, steps, dtype):
    """Greedy generation through ``prefill`` + ``decode_step`` on a cache of ``dtype``."""
    from tensorhive_fixed_amd.ops.decode_attention import KVCache

    S = max(lens)
    cache = KVCache(model.cfg, prompt.shape[0], S + steps, "cpu", dtype=dtype)
    live = torch.arange(S)[None, :] < torch.tensor(lens)[:, None]
    h = model.prefill(prompt[:, :S] * live, lens, cache)
    logits = [torch.mm(h, model.lm_head.t()).float()]
    for _ in range(steps - 1):
        logits.append(model.decode_step(logits[-1].argmax(-1), cache))
    return torch.stack(logits, dim=1), cache


def test_generate_kv_fp8_on_the_cpu():
    model, tokens = _tiny()
    prompt, lens = tokens[:, :17], [5, 17]
    ids, logits = model.generate(prompt, lens, max_new_tokens=8, return_logits=True, kv_fp8=True)
    assert ids.shape == (2, 8) and logits.shape == (2, 8, model.cfg.vocab_size) and logits.dtype == torch.float32
    assert torch.equal(ids, logits.argmax(-1))
    want, cache = _flow(model, prompt, lens, 8, FP8)
    assert cache.is_fp8 and cache.lens == [12, 24]
    assert torch.equal(logits, want)
    ids_g, logits_g = model.generate(prompt, lens, max_new_tokens=8, return_logits=True, kv_fp8=True, graph=True)
    assert torch.equal(ids_g, ids) and torch.equal(logits_g, logits)  # on the CPU a graph is the eager step


def test_generate_default_is_the_bf16_cache_bit_for_bit():
    """Without the flag nothing moves: the default run is the flow on a ``KVCache`` built without a dtype,
    whose prefill rows are the plain copies of the rotated K and of V, and differs from the FP8 run."""
    model, tokens = _tiny()
    prompt, lens = tokens[:, :17], [5, 17]
    ids, logits = model.generate(prompt, lens, max_new_tokens=8, return_logits=True)
    ids_f, logits_f = model.generate(prompt, lens, max_new_tokens=8, return_logits=True, kv_fp8=False)
    want, cache = _flow(model, prompt, lens, 8, BF)
    assert cache.kv.dtype == BF and cache.kv_scale is None
    assert torch.equal(logits, want) and torch.equal(logits_f, want) and torch.equal(ids, ids_f)
    _, logits8 = model.generate(prompt, lens, max_new_tokens=8, return_logits=True, kv_fp8=True)
    assert not torch.equal(logits8[:, 1:], logits[:, 1:])
    assert torch.equal(logits8[:, 0], logits[:, 0])  # token 0 comes from the bf16 prefill either way


def test_generate_workload_reports_the_cache(capsys):
    import json

    from tensorhive_fixed_amd.workloads import llama3_generate

    done = {}
    for flag in ([], ["--fp8-kv"]):
        assert llama3_generate.main(["--model", "tiny", "--batch", "2", "--prompt-len", "9", "--max-new-tokens", "4",
                                     "--device", "cpu", *flag]) == 0
        done[bool(flag)] = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert done[False]["kv_dtype"] == "bfloat16" and done[True]["kv_dtype"] == "float8_e4m3fn"
    cfg = _tiny()[0].cfg
    rows = cfg.n_layers * 2 * 2 * cfg.n_kv_heads * 13
    assert done[False]["kv_cache_mb"] == round(rows * 256 / 2 ** 20, 1)
    assert done[True]["kv_cache_mb"] == round(rows * 132 / 2 ** 20, 1)
