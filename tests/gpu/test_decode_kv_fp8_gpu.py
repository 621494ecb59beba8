"""The FP8 KV cache on the GPU (csrc/decode_attn_fp8.hip): attention against the fp64 oracle of
``tests/decode_kv_fp8_oracles.py`` with NaN codes and NaN scales in every dead row, the exact decode of
every finite e4m3 code at every byte position, the quantizing append bit for bit against the CPU rule,
the device-geometry form against the host form, reproducibility, isolation, the C entry points'
rejections, the quantizer on the device, and the flag through ``decode_graph`` and ``generate``.
``pytest -s`` prints the worst ``err / bound`` of the kernel tests when the module finishes."""
import functools
import math

import pytest
import torch

from tests import attention_oracles as ao
from tests import decode_kv_fp8_oracles as ko
from tests import decode_oracles as do

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
FP8 = torch.float8_e4m3fn
ULP = 2.0 ** -8
SMAX = do.SMAX
# Keys per workgroup step of the attention kernel: tiles of 128 (rep <= 4) or 64 (rep = 8) keys, two
# tiles per loop trip.  decode_oracles.KV_LENS has 63..65 and 255..257; these add T-1 / T / T+1 and
# 2T-1 / 2T / 2T+1 for the T in {64, 128, 256} they leave out.
STEP_LENS = [[127, 128, 129], [511, 512, 513]]
WORST = {}


def _record(what, err, rel):
    w = WORST.setdefault(what, [0.0, 0.0])
    w[0], w[1] = max(w[0], err / 2e-2), max(w[1], rel / 1e-2)


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from tensorhive_fixed_amd.ops import _lib
    lib = _lib.load(build_if_missing=True)
    for name in ("th_decode_attn_fp8", "th_decode_attn_fp8_dev", "th_decode_rope_append_fp8"):
        assert hasattr(lib, name), name
    yield
    print("\nworst err/bound (max abs, relative)")
    for k, (a, r) in sorted(WORST.items()):
        print(f"  {k:<28s} {a:.3f} {r:.3f}")


def _attn(q, cache, **kw):
    from tensorhive_fixed_amd.ops.decode_attention import decode_attention

    return decode_attention(q, cache, 0, **kw)


@functools.lru_cache(maxsize=None)
def _case(Hq, Hkv, lens):
    """An FP8 cache with NaN dead rows, q and the fp64 reference, shared by the split counts."""
    cache, q = ko.quantized_nan_dead_cache(Hq, Hkv, list(lens), DEV)
    return cache, q, ko.attention_fp64_fp8(q, cache)


@functools.lru_cache(maxsize=None)
def _profile_case(Hq, Hkv, profile):
    cache, q = ko.quantized_profile_dead_cache(Hq, Hkv, do.PROFILE_LENS, profile, DEV)
    return cache, q, ko.attention_fp64_fp8(q, cache)


def _close(o, ref, what):
    do.assert_attention_close(o, ref)
    od = o.detach().cpu().double()
    _record(what, (od - ref).abs().max().item(), ((od - ref).norm() / ref.norm()).item())


# ------------------------------------------------------------------------------- attention against fp64
@pytest.mark.parametrize("nsplit", do.NSPLITS, ids=lambda n: f"nsplit{n}")
@pytest.mark.parametrize("lens", do.KV_LENS, ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("Hq,Hkv", do.HEADS)
def test_attention_against_fp64(Hq, Hkv, lens, nsplit):
    cache, q, ref = _case(Hq, Hkv, tuple(lens))
    _close(_attn(q, cache, nsplit=nsplit), ref, "randn")


@pytest.mark.parametrize("nsplit", [1, 2, None], ids=lambda n: f"nsplit{n}")
@pytest.mark.parametrize("lens", STEP_LENS, ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("Hq,Hkv", do.HEADS)
def test_attention_around_the_step_sizes(Hq, Hkv, lens, nsplit):
    cache, q, ref = _case(Hq, Hkv, tuple(lens))
    _close(_attn(q, cache, nsplit=nsplit), ref, "randn, step tails")


@pytest.mark.parametrize("nsplit", do.NSPLITS, ids=lambda n: f"nsplit{n}")
@pytest.mark.parametrize("profile", ao.KEY_PROFILES)
@pytest.mark.parametrize("Hq,Hkv", [(8, 2), (8, 1)])
def test_attention_profiles_per_row(Hq, Hkv, profile, nsplit):
    cache, q, ref = _profile_case(Hq, Hkv, profile)
    err, rel = do.assert_rows_close(_attn(q, cache, nsplit=nsplit), ref, Hq)
    _record("profiles, per row", err, rel)


# --------------------------------------------------------------------------------------- exact decode
def _finite_codes():
    c = torch.arange(256, dtype=torch.uint8)
    return c[(c & 0x7F) != 0x7F]  # 254 of them


@pytest.mark.parametrize("rep", [1, 2, 4, 8])
def test_exact_decode_of_every_code_at_every_byte_position(rep):
    """One live key: p = 1, so o = bf16(code * vscale) exactly, a power-of-two vscale changing nothing.
    Row r of the 256 (sequence, KV head) rows holds code (j + r) mod 254 at byte j: every finite code
    sits at every byte position.  A fnuz reading, a wrong subnormal or sign, or a byte taken from another
    position of the 8-byte load all show."""
    from tensorhive_fixed_amd.ops.decode_attention import KVCache

    B, Hkv = 32, 8
    Hq = Hkv * rep
    cache = KVCache(do.attn_cfg(Hq, Hkv), B, SMAX, DEV, dtype=FP8)
    fin = _finite_codes()
    r = torch.arange(B * Hkv)[:, None]
    codes = fin[(torch.arange(128)[None, :] + r) % 254].view(B, Hkv, 128)
    vscale = (2.0 ** ((r % 5) - 3).float()).view(B, Hkv)
    g = torch.Generator().manual_seed(3)
    kv8 = cache.kv.view(torch.uint8)
    kv8.fill_(ko.NAN_CODE)
    cache.kv_scale.fill_(float("nan"))
    kv8[0, 1, :, :, 0] = codes.to(DEV)
    cache.kv_scale[0, 1, :, :, 0] = vscale.to(DEV)
    kv8[0, 0, :, :, 0] = torch.randint(0, 0x78, (B, Hkv, 128), generator=g, dtype=torch.uint8).to(DEV)
    cache.kv_scale[0, 0, :, :, 0] = 0.01
    cache.set_lens([1] * B)
    q = torch.randn(B, Hq * 128, generator=g).to(BF).to(DEV)
    want = (codes.view(FP8).float() * vscale[..., None]).to(BF)  # exact
    assert torch.equal(want.float(), codes.view(FP8).float() * vscale[..., None])
    want = want[:, :, None, :].expand(B, Hkv, rep, 128).reshape(B, Hq * 128)
    for kw in ({}, {"nsplit": 3}, {"device_geometry": True}):
        got = _attn(q, cache, **kw).cpu()
        assert torch.equal(got, want), (kw, (got != want).nonzero()[:4].tolist())


@pytest.mark.parametrize("Hq,Hkv", [(8, 1), (4, 1), (4, 2), (2, 2)])
def test_k_side_index_probe(Hq, Hkv):
    """One-hot q rows (one per dimension over the sequences and heads) against K rows of distinct codes
    and a distinctive V: the score of a key is one K byte, so a byte decoded from the wrong position or a
    scale taken from the wrong key moves the output far outside the bound."""
    from tensorhive_fixed_amd.ops.decode_attention import KVCache

    B, n = 128 // Hq, 200
    cache = KVCache(do.attn_cfg(Hq, Hkv), B, SMAX, DEV, dtype=FP8)
    g = torch.Generator().manual_seed(9)
    fin = _finite_codes()
    j, d = torch.arange(n)[:, None], torch.arange(128)[None, :]
    kcodes = torch.stack([fin[(37 * j + 11 * d + 5 * r) % 254] for r in range(B * Hkv)]).view(B, Hkv, n, 128)
    kscale = (0.004 * (1 + (torch.arange(n) % 7))).float().expand(B, Hkv, n)
    vcodes, vscale = ko.quantize_kv_rows(torch.randn(B, Hkv, n, 128, generator=g).to(BF))
    kv8 = cache.kv.view(torch.uint8)
    kv8.fill_(ko.NAN_CODE)
    cache.kv_scale.fill_(float("nan"))
    kv8[0, 0, :, :, :n] = kcodes.to(DEV)
    kv8[0, 1, :, :, :n] = vcodes.view(torch.uint8).to(DEV)
    cache.kv_scale[0, 0, :, :, :n] = kscale.to(DEV)
    cache.kv_scale[0, 1, :, :, :n] = vscale.to(DEV)
    cache.set_lens([n] * B)
    q = torch.zeros(B, Hq, 128)
    q.view(B * Hq, 128)[torch.arange(B * Hq), torch.arange(B * Hq) % 128] = 6.0  # scores up to 6 * 12.5 / 11.3
    q = q.view(B, Hq * 128).to(BF).to(DEV)
    ref = ko.attention_fp64_fp8(q, cache)
    for nsplit in (1, 3):
        _close(_attn(q, cache, nsplit=nsplit), ref, "k index probe")


# ------------------------------------------------------------------------------------------- append
@pytest.mark.parametrize("Hq,Hkv", [(8, 2), (4, 1)])
def test_append_bit_for_bit(Hq, Hkv):
    """The bf16 kernel's append on a bf16 cache and the FP8 append on an FP8 cache from the same qkv: q
    equal, K codes and scales the CPU quantization of the bf16 kernel's K row, V those of the input row,
    and no other byte or scale of the sentinel-filled cache changed."""
    from tensorhive_fixed_amd.ops.decode_attention import KVCache, rope_append

    pos = [0, 77, SMAX - 1]
    cfg = do.attn_cfg(Hq, Hkv, n_layers=2)
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(3, Hq + 2 * Hkv, 128, generator=g)
    qkv[0, Hq + Hkv] = 0  # a zero v row
    qkv[1, Hq + Hkv] = 0
    qkv[1, Hq + Hkv, 3:25] = torch.tensor([2.0 ** -e for e in range(22)])  # the ladder, down to zero codes
    qkv[2, Hq + Hkv, 101] = -9.0  # a row whose absmax is negative
    qkv[2, Hq, 64] = -11.0  # and a k row led by a negative element before the rotation
    qkv = qkv.view(3, -1).to(BF).to(DEV)
    ref = KVCache(cfg, 3, SMAX, DEV)
    ref.set_lens(pos)
    c8 = KVCache(cfg, 3, SMAX, DEV, dtype=FP8)
    c8.kv.view(torch.uint8).fill_(0x5A)
    c8.kv_scale.fill_(-7.0)
    c8.set_lens(pos)
    q_ref = rope_append(qkv, ref, 1)
    q = rope_append(qkv, c8, 1)
    assert torch.equal(q, q_ref)
    got, got_s, rows = c8.kv.view(torch.uint8).cpu(), c8.kv_scale.cpu(), ref.kv.cpu()
    touched = torch.zeros(got_s.shape, dtype=torch.bool)
    for b, p in enumerate(pos):
        touched[1, :, b, :, p] = True
        assert torch.equal(rows[1, 1, b, :, p], qkv[b].cpu().view(-1, 128)[Hq + Hkv:])  # v is the input row
        for j in range(2):
            codes, scale = ko.quantize_kv_rows(rows[1, j, b, :, p])
            assert torch.equal(got_s[1, j, b, :, p], scale), (j, b, got_s[1, j, b, :, p], scale)
            bad = (got[1, j, b, :, p] != codes.view(torch.uint8)).nonzero()
            assert bad.numel() == 0, (j, b, bad[:4].tolist())
    assert got_s[1, 1, 0, 0, pos[0]].item() == 1.0 and not bool(got[1, 1, 0, 0, pos[0]].any())  # the zero row
    assert bool((got[~touched] == 0x5A).all()) and bool((got_s[~touched] == -7.0).all())


# ------------------------------------------------------------------------------- other kernel checks
@pytest.mark.parametrize("nsplit", [None, 3, 8], ids=lambda n: f"nsplit{n}")
@pytest.mark.parametrize("lens", do.KV_LENS[1:] + STEP_LENS, ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("Hq,Hkv", do.HEADS)
def test_device_geometry_has_the_bits_of_the_host_rule(Hq, Hkv, lens, nsplit):
    cache, q, _ = _case(Hq, Hkv, tuple(lens))
    assert torch.equal(_attn(q, cache, nsplit=nsplit, device_geometry=True), _attn(q, cache, nsplit=nsplit))


@pytest.mark.parametrize("longest", [256, 512])
@pytest.mark.parametrize("Hq,Hkv", do.HEADS)
def test_new_token_lands_on_a_split_boundary(Hq, Hkv, longest):
    """``new=1`` with ``longest`` exactly 256 / 512: the live split count steps to 1 / 2 with this very
    key, under a grid fixed for 1024 rows."""
    lens = [longest - 1, 100, longest - 2]
    cache, q = ko.quantized_nan_dead_cache(Hq, Hkv, [n + 1 for n in lens], DEV, seed=longest)
    ref = ko.attention_fp64_fp8(q, cache)
    cache.set_lens(lens)
    host = _attn(q, cache, new=1)
    assert torch.equal(_attn(q, cache, new=1, device_geometry=True), host)
    _close(host, ref, "randn")
    for nsplit in (3, 8):
        assert torch.equal(_attn(q, cache, nsplit=nsplit, new=1, device_geometry=True),
                           _attn(q, cache, nsplit=nsplit, new=1))


@pytest.mark.parametrize("nsplit", [3, None])
def test_bit_reproducible(nsplit):
    cache, q, _ = _case(8, 2, (1, 200, 1024))
    assert torch.equal(_attn(q, cache, nsplit=nsplit), _attn(q, cache, nsplit=nsplit))


@pytest.mark.parametrize("Hq,Hkv", [(8, 2), (8, 1)])
def test_a_poisoned_sequence_leaves_the_others_alone(Hq, Hkv):
    lens = (257, 256, 255)
    cache, q, _ = _case(Hq, Hkv, lens)
    clean = {ns: _attn(q, cache, nsplit=ns) for ns in (None, 3)}
    codes, scales = cache.kv.view(torch.uint8).clone(), cache.kv_scale.clone()
    try:
        cache.kv.view(torch.uint8)[:, :, 1] = ko.NAN_CODE
        cache.kv_scale[:, :, 1] = float("nan")
        for ns, want in clean.items():
            got = _attn(q, cache, nsplit=ns)
            assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    finally:
        cache.kv.view(torch.uint8).copy_(codes)
        cache.kv_scale.copy_(scales)


def test_entry_point_rejections():
    """Straight through the C ABI: a negative code, nothing launched, output and workspace untouched."""
    from tensorhive_fixed_amd.ops import _lib

    lib = _lib.load()
    stream = _lib.stream_ptr(torch.device(DEV))
    Hq, Hkv, B = 8, 2, 3
    cache, q, ref = _case(Hq, Hkv, (257, 256, 255))
    kc, vc, ksc, vsc = cache.k(0), cache.v(0), cache.k_scale(0), cache.v_scale(0)
    sb, sh, ssb, ssh = kc.stride(0), kc.stride(1), ksc.stride(0), ksc.stride(1)
    o = torch.full((B, Hq * 128), 7.0, device=DEV, dtype=BF)
    ws = torch.full((B * Hq * 8 * 130,), 7.0, device=DEV)
    scale = 1.0 / math.sqrt(128)

    def host(B=B, Hq=Hq, Hkv=Hkv, Dh=128, Smax=SMAX, sb=sb, sh=sh, ssb=ssb, ssh=ssh, nsplit=2, chunk=129,
             kp=kc.data_ptr(), ksp=ksc.data_ptr()):
        return lib.th_decode_attn_fp8(q.data_ptr(), kp, vc.data_ptr(), ksp, vsc.data_ptr(), cache.lens_dev.data_ptr(),
                                      o.data_ptr(), ws.data_ptr(), B, Hq, Hkv, Dh, Smax, sb, sh, ssb, ssh, nsplit,
                                      chunk, 0, scale, stream)

    def dev(want=2, min_keys=256, cap=4, **kw):
        a = dict(B=B, Hq=Hq, Hkv=Hkv, Dh=128, Smax=SMAX, sb=sb, sh=sh, ssb=ssb, ssh=ssh)
        a.update(kw)
        return lib.th_decode_attn_fp8_dev(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), ksc.data_ptr(), vsc.data_ptr(),
                                          cache.lens_dev.data_ptr(), o.data_ptr(), ws.data_ptr(), a["B"], a["Hq"],
                                          a["Hkv"], a["Dh"], a["Smax"], a["sb"], a["sh"], a["ssb"], a["ssh"], cap,
                                          want, min_keys, 0, scale, stream)

    bad_geometry = [dict(Dh=64), dict(B=0), dict(Hq=6), dict(Hq=32, Hkv=2), dict(Smax=0), dict(Smax=(1 << 24) + 1),
                    dict(sh=sh + 8), dict(sb=sb + 8), dict(sh=SMAX * 128 - 16), dict(sb=Hkv * sh - 16),
                    dict(ssh=SMAX - 1), dict(ssb=Hkv * ssh - 1)]
    for kw in bad_geometry:
        assert host(**kw) < 0, kw
        assert dev(**kw) < 0, kw
    for kw in (dict(nsplit=0), dict(nsplit=1025), dict(chunk=0), dict(nsplit=1024, chunk=1 << 21),
               dict(kp=kc.data_ptr() + 8), dict(ksp=ksc.data_ptr() + 2)):
        assert host(**kw) < 0, kw
    for kw in (dict(cap=0), dict(cap=1025), dict(want=0), dict(min_keys=0)):
        assert dev(**kw) < 0, kw
    qkv = torch.zeros(B, (Hq + 2 * Hkv) * 128, device=DEV, dtype=BF)
    for kw in bad_geometry:
        a = dict(B=B, Hq=Hq, Hkv=Hkv, Dh=128, Smax=SMAX, sb=sb, sh=sh, ssb=ssb, ssh=ssh)
        a.update(kw)
        rc = lib.th_decode_rope_append_fp8(qkv.data_ptr(), cache.lens_dev.data_ptr(), ws.data_ptr(), ws.data_ptr(),
                                           o.data_ptr(), kc.data_ptr(), vc.data_ptr(), ksc.data_ptr(), vsc.data_ptr(),
                                           a["B"], a["Hq"], a["Hkv"], a["Dh"], a["Smax"], a["sb"], a["sh"], a["ssb"],
                                           a["ssh"], stream)
        assert rc < 0, kw
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()) and bool((ws == 7.0).all())
    assert host() == 0  # a good one runs
    torch.cuda.synchronize()
    _close(o, ref, "randn")
    assert torch.equal(o, _attn(q, cache, nsplit=2))


def test_quantizer_on_the_device_returns_the_cpu_bytes():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(5, 3, 700, 128, generator=g).to(BF)
    x[1, 2, 3] = 0
    x[2, 0, 5] = 0
    x[2, 0, 5, :22] = torch.tensor([2.0 ** -e for e in range(22)]).to(BF)
    x[3] *= 1e-3
    x[4, 1] *= 300.0
    c_c, s_c = ko.quantize_kv_rows(x)
    c_g, s_g = ko.quantize_kv_rows(x.to(DEV))
    assert c_g.is_cuda and c_g.dtype == FP8 and s_g.dtype == torch.float32
    assert torch.equal(s_g.cpu(), s_c)
    assert torch.equal(c_g.cpu().view(torch.uint8), c_c.view(torch.uint8))


# ------------------------------------------------------------------------------------------ tiny model
@functools.lru_cache(maxsize=None)
def _tiny_pair():
    from tensorhive_fixed_amd.models.llama3 import Llama, LlamaConfig

    cfg = LlamaConfig.tiny()
    cpu = Llama(cfg, device="cpu", seed=3)
    gpu = Llama(cfg, device=DEV, seed=0)
    gpu.load_state_dict(cpu.state_dict())
    gpu.quantize_decode_weights()
    tokens = torch.randint(0, cfg.vocab_size, (2, 64), generator=torch.Generator().manual_seed(11))
    return cpu, gpu, tokens


def _teacher_forced(model, tokens, lens, steps, step, dtype=FP8):
    """Incremental logits [B, 1 + steps, vocab]: bf16 prefill (prompts zero-padded to 64 columns) into a
    cache of ``dtype``, then ``step(next_tokens, cache)`` per position."""
    from tensorhive_fixed_amd.ops.decode_attention import KVCache

    cache = KVCache(model.cfg, tokens.shape[0], 64, tokens.device, dtype=dtype)
    prompt = torch.zeros_like(tokens)
    for b, n in enumerate(lens):
        prompt[b, :n] = tokens[b, :n]
    h = model.prefill(prompt, lens, cache)
    out = [torch.mm(h, model.lm_head.t()).float()]
    for i in range(steps):
        nxt = torch.stack([tokens[b, n + i] for b, n in enumerate(lens)])
        out.append(step(nxt, cache).clone())
    return torch.stack(out, dim=1)


@pytest.mark.parametrize("kw", [dict(stream_gemm=True), dict(fp8=True)], ids=["stream", "fp8"])
def test_decode_graph_on_an_fp8_cache_replays_the_eager_step(kw):
    _, gpu, tokens = _tiny_pair()
    toks, lens, steps = tokens.to(DEV), [5, 17], 20
    eager = _teacher_forced(gpu, toks, lens, steps, lambda t, c: gpu.decode_step(t, c, **kw))
    graphs = {}

    def replay(t, cache):
        if id(cache) not in graphs:
            assert cache.is_fp8
            graphs[id(cache)] = gpu.decode_graph(cache, **kw)
        return graphs[id(cache)].step(t)

    assert torch.equal(_teacher_forced(gpu, toks, lens, steps, replay), eager)


def test_generate_kv_fp8_graph_equals_eager():
    _, gpu, tokens = _tiny_pair()
    prompt = tokens[:, :17].to(DEV)
    kw = dict(max_new_tokens=8, return_logits=True, kv_fp8=True, stream_gemm=True)
    ids, logits = gpu.generate(prompt, [5, 17], **kw)
    assert ids.shape == (2, 8) and logits.shape == (2, 8, gpu.cfg.vocab_size) and logits.dtype == torch.float32
    assert torch.equal(ids, logits.argmax(-1))
    ids_g, logits_g = gpu.generate(prompt, [5, 17], graph=True, **kw)
    assert torch.equal(ids_g, ids) and torch.equal(logits_g, logits)


def test_kv_fp8_logits_against_the_cpu_flow():
    """The GPU FP8-cache flow against the CPU FP8-cache flow.  ``e_kv`` is the reference's own quantization
    movement (CPU FP8-cache flow against the CPU bf16 logits, no code under test): the two flows differ
    at bf16 level before the quantization, a code that flips moves an element by one whole step, and a
    moved row maximum re-grids the row, hence the ``2 * e_kv`` term.  A sanity bound; the kernel tests
    above carry the accuracy."""
    cpu, gpu, tokens = _tiny_pair()
    lens, steps = [5, 17], 20
    bf16_ref = cpu.logits(tokens).float()
    ref = _teacher_forced(cpu, tokens, lens, steps, lambda t, c: cpu.decode_step(t, c))
    full = gpu.logits(tokens.to(DEV)).float().cpu()
    inc = _teacher_forced(gpu, tokens.to(DEV), lens, steps, lambda t, c: gpu.decode_step(t, c)).cpu()
    rows = [slice(n - 1, n + steps) for n in lens]
    e_new = max((inc[b] - ref[b]).abs().max().item() for b in range(len(lens)))
    e_full = max((full[b, r] - bf16_ref[b, r]).abs().max().item() for b, r in enumerate(rows))
    peak = max(bf16_ref[b, r].abs().max().item() for b, r in enumerate(rows))
    e_kv = max((ref[b] - bf16_ref[b, r]).abs().max().item() for b, r in enumerate(rows))
    print(f"e_new {e_new:.5f}  e_full {e_full:.5f}  e_kv {e_kv:.5f}  max|logit| {peak:.4f}")
    assert e_new <= 2 * e_full + ULP * peak + 2 * e_kv
