"""The KV-cache attention kernels (csrc/decode_attn.hip, decode_attn_fp8.hip, extend_attn.hip) at every
length, stride and offset.

1. One sequence per length 1..520 (block kernel: old lengths 0..264) in one launch, on layer 1 of a cache
   whose layer 0 and dead rows are NaN, rep 1 / 2 / 4 / 8, split counts whose chunks are a multiple of no
   key tile: every (sequence, head) row against fp64, and the device-geometry form bit for bit against
   the host rule with the longest sequence at index 0 and at index 300.
2. The C ABI on padded strides, with ``Smax`` below the allocation, at append positions outside
   ``[0, Smax)`` and with arguments it must refuse.  Every buffer is a slice at least 64 rows inside a
   larger allocation (NaN around inputs, a bit pattern around outputs): a kernel that steps outside its
   rows shows as NaN or a broken pattern and cannot leave the allocation.
3. Offsets that only a large cache reaches: a batch offset of 2^32 bytes, and rows up to 2^24 of one run.

``pytest -s`` prints the worst ``err / bound`` per family and the peak memory of the large tests when the
module finishes."""
import functools
import math
import types

import pytest
import torch

from tests import decode_geometry_oracles as dg
from tests import decode_kv_fp8_oracles as ko
from tests import decode_oracles as do
from tests import extend_oracles as eo

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
FP8 = torch.float8_e4m3fn
FRAME = 64 * 128  # elements around every buffer handed to the ABI: 64 rows
SCALE = 1.0 / math.sqrt(128)
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
_PATTERN = {1: 0x5A, 2: 0x5A5A, 4: 0x5A5A5A5A}
WORST = {}
PEAK = {}


def _record(what, o, ref, Hq):
    o = o.detach().cpu().double().reshape(-1, Hq, 128)
    ref = ref.reshape(-1, Hq, 128)
    err = (o - ref).abs().amax(-1).max().item()
    rel = ((o - ref).norm(dim=-1) / ref.norm(dim=-1)).max().item()
    w = WORST.setdefault(what, [0.0, 0.0])
    w[0], w[1] = max(w[0], err / 2e-2), max(w[1], rel / 1e-2)


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from tensorhive_fixed_amd.ops import _lib
    lib = _lib.load(build_if_missing=True)
    for name in ("th_decode_attn", "th_decode_attn_dev", "th_decode_rope_append", "th_decode_attn_fp8",
                 "th_decode_attn_fp8_dev", "th_decode_rope_append_fp8", "th_extend_attn",
                 "th_decode_rope_append_block"):
        assert hasattr(lib, name), name
    yield
    print("\nworst per-row err/bound (max abs, relative)")
    for k, (a, r) in sorted(WORST.items()):
        print(f"  {k:<34s} {a:.3f} {r:.3f}")
    print("peak device memory of the large tests (GiB)")
    for k, v in sorted(PEAK.items()):
        print(f"  {k:<34s} {v / 2 ** 30:.2f}")


def _lib():
    from tensorhive_fixed_amd.ops import _lib as m

    return m.load(), m.stream_ptr(torch.device(DEV))


def _decode(q, cache, layer=1, **kw):
    from tensorhive_fixed_amd.ops.decode_attention import decode_attention

    return decode_attention(q, cache, layer, **kw)


def _extend(q, cache, layer=1, nsplit=None):
    from tensorhive_fixed_amd.ops.extend_attention import extend_attention

    return extend_attention(q, cache, layer, nsplit=nsplit)


# ------------------------------------------------------------------------------ 1. the length sweeps
@functools.lru_cache(maxsize=None)
def _sweep(Hq, Hkv, perm, fp8):
    return dg.sweep_cache(Hq, Hkv, dg.SWEEP_LENS[perm], DEV, fp8=fp8)


@functools.lru_cache(maxsize=None)
def _block_sweep(Hq, Hkv, T):
    return dg.sweep_block_cache(Hq, Hkv, dg.BLOCK_LENS, T, DEV)


_KINDS = pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
_PERMS = pytest.mark.parametrize("perm", list(dg.SWEEP_LENS))
_HEADS = pytest.mark.parametrize("Hq,Hkv", dg.HEADS)


@pytest.mark.parametrize("nsplit", dg.NSPLITS, ids=lambda n: f"nsplit{n}")
@_PERMS
@_KINDS
@_HEADS
def test_decode_attention_at_every_length(Hq, Hkv, fp8, perm, nsplit):
    """520 sequences, one per length, in one launch: every (sequence, head) row inside the bounds."""
    cache, q, ref = _sweep(Hq, Hkv, perm, fp8)
    o = _decode(q, cache, nsplit=nsplit)
    do.assert_rows_close(o, ref, Hq)
    _record("sweep decode " + ("fp8" if fp8 else "bf16"), o, ref, Hq)


@pytest.mark.parametrize("nsplit", dg.NSPLITS, ids=lambda n: f"nsplit{n}")
@pytest.mark.parametrize("T", dg.BLOCKS, ids=lambda t: f"T{t}")
@_HEADS
def test_extend_attention_at_every_length(Hq, Hkv, T, nsplit):
    cache, q, ref = _block_sweep(Hq, Hkv, T)
    o = _extend(q, cache, nsplit=nsplit)
    eo.assert_block_close(o, ref, Hq)
    _record("sweep block", o, ref, Hq)


@pytest.mark.parametrize("nsplit", [None, 3, 7], ids=lambda n: f"nsplit{n}")
@_PERMS
@_KINDS
@_HEADS
def test_device_geometry_has_the_bits_of_the_host_rule(Hq, Hkv, fp8, perm, nsplit):
    """B = 520: the kernel's reduction of the lengths takes nine trips of 64 lanes, and the longest
    sequence sits at index 0 or 300."""
    from tensorhive_fixed_amd.ops.decode_attention import (MIN_KEYS_PER_SPLIT, device_split_geometry,
                                                           pick_nsplit)

    cache, q, ref = _sweep(Hq, Hkv, perm, fp8)
    host = _decode(q, cache, nsplit=nsplit)
    got = _decode(q, cache, nsplit=nsplit, device_geometry=True)
    assert torch.equal(got, host), (got != host).any(-1).nonzero()[:8].flatten().tolist()
    do.assert_rows_close(got, ref, Hq)
    lens = cache.lens
    if nsplit is None:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        ns = pick_nsplit(cache.batch, Hkv, max(lens), cus)
        dev = device_split_geometry(lens, 0, -(-cus // (cache.batch * Hkv)), cache.max_len, MIN_KEYS_PER_SPLIT,
                                    pick_nsplit(cache.batch, Hkv, cache.max_len, cus))
    else:
        ns, dev = nsplit, device_split_geometry(lens, 0, nsplit, cache.max_len, min_keys=1, cap=nsplit)
    assert dev == dg.host_geometry(lens, 0, ns)


# ------------------------------------------------------------------- 2. the C ABI: frames and padded strides
def _flat(n, dtype, fill):
    """``n + 2 * FRAME`` elements: ``"nan"`` (NaN, the NaN code, or INT_MAX for the lengths) or ``"pattern"``."""
    buf = torch.empty(n + 2 * FRAME, device=DEV, dtype=dtype)
    if fill == "pattern":
        buf.view(_INT[buf.element_size()]).fill_(_PATTERN[buf.element_size()])
    elif dtype.is_floating_point:
        buf.fill_(float("nan"))
    else:
        buf.fill_(ko.NAN_CODE if dtype == torch.uint8 else 2 ** 31 - 1)
    return buf


def _framed(t, fill="nan"):
    """A copy of ``t`` in the middle of a larger buffer; returns (buffer, view)."""
    buf = _flat(t.numel(), t.dtype, fill)
    view = buf[FRAME: FRAME + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _out(shape, dtype):
    """An output of ``shape`` inside a larger buffer, all of it the bit pattern; (buffer, view)."""
    n = math.prod(shape)
    buf = _flat(n, dtype, "pattern")
    return buf, buf[FRAME: FRAME + n].view(shape)


def _frame_intact(buf, n):
    iv = buf.view(_INT[buf.element_size()])
    pat = _PATTERN[buf.element_size()]
    return bool((iv[:FRAME] == pat).all()) and bool((iv[FRAME + n:] == pat).all())


def _untouched(buf):
    return bool((buf.view(_INT[buf.element_size()]) == _PATTERN[buf.element_size()]).all())


def _padded(rows, pad_h, pad_b):
    """``rows [B, H, S, ...]`` at strides ``stride_h = S * row + pad_h`` and ``stride_b = H * stride_h + pad_b``
    inside a NaN buffer with a frame; returns (buffer, view, stride_b, stride_h)."""
    B, H, S = rows.shape[:3]
    E = rows.shape[3] if rows.dim() == 4 else 1
    sh = S * E + pad_h
    sb = H * sh + pad_b
    buf = _flat(B * sb, rows.dtype, "nan")
    view = buf.as_strided(rows.shape, (sb, sh, E, 1)[: rows.dim()], FRAME)
    view.copy_(rows)
    return buf, view, sb, sh


def _bits(t):
    return t.view(_INT[t.element_size()])


def _setup(kind, Hq, Hkv, kv, scales, q, lens, nsplit, pads=(24, 40), spads=(3, 5)):
    """Everything one attention call is handed.  ``kv [2, B, Hkv, S, 128]`` bf16 (``kind`` "bf16" / "block") or
    uint8 codes ("fp8", with ``scales [2, B, Hkv, S]``); pads in elements (bf16), bytes (FP8), floats (scales)."""
    a = types.SimpleNamespace(kind=kind, Hq=Hq, Hkv=Hkv, B=kv.shape[1], S=kv.shape[3], nsplit=nsplit)
    a.T = q.shape[1] if kind == "block" else 1
    a.kbuf, a.k, a.sb, a.sh = _padded(kv[0], *pads)
    a.vbuf, a.v, _, _ = _padded(kv[1], *pads)
    if kind == "fp8":
        a.ksbuf, a.ks, a.ssb, a.ssh = _padded(scales[0], *spads)
        a.vsbuf, a.vs, _, _ = _padded(scales[1], *spads)
    a.qbuf, a.q = _framed(q)
    a.obuf, a.o = _out(q.shape, BF)
    a.nws = a.B * a.T * Hq * nsplit * 130
    a.wsbuf, a.ws = _out((a.nws,), torch.float32)
    a.lbuf, a.lens = _framed(torch.tensor(lens, dtype=torch.int32, device=DEV))
    return a


def _attn(a, smax, chunk=None, dev=False, /, **kw):
    """One call of the entry point of ``a.kind`` (``dev``: its device-geometry form with a forced split
    count); keyword arguments replace what the call would pass.  Returns the status."""
    lib, stream = _lib()
    p = dict(B=a.B, T=a.T, Hq=a.Hq, Hkv=a.Hkv, Dh=128, Smax=smax, sb=a.sb, sh=a.sh, nsplit=a.nsplit, chunk=chunk,
             want=a.nsplit, min_keys=1, extra=0)
    if a.kind == "fp8":
        p.update(ssb=a.ssb, ssh=a.ssh)
    p.update(kw)
    head = (a.q.data_ptr(), a.k.data_ptr(), a.v.data_ptr())
    mid = (a.lens.data_ptr(), a.o.data_ptr(), a.ws.data_ptr())
    if a.kind == "block":
        return lib.th_extend_attn(*head, *mid, p["B"], p["T"], p["Hq"], p["Hkv"], p["Dh"], p["Smax"], p["sb"], p["sh"],
                                  p["nsplit"], p["chunk"], SCALE, stream)
    geo = (p["B"], p["Hq"], p["Hkv"], p["Dh"], p["Smax"], p["sb"], p["sh"])
    tail = ((p["nsplit"], p["want"], p["min_keys"], p["extra"]) if dev else (p["nsplit"], p["chunk"], p["extra"]))
    if a.kind == "fp8":
        fn = lib.th_decode_attn_fp8_dev if dev else lib.th_decode_attn_fp8
        return fn(*head, a.ks.data_ptr(), a.vs.data_ptr(), *mid, *geo, p["ssb"], p["ssh"], *tail, SCALE, stream)
    fn = lib.th_decode_attn_dev if dev else lib.th_decode_attn
    return fn(*head, *mid, *geo, *tail, SCALE, stream)


def _outputs_framed(a):
    torch.cuda.synchronize()
    return _frame_intact(a.obuf, a.o.numel()) and _frame_intact(a.wsbuf, a.nws)


def _kv_of(cache, layer):
    if cache.is_fp8:
        return cache.kv.view(torch.uint8)[layer], cache.kv_scale[layer]
    return cache.kv[layer], None


ABI_LENS = [1, 200, 513]
ABI_HEADS = [(4, 2), (8, 1)]
ATTN_ENTRIES = [("bf16", False), ("bf16", True), ("fp8", False), ("fp8", True), ("block", False)]


def _entry_id(e):
    return {"bf16": "th_decode_attn", "fp8": "th_decode_attn_fp8", "block": "th_extend_attn"}[e[0]] + \
        ("_dev" if e[1] else "")



@functools.lru_cache(maxsize=None)
def _abi_case(kind, Hq, Hkv):
    if kind == "block":
        return dg.sweep_block_cache(Hq, Hkv, ABI_LENS, 3, DEV)
    return dg.sweep_cache(Hq, Hkv, ABI_LENS, DEV, fp8=kind == "fp8")


@pytest.mark.parametrize("entry", ATTN_ENTRIES, ids=_entry_id)
@pytest.mark.parametrize("Hq,Hkv", ABI_HEADS)
def test_attention_on_padded_strides(Hq, Hkv, entry):
    """Head and batch strides with pads (NaN) that are no multiple of a row: the bits of the wrapper on a
    contiguous cache holding the same rows, with the same split count and chunk."""
    kind, dev = entry
    cache, q, ref = _abi_case(kind, Hq, Hkv)
    kv, scales = _kv_of(cache, 1)
    pads = (48, 80) if kind == "fp8" else (24, 40)
    a = _setup(kind, Hq, Hkv, kv, scales, q, ABI_LENS, 3, pads)
    chunk = dg.host_geometry(ABI_LENS, a.T if kind == "block" else 0, 3)[1]
    assert _attn(a, cache.max_len, chunk, dev) == 0
    assert _outputs_framed(a)
    want = _extend(q, cache, nsplit=3) if kind == "block" else _decode(q, cache, nsplit=3, device_geometry=dev)
    assert torch.equal(a.o, want)
    do.assert_rows_close(a.o.reshape(-1, Hq * 128), ref.reshape(-1, Hq * 128), Hq)
    _record("padded strides " + kind, a.o, ref, Hq)


def _tables(rows):
    from tensorhive_fixed_amd.ops.rope import rope_tables

    cos, sin = rope_tables(rows, 128, do.attn_cfg(1, 1).rope_theta, torch.device(DEV))
    return _framed(cos)[1], _framed(sin)[1]


def _append(kind, a, qkv, pos, smax, table_rows, /, **kw):
    """One call of the append of ``a.kind`` on ``a``'s cache buffers; returns (status, q_out buffer, view)."""
    lib, stream = _lib()
    cos, sin = _tables(table_rows)
    _, qkv_v = _framed(qkv)
    _, pos_v = _framed(torch.tensor(pos, dtype=torch.int32, device=DEV))
    qbuf, q_out = _out(tuple(qkv.shape[:-1]) + (a.Hq * 128,), BF)
    p = dict(B=a.B, T=a.T, Hq=a.Hq, Hkv=a.Hkv, Dh=128, Smax=smax, sb=a.sb, sh=a.sh)
    if kind == "fp8":
        p.update(ssb=a.ssb, ssh=a.ssh)
    p.update(kw)
    head = (qkv_v.data_ptr(), pos_v.data_ptr(), cos.data_ptr(), sin.data_ptr(), q_out.data_ptr(), a.k.data_ptr(),
            a.v.data_ptr())
    if kind == "block":
        rc = lib.th_decode_rope_append_block(*head, p["B"], p["T"], p["Hq"], p["Hkv"], p["Dh"], p["Smax"], p["sb"],
                                             p["sh"], stream)
    elif kind == "fp8":
        rc = lib.th_decode_rope_append_fp8(*head, a.ks.data_ptr(), a.vs.data_ptr(), p["B"], p["Hq"], p["Hkv"], p["Dh"],
                                           p["Smax"], p["sb"], p["sh"], p["ssb"], p["ssh"], stream)
    else:
        rc = lib.th_decode_rope_append(*head, p["B"], p["Hq"], p["Hkv"], p["Dh"], p["Smax"], p["sb"], p["sh"], stream)
    torch.cuda.synchronize()
    return rc, qbuf, q_out


def _cache_buffers(a):
    return [a.kbuf, a.vbuf] + ([a.ksbuf, a.vsbuf] if a.kind == "fp8" else [])


def _cache_views(a):
    return [a.k, a.v] + ([a.ks, a.vs] if a.kind == "fp8" else [])


def _single_appends(kind, Hq, Hkv, qkv3, pos, Smax, alloc):
    """What the wrapper's single-token append writes for every (b, t) whose row ``pos[b] + t`` is in
    ``[0, Smax)``, on a contiguous cache of ``alloc`` rows: {(b, t): (row, q, [k, v(, kscale, vscale)] rows)}."""
    from tensorhive_fixed_amd.ops.decode_attention import KVCache, rope_append

    B, T = qkv3.shape[:2]
    cache = KVCache(do.attn_cfg(Hq, Hkv, max_seq_len=alloc), B, alloc, DEV, dtype=FP8 if kind == "fp8" else BF)
    out = {}
    for t in range(T):
        rows = [p + t if 0 <= p + t < Smax else 0 for p in pos]
        cache.set_lens(rows)
        q = rope_append(qkv3[:, t].contiguous(), cache, 0)
        for b, p in enumerate(pos):
            if 0 <= p + t < Smax:
                kv = [_bits(cache.kv[0, j, b, :, p + t]).clone() for j in range(2)]
                if kind == "fp8":
                    kv += [cache.kv_scale[0, j, b, :, p + t].clone() for j in range(2)]
                out[(b, t)] = (p + t, q[b].clone(), kv)
    return out


def _check_append(a, before, qbuf, q_out, want):
    """The cache buffers are ``before`` with exactly the rows of ``want`` replaced; q_out holds the rows of
    ``want`` and the pattern everywhere else, frame included."""
    for j, (buf0, view, got) in enumerate(zip(before, _cache_views(a), _cache_buffers(a))):
        exp = _bits(buf0).clone()
        ev = exp.as_strided(view.shape, view.stride(), FRAME)
        for (b, t), (row, q, kv) in want.items():
            ev[b, :, row] = _bits(kv[j])
        assert torch.equal(_bits(got), exp), f"cache buffer {j}"
    expect_q = torch.full_like(_bits(qbuf), _PATTERN[2])
    eq = expect_q[FRAME: FRAME + q_out.numel()].view(a.B, a.T, -1)
    for (b, t), (row, q, kv) in want.items():
        eq[b, t] = _bits(q)
    assert torch.equal(_bits(qbuf), expect_q)


@pytest.mark.parametrize("kind", ["bf16", "fp8", "block"])
@pytest.mark.parametrize("Hq,Hkv", ABI_HEADS)
def test_appends_on_padded_strides(Hq, Hkv, kind):
    """The padded layout gets exactly the rows the contiguous call writes, with the same bits; every pad
    and frame byte is unchanged."""
    cache, _, _ = _abi_case("fp8" if kind == "fp8" else "bf16", Hq, Hkv)
    kv, scales = _kv_of(cache, 1)
    T = 3 if kind == "block" else 1
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(3, T, (Hq + 2 * Hkv) * 128, generator=g).to(BF).to(DEV)
    a = _setup(kind, Hq, Hkv, kv, scales, torch.zeros(3, T, Hq * 128, dtype=BF), ABI_LENS, 1,
               (48, 80) if kind == "fp8" else (24, 40))
    before = [b.clone() for b in _cache_buffers(a)]
    rc, qbuf, q_out = _append(kind, a, qkv if kind == "block" else qkv[:, 0].contiguous(), ABI_LENS, cache.max_len,
                              cache.max_len)
    assert rc == 0
    want = _single_appends(kind, Hq, Hkv, qkv, ABI_LENS, cache.max_len, cache.max_len)
    assert len(want) == 3 * T
    _check_append(a, before, qbuf, q_out, want)


SMAX_LOW, ALLOC = 512, 1024


def _low_smax_rows(Hkv, fp8, seed=3):
    """kv ``[2, 3, Hkv, 1024, 128]`` (and scales): randn rows below 512, NaN from there on."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn(2, 3, Hkv, ALLOC, 128, generator=g).to(BF)
    if not fp8:
        rows[:, :, :, SMAX_LOW:] = float("nan")
        return rows.to(DEV), None
    codes, scale = ko.quantize_kv_rows(rows)
    codes = codes.view(torch.uint8).clone()
    codes[:, :, :, SMAX_LOW:] = ko.NAN_CODE
    scale[:, :, :, SMAX_LOW:] = float("nan")
    return codes.to(DEV), scale.to(DEV)


def _fp64_row(q, k, v):
    """fp64 attention of ``q [Hq*128]`` over ``k / v [Hkv, n, 128]`` -> ``[Hq*128]``."""
    Hkv = k.shape[0]
    s = q.double().view(Hkv, -1, 128) @ k.double().transpose(-1, -2) / math.sqrt(128)
    return (s.softmax(-1) @ v.double()).reshape(-1)


@pytest.mark.parametrize("entry", ATTN_ENTRIES, ids=_entry_id)
def test_lengths_are_clamped_to_smax_below_the_allocation(entry):
    """``Smax = 512`` on 1024 allocated rows with NaN from row 512 on: device lengths past ``Smax`` and below
    zero give the bits of the clamped ones, a sequence of no keys gives exact zeros, and the rows are those
    of fp64 over the first ``min(len, 512)`` keys."""
    kind, dev = entry
    Hq, Hkv = 4, 2
    T = 4 if kind == "block" else 1
    kv, scales = _low_smax_rows(Hkv, kind == "fp8")
    g = torch.Generator().manual_seed(11)
    q = torch.randn((3, T, Hq * 128) if kind == "block" else (3, Hq * 128), generator=g).to(BF).to(DEV)
    wild, clamped = ([700, 510, -5], [512, 510, 0]) if kind == "block" else ([700, 512, -5], [512, 512, 0])
    chunk = -(-(SMAX_LOW + T) // 3)
    outs = []
    for lens in (wild, clamped):
        a = _setup(kind, Hq, Hkv, kv, scales, q, lens, 3, (48, 80) if kind == "fp8" else (24, 40))
        assert a.sh >= ALLOC * 128
        assert _attn(a, SMAX_LOW, chunk, dev) == 0
        assert _outputs_framed(a)
        outs.append(a.o.clone())
    assert torch.isfinite(outs[0].float()).all()
    assert torch.equal(outs[0], outs[1])
    kd = kv.cpu().double() if scales is None else kv.cpu().view(FP8).double() * scales.cpu().double()[..., None]
    ref = torch.zeros(3, T, Hq * 128, dtype=torch.float64)
    for b, n0 in enumerate(clamped):
        for t in range(T):
            n = min(n0 + t + 1, SMAX_LOW) if kind == "block" else n0
            if n:
                ref[b, t] = _fp64_row(q.cpu().view(3, T, -1)[b, t], kd[0, b, :, :n], kd[1, b, :, :n])
    o = outs[0].view(3, T, -1)
    if kind != "block":
        assert not bool(o[2].view(torch.int16).any())  # exact zeros
        o, ref = o[:2], ref[:2]
    do.assert_rows_close(o.reshape(-1, Hq * 128), ref.reshape(-1, Hq * 128), Hq)
    _record("Smax below allocation " + kind, o, ref, Hq)


@pytest.mark.parametrize("kind", ["bf16", "fp8", "block"])
def test_appends_outside_smax_write_nothing(kind):
    """Positions -1, ``Smax`` and ``Smax + 1`` leave every byte of the framed cache and of q_out alone while
    ``Smax - 1`` in the same launch is written; ``Smax`` is 512 on 1024 allocated rows, and the tables
    are those of 1024 rows."""
    Hq, Hkv = 4, 2
    if kind == "block":  # T = 2: rows -2 -1 | 512 513 | 513 514 | 510 511 | 511 (512) | (-1) 0
        T, pos = 2, [-2, SMAX_LOW, SMAX_LOW + 1, SMAX_LOW - 2, SMAX_LOW - 1, -1]
    else:
        T, pos = 1, [-1, SMAX_LOW, SMAX_LOW + 1, SMAX_LOW - 1]
    B = len(pos)
    kv = torch.full((2, B, Hkv, ALLOC, 128), 0x5A if kind == "fp8" else -7.0, device=DEV,
                    dtype=torch.uint8 if kind == "fp8" else BF)
    scales = torch.full((2, B, Hkv, ALLOC), -7.0, device=DEV) if kind == "fp8" else None
    g = torch.Generator().manual_seed(13)
    qkv = torch.randn(B, T, (Hq + 2 * Hkv) * 128, generator=g).to(BF).to(DEV)
    a = _setup(kind, Hq, Hkv, kv, scales, torch.zeros(B, T, Hq * 128, dtype=BF), [0] * B, 1,
               (48, 80) if kind == "fp8" else (24, 40))
    before = [b.clone() for b in _cache_buffers(a)]
    rc, qbuf, q_out = _append(kind, a, qkv if kind == "block" else qkv[:, 0].contiguous(), pos, SMAX_LOW, ALLOC)
    assert rc == 0
    want = _single_appends(kind, Hq, Hkv, qkv, pos, SMAX_LOW, ALLOC)
    assert sorted(want) == ([(3, 0), (3, 1), (4, 0), (5, 1)] if kind == "block" else [(3, 0)])
    _check_append(a, before, qbuf, q_out, want)


def test_entry_point_rejections():
    """The bf16 and block entry points straight through the C ABI: a non-zero status, nothing launched, the
    output, the workspace and the cache untouched; a good call afterwards runs."""
    Hq, Hkv = 8, 2
    cache, q, ref = dg.sweep_cache(Hq, Hkv, ABI_LENS, DEV)
    bcache, bq, bref = dg.sweep_block_cache(Hq, Hkv, ABI_LENS, 3, DEV)
    S = cache.max_len
    a = _setup("bf16", Hq, Hkv, cache.kv[1], None, q, ABI_LENS, 3, (0, 0))
    blk = _setup("block", Hq, Hkv, bcache.kv[1], None, bq, ABI_LENS, 3, (0, 0))
    sb, sh = a.sb, a.sh
    bad_geometry = [dict(Dh=64), dict(B=0), dict(Hq=6), dict(Hq=32), dict(Smax=0), dict(sh=sh + 4), dict(sb=sb + 4),
                    dict(sh=S * 128 - 8), dict(sb=Hkv * sh - 8)]
    bad_split = [dict(nsplit=0), dict(nsplit=1025), dict(chunk=0), dict(nsplit=1024, chunk=1 << 21)]
    for kw in bad_geometry:
        assert _attn(a, S, 172, False, **kw) != 0, kw
        assert _attn(a, S, 172, True, **kw) != 0, kw
    for kw in bad_split:
        assert _attn(a, S, 172, False, **kw) != 0, kw
    for kw in (dict(nsplit=0), dict(nsplit=1025), dict(want=0), dict(min_keys=0)):  # nsplit is the device form's cap
        assert _attn(a, S, 172, True, **kw) != 0, kw
    bs, bsb, bsh = bcache.max_len, blk.sb, blk.sh
    block_geometry = [dict(Dh=64), dict(B=0), dict(Hq=6), dict(Hq=32), dict(Smax=0), dict(sh=bsh + 4), dict(sb=bsb + 4),
                      dict(sh=bs * 128 - 8), dict(sb=Hkv * bsh - 8), dict(T=0), dict(T=9)]
    for kw in block_geometry + bad_split:
        assert _attn(blk, bs, 172, False, **kw) != 0, kw
    assert _untouched(a.obuf) and _untouched(a.wsbuf) and _untouched(blk.obuf) and _untouched(blk.wsbuf)
    g = torch.Generator().manual_seed(17)
    qkv = torch.randn(3, 3, (Hq + 2 * Hkv) * 128, generator=g).to(BF).to(DEV)
    for x, kind, cases, smax in ((a, "bf16", bad_geometry, S), (blk, "block", block_geometry, bs)):
        before = [b.clone() for b in _cache_buffers(x)]
        for kw in cases:
            rc, qbuf, _ = _append(kind, x, qkv if kind == "block" else qkv[:, 0].contiguous(), ABI_LENS, smax, smax, **kw)
            assert rc != 0, (kind, kw)
            assert _untouched(qbuf), (kind, kw)
        assert all(torch.equal(_bits(b0), _bits(b1)) for b0, b1 in zip(before, _cache_buffers(x)))
    # good calls run
    assert _attn(a, S, 171, False) == 0 and _outputs_framed(a)
    assert torch.equal(a.o, _decode(q, cache, nsplit=3))
    do.assert_rows_close(a.o, ref, Hq)
    a.o.view(torch.int16).fill_(_PATTERN[2])
    assert _attn(a, S, None, True) == 0 and _outputs_framed(a)
    assert torch.equal(a.o, _decode(q, cache, nsplit=3))
    assert _attn(blk, bs, 172, False) == 0 and _outputs_framed(blk)
    assert torch.equal(blk.o, _extend(bq, bcache, nsplit=3))
    eo.assert_block_close(blk.o, bref, Hq)


# --------------------------------------------------------------- 3. offsets that only a large cache reaches
def _need(nbytes):
    """Skip unless the device has 16 GB free and room for the test's ``nbytes``; start a peak-memory count."""
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    need = max(16 * 10 ** 9, nbytes + 2 ** 30)
    if free < need:
        pytest.skip(f"{free} bytes of device memory free, {need} needed")
    torch.cuda.reset_peak_memory_stats()


def _peak(what):
    torch.cuda.synchronize()
    PEAK[what] = max(PEAK.get(what, 0), torch.cuda.max_memory_allocated())
    torch.cuda.empty_cache()


BIG_LENS = [65, 300, 512]


def _big_case(kind, T=1):
    """A contiguous cache of 3 sequences x 1 head x 512 rows (NaN dead rows), q, the fp64 reference and the
    lengths; the block case keeps ``T`` live rows past every length."""
    from tensorhive_fixed_amd.ops.decode_attention import KVCache

    block = kind == "block"
    lens = [65, 300, 512 - T] if block else BIG_LENS
    g = torch.Generator().manual_seed(21)
    cfg = do.attn_cfg(1, 1, max_seq_len=512)
    src = KVCache(cfg, 3, 512, "cpu")
    rows = torch.randn(src.kv.shape, generator=g).to(BF)
    for b, n in enumerate(lens):
        rows[:, :, b, :, n + (T if block else 0):] = float("nan")
    src.kv.copy_(rows)
    src.set_lens(lens)
    q = torch.randn((3, T, 128) if block else (3, 128), generator=g).to(BF).to(DEV)
    if kind == "fp8":
        small = ko._quantized(src, DEV)
    else:
        small = KVCache(cfg, 3, 512, DEV)
        small.kv.copy_(src.kv)
        small.set_lens(lens)
    ref = (ko.attention_fp64_fp8(q, small) if kind == "fp8" else eo.extend_fp64(q, small) if block
           else do.attention_fp64(q, small))
    return small, q, ref, lens


def _spread(small, stride, dtype):
    """K and V of ``small`` (layer 0) with sequence b at element ``b * stride`` of an uninitialised buffer."""
    out = []
    for j in range(2):
        buf = torch.empty(2 * stride + 512 * 128, device=DEV, dtype=dtype)
        for b in range(3):
            buf[b * stride: b * stride + 512 * 128].copy_(small.kv[0, j, b, 0].view(dtype).reshape(-1))
        out.append(buf)
    return out


@pytest.mark.parametrize("entry", [("bf16", False), ("bf16", True), ("fp8", False), ("block", False)], ids=_entry_id)
def test_batch_offset_past_4_gib(entry):
    """``stride_b = stride_h`` of 2^30 bf16 elements (2^32 bytes of codes): sequence 2 starts 2^31 elements
    and 2^32 bytes (FP8: 2^33 bytes) into the buffers.  Per row against fp64, and the bits of the same
    rows in a contiguous cache."""
    kind, dev = entry
    esize = 1 if kind == "fp8" else 2
    stride = 1 << (32 if kind == "fp8" else 30)
    _need(2 * (2 * stride + 512 * 128) * esize)
    T = 2 if kind == "block" else 1
    small, q, ref, lens = _big_case(kind, T)
    k, v = _spread(small, stride, torch.uint8 if kind == "fp8" else BF)
    a = types.SimpleNamespace(kind=kind, Hq=1, Hkv=1, B=3, T=T, nsplit=3, k=k, v=v, sb=stride, sh=stride)
    if kind == "fp8":
        a.ks, a.vs, a.ssb, a.ssh = small.kv_scale[0, 0], small.kv_scale[0, 1], 512, 512
    _, a.q = _framed(q)
    a.obuf, a.o = _out(q.shape, BF)
    a.nws = 3 * T * 3 * 130
    a.wsbuf, a.ws = _out((a.nws,), torch.float32)
    _, a.lens = _framed(small.lens_dev)
    chunk = dg.host_geometry(lens, T if kind == "block" else 0, 3)[1]
    assert _attn(a, 512, chunk, dev) == 0
    assert _outputs_framed(a)
    want = _extend(q, small, 0, nsplit=3) if kind == "block" else _decode(q, small, 0, nsplit=3)
    assert torch.equal(a.o, want)
    do.assert_rows_close(a.o.reshape(-1, 128), ref.reshape(-1, 128), 1)
    _record("batch offset 2^32 B " + _entry_id(entry), a.o, ref, 1)
    del k, v, a
    _peak("batch offset " + _entry_id(entry))


@pytest.mark.parametrize("kind", ["bf16", "fp8", "block"])
def test_append_at_a_batch_offset_past_4_gib(kind):
    """The append of sequence 2 lands 4 GiB (FP8: 8 GiB) into the buffers, with the bits of the contiguous call."""
    esize = 1 if kind == "fp8" else 2
    stride = 1 << (32 if kind == "fp8" else 30)
    _need(2 * (2 * stride + 512 * 128) * esize)
    T = 2 if kind == "block" else 1
    pos = [65, 300, 512 - T]
    small, _, _, _ = _big_case("fp8" if kind == "fp8" else "bf16")
    k, v = _spread(small, stride, torch.uint8 if kind == "fp8" else BF)
    a = types.SimpleNamespace(kind=kind, Hq=1, Hkv=1, B=3, T=T, k=k, v=v, sb=stride, sh=stride)
    if kind == "fp8":
        a.ks, a.vs, a.ssb, a.ssh = small.kv_scale[0, 0].clone(), small.kv_scale[0, 1].clone(), 512, 512
    g = torch.Generator().manual_seed(23)
    qkv = torch.randn(3, T, 3 * 128, generator=g).to(BF).to(DEV)
    rc, qbuf, q_out = _append(kind, a, qkv if kind == "block" else qkv[:, 0].contiguous(), pos, 512, 512)
    assert rc == 0
    want = _single_appends(kind, 1, 1, qkv, pos, 512, 512)
    for (b, t), (row, q, kv) in want.items():
        assert torch.equal(_bits(q_out.view(3, T, -1)[b, t]), _bits(q))
        for j, buf in enumerate((k, v)):
            run = _bits(buf[b * stride: b * stride + 512 * 128]).view(512, 128)
            assert torch.equal(run[row], kv[j].view(-1)), (b, t, j)
            # the rows around it are those of before
            for r in (row - 1, row + T):
                if 0 <= r < 512 and not any(w[0] == r for (bb, _), w in want.items() if bb == b):
                    assert torch.equal(run[r], _bits(small.kv[0, j, b, 0, r]))
        if kind == "fp8":
            assert torch.equal(a.ks[b, 0, row], kv[2][0]) and torch.equal(a.vs[b, 0, row], kv[3][0])
    del k, v, a
    _peak("append at batch offset " + kind)


ROWS = 1 << 24  # the FP8 kernel's limit per (sequence, head) run


@pytest.mark.parametrize("kind", ["bf16", "fp8", "block"])
def test_rows_up_to_2_pow_24_of_one_run(kind):
    """One sequence of 2^24 - 3 keys (block: 2^24 - 5 old rows and 2 new), all zero but marked rows at key
    0, 2^23 - 1, 2^23 (byte 2^31 of the bf16 run) and the last: each carries about a quarter of the output,
    so one read from the wrong address is far outside the bounds of the closed form."""
    from tensorhive_fixed_amd.ops.decode_attention import KVCache

    fp8 = kind == "fp8"
    _need(2 * ROWS * (132 if fp8 else 256))
    T = 2 if kind == "block" else 0
    n = ROWS - 3 - T  # old rows
    keys = dg.marked_keys(n, 1 << 23) + [n + t for t in range(T)]
    k, v = dg.marked_rows(len(keys))
    cache = KVCache(do.attn_cfg(1, 1, max_seq_len=ROWS), 1, ROWS, DEV, dtype=FP8 if fp8 else BF)
    idx = torch.tensor(keys, device=DEV)
    if fp8:
        (kc, ks), (vc, vs) = ko.quantize_kv_rows(k), ko.quantize_kv_rows(v)
        for j, (c, s) in enumerate(((kc, ks), (vc, vs))):
            cache.kv.view(torch.uint8)[0, j, 0, 0, idx] = c.view(torch.uint8).to(DEV)
            cache.kv_scale[0, j, 0, 0, idx] = s.to(DEV)
        cache.kv.view(torch.uint8)[0, :, 0, 0, n + T:] = ko.NAN_CODE
        cache.kv_scale[0, :, 0, 0, n + T:] = float("nan")
        km, vm = kc.double() * ks.double()[:, None], vc.double() * vs.double()[:, None]
    else:
        cache.kv[0, 0, 0, 0, idx] = k.to(DEV)
        cache.kv[0, 1, 0, 0, idx] = v.to(DEV)
        cache.kv[0, :, 0, 0, n + T:] = float("nan")
        km, vm = k, v
    cache.set_lens([n])
    if kind == "block":
        q = torch.ones(1, T, 128, device=DEV, dtype=BF)
        o = _extend(q, cache, 0)
        ref = torch.stack([dg.marked_closed_form(km[: 5 + t], vm[: 5 + t], n + t + 1) for t in range(T)])[None]
        eo.assert_block_close(o, ref, 1)
    else:
        q = torch.ones(1, 128, device=DEV, dtype=BF)
        o = _decode(q, cache, 0)
        ref = dg.marked_closed_form(km, vm, n)[None]
        do.assert_rows_close(o, ref, 1)
    _record("2^24 rows " + kind, o, ref, 1)
    del cache
    _peak("2^24 rows " + kind)
