"""fp64 oracles of the streaming kernels and the one tolerance rule their tests share.

Every oracle takes the tensors the kernel takes (bf16 or f32), upcasts them to float64 and evaluates
the operation straight from its mathematics -- nothing here calls ``tensorhive_fixed_amd.ops`` or its
RoPE tables.  Each returns ``(ref, mag)`` per output (a dict ``name -> (ref, mag)`` where the op has
several): ``ref`` is the exact value, ``mag`` the sum of the absolute values of the terms that are
added or subtracted to form the element, i.e. the scale its fp32 rounding errors are relative to.

The kernels compute in fp32 and round once, so ``assert_rounded_close`` allows, per element and with
no element excepted,

    bf16 outputs:  |got - ref| <= 2^-8 |ref| + 2^-16 mag + 2^-126
    f32 outputs:   |got - ref| <= 2^-20 mag + 2^-126

2^-8 |ref| is the round-to-nearest-even half-ulp of bf16 (8 significant bits); 2^-16 mag is 256 fp32
ulps of the summed magnitudes (serial-plus-tree reductions of at most ~130 terms per lane, and
``__expf`` / ``__logf`` at |argument| <= 88, whose argument reduction costs |argument| ulps);
2^-126 is the flush-to-zero floor.  f32 outputs get 16 fp32 ulps of ``mag``.
"""
from __future__ import annotations

import struct

import torch

BF16_HALF_ULP = 2.0 ** -8     # never widened
BF16_FP32_TERM = 2.0 ** -16   # 256 fp32 ulps of mag
F32_FP32_TERM = 2.0 ** -20    # 16 fp32 ulps of mag
FLUSH_FLOOR = 2.0 ** -126

# name -> worst err/bound seen by assert_rounded_close in this process (printed by the GPU file)
WORST: dict[str, float] = {}


def f32(v: float) -> float:
    """``v`` rounded to binary32, as a ``float`` argument of the C ABI arrives in the kernel."""
    return struct.unpack("f", struct.pack("f", float(v)))[0]


def assert_rounded_close(got: torch.Tensor, ref: torch.Tensor, mag: torch.Tensor, name: str,
                         fp32_term: float | None = None) -> float:
    """Element-wise rounding bound (module docstring); returns the worst ``err / bound``.

    ``fp32_term`` replaces the default coefficient of ``mag`` for one output whose kernel arithmetic
    provably needs more; the derivation belongs next to the call."""
    if got.dtype == torch.bfloat16:
        half_ulp, term = BF16_HALF_ULP, BF16_FP32_TERM
    elif got.dtype == torch.float32:
        half_ulp, term = 0.0, F32_FP32_TERM
    else:
        raise TypeError(f"{name}: unexpected output dtype {got.dtype}")
    if fp32_term is not None:
        term = fp32_term
    ref = ref.to(torch.float64)
    mag = mag.to(torch.float64).expand_as(ref)
    assert tuple(got.shape) == tuple(ref.shape), f"{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    g = got.detach().to(device=ref.device, dtype=torch.float64)
    err = (g - ref).abs()
    bound = half_ulp * ref.abs() + term * mag + FLUSH_FLOOR
    ratio = err / bound
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))  # NaN / inf output
    worst = float(ratio.max()) if ratio.numel() else 0.0
    WORST[name] = max(WORST.get(name, 0.0), worst)
    bad = ratio > 1.0
    nbad = int(bad.sum())
    if nbad:
        flat = int(ratio.reshape(-1).argmax())
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ref.shape)) if ref.dim() else ()
        raise AssertionError(
            f"{name}: {nbad} of {ref.numel()} elements outside the rounding bound; worst at {idx}: "
            f"got {g.reshape(-1)[flat].item()!r} ref {ref.reshape(-1)[flat].item()!r} err/bound {worst:.3f}")
    return worst


# ----------------------------------------------------------------------------------------- RMSNorm
def rmsnorm_fwd_oracle(x: torch.Tensor, w: torch.Tensor, eps: float, addend: torch.Tensor | None = None):
    """y = x * rstd * w with rstd = (mean(x^2) + eps)^-1/2.  With ``addend`` the normalised row is
    xsum = bf16(x + addend) -- exactly defined: an fp32 (or fp64) sum of two bf16 values rounded to
    bf16 is the correctly rounded sum, 24 >= 2 * 8 + 2 significant bits make the double rounding
    innocuous."""
    out = {}
    xd = x.double()
    if addend is not None:
        xs = (xd + addend.double()).to(torch.bfloat16)
        out["xsum"] = (xs.double(), xs.double().abs())
        xd = xs.double()
    ms = xd.pow(2).mean(-1)
    rstd = (ms + f32(eps)).rsqrt()
    y = xd * rstd[:, None] * w.double()
    out["rstd"] = (rstd, rstd)  # a sum of non-negative terms: no cancellation
    out["y"] = (y, y.abs())
    return out


def rmsnorm_bwd_oracle(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor, eps: float,
                       dres: torch.Tensor | None = None, dw_prev: torch.Tensor | None = None):
    """dx = r g w - x (sum_j g w x) r^3 / D (+ dres);  dw = sum_t g x r (+ previous value)."""
    xd, gd, wd = x.double(), dy.double(), w.double()
    D = xd.shape[-1]
    r = (xd.pow(2).mean(-1, keepdim=True) + f32(eps)).rsqrt()
    gwx = gd * wd * xd
    c = r.pow(3) / D
    dx = r * gd * wd - xd * gwx.sum(-1, keepdim=True) * c
    mdx = (r * gd * wd).abs() + xd.abs() * gwx.abs().sum(-1, keepdim=True) * c
    if dres is not None:
        dx = dx + dres.double()
        mdx = mdx + dres.double().abs()
    gxr = gd * xd * r
    dw, mdw = gxr.sum(0), gxr.abs().sum(0)
    if dw_prev is not None:
        dw = dw + dw_prev.double()
        mdw = mdw + dw_prev.double().abs()
    return {"dx": (dx, mdx), "dw": (dw, mdw)}


# ------------------------------------------------------------------------------------------ SwiGLU
def swiglu_fwd_oracle(gu: torch.Tensor):
    g, u = gu.double().chunk(2, dim=-1)
    out = g * torch.sigmoid(g) * u
    return out, out.abs()


def swiglu_bwd_oracle(dout: torch.Tensor, gu: torch.Tensor):
    """dg = d u s (1 + g (1 - s)), du = d g s, packed [dg | du]; 1 - s is evaluated as sigmoid(-g)."""
    g, u = gu.double().chunk(2, dim=-1)
    d = dout.double()
    s, s1 = torch.sigmoid(g), torch.sigmoid(-g)
    dus = d * u * s
    dg = dus * (1 + g * s1)
    mdg = dus.abs() * (1 + g.abs() * s1)
    du = d * g * s
    return torch.cat([dg, du], -1), torch.cat([mdg, du.abs()], -1)


# -------------------------------------------------------------------------------------------- RoPE
def rope_oracle(qkv: torch.Tensor, S: int, n_rot_heads: int, Dh: int, theta: float, sign: float):
    """Rotate-half pairs (i, i + Dh/2) of the first ``n_rot_heads`` heads of every row by the angle
    ``pos * theta^(-2i/Dh)`` (times ``sign``), pos = row % S; the remaining columns pass through."""
    T, row = qkv.shape
    half = Dh // 2
    xd = qkv.double()
    pos = (torch.arange(T, device=qkv.device) % S).double()
    i = torch.arange(half, device=qkv.device, dtype=torch.float64)
    ang = pos[:, None] * torch.pow(torch.tensor(float(theta), dtype=torch.float64, device=qkv.device), -2.0 * i / Dh)
    c, s = ang.cos()[:, None, :], ang.sin()[:, None, :] * float(sign)
    rot = xd[:, : n_rot_heads * Dh].reshape(T, n_rot_heads, Dh)
    a, b = rot[..., :half], rot[..., half:]
    y = torch.cat([a * c - b * s, b * c + a * s], -1).reshape(T, n_rot_heads * Dh)
    m = torch.cat([(a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()], -1).reshape(T, n_rot_heads * Dh)
    ref, mag = xd.clone(), xd.abs()
    ref[:, : n_rot_heads * Dh] = y
    mag[:, : n_rot_heads * Dh] = m
    return ref, mag


# ----------------------------------------------------------------------------------- cross-entropy
def ce_oracle(logits: torch.Tensor, target: torch.Tensor, grad_scale: float, ignore_index: int = -100):
    """Per row: lse = log sum exp x, loss = lse - x[tgt], dlogits = (softmax - onehot) * grad_scale.
    A target equal to ``ignore_index``, negative, or >= V makes the row invalid: loss 0 and an all-zero
    gradient row (``lse`` is still the row's)."""
    x = logits.double()
    R, V = x.shape
    mx = x.max(-1).values
    lse = torch.logsumexp(x, -1)
    mlse = mx.abs() + (lse - mx).abs()
    valid = (target != ignore_index) & (target >= 0) & (target < V)
    t = torch.where(valid, target, torch.zeros_like(target))
    xt = x.gather(1, t[:, None])[:, 0]
    zero = torch.zeros_like(lse)
    loss = torch.where(valid, lse - xt, zero)
    mloss = torch.where(valid, mlse + xt.abs(), zero)
    p = (x - lse[:, None]).exp()
    onehot = torch.zeros_like(p)
    onehot[torch.arange(R, device=x.device), t] = 1.0
    gs = torch.where(valid, torch.full_like(lse, f32(grad_scale)), zero)[:, None]
    return {"loss": (loss, mloss), "lse": (lse, mlse), "dlogits": ((p - onehot) * gs, (p + onehot) * gs.abs())}


# ------------------------------------------------------------------------------------------- AdamW
def sumsq_oracle(g: torch.Tensor, prev: torch.Tensor | None = None):
    s = g.double().pow(2).sum().reshape(1)
    if prev is None:
        return s, s
    return s + prev.double().reshape(1), s + prev.double().abs().reshape(1)


def adamw_oracle(master: torch.Tensor, m: torch.Tensor, v: torch.Tensor, g: torch.Tensor, *, lr: float,
                 beta1: float, beta2: float, eps: float, weight_decay: float, step: int, grad_scale: float = 1.0,
                 norm_sq: torch.Tensor | None = None, clip: float = 0.0):
    """One decoupled-weight-decay Adam step on the *input* state.  Hyperparameters are rounded to f32
    first, as the C ABI receives them; the bias corrections are 1 - b^step of those.

    ``mag`` of ``master`` counts every term that is summed on the way: the decayed weight plus the two
    terms of the new first moment, each scaled by step_size / denominator (the second moment is a sum
    of non-negative terms and adds no cancellation)."""
    lr, b1, b2, eps, wd, gs, clip = (f32(a) for a in (lr, beta1, beta2, eps, weight_decay, grad_scale, clip))
    scale = gs
    if norm_sq is not None and clip > 0:
        tn = float(norm_sq.double().reshape(-1)[0].sqrt()) * gs
        scale *= min(1.0, clip / (tn + f32(1e-6)))
    gr = g.double() * scale
    m_a, m_b = b1 * m.double(), (1 - b1) * gr
    m2 = m_a + m_b
    mm = m_a.abs() + m_b.abs()
    v2 = b2 * v.double() + (1 - b2) * gr * gr
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    k = (lr / bc1) / (v2.sqrt() / bc2 ** 0.5 + eps)
    decayed = master.double() * (1 - lr * wd)
    new = decayed - k * m2
    mnew = decayed.abs() + k * mm
    return {"master": (new, mnew), "m": (m2, mm), "v": (v2, v2), "p": (new, mnew)}


# --------------------------------------------------------------------------------------- embedding
def embedding_bwd_oracle(ids: torch.Tensor, dy: torch.Tensor, V: int, prev: torch.Tensor | None = None):
    """gw[id] = sum of the dy rows whose token is id (+ the previous row when accumulating)."""
    D = dy.shape[-1]
    ref = torch.zeros(V, D, dtype=torch.float64, device=dy.device)
    mag = torch.zeros_like(ref)
    ref.index_add_(0, ids, dy.double())
    mag.index_add_(0, ids, dy.double().abs())
    if prev is not None:
        ref += prev.double()
        mag += prev.double().abs()
    return ref, mag
