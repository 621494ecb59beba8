"""fp64 oracles and score profiles for the attention kernels' tests (CPU only, plain torch).

``randn`` inputs give log2-domain scores of about N(0, 1.44^2): the running maximum of a row settles
in the first key tile and the forward's deferred rescale (threshold ``DEFER_THR`` log2 units) never
fires again.  The profiles here add a rank-one bias ``a_i * b_j`` to the score of (query i, key j) so
that the maximum moves by chosen amounts at chosen keys.

For one sequence (no batch axis; q, do ``[S, Hq, 128]``, k, v ``[S, Hkv, 128]``, all bf16):

* :func:`exact` -- o, natural-log lse, dq, dk, dv of the bf16 inputs in fp64, closed form;
* :func:`format_baseline` -- the same arithmetic with only the roundings bf16 operands and outputs
  force on any kernel (P and dS to bf16 before their products, delta from bf16(O), outputs to bf16);
* :func:`operand_model` -- the baseline plus the second bf16 rounding of an operand that has
  ``softmax_scale * log2(e)`` folded into it: Q for o, lse and dq; K for dk and dv, which still
  subtract the Q-side lse;
* :func:`late_rescales` -- how often a 32-row block walking 64-key tiles meets a tile whose maximum
  exceeds some row's maximum at its last rescale by more than the threshold.  It qualifies inputs
  from the kernel's documented constants; it is not an emulation of the kernel.
"""
import math

import torch

D = 128
SCALE = 1.0 / math.sqrt(D)
C_LOG2 = math.log2(math.e) * SCALE  # scores in log2 units = C_LOG2 * q.k
LN2 = math.log(2.0)
BLOCK_ROWS, TILE_KEYS, DEFER_THR = 32, 64, 8.0  # fa_fwd_kernel: rows per wave, F_BN, F_DEFER_THR
BF = torch.bfloat16

MOVING = ("ramp_up", "step", "mixed_rows", "rising_spikes")  # the max rises late, by more than the threshold
STILL = ("randn", "ramp_down", "sink")  # the max is settled after the first tile
PROFILES = ("randn", "ramp_up", "ramp_down", "sink", "step", "mixed_rows", "rising_spikes", "large")
KEY_PROFILES = PROFILES[:-1]  # those defined by a bias along the key axis
SPIKE_STEP = 4.0  # 4.5 put the last spike of S = 320 past the +-26 log2 units the profiles stay within
# E_m / E_b is a ratio of two maxima and moves with the draw (plain randn ranges over 1.7-4.3 across
# seeds), so the draws are fixed: the first seed per profile at which every shape of SHAPES, causal and
# full, meets the conditions tests/test_attention_oracles.py asserts.  Nothing here looks at a kernel.
SEEDS = {"randn": 0, "ramp_up": 5, "ramp_down": 0, "sink": 0, "step": 0, "mixed_rows": 0,
         "rising_spikes": 0, "large": 0}
SHAPES = ((1, 256, 4, 1), (2, 320, 2, 2), (1, 200, 4, 2))  # (B, S, Hq, Hkv) of the GPU tests

# Sequence lengths around the kernels' block sizes (tests/gpu/test_flash_tails_gpu.py): one row, below 8,
# a 32-row wave block / 64-key tile / 128-row workgroup / 256-key fused dK|dV block one short and one over,
# an odd count of 64-blocks, 256 + 7.  B = 2 and 4 / 2 heads throughout; batch entry 1 carries the other
# profile of TAIL_PROFILES.
TAIL_LENGTHS = (1, 2, 7, 31, 33, 63, 65, 97, 127, 129, 191, 193, 255, 257, 263)
TAIL_HEADS = (4, 2)
TAIL_PROFILES = ("randn", "ramp_up")
# ramp_up at its seed 5 misses E_m <= 4 E_b for dk / dv at several tail lengths, so the moving profile has a
# seed per length, chosen by the rule of SEEDS: the first seed at which both masks meet the conditions
# tests/test_attention_oracles.py asserts (``python -m tests.attention_oracles`` prints the table).
TAIL_SEEDS = {"randn": dict.fromkeys(TAIL_LENGTHS, 0),
              "ramp_up": {1: 1, 2: 0, 7: 0, 31: 1, 33: 0, 63: 2, 65: 0, 97: 0, 127: 1, 129: 0, 191: 1, 193: 1,
                          255: 4, 257: 0, 263: 1}}
ROPE_THETA = 500000.0

TENSORS = ("o", "dq", "dk", "dv")


def key_bias(profile: str, S: int) -> torch.Tensor:
    """b_j, the log2-domain bias of key j (float64 [S])."""
    j = torch.arange(S, dtype=torch.float64)
    if profile in ("randn", "large"):
        return torch.zeros(S, dtype=torch.float64)
    if profile == "ramp_up":
        return -12 + 24 * j / S
    if profile == "ramp_down":
        return 12 - 24 * j / S
    if profile == "sink":
        b = torch.full((S,), -6.0, dtype=torch.float64)
        b[0] = 8.0
        return b
    if profile in ("step", "mixed_rows"):
        h = 5.0 if profile == "step" else 4.5
        return torch.where(j < S / 2, -h, h).double()
    if profile == "rising_spikes":
        b = torch.full((S,), -6.0, dtype=torch.float64)
        last = torch.arange(TILE_KEYS - 1, S, TILE_KEYS)
        b[last] = -6.0 + SPIKE_STEP * (last // TILE_KEYS + 1).double()
        return b
    raise ValueError(f"unknown profile {profile!r}")


def row_gain(profile: str, S: int) -> torch.Tensor:
    """a_i, the gain of query row i on the key bias (float64 [S])."""
    a = torch.ones(S, dtype=torch.float64)
    if profile == "mixed_rows":
        a[1::2] = 0.8
    return a


def bias_direction() -> torch.Tensor:
    """16 ones at dims 0, 8, ..., 120 (e.e = 16)."""
    e = torch.zeros(D, dtype=torch.float64)
    e[0:D:8] = 1.0
    return e


def profile_inputs(S: int, Hq: int, Hkv: int, profile: str, seed: int, sigma: float = 1.0):
    """bf16 (q, k, v, do): ``randn * sigma`` (q and k; three times that for ``large``) plus the bias."""
    g = torch.Generator().manual_seed(seed)
    sig = sigma * (3.0 if profile == "large" else 1.0)
    q = torch.randn(S, Hq, D, generator=g, dtype=torch.float64) * sig
    k = torch.randn(S, Hkv, D, generator=g, dtype=torch.float64) * sig
    v = torch.randn(S, Hkv, D, generator=g, dtype=torch.float64)
    do = torch.randn(S, Hq, D, generator=g, dtype=torch.float64)
    e = bias_direction()
    q = q + row_gain(profile, S)[:, None, None] * e
    k = k + key_bias(profile, S)[:, None, None] * e / (16 * C_LOG2)
    return q.to(BF), k.to(BF), v.to(BF), do.to(BF)


def _bf(x: torch.Tensor) -> torch.Tensor:
    return x.to(BF).double()


def _same(x: torch.Tensor) -> torch.Tensor:
    return x


def _head_major(q, k, v, do):
    rep = q.shape[1] // k.shape[1]
    Q, dO = q.double().transpose(0, 1), do.double().transpose(0, 1)  # [Hq, S, D]
    K = k.double().transpose(0, 1).repeat_interleave(rep, 0)
    V = v.double().transpose(0, 1).repeat_interleave(rep, 0)
    return Q, K, V, dO, rep


def _mask(s: torch.Tensor, causal: bool) -> torch.Tensor:
    if not causal:
        return s
    S = s.shape[-1]
    return s.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))


def scores_log2(q: torch.Tensor, k: torch.Tensor, causal: bool) -> torch.Tensor:
    """fp64 scores in log2 units, [Hq, S, S], -inf above the diagonal when causal."""
    rep = q.shape[1] // k.shape[1]
    Q = q.double().transpose(0, 1)
    K = k.double().transpose(0, 1).repeat_interleave(rep, 0)
    return _mask(C_LOG2 * (Q @ K.transpose(1, 2)), causal)


def _solve(q, k, v, do, causal, r, s_q=None, s_k=None, grad_map=_same) -> dict:
    """Closed-form attention forward and backward.  ``r`` rounds where the format forces it; ``s_q`` are
    the natural-unit scores behind o, lse and dq, ``s_k`` those behind the P of dk and dv.  ``grad_map``
    acts on the head-major ``[H, S, D]`` dq and dk in fp64 before their output rounding (the rotary
    backward a kernel folds into its epilogue rounds once, after the rotation)."""
    Q, K, V, dO, rep = _head_major(q, k, v, do)
    Hq, S, _ = Q.shape
    s = _mask(SCALE * (Q @ K.transpose(1, 2)), causal) if s_q is None else _mask(s_q, causal)
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    o = r(r(P) @ V)
    delta = (dO * o).sum(-1, keepdim=True)
    dP = dO @ V.transpose(1, 2)
    dq = r(grad_map(SCALE * (r(P * (dP - delta)) @ K)))
    Pk = P if s_k is None else torch.exp(_mask(s_k, causal) - lse[..., None])
    dSk = Pk * (dP - delta)
    group = lambda x: x.view(Hq // rep, rep, S, D).sum(1)  # noqa: E731
    dk = r(grad_map(SCALE * group(r(dSk).transpose(1, 2) @ Q)))
    dv = r(group(r(Pk).transpose(1, 2) @ dO))
    t = lambda x: x.transpose(0, 1).contiguous()  # noqa: E731
    return {"o": t(o), "lse": lse, "dq": t(dq), "dk": t(dk), "dv": t(dv), "rowsum_k": Pk.sum(-1)}


def exact(q, k, v, do, causal: bool, grad_map=_same) -> dict:
    """o [S,Hq,D], lse [Hq,S] (natural log), dq, dk [S,Hkv,D], dv of the bf16 inputs, fp64 throughout."""
    return _solve(q, k, v, do, causal, _same, grad_map=grad_map)


def format_baseline(q, k, v, do, causal: bool, grad_map=_same) -> dict:
    return _solve(q, k, v, do, causal, _bf, grad_map=grad_map)


def rope_backward(S: int, theta: float = ROPE_THETA):
    """The rotary backward as a ``grad_map``: rotate-half pairs (i, i + D/2) of row ``pos`` turned by
    ``-pos * theta^(-2i/D)`` in fp64, the angles of ``tests/kernel_oracles.rope_oracle``."""
    i = torch.arange(D // 2, dtype=torch.float64)
    inv = torch.pow(torch.tensor(theta, dtype=torch.float64), -2.0 * i / D)
    ang = torch.arange(S, dtype=torch.float64)[:, None] * inv
    c, s = ang.cos(), -ang.sin()

    def turn(x: torch.Tensor) -> torch.Tensor:  # [H, S, D]
        a, b = x[..., :D // 2], x[..., D // 2:]
        return torch.cat([a * c - b * s, b * c + a * s], -1)

    return turn


def single_row_bounds(q, k, v, do) -> tuple[torch.Tensor, torch.Tensor]:
    """S = 1: P = 1 and dP = delta exactly, so dq = dk = 0 and any kernel output is the f32 cancellation
    of ``dP - delta``, two sums of 128 products each: ``|dS| <= 2 * 128 * 2^-24 * sum_d |dO_d v_d|`` per q
    head.  -> bounds on |dq| [1, Hq, D] (``|dS| * scale * |k_d|``) and |dk| [1, Hkv, D]
    (``scale * sum over the group's heads of |dS| * |q_d|``), each times ``1 + 2^-8`` for the output's
    bf16 rounding."""
    Q, K, V, dO, rep = _head_major(q, k, v, do)  # [Hq, 1, D]
    ds = 2 * D * 2.0 ** -24 * (dO * V).abs().sum(-1, keepdim=True)  # [Hq, 1, 1]
    out = 1 + 2.0 ** -8
    dq = ds * SCALE * K.abs() * out
    dk = SCALE * (ds * Q.abs()).view(Q.shape[0] // rep, rep, 1, D).sum(1) * out
    return dq.transpose(0, 1), dk.transpose(0, 1)


def operand_scores(q, k):
    """Natural-unit scores from bf16(q*c).k (Q side) and q.bf16(k*c) (K side), c = scale * log2(e).
    The operand is scaled as f32 operands are, by an f32 product of the f32 constants, then rounded."""
    Q, K, _, _, _ = _head_major(q, k, k, q)
    c = torch.tensor(SCALE, dtype=torch.float32) * torch.tensor(math.log2(math.e), dtype=torch.float32)
    s_q = LN2 * ((Q.float() * c).to(BF).double() @ K.transpose(1, 2))
    s_k = LN2 * (Q @ (K.float() * c).to(BF).double().transpose(1, 2))
    return s_q, s_k


def operand_model(q, k, v, do, causal: bool) -> dict:
    s_q, s_k = operand_scores(q, k)
    return _solve(q, k, v, do, causal, _bf, s_q, s_k)


def max_abs_errors(got: dict, ref: dict) -> dict:
    return {n: (got[n] - ref[n]).abs().max().item() for n in TENSORS + ("lse",)}


def late_rescales(scores: torch.Tensor, causal: bool) -> tuple[int, int]:
    """(fired, visits) over the tile visits after tile 0 of one head's log2-unit scores ``[S, S]``.

    A block of ``BLOCK_ROWS`` query rows walks the ``TILE_KEYS``-wide key tiles (causal: up to the
    tile holding its last row's diagonal).  Every row remembers its maximum at the block's last
    rescale; a visit fires when some row's tile maximum exceeds that by more than ``DEFER_THR``, and
    then every row of the block takes its running maximum."""
    S, Sk = scores.shape
    s = _mask(scores.double(), causal)
    fired = visits = 0
    for r0 in range(0, S, BLOCK_ROWS):
        rows = s[r0:r0 + BLOCK_ROWS]
        last = (min(r0 + BLOCK_ROWS, S) - 1) // TILE_KEYS if causal else (Sk - 1) // TILE_KEYS
        m = rows[:, :TILE_KEYS].max(-1).values
        for t in range(1, last + 1):
            mt = rows[:, t * TILE_KEYS:(t + 1) * TILE_KEYS].max(-1).values
            visits += 1
            if bool((mt - m > DEFER_THR).any()):
                fired += 1
                m = torch.maximum(m, mt)
    return fired, visits


def block_max_abs(got: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """max |got - ref| per (32-row block, head) of ``[S, H, D]`` tensors -> float64 [ceil(S/32), H]."""
    S, H, _ = ref.shape
    err = (got.double() - ref).abs().amax(-1)  # [S, H]
    pad = (-S) % BLOCK_ROWS
    if pad:
        err = torch.cat([err, torch.zeros(pad, H, dtype=err.dtype)])
    return err.view(-1, BLOCK_ROWS, H).amax(1)


def lse_tolerance_plain(s_log2: torch.Tensor) -> torch.Tensor:
    """``2e-3 + 2**-9 * |score|_max`` per row, the score in the units of lse (natural), [Hq, S]."""
    smax = (s_log2 * LN2).masked_fill(~torch.isfinite(s_log2), 0.0).abs().amax(-1)
    return 2e-3 + 2.0 ** -9 * smax


def lse_tolerance(exact_lse: torch.Tensor, model_lse: torch.Tensor, s_log2: torch.Tensor) -> torch.Tensor:
    """Per-row bound on |lse - lse_exact| (natural log), [Hq, S].

    ``2e-3 + 2**-9 * |score|_max`` of the row (natural units) allows for the scaled operand's rounding
    when one sign dominates the terms of q.k.  It is no bound when they cancel: the rounding moves a
    score by up to ``2**-9 * scale * sum_d |q_d k_d|`` however small the score itself is, and a causal
    row that sees a handful of keys has an lse error of just that.  The operand model -- fp64
    arithmetic on the inputs, no kernel -- alone exceeds the first form on such rows (CPU-tested), so
    the second term is at least the model's own error on that row."""
    return torch.maximum(lse_tolerance_plain(s_log2), 2e-3 + (model_lse - exact_lse).abs())


_CASES: dict = {}


def case(S: int, Hq: int, Hkv: int, profile: str, causal: bool, seed: int | None = None) -> dict:
    """Inputs and every fp64 result of one (shape, profile, mask), computed once and shared: ``q k v do``,
    ``exact``, ``E_b``, ``E_m`` (max-abs per tensor), ``lse_tol`` and
    ``lse_tol_plain`` [Hq, S], ``s_log2`` and the K-side
    natural-unit scores ``s_k``.  ``seed`` defaults to the profile's of ``SEEDS``."""
    seed = SEEDS[profile] if seed is None else seed
    key = (S, Hq, Hkv, profile, causal, seed)
    if key not in _CASES:
        q, k, v, do = profile_inputs(S, Hq, Hkv, profile, seed)
        ex = exact(q, k, v, do, causal)
        model = operand_model(q, k, v, do, causal)
        s2 = scores_log2(q, k, causal)
        _CASES[key] = {
            "q": q, "k": k, "v": v, "do": do, "exact": ex, "s_log2": s2,
            "E_b": max_abs_errors(format_baseline(q, k, v, do, causal), ex),
            "E_m": max_abs_errors(model, ex),
            "model_lse": model["lse"], "model_rowsum_k": model["rowsum_k"],
            "lse_tol": lse_tolerance(ex["lse"], model["lse"], s2), "lse_tol_plain": lse_tolerance_plain(s2),
            "s_k": _mask(operand_scores(q, k)[1], causal),
        }
    return _CASES[key]


def tail_case(S: int, profile: str, causal: bool) -> dict:
    """The :func:`case` of one tail length: ``TAIL_HEADS`` heads, the seed of ``TAIL_SEEDS``."""
    return case(S, *TAIL_HEADS, profile, causal, TAIL_SEEDS[profile][S])


_ROPE_CASES: dict = {}


def tail_rope_case(S: int, profile: str, causal: bool) -> dict:
    """:func:`tail_case` with the rotary backward folded into dq and dk: ``exact`` and the format
    baseline's ``E_b`` with the rotation applied in fp64 before the one output rounding."""
    key = (S, profile, causal)
    if key not in _ROPE_CASES:
        c = tail_case(S, profile, causal)
        args = (c["q"], c["k"], c["v"], c["do"], causal)
        ex = exact(*args, grad_map=rope_backward(S))
        _ROPE_CASES[key] = {"exact": ex, "E_b": max_abs_errors(format_baseline(*args, grad_map=rope_backward(S)), ex)}
    return _ROPE_CASES[key]


def ramp_must_rescale(S: int) -> bool:
    """ramp_up rises by ``24 (S - 64) / S`` log2 units from the last key of tile 0 to the last key.  Only a
    rise beyond ``DEFER_THR`` can fire the deferred rescale after tile 0: of ``TAIL_LENGTHS`` that leaves
    out S <= 64 (one tile) and S = 65, whose second tile holds one key 0.4 units up."""
    return 24.0 * (S - TILE_KEYS) / S > DEFER_THR


def tail_misses(c: dict, S: int, profile: str, causal: bool) -> list[str]:
    """What keeps the case ``c`` of a tail length from qualifying for the GPU margin (empty: it qualifies):
    scores within +-26 log2 units, a positive format baseline, the operand model within 4 x of it, and
    for the moving profile at least one late rescale per head where the ramp allows one.  S = 1 has one
    probability, 1: o, dq and dk have no format error at all and dq, dk are 0."""
    bad = []
    peak = c["s_log2"][torch.isfinite(c["s_log2"])].abs().max().item()
    if peak > 26:
        bad.append(f"max |score| {peak:.1f} log2 units")
    if c["E_b"]["lse"] != 0.0:
        bad.append("the format baseline moved lse")
    exact_zero = ("o", "dq", "dk") if S == 1 else ()
    for n in TENSORS:
        if n in exact_zero:
            if c["E_b"][n] != 0.0 or (n != "o" and c["exact"][n].abs().max().item() > 1e-18):
                bad.append(f"{n}: S = 1 should be exact")
        elif not c["E_b"][n] > 0:
            bad.append(f"{n}: E_b = 0")
        elif c["E_m"][n] > 4 * c["E_b"][n]:
            bad.append(f"{n}: operand rounding alone is {c['E_m'][n] / c['E_b'][n]:.2f} x the format baseline")
    if profile in MOVING and ramp_must_rescale(S):
        for h in range(c["s_log2"].shape[0]):
            fired, visits = late_rescales(c["s_log2"][h], causal)
            if visits and not fired:
                bad.append(f"head {h}: no late rescale in {visits} visits")
    return bad


def first_tail_seed(S: int, profile: str, limit: int = 64) -> int:
    """The rule behind ``TAIL_SEEDS``: the first seed at which both masks qualify."""
    for seed in range(limit):
        if not any(tail_misses(case(S, *TAIL_HEADS, profile, causal, seed), S, profile, causal)
                   for causal in (True, False)):
            return seed
    raise ValueError(f"no seed below {limit} qualifies {profile} at S = {S}")


if __name__ == "__main__":
    for name in TAIL_PROFILES:
        print(name, {S: first_tail_seed(S, name) for S in TAIL_LENGTHS})
