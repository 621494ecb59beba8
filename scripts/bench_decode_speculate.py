#!/usr/bin/env python
"""Block decode steps and speculative greedy generation (csrc/extend_attn.hip, ``Llama.extend_step``,
``Llama.generate(speculate=k)``) against the single-token path they build on.

    python scripts/bench_decode_speculate.py [--parts attn,step,e2e,agree] [--kv-lens 4096,8192] [--batches 1,2,8]
                                             [--runs 5] [--iters 1000] [--out FILE]

The method is that of ``scripts/bench_decode_kv_fp8.py``.  The parent process never touches the GPU: every
shape is a child process under its own time limit, started one after another, and the first child that
fails ends the script.  In a child the arms alternate (``--runs`` windows each, device events around the
calls of a window).  One JSON line per measurement:

* ``attn``: 32/8 heads, ``kv_len`` keys in all, for T in 1, 2, 4, 8: one ``extend_attention`` call (``block``)
  against one ``decode_attention`` call (``single``) and against T of them (``singles``, all a build without
  the block kernel can do for T tokens).  The calls rotate over cache layers so that no call finds its K/V in
  the last-level cache.  ``beats_singles``: the block mean is below the singles mean by more than the larger
  spread; ``ratio_to_single`` has 1.0 as its floor (equal K/V bytes).
* ``step``: Llama-3-8B shapes, random weights, 512 rows in the cache: ms per ``extend_step`` for every T with
  ``B * T <= 16`` against ``decode_step`` at the same B, on the weight-streaming and on the FP8 linears;
  ``break_even_tokens`` is ``t_extend(T) / t_decode``, the mean tokens a step must emit to pay for itself.
* ``e2e``: ``generate`` as ``llama3_generate --speculate 4 --fp8-weights`` runs it, 512-token prompts, 128 new
  tokens: the plain run, the oracle drafter (upper bound), the always-wrong drafter (the overhead, host sync
  and drafting included), and prompt lookup on a prompt that repeats a 64-token pattern against the plain run
  on that prompt; tokens/s over the decode part and the spread over ``--e2e-runs`` runs.  The weights are the
  random init with ``wo`` and ``w2`` zeroed and ``lm_head`` set to ``tok_emb``, a model that repeats its last
  token with a wide logit gap: a drafter can only be right about a model whose greedy choice survives the last
  bits in which a block step and single steps differ, which a plain random init's does not (``agree``).  Every
  arm runs the same weights, and no kernel's work depends on their values.
* ``agree``: the plain random init, 512 random cache rows, B 2: the logits of one ``extend_step`` of 5 tokens
  against 5 ``decode_step`` calls, with the top-2 gaps of the latter and, as the yardstick, how far the single
  steps on hipBLASLt and on the weight-streaming kernel are apart.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
BLOCKS = (1, 2, 4, 8)


def _stats(xs: list[float], nd: int = 2) -> dict:
    return {"mean": round(sum(xs) / len(xs), nd), "spread": round(max(xs) - min(xs), nd),
            "windows": [round(x, nd) for x in xs]}


def child_attn(args) -> int:
    import torch

    from tensorhive_fixed_amd.models.llama3 import LlamaConfig
    from tensorhive_fixed_amd.ops.decode_attention import KVCache, decode_attention
    from tensorhive_fixed_amd.ops.extend_attention import extend_attention

    dev = torch.device("cuda")
    Hq, Hkv, B, n = 32, 8, args.child_batch, args.child_kv_len
    per_layer = 2 * B * Hkv * n * 256
    L = max(8, min(64, -(-(1 << 30) // per_layer)))  # at least 1 GiB of K/V under the rotation
    cfg = LlamaConfig(dim=Hq * 128, n_layers=L, n_heads=Hq, n_kv_heads=Hkv, max_seq_len=n)
    cache = KVCache(cfg, B, n, dev)
    cache.kv.normal_()

    def window(fn, iters) -> float:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(iters):
            fn(i)
        b.record()
        b.synchronize()
        return 1000.0 * a.elapsed_time(b) / iters  # us per call of fn

    q1 = torch.randn(B, Hq * 128, device=dev, dtype=torch.bfloat16)
    for T in BLOCKS:
        qT = torch.randn(B, T, Hq * 128, device=dev, dtype=torch.bfloat16)
        blk_lens, one_lens = [n - T] * B, [n - 1] * B

        def singles(i, T=T):
            for t in range(T):
                decode_attention(q1, cache, (i * T + t) % L, new=1)

        arms = {"block": (blk_lens, lambda i: extend_attention(qT, cache, i % L)),
                "single": (one_lens, lambda i: decode_attention(q1, cache, i % L, new=1)),
                "singles": (one_lens, singles)}
        t = {k: [] for k in arms}
        for r in range(args.runs + 1):  # window 0 warms up
            for k, (lens, fn) in arms.items():
                cache.set_lens(lens)
                torch.cuda.synchronize()
                x = window(fn, args.iters if r else 2 * L)
                if r:
                    t[k].append(x)
        res = {"bench": "attn", "kv_len": n, "batch": B, "heads": [Hq, Hkv], "T": T, "layers_rotated": L,
               "runs": args.runs, "iters": args.iters, **{k + "_us": _stats(v) for k, v in t.items()}}
        gain = res["singles_us"]["mean"] - res["block_us"]["mean"]
        bar = max(res["singles_us"]["spread"], res["block_us"]["spread"])
        res.update({"ratio_to_single": round(res["block_us"]["mean"] / res["single_us"]["mean"], 3),
                    "ratio_to_singles": round(res["block_us"]["mean"] / res["singles_us"]["mean"], 3),
                    "beats_singles": gain > bar})
        print(json.dumps(res), flush=True)
    return 0


def _model(dev, copy_model: bool = False):
    """Llama-3-8B shapes, random init.  ``copy_model``: ``wo`` and ``w2`` zeroed and ``lm_head`` set to ``tok_emb``,
    so the residual stream is the embedding and greedy decoding repeats the last token with a wide logit gap."""
    import torch

    from tensorhive_fixed_amd.models.llama3 import Llama, LlamaConfig

    model = Llama(LlamaConfig.named("llama3-8b"), device=dev, dtype=torch.bfloat16, seed=0)
    if copy_model:
        with torch.no_grad():
            model.lm_head.copy_(model.tok_emb)
            for blk in model.layers:
                blk.wo.zero_()
                blk.w2.zero_()
    model.quantize_decode_weights()
    return model


def child_step(args) -> int:
    import time

    import torch

    from tensorhive_fixed_amd.ops.decode_attention import KVCache

    dev = torch.device("cuda")
    B, rows, iters = args.child_batch, 512, args.step_iters
    model = _model(dev)
    cache = KVCache(model.cfg, B, rows + iters * max(BLOCKS), dev)
    cache.kv.normal_(0, 0.5)
    tok = torch.randint(0, model.cfg.vocab_size, (B, max(BLOCKS)), device=dev)

    def window(fn) -> float:
        cache.set_lens([rows] * B)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return 1000.0 * (time.perf_counter() - t0) / iters  # ms per step, launch overhead included

    for mode, kw in (("stream_gemm", {"stream_gemm": True}), ("fp8", {"fp8": True})):
        arms = {"decode": lambda: model.decode_step(tok[:, 0].contiguous(), cache, **kw)}
        for T in BLOCKS:
            if B * T <= 16:
                arms[f"extend_T{T}"] = lambda T=T: model.extend_step(tok[:, :T].contiguous(), cache, **kw)
        t = {k: [] for k in arms}
        for r in range(args.runs + 1):  # window 0 warms up
            for k, fn in arms.items():
                x = window(fn)
                if r:
                    t[k].append(x)
        base = sum(t["decode"]) / len(t["decode"])
        for k, v in t.items():
            print(json.dumps({"bench": "step", "model": "llama3-8b", "batch": B, "cache_rows": rows, "mode": mode,
                              "arm": k, "runs": args.runs, "iters": iters, "ms": _stats(v, 3),
                              "break_even_tokens": round(sum(v) / len(v) / base, 3)}), flush=True)
    return 0


def child_agree(args) -> int:
    import torch

    from tensorhive_fixed_amd.ops.decode_attention import KVCache

    dev = torch.device("cuda")
    B, rows, T = args.child_batch, 512, 5
    model = _model(dev)
    caches = [KVCache(model.cfg, B, rows + T, dev) for _ in range(2)]
    caches[0].kv.normal_(0, 0.5)
    caches[1].kv.copy_(caches[0].kv)
    tok = torch.randint(0, model.cfg.vocab_size, (B, T), device=dev)

    def singles(**kw):
        caches[1].set_lens([rows] * B)
        return torch.stack([model.decode_step(tok[:, t].contiguous(), caches[1], **kw) for t in range(T)], dim=1)

    # the yardstick: two single-step paths that differ only in who runs the GEMMs
    base = (singles() - singles(stream_gemm=True)).abs().max().item()
    for mode, kw in (("default", {}), ("stream_gemm", {"stream_gemm": True}), ("fp8", {"fp8": True})):
        caches[0].set_lens([rows] * B)
        blk = model.extend_step(tok, caches[0], **kw)
        one = singles(**kw)
        top = one.topk(2, dim=-1).values
        gap = (top[..., 0] - top[..., 1]).flatten()
        print(json.dumps({"bench": "agree", "model": "llama3-8b", "batch": B, "cache_rows": rows, "T": T, "mode": mode,
                          "max_abs_logit": round(one.abs().max().item(), 4),
                          "max_abs_diff": round((blk - one).abs().max().item(), 5),
                          "single_default_vs_single_stream_max_abs_diff": round(base, 5),
                          "argmax_equal_rows": int((blk.argmax(-1) == one.argmax(-1)).sum()), "rows": B * T,
                          "top2_gap_min": round(gap.min().item(), 5),
                          "top2_gap_median": round(gap.median().item(), 5)}), flush=True)
    return 0


def child_e2e(args) -> int:
    import time

    import torch

    from tensorhive_fixed_amd.workloads.llama3_generate import _reference_drafter

    dev = torch.device("cuda")
    B, S, new, k = args.child_batch, 512, 128, 4
    model = _model(dev, copy_model=True)
    vocab = model.cfg.vocab_size
    g = torch.Generator(device=dev).manual_seed(0)
    rand = torch.randint(0, vocab, (B, S), device=dev, generator=g)
    rep = torch.randint(0, vocab, (B, 64), device=dev, generator=g).repeat(1, S // 64)
    kw = {"max_new_tokens": new, "fp8": True, "stream_gemm": True}
    lens = [S] * B

    def timed(tokens, **extra) -> tuple[float, dict]:
        marks, stats = {}, {}

        def on_step(i):
            if i == 0:
                torch.cuda.synchronize()
                marks["prefill"] = time.perf_counter()

        if "speculate" in extra:
            extra["spec_stats"] = stats
        model.generate(tokens, lens, on_step=on_step, **kw, **extra)
        torch.cuda.synchronize()
        return B * (new - 1) / (time.perf_counter() - marks["prefill"]), stats

    ids = model.generate(rand, lens, **kw).tolist()
    arms = {"plain": (rand, {}),
            "oracle": (rand, {"speculate": k, "draft_fn": _reference_drafter(ids, lens, vocab, True)}),
            "wrong": (rand, {"speculate": k, "draft_fn": _reference_drafter(ids, lens, vocab, False)}),
            "plain_repeat": (rep, {}),
            "lookup_repeat": (rep, {"speculate": k})}
    t = {a: [] for a in arms}
    steps = {}
    for r in range(args.e2e_runs + 1):  # run 0 warms up
        for a, (tokens, extra) in arms.items():
            tps, stats = timed(tokens, **dict(extra))
            if r:
                t[a].append(tps)
                steps[a] = stats.get("steps")
    for a, v in t.items():
        base = t["plain_repeat" if a.endswith("repeat") else "plain"]
        print(json.dumps({"bench": "e2e", "model": "llama3-8b", "batch": B, "prompt": S, "new_tokens": new,
                          "flags": "--fp8-weights --stream-gemm", "speculate": 0 if a.startswith("plain") else k,
                          "arm": a, "runs": args.e2e_runs, "tokens_per_s": _stats(v, 1), "steps": steps[a],
                          "tokens_per_step": steps[a] and round((new - 1) / steps[a], 3),
                          "speedup": round(sum(v) / sum(base), 3)}), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parts", default="attn,step,e2e,agree")
    ap.add_argument("--kv-lens", default="4096,8192")
    ap.add_argument("--batches", default="1,2,8", help="attention batches; step and e2e run those <= 2")
    ap.add_argument("--runs", type=int, default=5, help="interleaved windows per arm")
    ap.add_argument("--iters", type=int, default=1000, help="attention calls per window")
    ap.add_argument("--step-iters", type=int, default=20, help="model steps per window")
    ap.add_argument("--e2e-runs", type=int, default=3)
    ap.add_argument("--attn-timeout", type=int, default=120, help="seconds per attention child")
    ap.add_argument("--model-timeout", type=int, default=420, help="seconds per step / e2e child")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-kv-len", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--child-batch", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        sys.path.insert(0, str(ROOT))
        import torch

        if not torch.cuda.is_available():
            print("bench_decode_speculate: no GPU", file=sys.stderr)
            return 3
        return {"attn": child_attn, "step": child_step, "e2e": child_e2e, "agree": child_agree}[args.child](args)

    def run(extra: list[str], limit: int) -> bool:
        cmd = [sys.executable, str(Path(__file__).resolve()), "--runs", str(args.runs), "--iters", str(args.iters),
               "--step-iters", str(args.step_iters), "--e2e-runs", str(args.e2e_runs)] + extra
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"bench_decode_speculate: {' '.join(extra)} exceeded {limit} s: stopping", file=sys.stderr)
            return False
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        for ln in lines:
            print(ln, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(ln + "\n")
        if r.returncode != 0 or not lines:
            print(f"bench_decode_speculate: {' '.join(extra)} exited {r.returncode}: stopping\n{r.stderr[-2000:]}",
                  file=sys.stderr)
            return False
        return True

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    parts = args.parts.split(",")
    batches = [int(x) for x in args.batches.split(",") if x]
    if "attn" in parts:
        for n in (int(x) for x in args.kv_lens.split(",") if x):
            for B in batches:
                if not run(["--child", "attn", "--child-kv-len", str(n), "--child-batch", str(B)], args.attn_timeout):
                    return 1
    if "agree" in parts and not run(["--child", "agree", "--child-batch", "2"], args.model_timeout):
        return 1
    for part in ("step", "e2e"):
        if part in parts:
            for B in (b for b in batches if b <= 2):
                if not run(["--child", part, "--child-batch", str(B)], args.model_timeout):
                    return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
