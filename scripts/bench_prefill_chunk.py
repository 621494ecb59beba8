#!/usr/bin/env python
"""Chunked prefill (csrc/chunk_attn.hip, ``Llama.prefill_chunk``, ``generate(prefill_chunk=N)``) against what
a build without it does for the same job.

    python scripts/bench_prefill_chunk.py [--parts attn,e2e,gen] [--batches 1,8] [--runs 5] [--out FILE]
                                          [--min-keys N]

The method is that of ``scripts/bench_decode_speculate.py``: the parent never touches the GPU, every shape is
a child process under its own time limit, the first child that fails ends the script, and in a child the arms
alternate (window 0 warms up, ``--runs`` windows each are kept).  One JSON line per measurement:

* ``attn``: 32/8 heads; one ``chunk_attention`` call of T tokens on ``old`` cache rows (``chunk``) against the
  T / 8 ``extend_attention`` calls of 8 tokens that cover the same rows (``extend8``, the lengths advanced on
  the device between them as ``extend_step`` does) and, at ``old = 0``, against the flash forward at S = T
  (``flash``).  Where ``pick_chunk_nsplit`` splits the call over the keys (``nsplit`` > 1) a fourth arm,
  ``chunk_nsplit1``, forces the unsplit kernel, and ``split_wins`` says whether every ``chunk`` window lies
  below every one of its windows; ``--min-keys`` overrides ``MIN_KEYS_PER_CHUNK_SPLIT`` for a sweep of the
  rule.  Device events around ``--iters`` rounds; the calls rotate over cache layers.
* ``e2e``: Llama-3-8B shapes, random weights, B 8: ``prefill_chunk`` of 512 tokens on a 3584-row cache
  (``continue``) against ``prefill`` of all 4096 (``reprefill``); ``continue_wins``: the slowest ``continue``
  window is below the fastest ``reprefill`` window.
* ``gen``: ``generate(max_new_tokens=1)`` on 8 x 4096 prompts, one-shot against ``prefill_chunk=1024``: ms and
  ``torch.cuda.max_memory_allocated`` above what was allocated before the call.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SHAPES = ((512, 3584), (1024, 0), (1024, 3072), (1024, 7168), (64, 8192), (128, 8192))  # (chunk, old rows)


def _stats(xs: list[float], nd: int = 3) -> dict:
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], nd), "spread": round(xs[-1] - xs[0], nd), "windows": [round(x, nd) for x in xs]}


def child_attn(args) -> int:
    import torch

    from tensorhive_fixed_amd.models.llama3 import LlamaConfig
    from tensorhive_fixed_amd.ops.attention import flash_fwd
    from tensorhive_fixed_amd.ops import chunk_attention as ca
    from tensorhive_fixed_amd.ops.chunk_attention import chunk_attention
    from tensorhive_fixed_amd.ops.decode_attention import KVCache
    from tensorhive_fixed_amd.ops.extend_attention import extend_attention

    dev = torch.device("cuda")
    Hq, Hkv, B, smax = 32, 8, args.child_batch, max(T + old for T, old in SHAPES)
    if args.min_keys:
        ca.MIN_KEYS_PER_CHUNK_SPLIT = args.min_keys
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    L = max(4, min(32, (1 << 30) // (2 * B * Hkv * smax * 256)))  # about 1 GiB of K/V under the rotation
    cache = KVCache(LlamaConfig(dim=Hq * 128, n_layers=L, n_heads=Hq, n_kv_heads=Hkv, max_seq_len=smax), B, smax, dev)
    cache.kv.normal_()

    def window(fn, iters) -> float:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(iters):
            fn(i)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / iters  # ms per round

    for T, old in SHAPES:
        q = torch.randn(B, T, Hq * 128, device=dev, dtype=torch.bfloat16)
        q8 = [q[:, i: i + 8].contiguous() for i in range(0, T, 8)]
        new = [T] * B
        new_dev = torch.tensor(new, dtype=torch.int32, device=dev)

        def extend8(i):
            cache.set_lens([old] * B)
            for x in q8:
                extend_attention(x, cache, i % L)
                cache.advance(8)

        def chunk(i):
            cache.set_lens([old] * B)
            chunk_attention(q, cache, i % L, new, new_dev)

        def chunk_nsplit1(i):
            cache.set_lens([old] * B)
            chunk_attention(q, cache, i % L, new, new_dev, nsplit=1)

        nsplit = ca.pick_chunk_nsplit(B, Hkv, Hq // Hkv, T, old + T, cus)
        arms = {"chunk": chunk, "extend8": extend8}
        if nsplit > 1:  # otherwise `chunk` is the unsplit kernel itself
            arms["chunk_nsplit1"] = chunk_nsplit1
        if old == 0:
            qkv = torch.randn(B * T, (Hq + 2 * Hkv) * 128, device=dev, dtype=torch.bfloat16)
            arms["flash"] = lambda i: flash_fwd(qkv, B, T, Hq, Hkv, 128)
        t = {k: [] for k in arms}
        for r in range(args.runs + 1):  # window 0 warms up
            for k, fn in arms.items():
                torch.cuda.synchronize()
                x = window(fn, args.iters if r else 2)
                if r:
                    t[k].append(x)
        res = {"bench": "attn", "batch": B, "heads": [Hq, Hkv], "chunk": T, "old_rows": old, "layers_rotated": L,
               "runs": args.runs, "iters": args.iters, "nsplit": nsplit,
               "min_keys_per_split": ca.MIN_KEYS_PER_CHUNK_SPLIT, **{k + "_ms": _stats(v) for k, v in t.items()}}
        if nsplit > 1:
            res["ratio_to_nsplit1"] = round(res["chunk_ms"]["median"] / res["chunk_nsplit1_ms"]["median"], 3)
            res["split_wins"] = max(t["chunk"]) < min(t["chunk_nsplit1"])
        pairs = B * Hq * (T * old + T * (T + 1) // 2)
        res["chunk_tflops"] = round(4 * 128 * pairs / res["chunk_ms"]["median"] / 1e9, 1)
        res["ratio_to_extend8"] = round(res["chunk_ms"]["median"] / res["extend8_ms"]["median"], 3)
        if "flash" in arms:
            res["ratio_to_flash"] = round(res["chunk_ms"]["median"] / res["flash_ms"]["median"], 3)
        print(json.dumps(res), flush=True)
    return 0


def _timed(fn) -> float:
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0)


def child_e2e(args) -> int:
    import torch

    from tensorhive_fixed_amd.models.llama3 import Llama, LlamaConfig
    from tensorhive_fixed_amd.ops.decode_attention import KVCache

    dev = torch.device("cuda")
    B, old, T = 8, 3584, 512
    model = Llama(LlamaConfig.named("llama3-8b"), device=dev, dtype=torch.bfloat16, seed=0)
    cache = KVCache(model.cfg, B, old + T, dev)
    cache.kv.normal_(0, 0.5)
    tok = torch.randint(0, model.cfg.vocab_size, (B, old + T), device=dev)
    tail = tok[:, old:].contiguous()

    def cont():
        cache.set_lens([old] * B)
        model.prefill_chunk(tail, [T] * B, cache)

    arms = {"continue": cont, "reprefill": lambda: model.prefill(tok, [old + T] * B, cache)}
    t = {k: [] for k in arms}
    for r in range(args.runs + 1):  # window 0 warms up
        for k, fn in arms.items():
            x = _timed(fn)
            if r:
                t[k].append(x)
    print(json.dumps({"bench": "e2e", "model": "llama3-8b", "batch": B, "old_rows": old, "chunk": T, "runs": args.runs,
                      **{k + "_ms": _stats(v, 2) for k, v in t.items()},
                      "ratio": round(_stats(t["continue"])["median"] / _stats(t["reprefill"])["median"], 4),
                      "continue_wins": max(t["continue"]) < min(t["reprefill"])}), flush=True)
    return 0


def child_gen(args) -> int:
    import torch

    from tensorhive_fixed_amd.models.llama3 import Llama, LlamaConfig

    dev = torch.device("cuda")
    B, S, N = 8, 4096, 1024
    model = Llama(LlamaConfig.named("llama3-8b"), device=dev, dtype=torch.bfloat16, seed=0)
    tok = torch.randint(0, model.cfg.vocab_size, (B, S), device=dev)
    arms = {"one_shot": None, f"chunk_{N}": N}
    t, peak = {k: [] for k in arms}, {}
    for r in range(args.runs + 1):  # window 0 warms up
        for k, n in arms.items():
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            x = _timed(lambda: model.generate(tok, max_new_tokens=1, prefill_chunk=n))
            peak[k] = torch.cuda.max_memory_allocated() - base
            if r:
                t[k].append(x)
    print(json.dumps({"bench": "gen", "model": "llama3-8b", "batch": B, "prompt": S, "runs": args.runs,
                      **{k + "_ms": _stats(v, 2) for k, v in t.items()},
                      **{k + "_peak_mb": round(v / 2 ** 20, 1) for k, v in peak.items()}}), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parts", default="attn,e2e,gen")
    ap.add_argument("--batches", default="1,8", help="attention batches")
    ap.add_argument("--runs", type=int, default=5, help="interleaved windows per arm")
    ap.add_argument("--iters", type=int, default=20, help="attention rounds per window")
    ap.add_argument("--attn-timeout", type=int, default=240, help="seconds per attention child")
    ap.add_argument("--model-timeout", type=int, default=300, help="seconds per model child")
    ap.add_argument("--min-keys", type=int, default=0, help="override MIN_KEYS_PER_CHUNK_SPLIT (attention part)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-batch", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        sys.path.insert(0, str(ROOT))
        import torch

        if not torch.cuda.is_available():
            print("bench_prefill_chunk: no GPU", file=sys.stderr)
            return 3
        return {"attn": child_attn, "e2e": child_e2e, "gen": child_gen}[args.child](args)

    def run(extra: list[str], limit: int) -> bool:
        cmd = [sys.executable, str(Path(__file__).resolve()), "--runs", str(args.runs), "--iters", str(args.iters),
               "--min-keys", str(args.min_keys)] + extra
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"bench_prefill_chunk: {' '.join(extra)} exceeded {limit} s: stopping", file=sys.stderr)
            return False
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        for ln in lines:
            print(ln, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(ln + "\n")
        if r.returncode != 0 or not lines:
            print(f"bench_prefill_chunk: {' '.join(extra)} exited {r.returncode}: stopping\n{r.stderr[-2000:]}",
                  file=sys.stderr)
            return False
        return True

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    parts = args.parts.split(",")
    if "attn" in parts:
        for B in (int(x) for x in args.batches.split(",") if x):
            if not run(["--child", "attn", "--child-batch", str(B)], args.attn_timeout):
                return 1
    for part in ("e2e", "gen"):
        if part in parts and not run(["--child", part], args.model_timeout):
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
