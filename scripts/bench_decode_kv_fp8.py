#!/usr/bin/env python
"""Decode attention over an FP8 KV cache (csrc/decode_attn_fp8.hip) against the bf16 kernel
(csrc/decode_attn.hip) on the same values, and the end-to-end generate workload ``--graph --stream-gemm
--fp8-weights`` at a 4096-token prompt with and without ``--fp8-kv``.

    python scripts/bench_decode_kv_fp8.py [--kv-lens 512,4096,8192] [--batch 8] [--heads 32,8]
                                          [--runs 5] [--iters 1000] [--nsplits 0] [--e2e] [--e2e-runs 3]
                                          [--out FILE]

The method is that of ``scripts/bench_decode.py`` and ``scripts/bench_decode_linear_fp8.py``.  The parent
process never touches the GPU: every shape and every end-to-end run is a child process under its own
time limit, started one after another, and the first child that fails ends the script.  In a child the
arms alternate (``--runs`` windows each, device events around ``--iters`` calls); the calls of an arm
rotate over ``--layers`` cache layers so that no call finds its K/V in the last-level cache (the FP8
cache is quantized from the bf16 one, layer by layer).  One JSON line per shape and split count (``0``:
the wrapper's automatic choice, the same rule for both arms): mean and spread (max - min over the
windows) of both arms in microseconds per call, the bytes/s counted as the arm's own K/V bytes (scales
included), and whether the FP8 arm clears the bar: its mean below the bf16 mean by more than the larger of
the two spreads.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
E2E_ARMS = {"bf16_kv": [], "fp8_kv": ["--fp8-kv"]}


def child(args) -> int:
    import torch

    sys.path.insert(0, str(ROOT))
    from tensorhive_fixed_amd.models.llama3 import LlamaConfig
    from tensorhive_fixed_amd.ops.decode_attention import KVCache, decode_attention, pick_nsplit

    if not torch.cuda.is_available():
        print("bench_decode_kv_fp8: no GPU", file=sys.stderr)
        return 3
    dev = torch.device("cuda")
    Hq, Hkv = args.hq, args.hkv
    B, n, L = args.batch, args.child_kv_len, args.layers
    cfg = LlamaConfig(dim=Hq * 128, n_layers=L, n_heads=Hq, n_kv_heads=Hkv, max_seq_len=n)
    bf = KVCache(cfg, B, n, dev)
    bf.kv.normal_()
    bf.set_lens([n] * B)
    f8 = KVCache(cfg, B, n, dev, dtype=torch.float8_e4m3fn)
    for i in range(L):
        f8.fill(i, bf.k(i), bf.v(i))
    f8.set_lens([n] * B)
    q = torch.randn(B, Hq * 128, device=dev, dtype=torch.bfloat16)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count

    def window(fn) -> float:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(args.iters):
            fn(i)
        b.record()
        b.synchronize()
        return 1000.0 * a.elapsed_time(b) / args.iters  # us per call

    for ns in (int(v) for v in args.nsplits.split(",")):
        nsplit = ns or None
        arms = {"fp8": lambda i: decode_attention(q, f8, i % L, nsplit=nsplit),
                "bf16": lambda i: decode_attention(q, bf, i % L, nsplit=nsplit)}
        diff = (arms["fp8"](0).float() - arms["bf16"](0).float()).abs().max().item()  # the quantization itself
        for fn in arms.values():  # warm-up: code objects
            for i in range(2 * L):
                fn(i)
        torch.cuda.synchronize()
        t = {k: [] for k in arms}
        for _ in range(args.runs):
            for k, fn in arms.items():
                t[k].append(window(fn))
        rows = 2 * B * n * Hkv
        res = {"kv_len": n, "batch": B, "heads": [Hq, Hkv], "layers_rotated": L, "runs": args.runs,
               "iters": args.iters, "nsplit": nsplit or pick_nsplit(B, Hkv, n, cus), "nsplit_forced": bool(ns),
               "max_abs_diff_fp8_vs_bf16": diff}
        for arm, xs in t.items():
            mean = sum(xs) / len(xs)
            nbytes = rows * (132 if arm == "fp8" else 256)
            res[arm] = {"mean_us": round(mean, 2), "spread_us": round(max(xs) - min(xs), 2),
                        "windows_us": [round(x, 2) for x in xs], "bytes_per_call": nbytes,
                        "tb_per_s": round(nbytes / mean / 1e6, 3)}
        gain = res["bf16"]["mean_us"] - res["fp8"]["mean_us"]
        bar = max(res["bf16"]["spread_us"], res["fp8"]["spread_us"])
        res.update({"gain_us": round(gain, 2), "larger_spread_us": bar, "clears_the_bar": gain > bar})
        print(json.dumps(res), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kv-lens", default="512,4096,8192", help="'' for none")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--heads", default="32,8")
    ap.add_argument("--layers", type=int, default=8, help="cache layers the calls rotate over")
    ap.add_argument("--runs", type=int, default=5, help="interleaved windows per arm (at least 4)")
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--nsplits", default="0", help="split counts to measure, 0: the wrapper's automatic choice")
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds per child process")
    ap.add_argument("--e2e", action="store_true",
                    help="also run the llama3-8b generate workload --graph --stream-gemm --fp8-weights at a "
                         "4096-token prompt with and without --fp8-kv")
    ap.add_argument("--e2e-runs", type=int, default=3, help="alternating runs per arm (at least 2)")
    ap.add_argument("--e2e-timeout", type=int, default=300)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--child-kv-len", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.hq, args.hkv = (int(x) for x in args.heads.split(","))
    if args.runs < 4 or args.e2e_runs < 2:
        ap.error("--runs must be at least 4 and --e2e-runs at least 2")
    if args.child_kv_len is not None:
        return child(args)

    def emit(ln: str) -> None:
        print(ln, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(ln + "\n")

    def run(cmd: list[str], limit: int, tag: dict | None = None) -> dict | None:
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"bench_decode_kv_fp8: {' '.join(cmd[1:])} exceeded {limit} s: stopping", file=sys.stderr)
            return None
        last = None
        for ln in (ln for ln in r.stdout.splitlines() if ln.startswith("{")):
            last = {**(tag or {}), **json.loads(ln)}
            emit(json.dumps(last))
        if r.returncode != 0 or last is None:
            print(f"bench_decode_kv_fp8: {' '.join(cmd[1:])} exited {r.returncode}: stopping\n{r.stderr[-2000:]}",
                  file=sys.stderr)
            return None
        return last

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    base = [sys.executable, str(Path(__file__).resolve()), "--batch", str(args.batch), "--heads", args.heads,
            "--layers", str(args.layers), "--runs", str(args.runs), "--iters", str(args.iters),
            "--nsplits", args.nsplits]
    for n in (int(x) for x in args.kv_lens.split(",") if x):
        if run(base + ["--child-kv-len", str(n)], args.step_timeout) is None:
            return 1
    if args.e2e:
        cmd = [sys.executable, "-m", "tensorhive_fixed_amd.workloads.llama3_generate", "--model", "llama3-8b",
               "--batch", "8", "--prompt-len", "4096", "--max-new-tokens", "64", "--graph", "--stream-gemm",
               "--fp8-weights"]
        runs: dict[str, list[dict]] = {k: [] for k in E2E_ARMS}
        for _ in range(args.e2e_runs):
            for arm, extra in E2E_ARMS.items():
                done = run(cmd + extra, args.e2e_timeout, {"bench": "e2e", "arm": arm})
                if done is None:
                    return 1
                runs[arm].append(done)
        stat = {}
        for k, ds in runs.items():
            ms, pf = [d["decode_ms_per_token"] for d in ds], [d["prefill_ms"] for d in ds]
            stat[k] = {"mean_ms": round(sum(ms) / len(ms), 3), "spread_ms": round(max(ms) - min(ms), 3), "runs_ms": ms,
                       "prefill_mean_ms": round(sum(pf) / len(pf), 1), "prefill_runs_ms": pf,
                       "kv_cache_mb": ds[0]["kv_cache_mb"]}
            emit(json.dumps({"bench": "e2e_summary", "arm": k, **stat[k]}))
        gain = stat["bf16_kv"]["mean_ms"] - stat["fp8_kv"]["mean_ms"]
        bar = max(s["spread_ms"] for s in stat.values())
        emit(json.dumps({"bench": "e2e_bar", "gain_ms": round(gain, 3), "larger_spread_ms": bar,
                         "clears_the_bar": gain > bar,
                         "prefill_delta_ms": round(stat["fp8_kv"]["prefill_mean_ms"] - stat["bf16_kv"]["prefill_mean_ms"], 1)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
