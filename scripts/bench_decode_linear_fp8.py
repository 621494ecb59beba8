#!/usr/bin/env python
"""The FP8-weight streaming decode linear (csrc/decode_linear_fp8.hip) against what ``--stream-gemm``
dispatches today for the same shape, on the projection shapes of Llama-3-8B, and the end-to-end
generate workload ``--graph --stream-gemm`` with and without ``--fp8-weights``.

    python scripts/bench_decode_linear_fp8.py [--rows 1,8,16] [--shapes qkv,out,gate_up,down,lm_head]
                                              [--runs 5] [--iters 200] [--tiles 1,2]
                                              [--e2e] [--e2e-runs 3] [--out FILE]

The method is that of ``scripts/bench_decode_linear.py``.  The parent process never touches the GPU:
every shape (its weight copies are allocated once and serve all ``--rows``) and every end-to-end run is
a child process under its own time limit, and the first child that fails ends the script.  In a child
the arms alternate (``--runs`` windows each, device events around ``--iters`` calls).  The calls of an
arm rotate over distinct copies of its weight whose total is at least 512 MB (and never fewer than
two), twice the 256 MB last-level cache; the FP8 arm's copies are half the size, so it gets more of
them.  The comparison arm is what ``decode_step(stream_gemm=True)`` runs: ``decode_linear`` /
``decode_gate_up_swiglu`` where ``decode_linear.preferred`` holds, ``torch.mm`` (hipBLASLt) for the
down projection.  One JSON line per shape and row count: mean and spread (max - min over the windows)
of every arm in microseconds per call, the bytes/s counted as that arm's weight bytes, and whether the
FP8 arm clears the bar: its mean below the comparison arm's mean by more than the larger of the two
spreads.  ``--tiles`` adds FP8 arms with the tiles of output columns per workgroup forced.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
ROTATE_BYTES = 512 << 20

# name -> (form, N, K) of Llama-3-8B
SHAPES = {
    "qkv": ("bf16", 6144, 4096),
    "out": ("bf16", 4096, 4096),
    "gate_up": ("swiglu", 28672, 4096),
    "down": ("bf16", 4096, 14336),
    "lm_head": ("f32", 128256, 4096),
}
E2E_ARMS = {"graph_stream": ["--graph", "--stream-gemm"],
            "graph_stream_fp8": ["--graph", "--stream-gemm", "--fp8-weights"]}


def child(args) -> int:
    import torch

    sys.path.insert(0, str(ROOT))
    from tensorhive_fixed_amd.ops.decode_linear import decode_gate_up_swiglu, decode_linear, preferred
    from tensorhive_fixed_amd.ops.decode_linear_fp8 import (decode_gate_up_swiglu_fp8, decode_linear_fp8,
                                                            pick_tiles_fp8, quantize_weight_fp8)

    if not torch.cuda.is_available():
        print("bench_decode_linear_fp8: no GPU", file=sys.stderr)
        return 3
    dev = torch.device("cuda")
    name = args.child_shape
    form, N, K = SHAPES[name]
    out_dtype = torch.float32 if form == "f32" else torch.bfloat16
    copies = max(2, -(-ROTATE_BYTES // (2 * N * K)))
    copies8 = max(2, -(-ROTATE_BYTES // (N * K)))
    g = torch.Generator(device=dev).manual_seed(0)

    def fresh():
        return torch.empty(N, K, device=dev, dtype=torch.bfloat16).normal_(0, 0.02, generator=g)

    ws = [fresh() for _ in range(copies)]
    qs = [quantize_weight_fp8(ws[i] if i < copies else fresh()) for i in range(copies8)]
    torch.cuda.synchronize()

    for M in (int(m) for m in args.rows.split(",")):
        x = torch.randn(M, K, device=dev, dtype=torch.bfloat16, generator=g)
        streams = preferred(M, N, K)

        def base(i):
            w = ws[i % copies]
            if not streams:
                return torch.mm(x, w.t())
            if form == "swiglu":
                return decode_gate_up_swiglu(x, w)
            return decode_linear(x, w, out_dtype=out_dtype)

        def fp8(i, tiles=None):
            wq, s = qs[i % copies8]
            if form == "swiglu":
                return decode_gate_up_swiglu_fp8(x, wq, s, tiles=tiles)
            return decode_linear_fp8(x, wq, s, out_dtype=out_dtype, tiles=tiles)

        arms = {"fp8": fp8, "stream_gemm": base}
        for c in (int(v) for v in args.tiles.split(",") if v):
            arms[f"fp8_tiles{c}"] = lambda i, c=c: fp8(i, c)
        diff = (fp8(0).float() - base(0).float()).abs().max().item()  # copy 0 of both arms is the same weight

        def window(fn) -> float:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(args.iters):
                fn(i)
            b.record()
            b.synchronize()
            return 1000.0 * a.elapsed_time(b) / args.iters  # us per call

        for fn in arms.values():  # warm-up: code objects, algorithm choice
            for i in range(2 * copies8):
                fn(i)
        torch.cuda.synchronize()
        t = {k: [] for k in arms}
        for _ in range(args.runs):
            for k, fn in arms.items():
                t[k].append(window(fn))
        res = {"shape": name, "form": form, "M": M, "N": N, "K": K, "weight_copies": {"stream_gemm": copies, "fp8": copies8},
               "runs": args.runs, "iters": args.iters, "stream_gemm_runs": "decode_linear" if streams else "hipblaslt",
               "pick_tiles_fp8": pick_tiles_fp8(N // 2 if form == "swiglu" else N),
               "max_abs_diff_fp8_vs_stream_gemm": diff}
        for arm, xs in t.items():
            mean = sum(xs) / len(xs)
            nbytes = 2 * N * K if arm == "stream_gemm" else N * K
            res[arm] = {"mean_us": round(mean, 2), "spread_us": round(max(xs) - min(xs), 2),
                        "windows_us": [round(v, 2) for v in xs], "weight_tb_per_s": round(nbytes / mean / 1e6, 3)}
        gain = res["stream_gemm"]["mean_us"] - res["fp8"]["mean_us"]
        bar = max(res["stream_gemm"]["spread_us"], res["fp8"]["spread_us"])
        res.update({"gain_us": round(gain, 2), "larger_spread_us": bar, "clears_the_bar": gain > bar})
        print(json.dumps(res), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default="1,8,16", help="row counts M of x")
    ap.add_argument("--shapes", default=",".join(SHAPES), help="'' for none")
    ap.add_argument("--runs", type=int, default=5, help="interleaved windows per arm (at least 4)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--tiles", default="", help="extra FP8 arms with the tiles of output columns per workgroup forced, e.g. 1,2")
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds per child process")
    ap.add_argument("--e2e", action="store_true",
                    help="also run the llama3-8b generate workload --graph --stream-gemm with and without --fp8-weights")
    ap.add_argument("--e2e-runs", type=int, default=3, help="alternating runs per arm (at least 2)")
    ap.add_argument("--e2e-timeout", type=int, default=300)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--child-shape", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.runs < 4 or args.e2e_runs < 2:
        ap.error("--runs must be at least 4 and --e2e-runs at least 2")
    names = [s for s in args.shapes.split(",") if s]
    if any(s not in SHAPES for s in names):
        ap.error(f"--shapes: choose from {', '.join(SHAPES)}")
    if args.child_shape is not None:
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
            print(f"bench_decode_linear_fp8: {' '.join(cmd[1:])} exceeded {limit} s: stopping", file=sys.stderr)
            return None
        last = None
        for ln in (ln for ln in r.stdout.splitlines() if ln.startswith("{")):
            last = {**(tag or {}), **json.loads(ln)}
            emit(json.dumps(last))
        if r.returncode != 0 or last is None:
            print(f"bench_decode_linear_fp8: {' '.join(cmd[1:])} exited {r.returncode}: stopping\n{r.stderr[-2000:]}",
                  file=sys.stderr)
            return None
        return last

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    base = [sys.executable, str(Path(__file__).resolve()), "--rows", args.rows, "--runs", str(args.runs),
            "--iters", str(args.iters), "--tiles", args.tiles]
    for name in names:
        if run(base + ["--child-shape", name], args.step_timeout) is None:
            return 1
    if args.e2e:
        cmd = [sys.executable, "-m", "tensorhive_fixed_amd.workloads.llama3_generate", "--model", "llama3-8b",
               "--batch", "8", "--prompt-len", "512", "--max-new-tokens", "64"]
        ms: dict[str, list[float]] = {k: [] for k in E2E_ARMS}
        for _ in range(args.e2e_runs):
            for arm, extra in E2E_ARMS.items():
                done = run(cmd + extra, args.e2e_timeout, {"bench": "e2e", "arm": arm})
                if done is None:
                    return 1
                ms[arm].append(done["decode_ms_per_token"])
        stat = {k: {"mean_ms": round(sum(xs) / len(xs), 3), "spread_ms": round(max(xs) - min(xs), 3), "runs_ms": xs}
                for k, xs in ms.items()}
        for k, s in stat.items():
            emit(json.dumps({"bench": "e2e_summary", "arm": k, **s}))
        gain = stat["graph_stream"]["mean_ms"] - stat["graph_stream_fp8"]["mean_ms"]
        bar = max(s["spread_ms"] for s in stat.values())
        emit(json.dumps({"bench": "e2e_bar", "gain_ms": round(gain, 3), "larger_spread_ms": bar,
                         "clears_the_bar": gain > bar}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
