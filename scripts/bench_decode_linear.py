#!/usr/bin/env python
"""The weight-streaming decode linear (csrc/decode_linear.hip) against what ``decode_step`` runs today
(hipBLASLt through ``torch.mm``) on the projection shapes of Llama-3-8B, and the end-to-end generate
workload with and without ``--stream-gemm``.

    python scripts/bench_decode_linear.py [--rows 1,8,16] [--shapes qkv,out,gate_up,down,lm_head]
                                          [--runs 5] [--iters 200] [--tiles 1,2] [--e2e] [--out FILE]

The parent process never touches the GPU: every shape (its weight copies are allocated once and serve
all ``--rows``) and every end-to-end run is a child process under its own time limit, and the first
child that fails ends the script.  In a child the arms alternate (``--runs`` windows each, device
events around ``--iters`` calls).  Calls rotate over distinct copies of the weight whose total is at
least 512 MB (and never fewer than two), twice the 256 MB last-level cache, so that no call finds
its weight on chip.  The comparison arm is ``torch.mm`` for the bf16 rows, ``torch.mm`` + ``swiglu``
for gate|up and ``torch.mm`` + ``.float()`` for the LM head.  One JSON line per shape and row count:
mean and spread (max - min over the windows) of every arm in microseconds per call and the bytes/s
counted as the weight bytes.  ``--tiles`` adds arms with the kernel's tiles of output columns per workgroup
forced.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HBM_ACHIEVABLE_TBS = 6.3  # the streaming rate this chip reaches in practice (reference point only)
ROTATE_BYTES = 512 << 20

# name -> (form, N, K) of Llama-3-8B
SHAPES = {
    "qkv": ("bf16", 6144, 4096),
    "out": ("bf16", 4096, 4096),
    "gate_up": ("swiglu", 28672, 4096),
    "down": ("bf16", 4096, 14336),
    "lm_head": ("f32", 128256, 4096),
}


def child(args) -> int:
    import torch

    sys.path.insert(0, str(ROOT))
    from tensorhive_fixed_amd.ops.decode_linear import decode_gate_up_swiglu, decode_linear, pick_tiles
    from tensorhive_fixed_amd.ops.swiglu import swiglu

    if not torch.cuda.is_available():
        print("bench_decode_linear: no GPU", file=sys.stderr)
        return 3
    dev = torch.device("cuda")
    name = args.child_shape
    form, N, K = SHAPES[name]
    wbytes = 2 * N * K
    copies = max(2, -(-ROTATE_BYTES // wbytes))
    g = torch.Generator(device=dev).manual_seed(0)
    ws = [torch.empty(N, K, device=dev, dtype=torch.bfloat16).normal_(0, 0.02, generator=g) for _ in range(copies)]

    for M in (int(m) for m in args.rows.split(",")):
        x = torch.randn(M, K, device=dev, dtype=torch.bfloat16, generator=g)

        def ours(i, tiles=None):
            w = ws[i % copies]
            if form == "swiglu":
                return decode_gate_up_swiglu(x, w, tiles=tiles)
            return decode_linear(x, w, out_dtype=torch.float32 if form == "f32" else torch.bfloat16, tiles=tiles)

        def blas(i):
            y = torch.mm(x, ws[i % copies].t())
            return swiglu(y) if form == "swiglu" else y.float() if form == "f32" else y

        arms = {"decode_linear": ours, "hipblaslt": blas}
        for c in (int(v) for v in args.tiles.split(",") if v):
            arms[f"decode_linear_tiles{c}"] = lambda i, c=c: ours(i, c)
        diff = (ours(0).float() - blas(0).float()).abs().max().item()

        def window(fn) -> float:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(args.iters):
                fn(i)
            b.record()
            b.synchronize()
            return 1000.0 * a.elapsed_time(b) / args.iters  # us per call

        for fn in arms.values():  # warm-up: code objects, algorithm choice
            for i in range(2 * copies):
                fn(i)
        torch.cuda.synchronize()
        t = {k: [] for k in arms}
        for _ in range(args.runs):
            for k, fn in arms.items():
                t[k].append(window(fn))
        res = {"shape": name, "form": form, "M": M, "N": N, "K": K, "weight_copies": copies, "runs": args.runs,
               "iters": args.iters, "tiles": pick_tiles(N // 2 if form == "swiglu" else N), "bytes_per_call": wbytes,
               "max_abs_diff_vs_hipblaslt": diff}
        for arm, xs in t.items():
            mean = sum(xs) / len(xs)
            res[arm] = {"mean_us": round(mean, 2), "spread_us": round(max(xs) - min(xs), 2),
                        "windows_us": [round(v, 2) for v in xs], "tb_per_s": round(wbytes / mean / 1e6, 3)}
        res["hbm_achievable_tb_per_s"] = HBM_ACHIEVABLE_TBS
        res["not_slower_than_hipblaslt_within_its_spread"] = (
            res["decode_linear"]["mean_us"] <= res["hipblaslt"]["mean_us"] + res["hipblaslt"]["spread_us"])
        print(json.dumps(res), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default="1,8,16", help="row counts M of x")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--runs", type=int, default=5, help="interleaved windows per arm (at least 4)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--tiles", default="", help="extra arms with the tiles of output columns per workgroup forced, e.g. 1,2")
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds per child process")
    ap.add_argument("--e2e", action="store_true",
                    help="also run the llama3-8b generate workload with and without --stream-gemm, twice each")
    ap.add_argument("--e2e-timeout", type=int, default=400)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--child-shape", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.runs < 4:
        ap.error("--runs must be at least 4")
    names = [s for s in args.shapes.split(",") if s]
    if any(s not in SHAPES for s in names):
        ap.error(f"--shapes: choose from {', '.join(SHAPES)}")
    if args.child_shape is not None:
        return child(args)

    def run(cmd: list[str], limit: int) -> bool:
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"bench_decode_linear: {' '.join(cmd[1:])} exceeded {limit} s: stopping", file=sys.stderr)
            return False
        for ln in (ln for ln in r.stdout.splitlines() if ln.startswith("{")):
            print(ln, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(ln + "\n")
        if r.returncode != 0:
            print(f"bench_decode_linear: {' '.join(cmd[1:])} exited {r.returncode}: stopping\n{r.stderr[-2000:]}",
                  file=sys.stderr)
            return False
        return True

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    base = [sys.executable, str(Path(__file__).resolve()), "--rows", args.rows, "--runs", str(args.runs),
            "--iters", str(args.iters), "--tiles", args.tiles]
    for name in names:
        if not run(base + ["--child-shape", name], args.step_timeout):
            return 1
    if args.e2e:
        cmd = [sys.executable, "-m", "tensorhive_fixed_amd.workloads.llama3_generate", "--model", "llama3-8b",
               "--batch", "8", "--prompt-len", "512", "--max-new-tokens", "64"]
        for extra in ([], ["--stream-gemm"], [], ["--stream-gemm"]):
            if not run(cmd + extra, args.e2e_timeout):
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
