#!/usr/bin/env python
"""The MXFP4-weight streaming decode linear (csrc/decode_linear_mxfp4.hip) against the FP8 one on the
projection shapes of Llama-3-8B, the end-to-end generate workload ``--graph --mxfp4-weights`` against
``--graph --fp8-weights``, and what the two formats move in the logits.

    python scripts/bench_decode_linear_mxfp4.py [--rows 1,8,16] [--shapes qkv,out,gate_up,down,lm_head]
                                                [--runs 5] [--iters 200] [--tiles 1,2,4]
                                                [--e2e] [--e2e-runs 3] [--quality MODEL] [--out FILE]

The method is that of ``scripts/bench_decode_linear_fp8.py``: the parent process never touches the GPU,
every shape, end-to-end run and the quality run is a child process under its own time limit, and the
first child that fails ends the script.  In a shape's child the arms alternate (``--runs`` windows each,
device events around ``--iters`` calls); the calls of an arm rotate over distinct copies of its weight
whose total is at least 512 MB, twice the 256 MB last-level cache.  One JSON line per shape and row
count: mean and spread (max - min over the windows) of every arm in microseconds per call, the bytes/s
counted as the arm's own weight bytes (codes and scales), and ``fraction_of_yardstick``: the FP8 arm's
mean times 0.53125, the byte ratio, over the MXFP4 arm's mean.  ``--tiles`` adds MXFP4 arms with the
tiles of output columns per workgroup forced.  ``--quality MODEL`` prints the max and mean deviation of the
MXFP4 and the FP8 step's logits from the bf16 step's over 64 greedy tokens of random-init weights, and how
many of each run's ids agree with the bf16 run's.
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
BYTE_RATIO = 0.53125

# name -> (form, N, K) of Llama-3-8B
SHAPES = {
    "qkv": ("bf16", 6144, 4096),
    "out": ("bf16", 4096, 4096),
    "gate_up": ("swiglu", 28672, 4096),
    "down": ("bf16", 4096, 14336),
    "lm_head": ("f32", 128256, 4096),
}
E2E_ARMS = {"graph_fp8": ["--graph", "--fp8-weights"], "graph_mxfp4": ["--graph", "--mxfp4-weights"]}


def child(args) -> int:
    import torch

    sys.path.insert(0, str(ROOT))
    from tensorhive_fixed_amd.ops.decode_linear_fp8 import (decode_gate_up_swiglu_fp8, decode_linear_fp8,
                                                            quantize_weight_fp8)
    from tensorhive_fixed_amd.ops.decode_linear_mxfp4 import (decode_gate_up_swiglu_mxfp4, decode_linear_mxfp4,
                                                              pick_tiles_mxfp4, quantize_weight_mxfp4)

    if not torch.cuda.is_available():
        print("bench_decode_linear_mxfp4: no GPU", file=sys.stderr)
        return 3
    dev = torch.device("cuda")
    name = args.child_shape
    form, N, K = SHAPES[name]
    out_dtype = torch.float32 if form == "f32" else torch.bfloat16
    bytes8, bytes4 = N * K + 4 * N, N * K // 2 + N * K // 32
    copies8, copies4 = max(2, -(-ROTATE_BYTES // bytes8)), max(2, -(-ROTATE_BYTES // bytes4))
    g = torch.Generator(device=dev).manual_seed(0)
    q8, q4 = [], []
    for i in range(max(copies8, copies4)):
        w = torch.empty(N, K, device=dev, dtype=torch.bfloat16).normal_(0, 0.02, generator=g)
        if i < copies8:
            q8.append(quantize_weight_fp8(w))
        if i < copies4:
            q4.append(quantize_weight_mxfp4(w))
        del w
    torch.cuda.synchronize()

    for M in (int(m) for m in args.rows.split(",")):
        x = torch.randn(M, K, device=dev, dtype=torch.bfloat16, generator=g)

        def fp8(i):
            wq, s = q8[i % copies8]
            if form == "swiglu":
                return decode_gate_up_swiglu_fp8(x, wq, s)
            return decode_linear_fp8(x, wq, s, out_dtype=out_dtype)

        def mx(i, tiles=None):
            c, s = q4[i % copies4]
            if form == "swiglu":
                return decode_gate_up_swiglu_mxfp4(x, c, s, tiles=tiles)
            return decode_linear_mxfp4(x, c, s, out_dtype=out_dtype, tiles=tiles)

        arms = {"mxfp4": mx, "fp8": fp8}
        for c in (int(v) for v in args.tiles.split(",") if v):
            arms[f"mxfp4_tiles{c}"] = lambda i, c=c: mx(i, c)

        def window(fn) -> float:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(args.iters):
                fn(i)
            b.record()
            b.synchronize()
            return 1000.0 * a.elapsed_time(b) / args.iters  # us per call

        for fn in arms.values():  # warm-up: code objects, every copy touched once
            for i in range(copies4):
                fn(i)
        torch.cuda.synchronize()
        t = {k: [] for k in arms}
        for _ in range(args.runs):
            for k, fn in arms.items():
                t[k].append(window(fn))
        res = {"shape": name, "form": form, "M": M, "N": N, "K": K, "weight_copies": {"fp8": copies8, "mxfp4": copies4},
               "runs": args.runs, "iters": args.iters,
               "pick_tiles_mxfp4": pick_tiles_mxfp4(N // 2 if form == "swiglu" else N)}
        for arm, xs in t.items():
            mean = sum(xs) / len(xs)
            nbytes = bytes8 if arm == "fp8" else bytes4
            res[arm] = {"mean_us": round(mean, 2), "spread_us": round(max(xs) - min(xs), 2),
                        "windows_us": [round(v, 2) for v in xs], "weight_tb_per_s": round(nbytes / mean / 1e6, 3)}
        res["yardstick_us"] = round(BYTE_RATIO * res["fp8"]["mean_us"], 2)
        res["fraction_of_yardstick"] = round(res["yardstick_us"] / res["mxfp4"]["mean_us"], 3)
        print(json.dumps(res), flush=True)
    return 0


def quality(args) -> int:
    import torch

    sys.path.insert(0, str(ROOT))
    from tensorhive_fixed_amd.models.llama3 import Llama, LlamaConfig

    if not torch.cuda.is_available():
        print("bench_decode_linear_mxfp4: no GPU", file=sys.stderr)
        return 3
    cfg = LlamaConfig.named(args.child_quality)
    model = Llama(cfg, device="cuda", seed=0)
    tokens = torch.randint(0, cfg.vocab_size, (8, 128), device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    runs = {k: model.generate(tokens, max_new_tokens=64, return_logits=True, graph=True, **kw)
            for k, kw in (("bf16", {"stream_gemm": True}), ("fp8", {"fp8": True}), ("mxfp4", {"mxfp4": True}))}
    ids0, ref = runs["bf16"]
    res = {"bench": "quality", "model": args.child_quality, "weights": "random init", "batch": 8, "prompt": 128,
           "new_tokens": 64, "max_abs_bf16_logit": round(ref.abs().max().item(), 4)}
    for k in ("fp8", "mxfp4"):
        ids, logits = runs[k]
        # the runs feed their own ids back: compare logits only up to each sequence's first disagreement
        same = (ids == ids0).long().cumprod(dim=1)
        keep = torch.cat([torch.ones_like(same[:, :1]), same[:, :-1]], dim=1).bool()
        d = (logits - ref).abs()[keep]
        res[k] = {"max_abs_dev": round(d.max().item(), 4), "mean_abs_dev": round(d.mean().item(), 5),
                  "steps_compared": int(keep.sum()), "ids_equal": int((ids == ids0).sum()), "ids": int(ids.numel())}
    print(json.dumps(res), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default="1,8,16", help="row counts M of x")
    ap.add_argument("--shapes", default=",".join(SHAPES), help="'' for none")
    ap.add_argument("--runs", type=int, default=5, help="interleaved windows per arm (at least 3)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--tiles", default="", help="extra MXFP4 arms with the tiles of output columns per workgroup forced")
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds per child process")
    ap.add_argument("--e2e", action="store_true",
                    help="also run the llama3-8b generate workload --graph with --fp8-weights and with --mxfp4-weights")
    ap.add_argument("--e2e-runs", type=int, default=3, help="alternating runs per arm")
    ap.add_argument("--e2e-timeout", type=int, default=300)
    ap.add_argument("--quality", default=None, metavar="MODEL", help="logit deviation from the bf16 step, e.g. llama3-8b")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--child-shape", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-quality", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.runs < 3:
        ap.error("--runs must be at least 3")
    names = [s for s in args.shapes.split(",") if s]
    if any(s not in SHAPES for s in names):
        ap.error(f"--shapes: choose from {', '.join(SHAPES)}")
    if args.child_shape is not None:
        return child(args)
    if args.child_quality is not None:
        return quality(args)

    def run(cmd: list[str], limit: int, tag: dict | None = None) -> dict | None:
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"bench_decode_linear_mxfp4: {' '.join(cmd[1:])} exceeded {limit} s: stopping", file=sys.stderr)
            return None
        last = None
        for ln in (ln for ln in r.stdout.splitlines() if ln.startswith("{")):
            last = {**(tag or {}), **json.loads(ln)}
            print(json.dumps(last), flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(last) + "\n")
        if r.returncode != 0 or last is None:
            print(f"bench_decode_linear_mxfp4: {' '.join(cmd[1:])} exited {r.returncode}: stopping\n{r.stderr[-2000:]}",
                  file=sys.stderr)
            return None
        return last

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    me = [sys.executable, str(Path(__file__).resolve())]
    for name in names:
        if run(me + ["--rows", args.rows, "--runs", str(args.runs), "--iters", str(args.iters), "--tiles", args.tiles,
                     "--child-shape", name], args.step_timeout) is None:
            return 1
    if args.e2e:
        cmd = [sys.executable, "-m", "tensorhive_fixed_amd.workloads.llama3_generate", "--model", "llama3-8b",
               "--batch", "8", "--prompt-len", "512", "--max-new-tokens", "64"]
        for _ in range(args.e2e_runs):
            for arm, extra in E2E_ARMS.items():
                if run(cmd + extra, args.e2e_timeout, {"bench": "e2e", "arm": arm}) is None:
                    return 1
    if args.quality and run(me + ["--child-quality", args.quality], args.e2e_timeout) is None:
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
