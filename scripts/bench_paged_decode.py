#!/usr/bin/env python
"""Paged decode attention (csrc/paged_attn.hip) against the dense kernel (csrc/decode_attn.hip) on the
same rows.

    python scripts/bench_paged_decode.py [--kv-lens 4096,8192] [--ragged 512,8192] [--batch 8]
                                         [--heads 32,8] [--runs 5] [--iters 1000] [--out FILE]

The parent process never touches the GPU: every shape is a child process under its own time limit, and
the first child that fails ends the script.  In a child three arms alternate (``--runs`` windows each,
device events around ``--iters`` calls): the paged call through a permuted page table (no two logical
neighbours adjacent in the pool), the paged call through the identity table, and dense
``decode_attention``, the yardstick.  Calls rotate over ``--layers`` cache layers so that no call finds
its K/V in the last-level cache.  ``--ragged LO,HI`` is one more shape: lengths spread evenly from LO to
HI over the batch.  One JSON line per shape: mean and spread (max - min over the windows) of every arm
in microseconds per call, the achieved bytes/s counted as ``2 * sum(kv_len) * Hkv * 256 B`` per call,
the ratio of each paged arm to dense per window pair, the largest difference between the paged and the
dense output, and the pool's bytes beside the dense cache's.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def child(args) -> int:
    import torch

    sys.path.insert(0, str(ROOT))
    from tensorhive_fixed_amd.models.llama3 import LlamaConfig
    from tensorhive_fixed_amd.ops.decode_attention import KVCache, decode_attention, kv_cache_bytes, pick_nsplit
    from tensorhive_fixed_amd.ops.paged_attention import (PagedKVCache, paged_cache_bytes, paged_decode_attention,
                                                          pages_for)

    if not torch.cuda.is_available():
        print("bench_paged_decode: no GPU", file=sys.stderr)
        return 3
    dev = torch.device("cuda")
    Hq, Hkv, L = args.hq, args.hkv, args.layers
    lens = [int(x) for x in args.child_lens.split(",")]
    B, n = len(lens), max(lens)
    cfg = LlamaConfig(dim=Hq * 128, n_layers=L, n_heads=Hq, n_kv_heads=Hkv, max_seq_len=n)
    dense = KVCache(cfg, B, n, dev)
    dense.kv.normal_()
    dense.set_lens(lens)
    n_pages = sum(pages_for(x) for x in lens)

    def paged_copy(permute: bool) -> PagedKVCache:
        c = PagedKVCache(cfg, B, n, n_pages, dev)
        if permute:
            c.free_pages = list(range(0, n_pages, 2)) + list(range(1, n_pages, 2))
        for b, x in enumerate(lens):
            c.reserve(b, x)
        for i in range(L):
            c.fill(i, dense.k(i), dense.v(i))
        c.set_lens(lens)
        return c

    permuted, identity = paged_copy(True), paged_copy(False)
    q = torch.randn(B, Hq * 128, device=dev, dtype=torch.bfloat16)
    arms = {"paged_permuted": lambda i: paged_decode_attention(q, permuted, i % L),
            "paged_identity": lambda i: paged_decode_attention(q, identity, i % L),
            "dense": lambda i: decode_attention(q, dense, i % L)}
    ref = arms["dense"](0).float()
    diff = max((arms[a](0).float() - ref).abs().max().item() for a in ("paged_permuted", "paged_identity"))

    def window(fn) -> float:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(args.iters):
            fn(i)
        b.record()
        b.synchronize()
        return 1000.0 * a.elapsed_time(b) / args.iters  # us per call

    for fn in arms.values():  # warm-up: code objects, workspaces
        for i in range(2 * L):
            fn(i)
    torch.cuda.synchronize()
    t = {a: [] for a in arms}
    for _ in range(args.runs):
        for a, fn in arms.items():
            t[a].append(window(fn))
    nbytes = 2 * sum(lens) * Hkv * 256
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    res = {"kv_lens": lens if len(set(lens)) > 1 else n, "batch": B, "heads": [Hq, Hkv], "layers_rotated": L,
           "runs": args.runs, "iters": args.iters, "nsplit": pick_nsplit(B, Hkv, n, cus), "bytes_per_call": nbytes,
           "max_abs_diff_paged_vs_dense": diff, "pool_bytes_per_layer": paged_cache_bytes(cfg, n_pages) // L,
           "dense_bytes_per_layer": kv_cache_bytes(cfg, B, n) // L}
    for a, xs in t.items():
        mean = sum(xs) / len(xs)
        res[a] = {"mean_us": round(mean, 2), "spread_us": round(max(xs) - min(xs), 2),
                  "windows_us": [round(x, 2) for x in xs], "tb_per_s": round(nbytes / mean / 1e6, 3)}
    for a in ("paged_permuted", "paged_identity"):
        r = [x / y for x, y in zip(t[a], t["dense"])]
        res[a]["ratio_to_dense"] = {"mean": round(sum(r) / len(r), 4), "min": round(min(r), 4), "max": round(max(r), 4)}
    print(json.dumps(res), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kv-lens", default="4096,8192")
    ap.add_argument("--ragged", default="512,8192", help="LO,HI of one ragged batch ('' for none)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--heads", default="32,8")
    ap.add_argument("--layers", type=int, default=8, help="cache layers the calls rotate over")
    ap.add_argument("--runs", type=int, default=5, help="interleaved windows per arm (at least 4)")
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds per child process")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--child-lens", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.hq, args.hkv = (int(x) for x in args.heads.split(","))
    if args.runs < 4:
        ap.error("--runs must be at least 4")
    if args.child_lens is not None:
        return child(args)
    shapes = [[int(x)] * args.batch for x in args.kv_lens.split(",") if x]
    if args.ragged:
        lo, hi = (int(x) for x in args.ragged.split(","))
        shapes.append([lo + (hi - lo) * b // max(args.batch - 1, 1) for b in range(args.batch)])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for lens in shapes:
        cmd = [sys.executable, str(Path(__file__).resolve()), "--heads", args.heads, "--layers", str(args.layers),
               "--runs", str(args.runs), "--iters", str(args.iters), "--child-lens", ",".join(map(str, lens))]
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            print(f"bench_paged_decode: lengths {lens} exceeded {args.step_timeout} s: stopping", file=sys.stderr)
            return 1
        for ln in (x for x in r.stdout.splitlines() if x.startswith("{")):
            print(ln, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(ln + "\n")
        if r.returncode != 0:
            print(f"bench_paged_decode: lengths {lens} exited {r.returncode}: stopping\n{r.stderr[-2000:]}",
                  file=sys.stderr)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
