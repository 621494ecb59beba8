#!/usr/bin/env python
"""Decode attention (csrc/decode_attn.hip) against torch SDPA on the same cache slices, and the
end-to-end generate workload.

    python scripts/bench_decode.py [--kv-lens 512,4096,8192] [--batch 8] [--heads 32,8]
                                   [--runs 5] [--iters 1000] [--e2e] [--out FILE]

The parent process never touches the GPU: every shape (and the end-to-end run) is a child process
under its own time limit, and the first child that fails ends the script.  In a child the two arms
alternate (``--runs`` windows each, device events around ``--iters`` calls); calls rotate over
``--layers`` cache layers so that no call finds its K/V in the last-level cache.  One JSON line per
shape: mean and spread (max - min over the windows) of both arms in microseconds per call, the
achieved bytes/s of the kernel counted as ``2 * sum(kv_len) * Hkv * 256 B`` per call, and the
largest difference between the two arms' outputs.
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


def child(args) -> int:
    import torch
    import torch.nn.functional as Fn

    sys.path.insert(0, str(ROOT))
    from tensorhive_fixed_amd.models.llama3 import LlamaConfig
    from tensorhive_fixed_amd.ops.decode_attention import KVCache, decode_attention, pick_nsplit

    if not torch.cuda.is_available():
        print("bench_decode: no GPU", file=sys.stderr)
        return 3
    dev = torch.device("cuda")
    Hq, Hkv = args.hq, args.hkv
    B, n, L = args.batch, args.kv_len, args.layers
    cfg = LlamaConfig(dim=Hq * 128, n_layers=L, n_heads=Hq, n_kv_heads=Hkv, max_seq_len=n)
    cache = KVCache(cfg, B, n, dev)
    cache.kv.normal_()
    cache.set_lens([n] * B)
    q = torch.randn(B, Hq * 128, device=dev, dtype=torch.bfloat16)
    q4 = q.view(B, Hq, 1, 128)
    nsplit = args.nsplit or None

    def ours(i):
        return decode_attention(q, cache, i % L, nsplit=nsplit)

    def sdpa(i):
        return Fn.scaled_dot_product_attention(q4, cache.k(i % L), cache.v(i % L), enable_gqa=True)

    diff = (ours(0).float() - sdpa(0).reshape(B, Hq * 128).float()).abs().max().item()

    def window(fn) -> float:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(args.iters):
            fn(i)
        b.record()
        b.synchronize()
        return 1000.0 * a.elapsed_time(b) / args.iters  # us per call

    for fn in (ours, sdpa):  # warm-up: code objects, algorithm choice
        for i in range(2 * L):
            fn(i)
    torch.cuda.synchronize()
    t = {"decode_attn": [], "sdpa": []}
    for _ in range(args.runs):
        t["decode_attn"].append(window(ours))
        t["sdpa"].append(window(sdpa))
    nbytes = 2 * B * n * Hkv * 256
    res = {"kv_len": n, "batch": B, "heads": [Hq, Hkv], "layers_rotated": L, "runs": args.runs,
           "iters": args.iters,
           "nsplit": nsplit or pick_nsplit(B, Hkv, n, torch.cuda.get_device_properties(dev).multi_processor_count),
           "bytes_per_call": nbytes, "max_abs_diff_vs_sdpa": diff}
    for arm, xs in t.items():
        mean = sum(xs) / len(xs)
        res[arm] = {"mean_us": round(mean, 2), "spread_us": round(max(xs) - min(xs), 2),
                    "windows_us": [round(x, 2) for x in xs], "tb_per_s": round(nbytes / mean / 1e6, 3)}
    res["hbm_achievable_tb_per_s"] = HBM_ACHIEVABLE_TBS
    res["not_slower_than_sdpa_within_its_spread"] = (
        res["decode_attn"]["mean_us"] <= res["sdpa"]["mean_us"] + res["sdpa"]["spread_us"])
    print(json.dumps(res), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kv-lens", default="512,4096,8192")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--heads", default="32,8")
    ap.add_argument("--layers", type=int, default=8, help="cache layers the calls rotate over")
    ap.add_argument("--runs", type=int, default=5, help="interleaved windows per arm (at least 4)")
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--nsplit", type=int, default=0, help="0: the wrapper's automatic choice")
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds per child process")
    ap.add_argument("--e2e", action="store_true", help="also run the llama3-8b generate workload")
    ap.add_argument("--e2e-timeout", type=int, default=400)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--child-kv-len", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.hq, args.hkv = (int(x) for x in args.heads.split(","))
    if args.runs < 4:
        ap.error("--runs must be at least 4")
    if args.child_kv_len is not None:
        args.kv_len = args.child_kv_len
        return child(args)

    def run(cmd: list[str], limit: int) -> bool:
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"bench_decode: {' '.join(cmd[1:])} exceeded {limit} s: stopping", file=sys.stderr)
            return False
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        for ln in lines:
            print(ln, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(ln + "\n")
        if r.returncode != 0:
            print(f"bench_decode: {' '.join(cmd[1:])} exited {r.returncode}: stopping\n{r.stderr[-2000:]}",
                  file=sys.stderr)
            return False
        return True

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    base = [sys.executable, str(Path(__file__).resolve()), "--batch", str(args.batch), "--heads", args.heads,
            "--layers", str(args.layers), "--runs", str(args.runs), "--iters", str(args.iters),
            "--nsplit", str(args.nsplit)]
    for n in (int(x) for x in args.kv_lens.split(",")):
        if not run(base + ["--child-kv-len", str(n)], args.step_timeout):
            return 1
    if args.e2e:
        cmd = [sys.executable, "-m", "tensorhive_fixed_amd.workloads.llama3_generate", "--model", "llama3-8b",
               "--batch", "8", "--prompt-len", "512", "--max-new-tokens", "64"]
        if not run(cmd, args.e2e_timeout):
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
