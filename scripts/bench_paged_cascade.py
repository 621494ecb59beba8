#!/usr/bin/env python
"""Cascade decode attention (csrc/paged_cascade_attn.hip) against ``paged_decode_attention``
(csrc/paged_attn.hip, unchanged: the yardstick) on the same paged cache with a shared prefix.

    python scripts/bench_paged_cascade.py [--kv-len 4096] [--shared 3584,64] [--batch 8] [--heads 32,8]
                                          [--runs 5] [--iters 1000] [--e2e] [--out FILE]

The parent process never touches the GPU: every setting is a child process under its own time limit, and
the first child that fails ends the script.  In a child the two arms alternate (``--runs`` windows each,
device events around ``--iters`` calls) on one ``PagedKVCache`` whose sequences share the pages of their
first ``shared`` rows through a permuted table.  Calls rotate over ``--layers`` cache layers so that no
call finds its K/V in the last-level cache from the call before (inside a call the per-sequence arm does
re-read the shared pages once per sequence, which the caches may serve: that is the yardstick as it runs).
One JSON line per setting: mean and spread (max - min over the windows) of every arm in microseconds per
call, the ratio cascade / paged per window pair, the largest difference between the two outputs, the split
counts, and the K/V bytes each arm asks for, counted from shapes: ``2 * Hkv * 256 B`` times ``sum(kv_len)``
rows for the paged arm and times ``shared + sum(kv_len - shared)`` rows for cascade.

``--e2e`` then runs ``llama3_generate --paged-kv --shared-prefix S`` for the first ``S`` of ``--shared``, without
and with ``--cascade-decode``, two alternating runs each, and prints their JSON lines tagged with ``arm``.
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
    from tensorhive_fixed_amd.ops.decode_attention import pick_nsplit
    from tensorhive_fixed_amd.ops.paged_attention import PagedKVCache, paged_decode_attention, pages_for
    from tensorhive_fixed_amd.ops.paged_cascade_attention import paged_cascade_decode_attention, pick_prefix_splits

    if not torch.cuda.is_available():
        print("bench_paged_cascade: no GPU", file=sys.stderr)
        return 3
    dev = torch.device("cuda")
    Hq, Hkv, L, B, n, P = args.hq, args.hkv, args.layers, args.batch, args.kv_len, args.child_shared
    cfg = LlamaConfig(dim=Hq * 128, n_layers=L, n_heads=Hq, n_kv_heads=Hkv, max_seq_len=n)
    n_pages = pages_for(P) + B * (pages_for(n) - pages_for(P))
    cache = PagedKVCache(cfg, B, n, n_pages, dev)
    cache.pool.normal_()
    cache.free_pages = list(range(0, n_pages, 2)) + list(range(1, n_pages, 2))
    cache.reserve(0, n)
    cache.set_lens([n] + [0] * (B - 1))
    for b in range(1, B):
        cache.share_prefix(0, b, P)
        cache.reserve(b, n)
    cache.set_lens([n] * B)
    q = torch.randn(B, Hq * 128, device=dev, dtype=torch.bfloat16)
    arms = {"paged": lambda i: paged_decode_attention(q, cache, i % L),
            "cascade": lambda i: paged_cascade_decode_attention(q, cache, i % L, P)}
    diff = (arms["cascade"](0).float() - arms["paged"](0).float()).abs().max().item()

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
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    row_bytes = 2 * Hkv * 256
    nbytes = {"paged": B * n * row_bytes, "cascade": (P + B * (n - P)) * row_bytes}
    res = {"bench": "op", "kv_len": n, "shared": P, "batch": B, "heads": [Hq, Hkv], "layers_rotated": L,
           "runs": args.runs, "iters": args.iters, "nsplit_paged": pick_nsplit(B, Hkv, n, cus),
           "prefix_splits": pick_prefix_splits(B * (Hq // Hkv), Hkv, P // 64, cus),
           "nsplit_suffix": pick_nsplit(B, Hkv, n - P, cus), "max_abs_diff_cascade_vs_paged": diff}
    for a, xs in t.items():
        mean = sum(xs) / len(xs)
        res[a] = {"mean_us": round(mean, 2), "spread_us": round(max(xs) - min(xs), 2),
                  "windows_us": [round(x, 2) for x in xs], "bytes_per_call": nbytes[a],
                  "tb_per_s": round(nbytes[a] / mean / 1e6, 3)}
    r = [x / y for x, y in zip(t["cascade"], t["paged"])]
    res["cascade"]["ratio_to_paged"] = {"mean": round(sum(r) / len(r), 4), "min": round(min(r), 4),
                                        "max": round(max(r), 4)}
    print(json.dumps(res), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kv-len", type=int, default=4096)
    ap.add_argument("--shared", default="3584,64", help="shared rows (whole pages), one setting each")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--heads", default="32,8")
    ap.add_argument("--layers", type=int, default=16, help="cache layers the calls rotate over")
    ap.add_argument("--runs", type=int, default=5, help="interleaved windows per arm (at least 4)")
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds per child process")
    ap.add_argument("--e2e", action="store_true", help="also time llama3_generate with and without --cascade-decode")
    ap.add_argument("--e2e-new-tokens", type=int, default=64)
    ap.add_argument("--e2e-timeout", type=int, default=240, help="seconds per llama3_generate run")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--child-shared", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.hq, args.hkv = (int(x) for x in args.heads.split(","))
    if args.runs < 4:
        ap.error("--runs must be at least 4")
    if args.child_shared is not None:
        return child(args)
    shared = [int(x) for x in args.shared.split(",") if x]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def run(what: str, cmd: list[str], limit: int, tag: dict) -> bool:
        """One child under its time limit; its JSON lines are printed (and kept) with ``tag`` added."""
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"bench_paged_cascade: {what} exceeded {limit} s: stopping", file=sys.stderr)
            return False
        for ln in (x for x in r.stdout.splitlines() if x.startswith("{")):
            ln = json.dumps({**tag, **json.loads(ln)})
            print(ln, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(ln + "\n")
        if r.returncode != 0:
            print(f"bench_paged_cascade: {what} exited {r.returncode}: stopping\n{r.stderr[-2000:]}", file=sys.stderr)
        return r.returncode == 0

    for P in shared:
        cmd = [sys.executable, str(Path(__file__).resolve()), "--kv-len", str(args.kv_len), "--batch", str(args.batch),
               "--heads", args.heads, "--layers", str(args.layers), "--runs", str(args.runs), "--iters", str(args.iters),
               "--child-shared", str(P)]
        if not run(f"shared {P}", cmd, args.step_timeout, {}):
            return 1
    if args.e2e:
        S = shared[0]
        gen = [sys.executable, "-m", "tensorhive_fixed_amd.workloads.llama3_generate", "--batch", str(args.batch),
               "--prompt-len", str(args.kv_len - args.e2e_new_tokens), "--max-new-tokens", str(args.e2e_new_tokens),
               "--stream-gemm", "--paged-kv", "--shared-prefix", str(S), "--log-every", "1000"]
        for i in range(2):  # alternating: paged, cascade, paged, cascade
            for arm, extra in (("paged", []), ("cascade", ["--cascade-decode"])):
                if not run(f"llama3_generate {arm} run {i}", gen + extra, args.e2e_timeout,
                           {"bench": "e2e", "arm": arm, "run": i}):
                    return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
