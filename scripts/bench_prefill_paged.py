#!/usr/bin/env python
"""Chunk attention through a page table (csrc/chunk_attn.hip's paged kernels, ops/paged_chunk_attention.py) against
the dense call on the same rows, and ``generate(paged_kv=True, shared_prefix=N)`` against ``paged_kv`` alone.

    python scripts/bench_prefill_paged.py [--parts attn,e2e] [--runs 5] [--iters 20] [--out FILE]

The method is that of ``scripts/bench_prefill_chunk.py``: the parent never touches the GPU, every part is a child
process under its own time limit, the first child that fails ends the script, and in a child the arms alternate
(window 0 warms up, ``--runs`` windows each are kept).  One JSON line per measurement:

* ``attn``: 32/8 heads; one call of T tokens on ``old`` rows per sequence: ``chunk_attention`` on a dense cache
  (``dense``; the dense kernels are instruction for instruction those of the commit before the paged ones, see
  profiles/prefill_paged/README.md) against ``paged_chunk_attention`` on a pool with the same number of rows,
  through an identity table (``identity``) and a randomly permuted one (``permuted``), at the ``nsplit`` the rule
  picks for the call.  Device events around ``--iters`` rounds; the calls rotate over cache layers.
* ``e2e``: Llama-3-8B shapes, random weights, B 8, prompts of 4096 tokens that share their first 3584:
  ``generate(max_new_tokens=1, paged_kv=True)`` with and without ``shared_prefix=3584``, with the pages each holds.
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
SHAPES = ((8, 512, 3584), (1, 64, 8192), (1, 128, 8192))  # (batch, chunk, old rows)


def _stats(xs: list[float], nd: int = 4) -> dict:
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], nd), "spread": round(xs[-1] - xs[0], nd), "windows": [round(x, nd) for x in xs]}


def child_attn(args) -> int:
    import torch

    from tensorhive_fixed_amd.models.llama3 import LlamaConfig
    from tensorhive_fixed_amd.ops.chunk_attention import chunk_attention, pick_chunk_nsplit
    from tensorhive_fixed_amd.ops.decode_attention import KVCache
    from tensorhive_fixed_amd.ops.paged_attention import PagedKVCache, pages_for
    from tensorhive_fixed_amd.ops.paged_chunk_attention import paged_chunk_attention

    dev = torch.device("cuda")
    Hq, Hkv = 32, 8
    B, T, old = SHAPES[args.child_shape]
    smax = old + T
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    L = max(4, min(32, (1 << 30) // (2 * B * Hkv * smax * 256)))  # about 1 GiB of K/V under the rotation, per cache
    cfg = LlamaConfig(dim=Hq * 128, n_layers=L, n_heads=Hq, n_kv_heads=Hkv, max_seq_len=smax)
    dense = KVCache(cfg, B, smax, dev)
    dense.kv.normal_()
    dense.set_lens([old] * B)
    pools = {}
    for name in ("identity", "permuted"):
        c = PagedKVCache(cfg, B, smax, B * pages_for(smax), dev)
        c.pool.normal_()
        if name == "permuted":
            order = torch.randperm(c.n_pages, generator=torch.Generator().manual_seed(0)).tolist()
            c.free_pages = order
        for b in range(B):
            c.reserve(b, smax)
        c.fill(0, dense.k(0), dense.v(0))  # layer 0 holds the dense rows: the outputs there must be equal
        c.set_lens([old] * B)
        pools[name] = c
    q = torch.randn(B, T, Hq * 128, device=dev, dtype=torch.bfloat16)
    new = [T] * B
    new_dev = torch.tensor(new, dtype=torch.int32, device=dev)
    nsplit = pick_chunk_nsplit(B, Hkv, Hq // Hkv, T, smax, cus)
    arms = {"dense": lambda i: chunk_attention(q, dense, i % L, new, new_dev, nsplit=nsplit)}
    for name, c in pools.items():
        arms[name] = lambda i, c=c: paged_chunk_attention(q, c, i % L, new, new_dev, nsplit=nsplit)

    def window(fn, iters) -> float:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(iters):
            fn(i)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / iters  # ms per call

    same = all(torch.equal(arms["dense"](0), arms[k](0)) for k in pools)
    t = {k: [] for k in arms}
    for r in range(args.runs + 1):  # window 0 warms up
        for k, fn in arms.items():
            torch.cuda.synchronize()
            x = window(fn, args.iters if r else 2)
            if r:
                t[k].append(x)
    res = {"bench": "attn", "batch": B, "heads": [Hq, Hkv], "chunk": T, "old_rows": old, "nsplit": nsplit,
           "layers_rotated": L, "runs": args.runs, "iters": args.iters, "bits_equal_dense": bool(same),
           **{k + "_ms": _stats(v) for k, v in t.items()}}
    for k in pools:
        res[f"ratio_{k}"] = round(res[k + "_ms"]["median"] / res["dense_ms"]["median"], 3)
    print(json.dumps(res), flush=True)
    return 0


def child_e2e(args) -> int:
    import torch

    from tensorhive_fixed_amd.models.llama3 import Llama, LlamaConfig
    from tensorhive_fixed_amd.ops.paged_attention import pages_for

    dev = torch.device("cuda")
    B, S, N = 8, 4096, 3584
    model = Llama(LlamaConfig.named("llama3-8b"), device=dev, dtype=torch.bfloat16, seed=0)
    tok = torch.randint(0, model.cfg.vocab_size, (B, S), device=dev)
    tok[:, :N] = tok[:1, :N]
    arms = {"paged": None, "shared_prefix": N}
    t = {k: [] for k in arms}
    for r in range(args.runs + 1):  # window 0 warms up
        for k, n in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.generate(tok, max_new_tokens=1, paged_kv=True, shared_prefix=n)
            torch.cuda.synchronize()
            if r:
                t[k].append(1000.0 * (time.perf_counter() - t0))
    P = N // 64 * 64
    pages = {"paged": B * pages_for(S + 1), "shared_prefix": pages_for(P) + B * pages_for(S + 1 - P)}
    print(json.dumps({"bench": "e2e", "model": "llama3-8b", "batch": B, "prompt": S, "shared_prefix": N,
                      "runs": args.runs, **{k + "_ms": _stats(v, 2) for k, v in t.items()},
                      **{k + "_pages": v for k, v in pages.items()}, "prefix_pages": pages_for(P),
                      "prefix_share_of_pool": round(pages_for(P) / pages["shared_prefix"], 3),
                      "ratio": round(_stats(t["shared_prefix"])["median"] / _stats(t["paged"])["median"], 4)}),
          flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parts", default="attn,e2e")
    ap.add_argument("--runs", type=int, default=5, help="interleaved windows per arm")
    ap.add_argument("--iters", type=int, default=20, help="attention calls per window")
    ap.add_argument("--attn-timeout", type=int, default=120, help="seconds per attention child")
    ap.add_argument("--model-timeout", type=int, default=300, help="seconds for the model child")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-shape", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        sys.path.insert(0, str(ROOT))
        import torch

        if not torch.cuda.is_available():
            print("bench_prefill_paged: no GPU", file=sys.stderr)
            return 3
        return {"attn": child_attn, "e2e": child_e2e}[args.child](args)

    def run(extra: list[str], limit: int) -> bool:
        cmd = [sys.executable, str(Path(__file__).resolve()), "--runs", str(args.runs), "--iters", str(args.iters)] + extra
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"bench_prefill_paged: {' '.join(extra)} exceeded {limit} s: stopping", file=sys.stderr)
            return False
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        for ln in lines:
            print(ln, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(ln + "\n")
        if r.returncode != 0 or not lines:
            print(f"bench_prefill_paged: {' '.join(extra)} exited {r.returncode}: stopping\n{r.stderr[-2000:]}",
                  file=sys.stderr)
            return False
        return True

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    parts = args.parts.split(",")
    if "attn" in parts:
        for i in range(len(SHAPES)):
            if not run(["--child", "attn", "--child-shape", str(i)], args.attn_timeout):
                return 1
    if "e2e" in parts and not run(["--child", "e2e"], args.model_timeout):
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
