#!/usr/bin/env python3
"""Render the tables of profiles/attention_accuracy/README.md from the figures one run of
tests/gpu/test_attention_profiles_gpu.py leaves under TH_ATTN_ACCURACY_JSON.

    TH_ATTN_ACCURACY_JSON=acc.json python -m pytest tests/gpu/test_attention_profiles_gpu.py
    python scripts/attention_accuracy_table.py acc.json
"""
import json
import sys

FLAGS = ("kf_default", "kh", "fused_dkv", "regstage")
PROFILES = ("randn", "ramp_up", "ramp_down", "sink", "step", "mixed_rows", "rising_spikes", "large")


def main(path: str) -> None:
    rec = json.load(open(path))
    flash: dict = {}
    for key, vals in rec["flash"].items():  # the same profile in batch slot 0 and 1 of a shape: keep the worse
        profile, shape, mask, flag = key.split("|")[:4]
        cell = flash.setdefault((profile, shape, mask), {}).setdefault(flag, {})
        for n, r in vals.items():
            cell[n] = max(cell.get(n, 0.0), r)
    lse: dict = {}
    for key, vals in rec["lse"].items():
        k3 = tuple(key.split("|")[:3])
        lse[k3] = [max(a, b) for a, b in zip(lse.get(k3, [0.0, 0.0, 0.0]), vals)]
    rank = {p: i for i, p in enumerate(PROFILES)}
    order = sorted(flash, key=lambda k3: (rank[k3[0]], k3[1], k3[2]))
    print("| profile | shape | mask | o | lse err (of tolerance; of plain form) | "
          + " | ".join(f"{f} dq / dk / dv" for f in FLAGS) + " |")
    print("|---|---|---|---|---|" + "---|" * len(FLAGS))
    for k3 in order:
        row = flash[k3]
        e, r, p = lse[k3]
        cells = [" / ".join(f"{row[f][n]:.2f}" for n in ("dq", "dk", "dv")) for f in FLAGS]
        print(f"| {k3[0]} | {k3[1]} | {k3[2]} | {row['fwd']['o']:.2f} | {e:.1e} ({r:.2f}; {p:.2f}) | " + " | ".join(cells) + " |")
    print()
    print("| `large` case | max abs(rowsum(P) - 1) |")
    print("|---|---|")
    for key, v in rec["rowsum_large"].items():
        print(f"| {' '.join(key.split('|')[1:3] + key.split('|')[4:])} | {v:.4f} |")
    print()
    dec: dict = {}
    for key, (err, rel) in rec["decode"].items():
        profile, heads, _ = key.split("|")
        a = dec.setdefault((profile, heads), [0.0, 0.0])
        a[0], a[1] = max(a[0], err), max(a[1], rel)
    print("| decode profile | Hq/Hkv | worst row max-abs (limit 2e-2) | worst row relative (limit 1e-2) |")
    print("|---|---|---|---|")
    for (profile, heads), (err, rel) in sorted(dec.items(), key=lambda kv: (rank[kv[0][0]], kv[0][1])):
        print(f"| {profile} | {heads} | {err:.2e} | {rel:.2e} |")


if __name__ == "__main__":
    main(sys.argv[1])
