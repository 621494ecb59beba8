#!/usr/bin/env python3
"""Render the tables of profiles/attention_accuracy/README.md from the figures one run of
tests/gpu/test_attention_profiles_gpu.py and tests/gpu/test_flash_tails_gpu.py leaves under
TH_ATTN_ACCURACY_JSON (the tails file adds its figures to the file under "tails").

    TH_ATTN_ACCURACY_JSON=acc.json python -m pytest tests/gpu/test_attention_profiles_gpu.py \\
        tests/gpu/test_flash_tails_gpu.py
    python scripts/attention_accuracy_table.py acc.json
"""
import json
import sys

FLAGS = ("kf_default", "kh", "fused_dkv", "regstage")
PROFILES = ("randn", "ramp_up", "ramp_down", "sink", "step", "mixed_rows", "rising_spikes", "large")


def tails(rec: dict) -> None:
    """Worst ratio to E_b per length, mask and flag set over both profiles and batch entries, and the worst
    share of the lse tolerance over both forwards.  S = 1 has E_b = 0 for o, dq and dk (own bounds): '-'."""
    cells: dict = {}
    for key, vals in rec["flash"].items():
        S, _, mask, flag = key.split("|")[:4]
        cell = cells.setdefault((int(S[1:]), mask), {}).setdefault(flag, {})
        for n, r in vals.items():
            cell[n] = max(cell.get(n, 0.0), r)
    for key, vals in rec["rope"].items():
        S, _, mask, flag = key.split("|")[:4]
        cell = cells.setdefault((int(S[1:]), mask), {}).setdefault("rope " + flag, {})
        for n, r in vals.items():
            cell[n] = max(cell.get(n, 0.0), r)
    lse: dict = {}
    for key, (_, share) in rec["lse"].items():
        S, _, mask = key.split("|")[:3]
        lse[(int(S[1:]), mask)] = max(lse.get((int(S[1:]), mask), 0.0), share)
    bwd = ("kh", "fused_dkv", "regstage")
    rope = ("rope kf_default", "rope kh")

    def show(cell, names):
        return " / ".join(f"{cell[n]:.2f}" if n in cell else "-" for n in names) if cell else ""

    print("| S | mask | o fwd / fwd_regstage | lse (of tolerance) | " + " | ".join(f"{f} dq / dk / dv" for f in bwd)
          + " | " + " | ".join(f"{f} dq / dk" for f in rope) + " |")
    print("|---|---|---|---|" + "---|" * (len(bwd) + len(rope)))
    for (S, mask), row in sorted(cells.items()):
        o = " / ".join(f"{row[f]['o']:.2f}" if "o" in row.get(f, {}) else "-" for f in ("fwd", "fwd_regstage"))
        print(f"| {S} | {mask} | {o} | {lse[(S, mask)]:.2f} | "
              + " | ".join(show(row.get(f), ("dq", "dk", "dv")) for f in bwd) + " | "
              + " | ".join(show(row.get(f), ("dq", "dk")) for f in rope) + " |")
    print()


def main(path: str) -> None:
    rec = json.load(open(path))
    if "tails" in rec:
        tails(rec["tails"])
    if "flash" not in rec:
        return
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
