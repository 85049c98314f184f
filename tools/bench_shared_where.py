#!/usr/bin/env python3
"""Shared scans over range predicates (ScanEngine.shared_scan_where) against the equality shared scan and against P
single-predicate launches: HIP events over back-to-back launches after a warm-up, all series of a comparison interleaved
in ONE process (the way tools/ab_opts.py does).  Writes profiles/r04_shared_where.txt.

    python tools/bench_shared_where.py [--out profiles/r04_shared_where.txt] [--rounds 5] [--burst 20] [--scale 1.0]

Column shapes: the README's -- 1e9 x c bit for P <= 8, 2.5e8 x c bit for larger P, random column (splitmix); ranges of
about 1/8 selectivity; hit counts on.  --scale shrinks the row counts (smoke runs on a busy box)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from shared_simd_scan_amd import ScanEngine, lib  # noqa: E402
from shared_simd_scan_amd.engine import shared_where_kernel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r04_shared_where.txt"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--burst", type=int, default=20)
ap.add_argument("--scale", type=float, default=1.0)
args = ap.parse_args()

eng = ScanEngine(0)
L = lib()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def rows_for(P):
    return int((1e9 if P <= 8 else 2.5e8) * args.scale)


def ranges(c, P, seed):
    """P ranges of about 1/8 selectivity on a uniform column"""
    rng = np.random.default_rng(seed)
    width = max((1 << c) // 8, 1)
    los = rng.integers(0, (1 << c) - width + 1, size=P)
    return [("between", int(lo), int(lo) + width - 1) for lo in los]


def measure(series):
    """series: {name: callable}; interleaved rounds of `burst` back-to-back launches -> {name: sorted ms per launch}"""
    times = {k: [] for k in series}
    for _ in range(args.rounds):
        for name, fn in series.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.burst):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.burst)
    return {k: sorted(v) for k, v in times.items()}


def med(t):
    return t[len(t) // 2]


def out_buffer(n, P, layout):
    nb = (n + 7) // 8
    shape = (P, (nb + 255) // 256 * 256) if layout == "per_predicate" else (nb * P,)
    return torch.empty(shape, dtype=torch.uint8, device="cuda")


def last_kernel():
    return L.mi355_ctx_last_launch(eng._ctx).decode().strip().split(" grid=")[0]


say(f"# shared where-scans on {torch.cuda.get_device_name(0)}; rounds={args.rounds} burst={args.burst} scale={args.scale}; ms per launch, median of the rounds")
say()
say("## 1. table kernel against the equality shared scan at the same (c, P, layout)")
say("# eq_a / eq_b: the SAME equality scan measured twice, interleaved with each other and with the where-scan: their spread is the")
say("# noise of the box.  small: one launch over one tile per wave (the prologue, the launch and one tile), where-scan / equality scan.")
say("# (small includes the host's enqueue time where that is longer than the kernel.)  allowed: where <= max(eq_a, eq_b) + |eq_a - eq_b| + small(where).")
for c in (9, 12, 16):
    for P in (8, 64):
        n = rows_for(P)
        col = eng.generate("splitmix", n, c, 42)
        n_small = 256 * 2 * 4 * 4096  # one 64 x 64-value tile for every wave of a two-blocks-per-CU grid
        col_small = eng.slice_rows(col, 0, min(n_small, n))
        hits = torch.zeros(P, dtype=torch.int64, device="cuda")
        keys = [(37 * k + 3) % (1 << c) for k in range(P)]
        preds = ranges(c, P, 100 * c + P)
        for layout in ("per_predicate", "linear"):
            out = out_buffer(n, P, layout)
            eq = lambda: eng.shared_scan(keys, col, layout=layout, out=out, hits=hits)  # noqa: E731
            wh = lambda: eng.shared_scan_where(preds, col, layout=layout, out=out, hits=hits)  # noqa: E731
            eq_s = lambda: eng.shared_scan(keys, col_small, layout=layout, out=out, hits=hits)  # noqa: E731
            wh_s = lambda: eng.shared_scan_where(preds, col_small, layout=layout, out=out, hits=hits)  # noqa: E731
            eq()
            k_eq = last_kernel()
            wh()
            k_wh = last_kernel()
            t = measure({"eq_a": eq, "where": wh, "eq_b": eq})
            s = measure({"eq_small": eq_s, "where_small": wh_s})
            a, b, w = med(t["eq_a"]), med(t["eq_b"]), med(t["where"])
            spread = abs(a - b)
            allowed = max(a, b) + spread + med(s["where_small"])
            table = shared_where_kernel(c, P, layout).startswith("shared_where_lut")
            verdict = ("within" if w <= allowed else "SLOWER than allowed") if table else "compare chain (tables do not fit): recorded, not judged"
            say(f"c={c:2d} P={P:3d} {layout:13s} n={n:.1e}  eq_a {a:.4f}  eq_b {b:.4f}  where {w:.4f}  ratio {w / min(a, b):.3f}  spread {spread:.4f}"
                f"  small {med(s['where_small']):.4f} / {med(s['eq_small']):.4f}  allowed {allowed:.4f}  {verdict}")
            say(f"      equality: {k_eq}   where: {k_wh}")
            del out
        if P > 8 and shared_where_kernel(c, P, "linear", False).startswith("shared_where_lut"):
            # like for like: at P > 8 the equality scan above runs its dword-entry kernels (32 keys per lookup), which ranges do not
            # have yet.  Its byte-entry multi-pass kernel -- the organisation of the where-scan -- still runs linear rows without hit
            # counts when option kernel_flags = 2 keeps the row-per-lane kernels out: the same tile loop on both sides.
            out = out_buffer(n, P, "linear")
            eng.set_option("kernel_flags", 2)
            eq = lambda: eng.shared_scan(keys, col, layout="linear", out=out, hits=False)  # noqa: E731
            wh = lambda: eng.shared_scan_where(preds, col, layout="linear", out=out, hits=False)  # noqa: E731
            eq_s = lambda: eng.shared_scan(keys, col_small, layout="linear", out=out, hits=False)  # noqa: E731
            wh_s = lambda: eng.shared_scan_where(preds, col_small, layout="linear", out=out, hits=False)  # noqa: E731
            eq()
            k_eq = last_kernel()
            wh()
            k_wh = last_kernel()
            t = measure({"eq_a": eq, "where": wh, "eq_b": eq})
            s = measure({"eq_small": eq_s, "where_small": wh_s})
            eng.set_option("kernel_flags", 0)
            a, b, w = med(t["eq_a"]), med(t["eq_b"]), med(t["where"])
            allowed = max(a, b) + abs(a - b) + med(s["where_small"])
            say(f"c={c:2d} P={P:3d} linear, no hits, byte tables on both sides n={n:.1e}  eq_a {a:.4f}  eq_b {b:.4f}  where {w:.4f}  ratio {w / min(a, b):.3f}"
                f"  spread {abs(a - b):.4f}  small {med(s['where_small']):.4f} / {med(s['eq_small']):.4f}  allowed {allowed:.4f}  {'within' if w <= allowed else 'SLOWER than allowed'}")
            say(f"      equality: {k_eq}   where: {k_wh}")
            del out
        del col, col_small
        torch.cuda.empty_cache()

say()
say("## 2. against what a caller does without the shared call: P launches of scan_where, each reading the column again")
say("# ratio = time of the chain of P launches / time of the one shared call (above 1: the shared call pays)")
for c in (9, 17, 21):
    for P in (2, 4, 8, 64):
        n = rows_for(P)
        col = eng.generate("splitmix", n, c, 42)
        preds = ranges(c, P, 7 * c + P)
        out = out_buffer(n, P, "per_predicate")
        hits = torch.zeros(P, dtype=torch.int64, device="cuda")
        hit1 = [hits[k:k + 1] for k in range(P)]

        def chain():
            for k, (_, lo, hi) in enumerate(preds):
                eng.scan_where("between", lo, col, b=hi, bitmap=out[k], hits=hit1[k])

        shared = lambda: eng.shared_scan_where(preds, col, out=out, hits=hits)  # noqa: E731
        shared()
        k_wh = last_kernel()
        t = measure({"chain": chain, "shared": shared})
        ch, sh = med(t["chain"]), med(t["shared"])
        say(f"c={c:2d} P={P:3d} n={n:.1e}  {P} launches {ch:.4f}  shared {sh:.4f}  ratio {ch / sh:.2f}  ({n * P / sh / 1e9:.0f} G value-predicates/s)  {k_wh}")
        del col, out
        torch.cuda.empty_cache()

with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
