#!/usr/bin/env python3
"""Column-against-column scans (ScanEngine.scan_columns, `col1 < col2`) against scan2 on the same two columns (`col1 < k AND
col2 >= k`: the same algorithmic bytes; two launches and an intermediate bitmap when the widths differ) and against what a
caller does without either: decompress both columns, compare in torch, pack the bits.  HIP events over back-to-back launches,
every shape warmed, all series of a line interleaved in ONE process.  Writes profiles/r06_scan_columns.txt.

    python tools/bench_columns.py [--out profiles/r06_scan_columns.txt] [--rows 1000000000] [--rounds 5] [--burst 20]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from shared_simd_scan_amd import ScanEngine, lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_scan_columns.txt"))
ap.add_argument("--rows", type=int, default=1_000_000_000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--burst", type=int, default=20)
args = ap.parse_args()
assert args.rounds >= 5 and args.burst >= 1 and args.rows % 8 == 0

eng = ScanEngine(0)
L = lib()
n = args.rows
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def measure(series):
    """series: {name: callable}; alternating rounds of `burst` back-to-back launches -> {name: sorted ms per launch}"""
    times = {k: [] for k in series}
    for fn in series.values():  # every shape warmed
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, fn in series.items():
            fn()
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


def spread(t):
    return (t[-1] - t[0]) / med(t)


def kernels():
    return " + ".join(ln.split(" grid=")[0] for ln in L.mi355_ctx_last_launch(eng._ctx).decode().strip().split("\n"))


def status_quo(col1, col2):
    """decompress both columns, compare, pack the bits -> ms (one timed run after one untimed)"""
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device="cuda")

    def route():
        a, b = eng.decompress(col1), eng.decompress(col2)
        if max(col1.c, col2.c) == 32:  # int32 holds the bit pattern: compare as unsigned
            bits = (a ^ -(1 << 31)) < (b ^ -(1 << 31))
        else:
            bits = a < b
        del a, b
        return (bits.view(-1, 8).to(torch.uint8) * w).sum(1).to(torch.uint8), bits.sum()

    route()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    bm, cnt = route()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), int(cnt.item()), bm


say(f"# column-against-column scans on {torch.cuda.get_device_name(0)}; rows={n} rounds={args.rounds} burst={args.burst}")
say("# ms per launch: median of the rounds [fastest .. slowest]; spread = (slowest - fastest) / median; launches back to back")
say("# columns: col1 < col2 (scan_columns '<', a = 0).  scan2: col1 < k AND col2 >= k on the same columns, same build, same process")
say("# TB/s: algorithmic bytes n*c1/8 + n*c2/8 (+ n/8 bitmap) (+ n/8 mask) over the columns median")
say("# status quo: decompress both columns to int32, torch compare, pack the bits; one timed run")
say()

gate = None
for c1, c2 in ((9, 9), (12, 12), (9, 12), (12, 9), (17, 21), (32, 32)):
    col1 = eng.generate("splitmix", n, c1, 42)
    col2 = eng.generate("splitmix", n, c2, 4242)
    bm, bm2 = eng.alloc_bitmap(n), eng.alloc_bitmap(n)
    hits, hits2 = (torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(2))
    k1, k2 = 1 << (c1 - 1), 1 << (c2 - 1)
    variants = [("bitmap+hits", False, None), ("count-only", True, None)]
    if (c1, c2) == (9, 9):
        variants.append(("bitmap+hits, AND-mask", False, eng.scan_where("<", 300, col1)[0]))
    for name, count_only, mask in variants:
        cols = lambda: eng.scan_columns(col1, "<", col2, mask=mask, bitmap=bm, hits=hits, count_only=count_only)  # noqa: E731
        two = lambda: eng.scan2(col1, "<", k1, col2, ">=", k2, bitmap=bm2, hits=hits2, count_only=count_only)  # noqa: E731
        cols()
        k_cols = kernels()
        two()
        k_two = kernels()
        t = measure({"scan2_a": two, "columns": cols, "scan2_b": two})
        s2 = sorted(t["scan2_a"] + t["scan2_b"])
        nbytes = n * c1 / 8 + n * c2 / 8 + (0 if count_only else n / 8) + (n / 8 if mask is not None else 0)
        tc = t["columns"]
        say(f"({c1:2d},{c2:2d}) {name:22s} columns {med(tc):.4f} ms [{tc[0]:.4f} .. {tc[-1]:.4f}] spread {100 * spread(tc):.1f}%  "
            f"{nbytes / med(tc) / 1e9:.2f} TB/s | scan2{'' if mask is None else ' (no mask)'} {med(s2):.4f} ms [{s2[0]:.4f} .. {s2[-1]:.4f}] "
            f"spread {100 * spread(s2):.1f}% | columns / scan2 {med(tc) / med(s2):.3f}")
        say(f"        columns: {k_cols}   scan2: {k_two}   hits {int(hits.item())}")
        if (c1, c2) == (9, 9) and name == "bitmap+hits":
            gate = (med(tc), med(s2), max(spread(tc), spread(s2)))
    del bm2, mask, variants
    ms, cnt, ref = status_quo(col1, col2)
    eng.scan_columns(col1, "<", col2, bitmap=bm, hits=hits)
    same = bool(torch.equal(ref, bm)) and cnt == int(hits.item())
    say(f"({c1:2d},{c2:2d}) status quo             {ms:.3f} ms   (its bitmap and count {'equal' if same else 'DIFFER FROM'} scan_columns')")
    say()
    del col1, col2, bm, ref
    torch.cuda.empty_cache()

if gate:
    c, s, sp = gate
    margin = max(0.05, sp)
    say(f"# target (9,9) bitmap+hits: columns median <= (1 + margin) x scan2 median, margin = max(5%, round-to-round spread) = {100 * margin:.1f}%: "
        f"{c:.4f} vs {s:.4f} ms, ratio {c / s:.3f}: {'MET' if c <= (1 + margin) * s else 'MISSED'}")

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
