#!/usr/bin/env python3
"""The scan when its column is NOT hot: two columns scanned alternately, launches back to back, so that whatever one scan
leaves in the Infinity Cache (option "llc_resident_mib") is evicted by the other before it is used again.

    python tools/alt_columns.py [--rows 1e9] [--bits 9] [--steps 50] [--warmup 10] [--one-bitmap] [--pattern abab|aabb] [--opt llc_resident_mib=0]
prints one JSON line; ms_per_step is the time of ONE scan (a step is one round of the pattern: its time / its length).
--pattern aabb: every column is scanned twice before the other one's turn -- auto's worst case: each second scan is a repeat
and fills the cache with default-policy loads that no third scan comes to use.
--one-bitmap: both scans write the same bitmap (default: each column has its own, which doubles the bitmap bytes that
compete for the cache)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from shared_simd_scan_amd import ScanEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=float, default=1e9)
ap.add_argument("--bits", type=int, default=9)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--one-bitmap", action="store_true")
ap.add_argument("--pattern", default="abab", choices=["abab", "aabb"])
ap.add_argument("--opt", default="", help="name=value[,name=value]")
args = ap.parse_args()

eng = ScanEngine(0)
for kv in filter(None, args.opt.split(",")):
    k, v = kv.split("=")
    eng.set_option(k, int(v))
n, c = int(args.rows), args.bits
cols = [eng.generate("splitmix", n, c, 42 + i) for i in range(2)]
bms = [eng.alloc_bitmap(n) for _ in range(1 if args.one_bitmap else 2)]
hits = torch.zeros(1, dtype=torch.int64, device="cuda")


order = [0, 1] if args.pattern == "abab" else [0, 0, 1, 1]


def pair():
    for i in order:
        eng.scan(3, cols[i], bitmap=bms[i % len(bms)], hits=hits)


times = []
for _ in range(args.rounds):
    for _ in range(args.warmup):
        pair()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        pair()
    e1.record()
    e1.synchronize()
    times.append(e0.elapsed_time(e1) / args.steps / len(order))
times.sort()
print(json.dumps({"workload": "scan_eq, two columns, order " + args.pattern, "rows": n, "bits": c, "bitmaps": len(bms), "opt": args.opt,
                  "ms_per_step": round(times[len(times) // 2], 5), "rounds_ms": [round(t, 5) for t in times]}))
