#!/usr/bin/env python3
"""lookup (ScanEngine.lookup: a packed column mapped through a device-resident packed table) in both tiers, against the route a
caller had without the call -- decompress the column, torch index into the decoded table, re-pack -- and as the first half of
the chain lookup -> group_aggregate.  HIP events over back-to-back launches, every shape warmed, all series of a case
interleaved in ONE process.  Writes profiles/r09_lookup.txt.

    python tools/bench_lookup.py [--out profiles/r09_lookup.txt] [--scale 1.0] [--rounds 5] [--burst 20]

Shapes (rows times --scale): 1e9 rows x 12 bit through a table of 2^12 rows x 8 bit (the LDS tier); 2.5e8 rows x 24 bit through
a table of 2^24 rows x 8 bit (the global tier).  The keys are uniform over the table's rows, the table's entries uniform over
[0, 2^ct): every row hits, so the route needs no bound check.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from shared_simd_scan_amd import ScanEngine, lib, lookup_kernel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_lookup.txt"))
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--burst", type=int, default=20)
args = ap.parse_args()
assert args.rounds >= 3 and args.burst >= 1

eng = ScanEngine(0)
L = lib()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def measure(series):
    """series: {name: (callable, burst)}; alternating rounds of `burst` back-to-back calls -> {name: sorted ms per call}"""
    times = {k: [] for k in series}
    for fn, _ in series.values():  # every shape warmed
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, (fn, burst) in series.items():
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(burst):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / burst)
    return {k: sorted(v) for k, v in times.items()}


def med(t):
    return t[len(t) // 2]


def fmt(t):
    return f"{med(t):.4f} ms [{t[0]:.4f} .. {t[-1]:.4f}]"


def kernel():
    ln = L.mi355_ctx_last_launch(eng._ctx).decode().strip().split("\n")[-1]
    return ln.split(" flags=")[0]


say(f"# lookup on {torch.cuda.get_device_name(0)}; scale={args.scale} rounds={args.rounds} burst={args.burst}")
say("# ms per call: median of the rounds [fastest .. slowest]; calls back to back; GB/s: the column's bytes n*c/8 + the result's n*ct/8 over the median")
say("# route without the call: decompress -> torch.index_select on the decoded table (int32) -> pack_u32_dev; it moves at least n*(c + 4*32 + ct)/8 bytes")
say("# chain: lookup -> group_aggregate(keys = the looked-up column, values = a 17-bit column); group_aggregate alone: on the looked-up column")
say()

N12, N24 = int(1_000_000_000 * args.scale) // 2048 * 2048, int(250_000_000 * args.scale) // 2048 * 2048
# (rows, c, log2 of the table's rows, ct)
CASES = [(N12, 12, 12, 8), (N24, 24, 24, 8)]
for n, c, lt, ct in CASES:
    T = 1 << lt
    col = eng.generate("splitmix", n, c, 42)  # uniform over [0, 2^c) = the table's rows
    entries = torch.randint(0, 1 << ct, (T,), dtype=torch.int32, device="cuda")
    table = eng.compress(entries, ct)
    out = eng.alloc_packed(n, ct)
    values = eng.generate("splitmix", n, 17, 7)
    agg = torch.empty((1 << ct, 4), dtype=torch.int64, device="cuda")
    dec = torch.empty(n, dtype=torch.int32, device="cuda")
    tier = lookup_kernel(c, T, ct)

    def look():
        return eng.lookup(col, table, out=out.data)

    def route():
        eng.decompress(col, out=dec)
        return eng.compress(torch.index_select(entries, 0, dec), ct)

    def group():
        eng.group_aggregate(out, values, out=agg)

    def chain():
        eng.group_aggregate(look(), values, out=agg)

    look()
    k = kernel()
    slow = max(1, args.burst // 10)
    t = measure({"lookup": (look, args.burst), "route": (route, slow), "group_aggregate": (group, args.burst), "chain": (chain, args.burst)})
    tl = t["lookup"]
    moved = n * c / 8 + n * ct / 8
    say(f"{n} rows x {c} bit through a table of 2^{lt} rows x {ct} bit, {tier}")
    say(f"    lookup {fmt(tl)}  {moved / med(tl) / 1e6:.0f} GB/s ({(c + ct) / 8:.3f} bytes a row)   {k}")
    say(f"    route without the call {fmt(t['route'])} | route / lookup {med(t['route']) / med(tl):.1f}"
        f"   {n * (c + 4 * 32 + ct) / 8 / med(t['route']) / 1e6:.0f} GB/s of its least traffic")
    say(f"    group_aggregate alone {fmt(t['group_aggregate'])}")
    say(f"    chain lookup -> group_aggregate {fmt(t['chain'])} | chain / (lookup + group_aggregate) {med(t['chain']) / (med(tl) + med(t['group_aggregate'])):.3f}")
    look()
    nb = (n * ct + 7) // 8
    say(f"    results {'agree' if torch.equal(out.data[:nb], route().data[:nb]) else 'DIFFER'} with the route")
    say()
    del col, entries, table, out, values, dec
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
