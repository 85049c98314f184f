#!/usr/bin/env python3
"""Grouped aggregates (ScanEngine.group_aggregate: sum, count, min, max of one packed column per value of another) against
what a caller does without the call -- per group one scan_where(keys == g [AND mask]) and one aggregate(values, bitmap): 2 G
launches that read both columns G times -- and against two floors on the same data: histogram(keys), one LDS atomic per row,
and a trivial read of the two columns' bytes (torch sums over the buffers).  HIP events over back-to-back launches, every shape
warmed, all series of a case interleaved in ONE process.  Writes profiles/r07_group_aggregate.txt.

    python tools/bench_group_aggregate.py [--out profiles/r07_group_aggregate.txt] [--rows 1000000000] [--rounds 5] [--burst 20]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from shared_simd_scan_amd import ScanEngine, lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_group_aggregate.txt"))
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


def spread(t):
    return (t[-1] - t[0]) / med(t)


def fmt(t):
    return f"{med(t):.4f} ms [{t[0]:.4f} .. {t[-1]:.4f}] spread {100 * spread(t):.1f}%"


def kernels():
    return " + ".join(ln.split(" grid=")[0] + " grid=" + ln.split(" grid=")[1].split(" ")[0]
                      for ln in L.mi355_ctx_last_launch(eng._ctx).decode().strip().split("\n"))


say(f"# grouped aggregates on {torch.cuda.get_device_name(0)}; rows={n} rounds={args.rounds} burst={args.burst}")
say("# ms per call: median of the rounds [fastest .. slowest]; spread = (slowest - fastest) / median; calls back to back")
say("# group_aggregate: one call (init launch + aggregation launch).  chain (2^ck <= 8): per group scan_where(keys == g [AND mask])")
say("#   + aggregate(values, bitmap), the calls as they were before group_aggregate existed; same process, interleaved rounds")
say("# histogram: histogram(keys [, mask]) on the same keys -- one LDS atomic per row.  stream: torch.sum over both buffers as int64")
say("# TB/s: algorithmic bytes n*ck/8 + n*cv/8 (+ n/8 mask) over the group_aggregate median")
say()

CASES = [(2, 9, "uniform", False), (3, 17, "uniform", False), (3, 17, "one group", False), (5, 12, "uniform", False),
         (8, 12, "uniform", False), (12, 32, "uniform", False), (3, 17, "uniform", True)]
gates = []
for ck, cv, kind, masked in CASES:
    groups = 1 << ck
    keys = eng.generate("mod", n, ck, 1) if kind == "one group" else eng.generate("splitmix", n, ck, 42)
    vals = eng.generate("splitmix", n, cv, 4242)
    mask = None
    if masked:  # one row in eight: a 9-bit column below 64
        sel = eng.generate("splitmix", n, 9, 777)
        mask = eng.scan_where("<", 64, sel)[0]
        del sel
    out = torch.empty((groups, 4), dtype=torch.int64, device="cuda")
    hist = torch.empty(groups, dtype=torch.int64, device="cuda")
    grouped = lambda: eng.group_aggregate(keys, vals, mask=mask, out=out)  # noqa: E731
    histo = lambda: eng.histogram(keys, mask=mask, out=hist)  # noqa: E731
    kb, vb = keys.data[: keys.data.numel() // 8 * 8].view(torch.int64), vals.data[: vals.data.numel() // 8 * 8].view(torch.int64)
    stream = lambda: (kb.sum(), vb.sum())  # noqa: E731
    series = {"group_aggregate": (grouped, args.burst), "histogram": (histo, args.burst), "stream": (stream, args.burst)}
    chain_out = None
    if groups <= 8:
        bm = eng.alloc_bitmap(n)
        hits = torch.empty(1, dtype=torch.int64, device="cuda")
        chain_out = torch.empty((groups, 4), dtype=torch.int64, device="cuda")

        def chain():
            for g in range(groups):
                eng.scan_where("==", g, keys, and_mask=mask, bitmap=bm, hits=hits)
                eng.aggregate(vals, mask=bm, out=chain_out[g])

        series["chain"] = (chain, max(1, args.burst // groups))
    grouped()
    k_grouped = kernels()
    t = measure(series)
    tg = t["group_aggregate"]
    nbytes = n * ck / 8 + n * cv / 8 + (n / 8 if masked else 0)
    name = f"({ck:2d},{cv:2d}) {kind}{' under a 1/8 mask' if masked else ''}"
    say(f"{name}")
    say(f"    group_aggregate {fmt(tg)}  {nbytes / med(tg) / 1e9:.2f} TB/s   {k_grouped}")
    if "chain" in t:
        tc = t["chain"]
        say(f"    chain of {groups} x (scan_where + aggregate) {fmt(tc)} | chain / group_aggregate {med(tc) / med(tg):.2f}")
    say(f"    histogram(keys) {fmt(t['histogram'])} | group_aggregate / histogram {med(tg) / med(t['histogram']):.2f}")
    say(f"    stream floor    {fmt(t['stream'])} | group_aggregate / stream {med(tg) / med(t['stream']):.2f}")
    # the results agree: counts with the histogram's, everything with the chain's where there is one
    grouped()
    histo()
    ok = bool(torch.equal(out[:, 1], hist))
    if chain_out is not None:
        chain()
        ok = ok and bool(torch.equal(out, chain_out))
    torch.cuda.synchronize()
    say(f"    results {'agree' if ok else 'DIFFER'} (counts with histogram{', all four columns with the chain' if chain_out is not None else ''}); "
        f"populated groups {int((out[:, 1] > 0).sum().item())} of {groups}, rows counted {int(out[:, 1].sum().item())}")
    say()
    if "chain" in t and kind == "uniform" and not masked:
        gates.append((groups, med(tg), med(t["chain"]), max(spread(tg), spread(t["chain"]))))
    del keys, vals, mask, out, hist, kb, vb, chain_out
    torch.cuda.empty_cache()

for groups, g, c, sp in gates:
    margin = max(0.05, sp)
    say(f"# target at {groups} groups: group_aggregate median < chain median / (1 + margin), margin = max(5%, round-to-round spread) = "
        f"{100 * margin:.1f}%: {g:.4f} vs {c:.4f} ms, chain / group_aggregate {c / g:.2f}: {'MET' if g * (1 + margin) < c else 'MISSED'}")

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
