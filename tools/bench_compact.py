#!/usr/bin/env python3
"""compact (ScanEngine.compact: the rows a bitmap selects, as a packed column) against the route the library offered before it --
bitmap_to_rowids -> gather -> pack_u32_dev --, and lookup on the full column against compact -> lookup on the compacted one.  HIP
events over back-to-back launches, every shape warmed, all series of a case interleaved in ONE process.  Writes
profiles/r10_compact.txt.

    python tools/bench_compact.py [--out profiles/r10_compact.txt] [--scale 1.0] [--rounds 5] [--burst 20]

Shapes (rows times --scale): 1e9 rows x 9 bit and 2.5e8 rows x 17 bit.  Bitmaps: random of density 1/512, 1/64, 1/8 and 1/2 (the
AND of 9, 6, 3, 1 uniform random bitmaps), and one clustered: runs of 64 Ki rows, one run in eight (at random) all ones.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from shared_simd_scan_amd import PackedColumn, ScanEngine, lib, lookup_kernel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_compact.txt"))
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--burst", type=int, default=20)
args = ap.parse_args()
assert args.rounds >= 3 and args.burst >= 1

eng = ScanEngine(0)
L = lib()
lines = []
RUN = 65536  # rows of a clustered run


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


def bitmap_of(kind, n):
    """-> uint8[n / 8] device tensor; n is a multiple of RUN"""
    g = torch.Generator(device="cuda").manual_seed(1234)
    nb = n // 8
    if kind == "clustered":
        runs = torch.rand(n // RUN, generator=g, device="cuda") < 0.125
        return (runs.to(torch.uint8) * 255).repeat_interleave(RUN // 8)
    b = torch.randint(0, 256, (nb,), dtype=torch.uint8, generator=g, device="cuda")
    for _ in range(kind - 1):
        b &= torch.randint(0, 256, (nb,), dtype=torch.uint8, generator=g, device="cuda")
    return b


say(f"# compact on {torch.cuda.get_device_name(0)}; scale={args.scale} rounds={args.rounds} burst={args.burst}")
say("# ms per call: median of the rounds [fastest .. slowest]; calls back to back")
say("# GB/s: (n*c/8 + 2*n/8 + m*c/8) over the median -- the column, the bitmap read twice, the m selected values")
say("# route: bitmap_to_rowids -> gather -> pack_u32_dev (8 bytes of row id and 4 of int32 written and re-read per selected row)")
say("# lookup: through a table of 2^c rows x 8 bit; compact -> lookup: the same table, on the compacted column")
say()

N9, N17 = int(1_000_000_000 * args.scale) // RUN * RUN, int(250_000_000 * args.scale) // RUN * RUN
BITMAPS = [("random 1/512", 9), ("random 1/64", 6), ("random 1/8", 3), ("random 1/2", 1), ("clustered 1/8 (64 Ki-row runs)", "clustered")]
for n, c in ((N9, 9), (N17, 17)):
    col = eng.generate("splitmix", n, c, 42)
    table = eng.compress(torch.randint(0, 256, (1 << c,), dtype=torch.int32, device="cuda"), 8)
    full_out = eng.alloc_packed(n, 8)
    say(f"{n} rows x {c} bit; lookup tier {lookup_kernel(c, 1 << c, 8)}")
    for name, kind in BITMAPS:
        bitmap = bitmap_of(kind, n)
        out = eng.alloc_packed(n, c)
        _, count = eng.compact(col, bitmap, out=out.data)
        m = int(count.item())
        small_out = eng.alloc_packed(max(m, 1), 8)

        def compact():
            return eng.compact(col, bitmap, out=out.data)

        def route():
            rowids, cnt = eng.bitmap_to_rowids(bitmap, n, max(m, 1))
            return eng.compress(eng.gather(col, rowids, cnt)[:m], c)

        def look():
            return eng.lookup(col, table, out=full_out.data)

        def chain():
            compact()
            return eng.lookup(PackedColumn(out.data, m, c), table, out=small_out.data)

        slow = max(1, args.burst // 10)
        t = measure({"compact": (compact, args.burst), "route": (route, slow), "lookup": (look, args.burst), "chain": (chain, args.burst)})
        tc = t["compact"]
        moved = n * c / 8 + 2 * n / 8 + m * c / 8
        say(f"  {name}: m = {m} ({m / n:.5f} of the rows)")
        say(f"    compact {fmt(tc)}  {moved / med(tc) / 1e6:.0f} GB/s")
        say(f"    route   {fmt(t['route'])} | route / compact {med(t['route']) / med(tc):.2f}")
        say(f"    lookup on the full column {fmt(t['lookup'])} | compact -> lookup {fmt(t['chain'])} | chain / lookup {med(t['chain']) / med(t['lookup']):.2f}")
        compact()
        nb = (m * c + 7) // 8
        say(f"    results {'agree' if torch.equal(out.data[:nb], route().data[:nb]) else 'DIFFER'} with the route")
        del bitmap, out, small_out
        torch.cuda.empty_cache()
    say()
    del col, table, full_out
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
