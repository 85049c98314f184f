#!/usr/bin/env python3
"""Semi-join (ScanEngine.semi_join: a packed column filtered by a device-resident bitmap set) in both tiers, against scan_in
with the equivalent key list where one exists (at most 1024 keys) and against the route a caller had without the call:
decompress the column, gather through torch on a byte table, re-pack a bitmap.  HIP events over back-to-back launches, every
shape warmed, all series of a case interleaved in ONE process.  Writes profiles/r08_semijoin.txt.

    python tools/bench_semijoin.py [--out profiles/r08_semijoin.txt] [--scale 1.0] [--rounds 5] [--burst 20]

Shapes: 1e9 rows x 9 bit, 2.5e8 rows x 20 bit and x 32 bit (times --scale).  The foreign keys are uniform over [0, m) (m the set's
size, cut at 2^c), the set is random bytes: half of the keys qualify.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from shared_simd_scan_amd import ScanEngine, lib, semi_join_kernel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_semijoin.txt"))
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


def foreign_keys(n, c, reach_bits):
    """n keys uniform over [0, 2^reach_bits) as a c-bit packed column"""
    if reach_bits >= c:
        return eng.generate("splitmix", n, c, 42)
    narrow = eng.generate("splitmix", n, reach_bits, 42)
    col = eng.compress(eng.decompress(narrow), c)
    del narrow
    return col


say(f"# semi_join on {torch.cuda.get_device_name(0)}; scale={args.scale} rounds={args.rounds} burst={args.burst}")
say("# ms per call: median of the rounds [fastest .. slowest]; calls back to back; TB/s: the column's bytes n*c/8 + the bitmap's n/8 over the median")
say("# scan_in: the same predicate as a key list (the set's members), where the set has at most 1024 of them")
say("# route without the call: decompress -> torch index of a byte table (one byte per key of the set) -> eight bools to a byte")
say()

N9, N20 = int(1_000_000_000 * args.scale) // 8192 * 8192, int(250_000_000 * args.scale) // 8192 * 8192
# (rows, width, log2 of the set's size, time the route without the call)
CASES = [(N9, 9, 9, True), (N9, 9, 16, False), (N20, 20, 9, False), (N20, 20, 16, True), (N20, 32, 16, False),
         (N20, 20, 20, True), (N20, 32, 20, False), (N20, 32, 24, True), (N20, 32, 28, False), (N20, 32, 32, False)]
weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device="cuda")
for n, c, lm, with_route in CASES:
    m = 1 << lm
    reach_bits = min(lm, c)
    col = foreign_keys(n, c, reach_bits)
    sset = torch.randint(0, 256, (m // 8,), dtype=torch.uint8, device="cuda")
    bitmap = eng.alloc_bitmap(n)
    tier = semi_join_kernel(c, m)
    join = lambda: eng.semi_join(col, sset, m, bitmap=bitmap)  # noqa: E731
    series = {"semi_join": (join, args.burst)}
    members = None
    if (1 << reach_bits) <= 1024 and c <= 16:  # (above 16 bits scan_in is a compare chain over the keys: another kernel's cost)
        bits = (sset[: (1 << reach_bits) // 8].unsqueeze(1) & weights.unsqueeze(0)) != 0
        members = torch.nonzero(bits.reshape(-1)).reshape(-1).cpu().tolist()
        if 1 <= len(members) <= 1024:
            bitmap_in = eng.alloc_bitmap(n)
            series["scan_in"] = (lambda: eng.scan_in(members, col, bitmap=bitmap_in), args.burst)
    if with_route:
        table = ((sset.unsqueeze(1) & weights.unsqueeze(0)) != 0).reshape(-1)  # one bool per key
        dec = torch.empty(n, dtype=torch.int32, device="cuda")

        def route():
            eng.decompress(col, out=dec)
            idx = dec.long() & 0xFFFFFFFF if c == 32 else dec.long()
            if m < (1 << c):
                ok = idx < m
                hit = table[idx.clamp_(max=m - 1)] & ok
            else:
                hit = table[idx]
            return (hit.reshape(-1, 8).to(torch.uint8) * weights).sum(dim=1, dtype=torch.uint8)

        series["route"] = (route, max(1, args.burst // 10))
    join()
    k = kernel()
    t = measure(series)
    tj = t["semi_join"]
    say(f"{n} rows x {c} bit, set of 2^{lm} bits ({m // 8} bytes), {tier}")
    say(f"    semi_join {fmt(tj)}  {(n * c / 8 + n / 8) / med(tj) / 1e9:.2f} TB/s   {k}")
    if "scan_in" in t:
        say(f"    scan_in, {len(members)} keys {fmt(t['scan_in'])} | semi_join / scan_in {med(tj) / med(t['scan_in']):.3f}")
        eng.scan_in(members, col, bitmap=bitmap_in)
        join()
        say(f"    results {'agree' if torch.equal(bitmap, bitmap_in) else 'DIFFER'} with scan_in")
        del bitmap_in
    if "route" in t:
        say(f"    route without the call {fmt(t['route'])} | route / semi_join {med(t['route']) / med(tj):.1f}")
        join()
        say(f"    results {'agree' if torch.equal(bitmap, route()) else 'DIFFER'} with the route")
        del table, dec
    say()
    del col, sset, bitmap
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
