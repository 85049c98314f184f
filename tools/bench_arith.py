#!/usr/bin/env python3
"""arith (ScanEngine.arith: a packed column computed row by row from two others) against the route the library offered before it
-- decompress both columns -> torch arithmetic on two int32 tensors -> compress --, with lookup in its LDS tier on the same n and
output width as the pipeline's yardstick (arith's pipeline is lookup's, with a second input and arithmetic in place of the table).
HIP events over back-to-back launches, every shape warmed, all series of a shape interleaved in ONE process.  Writes
profiles/r11_arith.txt.

    python tools/bench_arith.py [--out profiles/r11_arith.txt] [--scale 1.0] [--rounds 5] [--burst 20]

Shapes (rows times --scale): 1e9 rows 9 x 9 -> 10 bit, x + y (arith_exact_kernel); the same into 9 bit (arith_checked_kernel: a
sum of 512 or more becomes miss and is counted); 2.5e8 rows 20 x 4 -> 24 bit, x * y (arith_exact_kernel).  The yardstick's column
has 9 bits at the first two shapes and 12 at the third (a table of 2^c rows must fit the LDS tier at the output width).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from shared_simd_scan_amd import ScanEngine, arith_kernel, lookup_kernel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_arith.txt"))
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--burst", type=int, default=20)
args = ap.parse_args()
assert args.rounds >= 3 and args.burst >= 1

eng = ScanEngine(0)
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


say(f"# arith on {torch.cuda.get_device_name(0)}; scale={args.scale} rounds={args.rounds} burst={args.burst}")
say("# ms per call: median of the rounds [fastest .. slowest]; calls back to back")
say("# GB/s: (c1 + c2 + co) * n / 8 over the median (lookup: (c + co) * n / 8) -- what the packed columns hold")
say("# route: decompress(col1), decompress(col2) -> torch arithmetic on the int32 tensors -> compress")
say("# lookup: a column of c bits through a table of 2^c rows x co bit, LDS tier -- the same pipeline with one input")
say()

N_BIG, N_SMALL = int(1_000_000_000 * args.scale) // 2048 * 2048, int(250_000_000 * args.scale) // 2048 * 2048
MISS = 511


def sum_or_miss(s):
    return torch.where(s < 512, s, MISS)


# (name, n, op, c1, c2, co, the yardstick's column width, the route's arithmetic)
SHAPES = [
    ("linear exact  x + y", N_BIG, "linear", 9, 9, 10, 9, lambda x, y: x + y),
    ("linear checked x + y < 512 else miss", N_BIG, "linear", 9, 9, 9, 9, lambda x, y: sum_or_miss(x + y)),
    ("mul exact  x * y", N_SMALL, "mul", 20, 4, 24, 12, lambda x, y: x * y),
]
for name, n, op, c1, c2, co, cl, torch_op in SHAPES:
    col1, col2 = eng.generate("splitmix", n, c1, 42), eng.generate("splitmix", n, c2, 43)
    out = eng.alloc_packed(n, co)
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    lcol = eng.generate("splitmix", n, cl, 44)
    table = eng.compress(torch.randint(0, 1 << co, (1 << cl,), dtype=torch.int32, device="cuda"), co)
    lout = eng.alloc_packed(n, co)
    kernel = arith_kernel(op, c1, c2, co=co)
    checked = kernel == "arith_checked_kernel"
    assert lookup_kernel(cl, 1 << cl, co) == "lookup_lds_kernel"

    def arith():
        return eng.arith(op, col1, col2, co=co, miss=MISS if checked else 0, out=out.data, out_of_range=counter if checked else None)

    def route():
        return eng.compress(torch_op(eng.decompress(col1), eng.decompress(col2)), co)

    def look():
        return eng.lookup(lcol, table, out=lout.data)

    slow = max(1, args.burst // 10)
    t = measure({"arith": (arith, args.burst), "route": (route, slow), "lookup": (look, args.burst)})
    ta = t["arith"]
    say(f"{name}: {n} rows, {c1} x {c2} -> {co} bit, {kernel}")
    say(f"    arith   {fmt(ta)}  {(c1 + c2 + co) * n / 8 / med(ta) / 1e6:.0f} GB/s")
    say(f"    route   {fmt(t['route'])} | route / arith {med(t['route']) / med(ta):.2f}")
    say(f"    lookup ({cl} -> {co} bit) {fmt(t['lookup'])}  {(cl + co) * n / 8 / med(t['lookup']) / 1e6:.0f} GB/s | arith / lookup {med(ta) / med(t['lookup']):.2f}")
    arith()
    nb = (n * co + 7) // 8
    same = torch.equal(out.data[:nb], route().data[:nb])
    say(f"    results {'agree' if same else 'DIFFER'} with the route" + (f"; {int(counter.item())} rows out of range" if checked else ""))
    say()
    del col1, col2, out, lcol, table, lout
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
