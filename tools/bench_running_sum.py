#!/usr/bin/env python3
"""running_sum and delta (ScanEngine.running_sum / delta: prefix sums and differences of a packed column, packed in and out) against
the route the library offered before them -- decompress -> torch.cumsum in int64 -> range select -> compress, and decompress ->
torch.diff -> compress.  HIP events over back-to-back calls, every shape warmed, the series of a case interleaved in ONE process;
every output is compared with the route's before it is timed.  Writes profiles/r21_running_sum.txt.

    python tools/bench_running_sum.py [--out profiles/r21_running_sum.txt] [--scale 1.0] [--rounds 5] [--burst 5]
    python tools/bench_running_sum.py --only-call 20   # nothing but 20 calls of the first shape: for a kernel trace of the three launches

Shapes (rows times --scale), uniform random values unless noted; true results fit 32 bits.  Gated: 1e9 rows of 2-bit deltas into 31
bit (delta_decode, the checked kernel), 2.5e8 x 4 bit into 31 bit (checked), the positions of a 1e9-row bitmap at density 1/8 into 30
bit (exact), delta of a sorted 2.5e8 x 24-bit column with its descent count.  Reported: 2.5e8 x 6 bit under a 1/8 mask, the call
against its byte floor (a count-only scan of the column plus arith at the same output width), a column whose every row is out of
range.  The gate: the call's median below the route's, and no round of the call as slow as the route's fastest.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from shared_simd_scan_amd import PackedColumn, ScanEngine, delta_kernel, running_sum_kernel, running_sum_workspace_words  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_running_sum.txt"))
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--burst", type=int, default=5)
ap.add_argument("--only-call", type=int, default=0)
args = ap.parse_args()
assert args.rounds >= 3 and args.burst >= 1

eng = ScanEngine(0)
lines = []
ALIGN = 65536  # rows: every shape is a multiple


def say(s=""):
    """prints the line and rewrites the file: what has been measured is kept whatever happens to the rest"""
    print(s, flush=True)
    lines.append(s)
    if args.only_call:
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def measure(series):
    """series: {name: (callable, burst)}; alternating rounds of `burst` back-to-back calls -> {name: sorted ms per call}"""
    times = {k: [] for k in series}
    for fn, _ in series.values():  # every shape warmed
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
    return f"{med(t):.3f} ms [{t[0]:.3f} .. {t[-1]:.3f}]"


def once_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def slow_burst(fn):
    return 1 if once_ms(fn) > 20 else max(1, args.burst // 2)


def report(name, what, same, t, gated, call):
    tc, tr = t[call], t["route"]
    verdict = ""
    if gated:
        verdict = " | gate: ok" if med(tc) < med(tr) and tc[-1] < tr[0] else " | gate: **LOSES**"
    elif med(tc) >= med(tr):
        verdict = " | **slower than the route** (reported, not gated)"
    say(f"  {name}: {what}; results {'agree' if same else 'DIFFER'}")
    say(f"    {call} {fmt(tc)} | route {fmt(tr)} | route / {call} {med(tr) / med(tc):.2f}{verdict}")


class SumCase:
    """one running_sum shape: its buffers, the call and the route"""

    def __init__(self, col, b, k, co, exclusive=False, mask=None, miss=0):
        self.col, self.b, self.k, self.co, self.exclusive, self.mask, self.miss = col, b, k, co, exclusive, mask, miss
        n = col.n
        self.out = torch.empty((n * co + 7) // 8 + 256, dtype=torch.uint8, device="cuda")
        self.result = torch.empty(2, dtype=torch.int64, device="cuda")
        self.ws = torch.empty(running_sum_workspace_words(n), dtype=torch.int64, device="cuda")
        self.dense = torch.empty(n, dtype=torch.int32, device="cuda")
        self.sel = None
        if mask is not None:  # the route is handed the mask as booleans ready-made
            self.sel = eng.decompress(PackedColumn(mask, n, 1))[:n].to(torch.bool)

    def call(self):
        return eng.running_sum(self.col, mask=self.mask, b=self.b, k=self.k, exclusive=self.exclusive, co=self.co, miss=self.miss, out=self.out,
                               result=self.result, workspace=self.ws)

    def route(self):
        n = self.col.n
        t = eng.decompress(self.col, out=self.dense)[:n].to(torch.int64)
        if self.b:
            t += self.b
        if self.sel is not None:
            t = torch.where(self.sel, t, 0)
        r = torch.cumsum(t, 0)
        if self.exclusive:
            r -= t
        if self.k:
            r += self.k
        inside = (r >= 0) & (r < (1 << self.co))
        r = torch.where(inside, r, self.miss)
        return eng.compress(r.to(torch.int32), self.co), (~inside).sum()

    def run(self, name, gated, extra=None):
        n, co = self.col.n, self.co
        want, want_outside = self.route()
        got, result = self.call()
        nb = (n * co + 7) // 8
        same = torch.equal(got.data[:nb], want.data[:nb]) and int(result[1].item()) == int(want_outside.item())
        del want
        torch.cuda.empty_cache()
        series = {"running_sum": (self.call, args.burst), "route": (self.route, slow_burst(self.route))}
        if extra:
            series.update(extra)
        t = measure(series)
        fam = running_sum_kernel(self.col.c, n, self.b, self.k, co)
        report(name, f"n = {n}, {self.col.c} bit -> {co} bit, b = {self.b}, k = {self.k}, {'exclusive' if self.exclusive else 'inclusive'}, "
               f"{'masked, ' if self.mask is not None else ''}{int(result[1].item())} rows replaced, {fam}", same, t, gated, "running_sum")
        return t


def delta_case(col, name, gated):
    n, c = col.n, col.c
    out = torch.empty((n * c + 7) // 8 + 256, dtype=torch.uint8, device="cuda")
    cnt = torch.empty(1, dtype=torch.int64, device="cuda")
    dense = torch.empty(n, dtype=torch.int32, device="cuda")
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call():
        return eng.delta(col, out=out, out_of_range=cnt)

    def route():
        d = torch.diff(eng.decompress(col, out=dense)[:n], prepend=zero)
        return eng.compress(d, c), (d < 0).sum()

    want, descents = route()
    got = call()
    nb = (n * c + 7) // 8
    same = torch.equal(got.data[:nb], want.data[:nb]) and int(cnt.item()) == int(descents.item())
    del want
    torch.cuda.empty_cache()
    t = measure({"delta": (call, args.burst), "route": (route, slow_burst(route))})
    report(name, f"n = {n}, {c} bit -> {c} bit, k = 0, {int(cnt.item())} descents, {delta_kernel(c, 0, c)}", same, t, gated, "delta")


N1 = int(1_000_000_000 * args.scale) // ALIGN * ALIGN
N4 = int(250_000_000 * args.scale) // ALIGN * ALIGN

if args.only_call:
    case = SumCase(eng.generate("splitmix", N1, 2, 42), 0, 1000, 31)
    for _ in range(args.only_call):
        case.call()
    eng.synchronize()
    print(f"{args.only_call} calls of running_sum on {N1} rows x 2 bit -> 31 bit")
    sys.exit(0)

say(f"# running_sum and delta on {torch.cuda.get_device_name(0)}; scale={args.scale} rounds={args.rounds} burst={args.burst}")
say("# ms per call: median of the rounds [fastest .. slowest]; calls back to back; the call writes the packed column, its two result")
say("# words (or delta's counter) and uses a workspace of its caller's")
say("# route: decompress -> int64 (+ b, mask) -> torch.cumsum -> (- own term, + k) -> range select -> int32 -> compress, with the count")
say("#        of replaced rows; delta: decompress -> torch.diff -> compress, with the count of descents")
say("# gate: the call's median below the route's and its slowest round below the route's fastest")
say()

say("gated")
SumCase(eng.generate("splitmix", N1, 2, 42), 0, 1000, 31).run("1e9 x 2-bit deltas -> 31 bit (delta_decode)", True)
torch.cuda.empty_cache()
SumCase(eng.generate("splitmix", N4, 4, 42), 0, 1000, 31).run("2.5e8 x 4 bit -> 31 bit", True)
torch.cuda.empty_cache()
bitmap, hits = eng.scan_where("<", 512, eng.generate("splitmix", N1, 12, 7))  # density 1/8
SumCase(PackedColumn(bitmap, N1, 1), 0, 0, 30, exclusive=True).run("positions of a 1e9-row bitmap at density 1/8 -> 30 bit", True)
del bitmap
torch.cuda.empty_cache()
asc = (torch.arange(N4, dtype=torch.int64, device="cuda") * (1 << 24) // N4).to(torch.int32)
delta_case(eng.compress(asc, 24), "delta of a sorted 2.5e8 x 24-bit column, descents counted", True)
del asc
torch.cuda.empty_cache()
say()

say("reported, not gated")
col6 = eng.generate("splitmix", N4, 6, 42)
mask, hits = eng.scan_where("<", 512, eng.generate("splitmix", N4, 12, 9))
SumCase(col6, 0, 0, 31, mask=mask).run("2.5e8 x 6 bit under a 1/8 mask -> 31 bit", False)
del mask
torch.cuda.empty_cache()
SumCase(col6, 0, -(1 << 40), 31).run("2.5e8 x 6 bit, every row out of range", False)
torch.cuda.empty_cache()
# the byte floor: one read of the column that writes nothing (a count-only scan) plus one read with the packed write (arith, x + 0 x)
col4 = eng.generate("splitmix", N4, 4, 42)
floor_out = torch.empty((N4 * 31 + 7) // 8 + 256, dtype=torch.uint8, device="cuda")
hits = torch.empty(1, dtype=torch.int64, device="cuda")
case = SumCase(col4, 0, 1000, 31)
t = measure({"running_sum": (case.call, args.burst),
             "count-only scan": (lambda: eng.scan_combine("<", 3, col4, hits=hits, count_only=True), args.burst),
             "arith": (lambda: eng.arith("linear", col4, col4, a=1, b=0, k=1000, co=31, out=floor_out), args.burst)})
floor = med(t["count-only scan"]) + med(t["arith"])
say(f"  byte floor, 2.5e8 x 4 bit -> 31 bit: running_sum {fmt(t['running_sum'])} | count-only scan {fmt(t['count-only scan'])} + arith {fmt(t['arith'])} = "
    f"{floor:.3f} ms | running_sum / floor {med(t['running_sum']) / floor:.2f}")

print(f"wrote {args.out}")
