#!/usr/bin/env python3
"""run_aggregate (ScanEngine.run_aggregate: sum, count, min, max of a packed column per run of a table of run ends) against the
routes the library offered before it -- the torch route: decompress of the values -> segment ids by torch.repeat_interleave of the
run lengths -> index_add_ / scatter_reduce_(amin, amax) / bincount; and, for the sum alone and where the running sum fits 32 bits,
the packed five-call chain lookup(arith(ends - 1), running_sum(y)) -> delta.  HIP events over back-to-back calls, every shape
warmed, the series of a case interleaved in ONE process; every output is compared with the route's before it is timed.  Writes
profiles/r24_run_aggregate.txt.

    python tools/bench_run_aggregate.py [--out profiles/r24_run_aggregate.txt] [--scale 1.0] [--rounds 5] [--burst 5]

Shapes (rows times --scale).  Gated: 1e9 rows x 9 bit with mean run 4096 and with mean run 64; the runs of a sorted uniform
2.5e8 x 17-bit key (r = 131072) over a 17-bit value column; 1e9 x 9 bit, mean run 64, under a 1/8 mask.  Reported: mean run 4 (the
dense path), a tile span of exactly S and of S + 1 runs throughout, one run over everything (2.5e8 rows), 63 zero-length runs in front of every
run, 32-bit values, sorted_group_aggregate of 2.5e8 sparse 32-bit keys against decompress -> torch.unique(return_inverse) ->
scatter_reduce_, the ratio to `aggregate` of the same column under the same mask (one pass: the byte floor), the ratio to the
five-call chain.  The gate: the call's median below the route's, and no round of the call as slow as the route's fastest.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from shared_simd_scan_amd import PackedColumn, ScanEngine, run_aggregate_span_slots  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_run_aggregate.txt"))
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--burst", type=int, default=5)
args = ap.parse_args()
assert args.rounds >= 3 and args.burst >= 1

eng = ScanEngine(0)
lines = []
ALIGN = 65536  # rows: every shape is a multiple
I32_MAX = (1 << 31) - 1


def say(s=""):
    """prints the line and rewrites the file: what has been measured is kept whatever happens to the rest"""
    print(s, flush=True)
    lines.append(s)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def measure(series):
    """series: {name: (callable, burst)}; alternating rounds of `burst` back-to-back calls -> {name: ms per call, in round order}"""
    times = {k: [] for k in series}
    for fn, _ in series.values():  # every shape warmed
        fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, (fn, burst) in series.items():
            if burst > 1:
                fn()  # (a series timed one call at a time is a slow one: no extra call in front)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(burst):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / burst)
    return times


def med(t):
    return sorted(t)[len(t) // 2]


def fmt(t):
    return f"{med(t):.3f} ms [{' '.join(f'{x:.3f}' for x in t)}]"


def once_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def slow_burst(fn):
    return 1 if once_ms(fn) > 20 else max(1, args.burst // 2)


def report(name, what, same, t, gated, call="run_aggregate", route="route"):
    tc, tr = t[call], t[route]
    verdict = ""
    if gated:
        verdict = " | gate: ok" if med(tc) < med(tr) and max(tc) < min(tr) else " | gate: **LOSES**"
    elif med(tc) >= med(tr):
        verdict = " | **slower than the route** (reported, not gated)"
    say(f"  {name}: {what}; results {'agree' if same else 'DIFFER'}")
    say(f"    {call} {fmt(tc)} | {route} {fmt(tr)} | {route} / {call} {med(tr) / med(tc):.2f}{verdict}")


def random_ends(n, mean, seed):
    """ends of runs of geometric length around `mean`, the last one n -> int64[r] on the device, built in slices"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    parts, step = [], 1 << 27
    for at in range(0, n, step):
        m = min(step, n - at)
        parts.append(torch.nonzero(torch.rand(m, generator=g, device="cuda") < 1.0 / mean).flatten() + (at + 1))
    e = torch.cat(parts)
    if e.numel() == 0 or int(e[-1].item()) != n:
        e = torch.cat([e, torch.tensor([n], dtype=torch.int64, device="cuda")])
    return e


def ends_column(ends, n, ce=None):
    return eng.compress(ends.to(torch.int32), ce or max(1, max(n, int(ends[-1].item())).bit_length()))


def empty_of(table_sum, count, mn, mx):
    """the four columns of the torch route in the call's layout: a run without a row reads (0, 0, -1, 0)"""
    none = count == 0
    return torch.stack([table_sum, count, torch.where(none, torch.full_like(mn, -1), mn), torch.where(none, torch.zeros_like(mx), mx)], dim=1)


class Case:
    def __init__(self, vcol, ends, keep=None, ce=None):
        """vcol: the values; ends: int64[r]; keep: bool[n] on the device, the rows a mask selects (None: every row)"""
        self.vcol, self.n, self.r = vcol, vcol.n, int(ends.numel())
        self.ecol = ends_column(ends, self.n, ce)
        self.lengths = torch.diff(ends, prepend=torch.zeros(1, dtype=torch.int64, device="cuda"))
        self.keep = keep
        self.mask = None
        if keep is not None:
            self.mask, _ = eng.scan_where("==", 1, eng.compress(keep.to(torch.int32), 1))
        self.table = torch.empty((self.r, 4), dtype=torch.int64, device="cuda")
        self.dense = torch.empty(self.n, dtype=torch.int32, device="cuda")
        self.four = torch.empty(4, dtype=torch.int64, device="cuda")

    def call(self):
        return eng.run_aggregate(self.vcol, self.ecol, mask=self.mask, out=self.table)

    def whole(self):
        return eng.aggregate(self.vcol, mask=self.mask, out=self.four)

    def route(self):
        r = self.r
        x = eng.decompress(self.vcol, out=self.dense)[: self.n]
        seg = torch.repeat_interleave(torch.arange(r, device="cuda"), self.lengths)[: self.n]
        if self.keep is not None:
            x, seg = x[self.keep], seg[self.keep]
        total = torch.zeros(r, dtype=torch.int64, device="cuda").index_add_(0, seg, x.to(torch.int64))
        mn = torch.full((r,), I32_MAX, dtype=torch.int32, device="cuda").scatter_reduce_(0, seg, x, "amin")
        mx = torch.zeros(r, dtype=torch.int32, device="cuda").scatter_reduce_(0, seg, x, "amax")
        count = torch.bincount(seg, minlength=r)
        return empty_of(total, count, mn.to(torch.int64), mx.to(torch.int64))

    def run(self, name, gated, extra=None):
        want = self.route()
        self.call()
        same = torch.equal(self.table, want)
        del want
        torch.cuda.empty_cache()
        series = {"run_aggregate": (self.call, args.burst), "route": (self.route, slow_burst(self.route)), "aggregate": (self.whole, args.burst)}
        if extra:
            series.update(extra)
        t = measure(series)
        what = f"n = {self.n}, values {self.vcol.c} bit, ends {self.ecol.c} bit, r = {self.r} (mean run {self.n / max(self.r, 1):.1f})"
        if self.keep is not None:
            what += f", {int(self.keep.sum().item())} rows selected"
        report(name, what, same, t, gated)
        say(f"    byte floor: aggregate of the same column under the same mask {fmt(t['aggregate'])} | run_aggregate / aggregate {med(t['run_aggregate']) / med(t['aggregate']):.2f}")
        return t

    def free(self):
        del self.dense, self.table
        torch.cuda.empty_cache()


N1 = int(1_000_000_000 * args.scale) // ALIGN * ALIGN
N4 = int(250_000_000 * args.scale) // ALIGN * ALIGN
NC = int(15_000_000 * args.scale) // ALIGN * ALIGN  # 9-bit values: the running sum stays inside 32 bits

say(f"# run_aggregate on {torch.cuda.get_device_name(0)}; scale={args.scale} rounds={args.rounds} burst={args.burst}")
say("# ms per call: median of the rounds [every round, in order]; calls back to back; the call writes its table of r x 4 words")
say("# route: decompress -> torch.repeat_interleave(arange(r), lengths) -> index_add_ / scatter_reduce_(amin, amax) / bincount")
say("#        (lengths and, under a mask, the selection as a bool tensor are handed to the route ready-made)")
say("# gate: the call's median below the route's and its slowest round below the route's fastest")
say(f"# span slots S: {run_aggregate_span_slots(9)} at 9 bit, {run_aggregate_span_slots(17)} at 17 bit, {run_aggregate_span_slots(32)} at 32 bit")
say()

say("gated")
col9 = eng.generate("splitmix", N1, 9, 42)
for mean, seed in ((4096, 1), (64, 2)):
    case = Case(col9, random_ends(N1, mean, seed))
    case.run(f"1e9 x 9 bit, mean run {mean}", True)
    case.free()
g = torch.Generator(device="cuda").manual_seed(3)
keys = torch.sort(torch.randint(0, 1 << 17, (N4,), generator=g, device="cuda", dtype=torch.int32)).values
ends17 = torch.nonzero(torch.cat([keys[1:] != keys[:-1], torch.ones(1, dtype=torch.bool, device="cuda")])).flatten() + 1
del keys
col17 = eng.generate("splitmix", N4, 17, 43)
case = Case(col17, ends17)
case.run("the runs of a sorted uniform 2.5e8 x 17-bit key over a 17-bit value column", True)
case.free()
del col17, ends17
keep = torch.rand(N1, generator=g, device="cuda") < 0.125
case = Case(col9, random_ends(N1, 64, 2), keep=keep)
case.run("1e9 x 9 bit, mean run 64, under a 1/8 mask", True)
case.free()
del keep
torch.cuda.empty_cache()
say()

say("reported, not gated")
case = Case(col9, random_ends(N1, 4, 4))
case.run("1e9 x 9 bit, mean run 4 (the dense path)", False)
case.free()
S = run_aggregate_span_slots(9)
q = 2048 // S
for extra in (0, 1):
    # every tile addresses exactly S runs of 2048 / S rows, or S + 1 with the runs shifted by one row
    e = torch.arange(q - extra, N1 + 1, q, dtype=torch.int64, device="cuda")
    if int(e[-1].item()) != N1:
        e = torch.cat([e, torch.tensor([N1], dtype=torch.int64, device="cuda")])
    case = Case(col9, e)
    case.run(f"1e9 x 9 bit, every tile a span of S{' + 1' if extra else ''} = {S + extra} runs", False)
    case.free()
# (2.5e8 rows: the route's atomics all meet in one word)
col9q = PackedColumn(col9.data, N4, 9)
case = Case(col9q, torch.tensor([N4], dtype=torch.int64, device="cuda"))
case.run("2.5e8 x 9 bit, one run over everything", False)
case.free()
ends = random_ends(N1, 4096, 1)
z = ends.repeat_interleave(64)
z.view(-1, 64)[:, :63] = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), ends[:-1]])[:, None]  # a run of length zero ends where the run in front ends
case = Case(col9, z)
case.run("1e9 x 9 bit, mean run 4096 with 63 zero-length runs in front of every run", False)
case.free()
del z, ends, col9
torch.cuda.empty_cache()
col32 = eng.generate("splitmix", N4, 32, 44)


class Case32(Case):
    def route(self):  # 32-bit values: the route's minimum and maximum in int64
        r = self.r
        x = eng.decompress(self.vcol, out=self.dense)[: self.n].to(torch.int64) & 0xFFFFFFFF
        seg = torch.repeat_interleave(torch.arange(r, device="cuda"), self.lengths)[: self.n]
        total = torch.zeros(r, dtype=torch.int64, device="cuda").index_add_(0, seg, x)
        mn = torch.full((r,), 1 << 40, dtype=torch.int64, device="cuda").scatter_reduce_(0, seg, x, "amin")
        mx = torch.zeros(r, dtype=torch.int64, device="cuda").scatter_reduce_(0, seg, x, "amax")
        return empty_of(total, torch.bincount(seg, minlength=r), mn, mx)


case = Case32(col32, random_ends(N4, 64, 5), ce=32)
case.run("2.5e8 x 32 bit with 32-bit ends, mean run 64", False)
case.free()
del col32
torch.cuda.empty_cache()

# the five-call chain, for the sum alone, where the running sum fits 32 bits
colc = eng.generate("splitmix", NC, 9, 45)
case = Case(colc, random_ends(NC, 64, 6))
ecol = PackedColumn(case.ecol.data, case.r, case.ecol.c)


def chain():
    sums, _ = eng.running_sum(colc, co=32)
    return eng.delta(eng.lookup(eng.arith("linear", ecol, ecol, a=1, b=0, k=-1, co=ecol.c), sums), first=0, co=32)


case.call()
per_run = eng.decompress(chain())[: case.r].to(torch.int64) & 0xFFFFFFFF
same = torch.equal(per_run, case.table[:, 0])
t = measure({"run_aggregate": (case.call, args.burst), "chain": (chain, args.burst)})
report("1.5e7 x 9 bit, mean run 64, the sums alone", f"n = {NC}, r = {case.r}", same, t, False, route="chain")
case.free()
del colc
torch.cuda.empty_cache()

# the whole sort-based GROUP BY of a sparse key
g = torch.Generator(device="cuda").manual_seed(7)
domain = torch.randint(-(1 << 31), (1 << 31) - 1, (1 << 20,), generator=g, device="cuda", dtype=torch.int64).to(torch.int32)
keys32 = domain[torch.randint(0, 1 << 20, (N4,), generator=g, device="cuda")]
kcol = eng.compress(keys32, 32)
vcol = eng.generate("splitmix", N4, 17, 46)
dense = torch.empty(N4, dtype=torch.int32, device="cuda")


def group_route():
    k = eng.decompress(kcol)[:N4].to(torch.int64) & 0xFFFFFFFF
    x = eng.decompress(vcol, out=dense)[:N4]
    u, inv = torch.unique(k, return_inverse=True)
    r = u.numel()
    total = torch.zeros(r, dtype=torch.int64, device="cuda").index_add_(0, inv, x.to(torch.int64))
    mn = torch.full((r,), I32_MAX, dtype=torch.int32, device="cuda").scatter_reduce_(0, inv, x, "amin")
    mx = torch.zeros(r, dtype=torch.int32, device="cuda").scatter_reduce_(0, inv, x, "amax")
    return u, empty_of(total, torch.bincount(inv, minlength=r), mn.to(torch.int64), mx.to(torch.int64))


def group_call():
    return eng.sorted_group_aggregate(kcol, vcol)


u, want = group_route()
gk, table, groups = group_call()
d = int(groups.item())
same = d == u.numel() and torch.equal(table[:d], want) and torch.equal(eng.decompress(PackedColumn(gk.data, d, 32))[:d].to(torch.int64) & 0xFFFFFFFF, u)
del u, want, gk, table
torch.cuda.empty_cache()
t = measure({"sorted_group_aggregate": (group_call, 1), "route": (group_route, 1)})
report("sorted_group_aggregate of 2.5e8 sparse 32-bit keys over 17-bit values", f"n = {N4}, {d} groups; route: decompress x 2 -> torch.unique(return_inverse) -> "
       "index_add_ / scatter_reduce_ / bincount", same, t, False, call="sorted_group_aggregate")

print(f"wrote {args.out}")
