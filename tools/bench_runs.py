#!/usr/bin/env python3
"""run_encode and run_decode (ScanEngine.run_encode / run_decode: a packed column's runs as two packed columns, and back) against the
route the library offered before them -- decompress -> torch.unique_consecutive(return_counts=True) -> cumsum -> compress x 2 for
the encoder, decompress x 2 -> torch.diff -> torch.repeat_interleave -> compress for the decoder.  HIP events over back-to-back
calls, every shape warmed, the series of a case interleaved in ONE process; every output is compared with the route's before it
is timed.  Writes profiles/r22_runs.txt.

    python tools/bench_runs.py [--out profiles/r22_runs.txt] [--scale 1.0] [--rounds 5] [--burst 5]

Shapes (rows times --scale).  Gated: 1e9 rows x 9 bit with mean run 4096 and with mean run 64, encode and decode; a sorted uniform
2.5e8 x 17-bit column, encode; the expansion of a 1-bit column over the runs of the first shape into a row bitmap.  Reported: a
random column with r ~ n (the encoder's worst case), 32 x 32 bit, a table with long stretches of zero-length runs, the encoder
against two count-only scans of the column (its byte floor), the decoder against arith into the same width.  The gate: the call's
median below the route's, and no round of the call as slow as the route's fastest.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from shared_simd_scan_amd import PackedColumn, ScanEngine, compressed_buffer_size, run_encode_workspace_words  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_runs.txt"))
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--burst", type=int, default=5)
args = ap.parse_args()
assert args.rounds >= 3 and args.burst >= 1

eng = ScanEngine(0)
lines = []
ALIGN = 65536  # rows: every shape is a multiple


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
            fn()
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


def report(name, what, same, t, gated, call):
    tc, tr = t[call], t["route"]
    verdict = ""
    if gated:
        verdict = " | gate: ok" if med(tc) < med(tr) and max(tc) < min(tr) else " | gate: **LOSES**"
    elif med(tc) >= med(tr):
        verdict = " | **slower than the route** (reported, not gated)"
    say(f"  {name}: {what}; results {'agree' if same else 'DIFFER'}")
    say(f"    {call} {fmt(tc)} | route {fmt(tr)} | route / {call} {med(tr) / med(tc):.2f}{verdict}")


def payload(n, c):
    return (n * c + 7) // 8


def runs_column(n, c, mean, seed):
    """n rows of c bits in runs of geometric length around `mean`: cumsum(head marks) mod 2^c, built in slices"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.empty(n, dtype=torch.int32, device="cuda")
    carry, step = 0, 1 << 27
    for at in range(0, n, step):
        m = min(step, n - at)
        heads = (torch.rand(m, generator=g, device="cuda") < 1.0 / mean).to(torch.int32)
        part = torch.cumsum(heads, 0, dtype=torch.int32) + carry
        carry = int(part[-1].item())
        x[at: at + m] = part & ((1 << c) - 1)
    col = eng.compress(x, c)
    del x
    torch.cuda.empty_cache()
    return col


class EncodeCase:
    def __init__(self, col, ce=None):
        self.col = col
        n, c = col.n, col.c
        self.ce = ce = ce or max(1, n.bit_length())
        self.values = torch.empty(compressed_buffer_size(c, n), dtype=torch.uint8, device="cuda")
        self.ends = torch.empty(compressed_buffer_size(ce, n), dtype=torch.uint8, device="cuda")
        self.count = torch.empty(1, dtype=torch.int64, device="cuda")
        self.ws = torch.empty(run_encode_workspace_words(n), dtype=torch.int64, device="cuda")
        self.dense = torch.empty(n, dtype=torch.int32, device="cuda")

    def call(self):
        return eng.run_encode(self.col, ends_width=self.ce, values=self.values, ends=self.ends, count=self.count, workspace=self.ws)

    def count_only(self):
        return eng.run_encode(self.col, capacity=0, ends_width=self.ce, values=False, ends=False, count=self.count, workspace=self.ws)

    def route(self):
        x = eng.decompress(self.col, out=self.dense)[: self.col.n]
        v, counts = torch.unique_consecutive(x, return_counts=True)
        e = torch.cumsum(counts, 0)
        return eng.compress(v, self.col.c), eng.compress(e.to(torch.int32), self.ce)

    def run(self, name, gated, extra=None):
        n, c, ce = self.col.n, self.col.c, self.ce
        want_v, want_e = self.route()
        self.call()
        r = int(self.count.item())
        same = r == want_v.n and torch.equal(self.values[: payload(r, c)], want_v.data[: payload(r, c)]) and \
            torch.equal(self.ends[: payload(r, ce)], want_e.data[: payload(r, ce)])
        del want_v, want_e
        torch.cuda.empty_cache()
        series = {"run_encode": (self.call, args.burst), "route": (self.route, slow_burst(self.route))}
        if extra:
            series.update(extra)
        t = measure(series)
        report(name, f"n = {n}, {c} bit, ends {ce} bit, r = {r} (mean run {n / max(r, 1):.1f})", same, t, gated, "run_encode")
        return t, r


class DecodeCase:
    def __init__(self, vcol, ecol, n):
        self.vcol, self.ecol, self.n = vcol, ecol, n
        self.out = torch.empty(compressed_buffer_size(vcol.c, n), dtype=torch.uint8, device="cuda")
        self.unc = torch.empty(1, dtype=torch.int64, device="cuda")
        self.zero = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call(self):
        return eng.run_decode(self.vcol, self.ecol, self.n, out=self.out, uncovered=self.unc)

    def route(self):
        r = self.vcol.n
        v = eng.decompress(self.vcol)[:r]
        e = eng.decompress(self.ecol)[:r]
        lengths = torch.diff(e, prepend=self.zero)
        return eng.compress(torch.repeat_interleave(v, lengths, output_size=self.n), self.vcol.c)

    def run(self, name, gated, extra=None):
        want = self.route()
        got = self.call()
        nb = payload(self.n, self.vcol.c)
        same = torch.equal(got.data[:nb], want.data[:nb]) and int(self.unc.item()) == 0
        del want
        torch.cuda.empty_cache()
        series = {"run_decode": (self.call, args.burst), "route": (self.route, slow_burst(self.route))}
        if extra:
            series.update(extra)
        t = measure(series)
        report(name, f"n = {self.n}, r = {self.vcol.n}, values {self.vcol.c} bit, ends {self.ecol.c} bit", same, t, gated, "run_decode")
        return t


def both(col, name, gated):
    """encode, then decode of what the encoder left -> (values column, ends column)"""
    enc = EncodeCase(col)
    t, r = enc.run(f"{name}, encode", gated)
    vcol, ecol = PackedColumn(enc.values, r, col.c), PackedColumn(enc.ends, r, enc.ce)
    del enc.dense
    torch.cuda.empty_cache()
    DecodeCase(vcol, ecol, col.n).run(f"{name}, decode", gated)
    return vcol, ecol


N1 = int(1_000_000_000 * args.scale) // ALIGN * ALIGN
N4 = int(250_000_000 * args.scale) // ALIGN * ALIGN

say(f"# run_encode and run_decode on {torch.cuda.get_device_name(0)}; scale={args.scale} rounds={args.rounds} burst={args.burst}")
say("# ms per call: median of the rounds [every round, in order]; calls back to back; the encoder writes both packed columns and its count")
say("# and uses a workspace of its caller's; the decoder writes the packed column and its counter")
say("# encoder's route: decompress -> torch.unique_consecutive(return_counts=True) -> cumsum -> compress x 2")
say("# decoder's route: decompress x 2 -> torch.diff -> torch.repeat_interleave -> compress")
say("# gate: the call's median below the route's and its slowest round below the route's fastest")
say()

say("gated")
col = runs_column(N1, 9, 4096, 1)
vcol, ecol = both(col, "1e9 x 9 bit, mean run 4096", True)
# a 1-bit column over those runs (a scan's result bitmap) expanded into the bitmap over the rows
bits, _ = eng.scan_where("<", 256, vcol)
DecodeCase(PackedColumn(bits, vcol.n, 1), ecol, N1).run("a 1-bit column over the runs of that shape -> the row bitmap", True)
del col, vcol, ecol, bits
torch.cuda.empty_cache()
col = runs_column(N1, 9, 64, 2)
both(col, "1e9 x 9 bit, mean run 64", True)
del col
torch.cuda.empty_cache()
g = torch.Generator(device="cuda").manual_seed(3)
asc = torch.sort(torch.randint(0, 1 << 17, (N4,), generator=g, device="cuda", dtype=torch.int32)).values
col17 = eng.compress(asc, 17)
del asc
torch.cuda.empty_cache()
EncodeCase(col17).run("a sorted uniform 2.5e8 x 17-bit column, encode", True)
del col17
torch.cuda.empty_cache()
say()

say("reported, not gated")
rnd = eng.generate("splitmix", N4, 9, 42)
enc = EncodeCase(rnd)
hits = torch.empty(1, dtype=torch.int64, device="cuda")
t, r = enc.run("a random 2.5e8 x 9-bit column, r ~ n (the encoder's worst case)", False,
               extra={"count-only scan": (lambda: eng.scan_combine("<", 3, rnd, hits=hits, count_only=True), args.burst),
                      "count only": (enc.count_only, args.burst)})
floor = 2 * med(t["count-only scan"])
say(f"    byte floor: two count-only scans of the column {floor:.3f} ms ({fmt(t['count-only scan'])} each) | run_encode / floor {med(t['run_encode']) / floor:.2f}"
    f" | count_runs {fmt(t['count only'])}")
del enc, rnd
torch.cuda.empty_cache()
col32 = runs_column(N4, 32, 64, 4)
enc = EncodeCase(col32, ce=32)
t, r = enc.run("2.5e8 x 32 bit with 32-bit ends, mean run 64, encode", False)
vcol, ecol = PackedColumn(enc.values, r, 32), PackedColumn(enc.ends, r, 32)
del enc.dense
torch.cuda.empty_cache()
floor_out = torch.empty(compressed_buffer_size(32, N4), dtype=torch.uint8, device="cuda")
t = DecodeCase(vcol, ecol, N4).run("2.5e8 x 32 bit with 32-bit ends, mean run 64, decode", False,
                                   extra={"arith": (lambda: eng.arith("linear", col32, col32, a=1, b=0, k=0, co=32, out=floor_out), args.burst)})
say(f"    against arith into the same width: arith {fmt(t['arith'])} | run_decode / arith {med(t['run_decode']) / med(t['arith']):.2f}")
del enc, vcol, ecol, col32, floor_out
torch.cuda.empty_cache()
# long stretches of zero-length runs: every 64th count is 4096, the others zero
rz = N4 // 64
counts = torch.zeros(rz, dtype=torch.int32, device="cuda")
counts[63::64] = 4096
ends = torch.cumsum(counts, 0, dtype=torch.int64)
nz = int(ends[-1].item())
vz = eng.generate("splitmix", rz, 9, 5)
ez = eng.compress(ends.to(torch.int32), max(1, nz.bit_length()))
DecodeCase(vz, ez, nz).run("a table with 63 zero-length runs in front of every run of 4096 rows, decode", False)

print(f"wrote {args.out}")
