#!/usr/bin/env python3
"""search_sorted (ScanEngine.search_sorted: a packed column's positions in a sorted packed table, the bitmap of the rows whose value
occurs in it and their number) against the route the library offered before it -- decompress -> torch.searchsorted -> compress,
with torch.isin for the bitmap; int64 where values reach 2^31.  HIP events over back-to-back calls, every shape warmed, the series
of a case interleaved in ONE process; every output is compared with the route's before it is timed.  Writes
profiles/r23_search_sorted.txt.

    python tools/bench_search_sorted.py [--out profiles/r23_search_sorted.txt] [--scale 1.0] [--rounds 5] [--burst 5]

Shapes (rows times --scale).  Gated: 1e9 rows x 9 bit into 256 edges (the LDS tier, positions under side="right"); 2.5e8 x 32 bit
against 1e6 sorted 32-bit keys (the global tier, exact positions); the same with the found bitmap and the hit count only.
Reported: 2^24 entries, and L and L + 1 entries (the tier boundary from both sides); a sorted probe column; sparse_lookup end to end
against torch; the call against lookup on the same n and output width (its floor).  The gate: the call's median below the
route's, and no round of the call as slow as the route's fastest.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from shared_simd_scan_amd import PackedColumn, ScanEngine, compressed_buffer_size, search_sorted_kernel, search_sorted_stride  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_search_sorted.txt"))
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--burst", type=int, default=5)
args = ap.parse_args()
assert args.rounds >= 3 and args.burst >= 1

eng = ScanEngine(0)
lines = []
ALIGN = 65536  # rows: every shape is a multiple
LMAX = 98240 // 4  # MI355_SEARCH_LDS_MAX_BYTES / 4: the largest table of the LDS tier
assert search_sorted_stride(LMAX) == 1 and search_sorted_stride(LMAX + 1) == 2


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


def report(name, what, same, t, gated, call="search_sorted"):
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


def dense(col):
    """the column's values as torch compares them: int32 below 32 bits, int64 (unsigned) at 32"""
    x = eng.decompress(col)[: col.n]
    return x if col.c < 32 else x.to(torch.int64) & 0xFFFFFFFF


def sorted_table(rows, ct, seed):
    """`rows` sorted values of ct bits (repeats as they fall) -> (PackedColumn, what torch searches: int32, or int64 at 32 bits)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.sort(torch.randint(0, 1 << ct, (rows,), generator=g, device="cuda", dtype=torch.int64)).values
    return eng.compress(t.to(torch.int32), ct), (t if ct == 32 else t.to(torch.int32))


def probe_column(n, c, table64, seed, share=0.5):
    """n rows of c bits: `share` of them entries of the table, the others uniform"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.empty(n, dtype=torch.int32, device="cuda")
    step = 1 << 27
    for at in range(0, n, step):
        m = min(step, n - at)
        v = torch.randint(0, 1 << c, (m,), generator=g, device="cuda", dtype=torch.int64)
        pick = table64[torch.randint(0, table64.numel(), (m,), generator=g, device="cuda")].to(torch.int64)
        v = torch.where(torch.rand(m, generator=g, device="cuda") < share, pick, v)
        x[at: at + m] = v.to(torch.int32)  # (wraps into the int32 view of the same 32 bits)
        del v, pick
    col = eng.compress(x, c)
    del x
    torch.cuda.empty_cache()
    return col


class Case:
    """one column against one table: positions (side, exact) or the found bitmap and the hit count"""

    def __init__(self, col, table, table_t, side="left", exact=False, member=False):
        self.col, self.table, self.table_t, self.side, self.exact, self.member = col, table, table_t, side, exact, member
        n, rows = col.n, table.n
        self.co = max(1, rows.bit_length())
        self.out = torch.empty(compressed_buffer_size(self.co, n), dtype=torch.uint8, device="cuda")
        self.found = torch.empty((n + 7) // 8, dtype=torch.uint8, device="cuda")
        self.hits = torch.empty(1, dtype=torch.int64, device="cuda")

    def call(self):
        if self.member:
            return eng.search_sorted(self.col, self.table, out=False, found=self.found, hits=self.hits)
        return eng.search_sorted(self.col, self.table, side=self.side, exact=self.exact, miss=self.table.n if self.exact else 0, co=self.co, out=self.out)

    def route(self):
        x = dense(self.col)
        if self.member:
            m = torch.isin(x, self.table_t)
            return eng.compress(m.to(torch.int32), 1), m.sum()
        pos = torch.searchsorted(self.table_t, x, right=self.side == "right", out_int32=True)
        if self.exact:
            rows = self.table.n
            hit = self.table_t[torch.clamp(pos, max=rows - 1).to(torch.int64)] == x
            if self.side == "left":
                hit &= pos < rows
            pos = torch.where(hit, pos, torch.full_like(pos, rows))
        return eng.compress(pos, self.co), None

    def run(self, name, gated, extra=None):
        n, rows = self.col.n, self.table.n
        want, want_hits = self.route()
        self.call()
        if self.member:
            nb = (n + 7) // 8
            same = torch.equal(self.found[:nb], want.data[:nb]) and int(self.hits.item()) == int(want_hits.item())
            what = "found bitmap and hits"
        else:
            nb = payload(n, self.co)
            same = torch.equal(self.out[:nb], want.data[:nb])
            what = f"positions at {self.co} bit, side {self.side}{', exact' if self.exact else ''}"
        del want
        torch.cuda.empty_cache()
        series = {"search_sorted": (self.call, args.burst), "route": (self.route, slow_burst(self.route))}
        if extra:
            series.update(extra)
        t = measure(series)
        kernel = search_sorted_kernel(self.col.c, self.table.c, self.co, rows)
        report(name, f"n = {n}, {self.col.c} bit, {rows} entries of {self.table.c} bit, {what}, {kernel}, S = {search_sorted_stride(rows)}", same, t, gated)
        return t


N1 = int(1_000_000_000 * args.scale) // ALIGN * ALIGN
N4 = int(250_000_000 * args.scale) // ALIGN * ALIGN

say(f"# search_sorted on {torch.cuda.get_device_name(0)}; scale={args.scale} rounds={args.rounds} burst={args.burst}")
say("# ms per call: median of the rounds [every round, in order]; calls back to back")
say("# route: decompress -> torch.searchsorted(out_int32) [-> the equal-entry test -> torch.where] -> compress; int64 values at 32 bits;")
say("# for the bitmap: decompress -> torch.isin -> compress at 1 bit, and sum")
say("# gate: the call's median below the route's and its slowest round below the route's fastest")
say()

say("gated")
edges, edges_t = sorted_table(256, 9, 1)
col9 = eng.generate("splitmix", N1, 9, 42)
floor9 = torch.empty(compressed_buffer_size(9, N1), dtype=torch.uint8, device="cuda")
recode = eng.generate("splitmix", 512, 9, 7)
t = Case(col9, edges, edges_t, side="right").run("1e9 x 9 bit into 256 edges", True, extra={"lookup": (lambda: eng.lookup(col9, recode, out=floor9), args.burst)})
say(f"    its floor, lookup of the same column through a 512-entry table into 9 bit: {fmt(t['lookup'])} | search_sorted / lookup {med(t['search_sorted']) / med(t['lookup']):.2f}")
del col9, floor9
torch.cuda.empty_cache()
keys, keys_t = sorted_table(1_000_000, 32, 2)
col32 = probe_column(N4, 32, keys_t, 3)
Case(col32, keys, keys_t, exact=True).run("2.5e8 x 32 bit against 1e6 sorted 32-bit keys", True)
Case(col32, keys, keys_t, member=True).run("the same, found bitmap and hits only", True)
say()

say("reported, not gated")
big, big_t = sorted_table(1 << 24, 32, 4)
Case(col32, big, big_t).run("2^24 entries", False)
del big, big_t
for rows in (LMAX, LMAX + 1):
    tab, tab_t = sorted_table(rows, 32, 5)
    Case(col32, tab, tab_t).run(f"{'L' if rows == LMAX else 'L + 1'} entries (the tier boundary)", False)
    del tab, tab_t
sorted_probe = eng.compress(torch.sort(dense(col32)).values.to(torch.int32), 32)
Case(sorted_probe, keys, keys_t, exact=True).run("a sorted probe column against the 1e6 keys", False)
del sorted_probe
torch.cuda.empty_cache()
# the call against lookup on the same n and output width: a 20-bit column through a 1e6-entry table of 20-bit entries
idx20 = eng.generate("splitmix", N4, 20, 9)
tab20 = eng.generate("splitmix", 1_000_000, 20, 10)
out20 = torch.empty(compressed_buffer_size(20, N4), dtype=torch.uint8, device="cuda")
t = Case(col32, keys, keys_t, exact=True).run("against lookup on the same n and output width (2.5e8 rows, 1e6 entries, 20 bit out)", False,
                                             extra={"lookup": (lambda: eng.lookup(idx20, tab20, out=out20), args.burst)})
say(f"    lookup {fmt(t['lookup'])} | search_sorted / lookup {med(t['search_sorted']) / med(t['lookup']):.2f}")
del idx20, tab20, out20
torch.cuda.empty_cache()
# sparse_lookup end to end: the dimension's keys in random order with a 9-bit attribute
g = torch.Generator(device="cuda").manual_seed(11)
perm = torch.randperm(keys.n, generator=g, device="cuda")
dim_t = keys_t[perm]
dim_keys = eng.compress(dim_t.to(torch.int32), 32)
dim_attr = eng.generate("splitmix", keys.n, 9, 12)


def sparse_call():
    return eng.sparse_lookup(col32, dim_keys, dim_attr, miss=511)


def sparse_route():
    k, order = torch.sort(dense(dim_keys), stable=True)
    a = dense(dim_attr)[order]
    x = dense(col32)
    pos = torch.searchsorted(k, x)
    at = torch.clamp(pos, max=k.numel() - 1)
    return eng.compress(torch.where(k[at] == x, a[at], torch.full_like(a[at], 511)), 9)


want, got = sparse_route(), sparse_call()
same = torch.equal(got.data[: payload(N4, 9)], want.data[: payload(N4, 9)])
del want, got
torch.cuda.empty_cache()
t = measure({"sparse_lookup": (sparse_call, max(1, args.burst // 2)), "route": (sparse_route, slow_burst(sparse_route))})
report("sparse_lookup end to end", f"n = {N4}, 32-bit keys, a dimension of {keys.n} rows in random order, a 9-bit attribute", same, t, False, call="sparse_lookup")

print(f"wrote {args.out}")
