#!/usr/bin/env python3
"""key_index (ScanEngine.key_index: the first or last row of every key of a packed column, as the packed table lookup reads)
against the route the library offered before it -- decompress -> int64 -> torch.Tensor.scatter_reduce_(amin / amax,
include_self=False) of the row index into a dense table -> compress.  HIP events over back-to-back calls, every shape warmed, the
series of a case interleaved in ONE process; every table is compared with the route's before it is timed.  Writes
profiles/r20_key_index.txt.

    python tools/bench_key_index.py [--out profiles/r20_key_index.txt] [--scale 1.0] [--rounds 5] [--burst 5]

Shapes (rows times --scale), uniform random keys over the domain 2^c unless noted.  Gated, one per tier: 2.5e8 rows x 14 bit (the
LDS tier, heavy duplicates: "the latest row per key", keep = last) and 2.5e8 x 24 bit (the global tier, keep = first).  Reported: a
1e6-row permutation at 20 bit, a 4096-row dimension at 12 bit, an all-equal and a sorted column at 24 bit (keep = first at 2.5e8
rows, keep = last at a 64th of them: the route's amax on one address does not end within minutes at the full size), and the
three-call join (key_index -> lookup -> lookup) against the route through torch indexing.  The gate: the call's median below the route's, and no
round of the call as slow as the route's fastest.  The route is handed the row indices (an int64 arange) ready-made.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from shared_simd_scan_amd import PackedColumn, ScanEngine, key_index_kernel  # noqa: E402,F401

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_key_index.txt"))
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


def report(name, what, same, t, gated, call="key_index"):
    tc, tr = t[call], t["route"]
    verdict = ""
    if gated:
        verdict = " | gate: ok" if med(tc) < med(tr) and tc[-1] < tr[0] else " | gate: **LOSES**"
    elif med(tc) >= med(tr):
        verdict = " | **slower than the route** (reported, not gated)"
    say(f"  {name}: {what}; results {'agree' if same else 'DIFFER'}")
    say(f"    {call} {fmt(tc)} | route {fmt(tr)} | route / {call} {med(tr) / med(tc):.2f}{verdict}")


def key_index_case(col, keep, name, gated, extra=None):
    """the first / last row of every key of `col` over its whole domain, at the width that holds n, miss = n"""
    n, c = col.n, col.c
    m = 1 << c
    ct = max(1, n.bit_length())
    dense = torch.empty(n, dtype=torch.int32, device="cuda")
    rows = torch.arange(n, dtype=torch.int64, device="cuda")
    out = torch.empty((m * ct + 7) // 8 + 256, dtype=torch.uint8, device="cuda")
    cnt = torch.empty(4, dtype=torch.int64, device="cuda")

    def route():
        k = eng.decompress(col, out=dense)[:n].to(torch.int64)
        table = torch.full((m,), n, dtype=torch.int64, device="cuda")
        table.scatter_reduce_(0, k, rows, reduce="amin" if keep == "first" else "amax", include_self=False)
        return eng.compress(table.to(torch.int32), ct)

    def call():
        return eng.key_index(col, m, ct, keep=keep, out=out, counts=cnt)

    want = route()
    table, counts = call()
    nb = (m * ct + 7) // 8
    members = int(counts[0].item())
    same = torch.equal(table.data[:nb], want.data[:nb]) and counts[1:].tolist() == [0, n, 0]
    del want
    torch.cuda.empty_cache()
    series = {"key_index": (call, args.burst), "route": (route, slow_burst(route))}
    if extra:
        series.update(extra(col))
    t = measure(series)
    report(name, f"n = {n}, keep = {keep}, {members} of {m} keys have a row, table of {ct} bit, {key_index_kernel(c, m)}", same, t, gated)
    for other in t:
        if other not in ("key_index", "route"):
            slower = " | **key_index is slower**" if med(t["key_index"]) > med(t[other]) else ""
            say(f"    beside {other} {fmt(t[other])}: key_index / {other} {med(t['key_index']) / med(t[other]):.2f}{slower}")
    del dense, rows, out
    torch.cuda.empty_cache()


def beside_value_set(col):
    """value_set on the same column: the same pipeline with a bit where key_index keeps a row"""
    m = 1 << col.c
    sbuf = torch.empty((m + 7) // 8 + 32, dtype=torch.uint8, device="cuda")
    cnt = torch.empty(2, dtype=torch.int64, device="cuda")
    return {"value_set": (lambda: eng.value_set(col, m, out=sbuf, counts=cnt), args.burst)}


def join_case(n_fact, name):
    """SELECT d.a FROM fact f JOIN dim d ON f.fk = d.pk: a dimension of 1e6 rows whose pk is a random subset of a 20-bit domain
    in random order, a 12-bit attribute, a fact column of 20-bit foreign keys (about 5 % absent from the dimension)"""
    ck, ca, miss = 20, 12, 4095
    rows_dim = 1_000_000
    g = torch.Generator(device="cuda").manual_seed(77)
    pk = torch.randperm(1 << ck, device="cuda", generator=g)[:rows_dim].to(torch.int32)
    attr = torch.randint(0, 1 << ca, (rows_dim,), dtype=torch.int32, device="cuda", generator=g)
    pcol, acol = eng.compress(pk, ck), eng.compress(attr, ca)
    fcol = eng.generate("splitmix", n_fact, ck, 7)
    del pk, attr
    dense_pk, dense_attr = torch.empty(rows_dim, dtype=torch.int32, device="cuda"), torch.empty(rows_dim + 1, dtype=torch.int32, device="cuda")
    dense_fk = torch.empty(n_fact, dtype=torch.int32, device="cuda")
    dim_rows = torch.arange(rows_dim, dtype=torch.int64, device="cuda")

    def route():
        p = eng.decompress(pcol, out=dense_pk)[:rows_dim].to(torch.int64)
        a = eng.decompress(acol, out=dense_attr)
        a[rows_dim] = miss
        table = torch.full((1 << ck,), rows_dim, dtype=torch.int64, device="cuda")
        table[p] = dim_rows
        f = eng.decompress(fcol, out=dense_fk)[:n_fact].to(torch.int64)
        return eng.compress(a[table[f]], ca)

    def call():
        index, _ = eng.key_index(pcol)
        return eng.lookup(eng.lookup(fcol, index, miss=rows_dim), acol, miss=miss)

    want, got = route(), call()
    nb = (n_fact * ca + 7) // 8
    same = torch.equal(got.data[:nb], want.data[:nb])
    del want, got
    torch.cuda.empty_cache()
    t = measure({"join": (call, max(1, args.burst // 2)), "route": (route, slow_burst(route))})
    report(name, f"{n_fact} fact rows x {ck} bit, dimension of {rows_dim} rows, attribute of {ca} bit; join here is key_index -> lookup -> lookup",
           same, t, False, call="join")


say(f"# key_index on {torch.cuda.get_device_name(0)}; scale={args.scale} rounds={args.rounds} burst={args.burst}")
say("# ms per call: median of the rounds [fastest .. slowest]; calls back to back; key_index writes the table (2^c entries at the")
say("# width that holds n, miss = n) and four counts")
say("# route: decompress -> int64 -> scatter_reduce_(amin / amax, include_self=False) of the row index into a dense int64 table ->")
say("#        int32 -> compress at the same width; the row indices (an int64 arange) are handed to it ready-made")
say("# gate: the call's median below the route's and its slowest round below the route's fastest")
say()

N4 = int(250_000_000 * args.scale) // ALIGN * ALIGN
say("uniform random over the domain 2^c, no mask (gated, one shape per tier)")
key_index_case(eng.generate("splitmix", N4, 14, 42), "last", "2.5e8 x 14 bit, the latest row per key", True, extra=beside_value_set)
col24 = eng.generate("splitmix", N4, 24, 42)
key_index_case(col24, "first", "2.5e8 x 24 bit", True, extra=beside_value_set)
del col24
torch.cuda.empty_cache()
say()

say("reported, not gated")
g = torch.Generator(device="cuda").manual_seed(1234)
perm = torch.randperm(1 << 20, device="cuda", generator=g)[:1_000_000].to(torch.int32)
key_index_case(eng.compress(perm, 20), "first", "1e6-row permutation, 20 bit", False)
del perm
key_index_case(eng.compress(torch.randperm(4096, device="cuda", generator=g).to(torch.int32), 12), "first", "4096-row dimension, 12 bit", False)
# keep = last on a 64th of the rows: there every later row of a key wins, and the route's amax on one address (the all-equal
# column) does not end within minutes at 2.5e8 rows
for keep, rows in (("first", N4), ("last", N4 // 64 // ALIGN * ALIGN)):
    print(f"  ... all equal and sorted, keep = {keep}, {rows} rows", flush=True)
    key_index_case(eng.generate("mod", rows, 24, 1), keep, f"all equal, 24 bit, {rows} rows", False)
    asc = (torch.arange(rows, dtype=torch.int64, device="cuda") * (1 << 24) // rows).to(torch.int32)
    key_index_case(eng.compress(asc, 24), keep, f"sorted, 24 bit, {rows} rows", False)
    del asc
    torch.cuda.empty_cache()
print("  ... the join", flush=True)
join_case(N4, "the three-call join")

print(f"wrote {args.out}")
