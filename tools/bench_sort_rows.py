#!/usr/bin/env python3
"""sort_rows (ScanEngine.sort_rows: the row ids of a packed column's qualifying rows in value order, with the values) against the
route the library offered before it -- decompress -> torch.sort(stable=True); under a mask bitmap_to_rowids -> gather ->
torch.sort(stable=True) -> index into the ids; for ORDER BY v DESC LIMIT k, top_k -> sort_rows against decompress ->
torch.topk(sorted=True).  HIP events over back-to-back calls, every shape warmed, the series of a case interleaved in ONE
process; every result is compared with the route's before it is timed.  Writes profiles/r16_sort_rows.txt.

    python tools/bench_sort_rows.py [--out profiles/r16_sort_rows.txt] [--scale 1.0] [--rounds 5] [--burst 5]

Shapes (rows times --scale), uniform random values: 2.5e8 rows x 8, 9, 12, 16 bit (gated) and x 17, 24, 32 bit (reported), without
a mask; 1e9 rows x 9 bit under a random mask of density 1/8 (gated); 1e9 rows x 9 bit, the top 1e6 in order (gated).  Reported: an
all-equal and a sorted column of 2.5e8 rows x 9 bit, and the step from 8 to 9 bit (the cost of the second pass).  The gate: the
call's median below the route's, and no round of the call as slow as the route's fastest.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from shared_simd_scan_amd import PackedColumn, ScanEngine, sort_rows_passes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_sort_rows.txt"))
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--burst", type=int, default=5)
args = ap.parse_args()
assert args.rounds >= 3 and args.burst >= 1

eng = ScanEngine(0)
lines = []
medians = {}
ALIGN = 65536  # rows: every shape, and every shrunk one, is a multiple


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


def ordered(vals, c):
    """int32 values as torch orders them -> in the values' own order: c = 32 flips the sign bit (one more pass of the route)"""
    return vals.bitwise_xor_(-(1 << 31)) if c == 32 else vals


def once_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def report(name, what, same, t, gated, key=None):
    ts, tr = t["sort_rows"], t["route"]
    verdict = ""
    if gated:
        verdict = " | gate: ok" if med(ts) < med(tr) and ts[-1] < tr[0] else " | gate: **LOSES**"
    elif med(ts) >= med(tr):
        verdict = " | **slower than the route** (reported, not gated)"
    say(f"  {name}: {what}; results {'agree' if same else 'DIFFER'}")
    say(f"    sort_rows {fmt(ts)} | route {fmt(tr)} | route / sort_rows {med(tr) / med(ts):.2f}{verdict}")
    if key:
        medians[key] = med(ts)


def sort_case(col, mask, name, gated, key=None):
    """ORDER BY v: every qualifying row's id and value; a shape torch refuses or cannot hold is halved (that case only)"""
    while True:
        n, c = col.n, col.c
        q = n if mask is None else int(eng.bitmap_count(mask, n).item())
        try:
            dense = torch.empty(max(q, 1), dtype=torch.int32, device="cuda")

            def route():
                if mask is None:
                    vals = eng.decompress(col, out=dense)
                    sv, idx = torch.sort(ordered(vals, c), stable=True)
                    return idx, sv
                rowids, cnt = eng.bitmap_to_rowids(mask, n, max(q, 1))
                vals = eng.gather(col, rowids, cnt, out=dense)[:q]
                sv, idx = torch.sort(ordered(vals, c), stable=True)
                return rowids[idx], sv

            def call():
                return eng.sort_rows(col, mask=mask, capacity=q, with_values=True)

            want_ids, want_vals = route()
            ids, count, vals = call()
            same = int(count.item()) == q and torch.equal(ids[:q], want_ids[:q]) and torch.equal(ordered(vals[:q].clone(), c), want_vals[:q])
            del want_ids, want_vals, ids, vals
            slow = 1 if once_ms(route) > 20 else max(1, args.burst // 2)
            t = measure({"sort_rows": (call, args.burst), "route": (route, slow)})
        except RuntimeError as e:
            say(f"  {name}, {n} rows: torch refuses or runs out of memory ({str(e).splitlines()[0][:100]}); halving this shape")
            torch.cuda.empty_cache()
            half = n // 2 // ALIGN * ALIGN
            col = PackedColumn(col.data, half, col.c)
            mask = None if mask is None else mask[: half // 8]
            continue
        report(name, f"n = {n}, q = {q}, {sort_rows_passes(c)} pass(es)", same, t, gated, key)
        return


def limit_case(col, k, name):
    """ORDER BY v DESC LIMIT k: top_k -> sort_rows under its bitmap against decompress -> torch.topk(sorted=True).  torch breaks
    ties its own way: the values are compared, and the ids by the values they name"""
    n, c = col.n, col.c
    dense = torch.empty(n, dtype=torch.int32, device="cuda")
    bitmap = eng.alloc_bitmap(n)

    def route():
        return torch.topk(ordered(eng.decompress(col, out=dense), c), k, sorted=True)

    def call():
        top, _ = eng.top_k(col, k, largest=True, out=bitmap)
        return eng.sort_rows(col, descending=True, mask=top, capacity=k, with_values=True)

    want = route().values
    ids, count, vals = call()
    taken = eng.gather(col, ids, count)
    same = int(count.item()) == k and torch.equal(ordered(vals.clone(), c), want) and torch.equal(taken[:k], vals) and bool((ids[1:] != ids[:-1]).all())
    slow = 1 if once_ms(route) > 20 else max(1, args.burst // 2)
    t = measure({"sort_rows": (call, args.burst), "route": (route, slow)})
    report(name, f"n = {n}, k = {k}; sort_rows here is top_k -> sort_rows", same, t, True)


say(f"# sort_rows on {torch.cuda.get_device_name(0)}; scale={args.scale} rounds={args.rounds} burst={args.burst}")
say("# ms per call: median of the rounds [fastest .. slowest]; calls back to back; sort_rows returns row ids (int64) and values")
say("# route: decompress -> torch.sort(stable=True) (values and indices); under a mask bitmap_to_rowids -> gather -> torch.sort(stable=True)")
say("#        -> ids[indices]; c = 32 flips the sign bit in between (int32 order is not the values'); LIMIT k: decompress -> torch.topk(sorted=True)")
say("# gate: sort_rows' median below the route's and its slowest round below the route's fastest (uniform shapes of at most 16 bit)")
say()

N1, N4 = int(1_000_000_000 * args.scale) // ALIGN * ALIGN, int(250_000_000 * args.scale) // ALIGN * ALIGN
say(f"{N4} rows, uniform random, no mask")
for c in (8, 9, 12, 16, 17, 24, 32):
    sort_case(eng.generate("splitmix", N4, c, 42), None, f"{c} bit", c <= 16, key=c)
    torch.cuda.empty_cache()
if 8 in medians and 9 in medians:
    say(f"  the step from one pass to two: 9 bit / 8 bit = {medians[9] / medians[8]:.2f} ({medians[9] - medians[8]:+.3f} ms); the last pass of 8 bit scatters"
        " ids and values into 256 buckets, that of 9 bit into 2")
say()

say(f"{N1} rows x 9 bit, uniform random, under a random mask of density 1/8")
col = eng.generate("splitmix", N1, 9, 42)
g = torch.Generator(device="cuda").manual_seed(1234)
mask = torch.randint(0, 256, (N1 // 8,), dtype=torch.uint8, generator=g, device="cuda")
for _ in range(2):
    mask &= torch.randint(0, 256, (N1 // 8,), dtype=torch.uint8, generator=g, device="cuda")
sort_case(col, mask, "mask 1/8", True)
del mask
torch.cuda.empty_cache()
say()
say(f"{N1} rows x 9 bit, uniform random: ORDER BY v DESC LIMIT k")
limit_case(col, min(1_000_000, N1 // 4), "k = 1e6")
del col
torch.cuda.empty_cache()
say()

say(f"{N4} rows x 9 bit, all equal (reported, not gated): one bucket takes every row, every rank of a step comes from one offset")
sort_case(eng.generate("mod", N4, 9, 1), None, "all equal", False)
torch.cuda.empty_cache()
say()
say(f"{N4} rows x 9 bit, sorted ascending (reported, not gated): every span scatters into one or two buckets")
asc = (torch.arange(N4, dtype=torch.int64, device="cuda") * 512 // N4).to(torch.int32)
sort_case(eng.compress(asc, 9), None, "sorted", False)

print(f"wrote {args.out}")
