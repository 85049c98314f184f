#!/usr/bin/env python3
"""value_set (ScanEngine.value_set: the set of a packed column's values as a bitmap over the value domain) and dense_codes
(value_set -> set_ranks -> lookup) against the routes the library offered before them -- decompress -> torch.unique; under a mask
bitmap_to_rowids -> gather -> torch.unique; for the codes decompress -> torch.unique(return_inverse=True) -> compress.  HIP events
over back-to-back calls, every shape warmed, the series of a case interleaved in ONE process; every result is compared with the
route's before it is timed.  Writes profiles/r19_value_set.txt.

    python tools/bench_value_set.py [--out profiles/r19_value_set.txt] [--scale 1.0] [--rounds 5] [--burst 5]

Shapes (rows times --scale), uniform random values.  Gated: 1e9 rows x 9 bit, 2.5e8 x 17 bit and x 24 bit over the domain 2^c;
1e9 x 9 bit under a random mask of density 1/8; dense_codes of 2.5e8 x 24 bit.  Reported: 2.5e8 x 32 bit into a set of 2^32 bits;
all-equal, sorted and Zipf-like columns (every lane of a wave hits one word); the LDS tier beside histogram on the same column at
9, 12 and 14 bit and beside a count-only scan (the byte floor); the global tier beside semi_join against a set of the same size
(the same gather without the atomics).  The gate: the call's median below the route's, and no round of the call as slow as the
route's fastest.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from shared_simd_scan_amd import PackedColumn, ScanEngine, value_set_kernel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_value_set.txt"))
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--burst", type=int, default=5)
args = ap.parse_args()
assert args.rounds >= 3 and args.burst >= 1

eng = ScanEngine(0)
lines = []
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


def once_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def slow_burst(fn):
    return 1 if once_ms(fn) > 20 else max(1, args.burst // 2)


def report(name, what, same, t, gated, call="value_set"):
    tc, tr = t[call], t["route"]
    verdict = ""
    if gated:
        verdict = " | gate: ok" if med(tc) < med(tr) and tc[-1] < tr[0] else " | gate: **LOSES**"
    elif med(tc) >= med(tr):
        verdict = " | **slower than the route** (reported, not gated)"
    say(f"  {name}: {what}; results {'agree' if same else 'DIFFER'}")
    say(f"    {call} {fmt(tc)} | route {fmt(tr)} | route / {call} {med(tr) / med(tc):.2f}{verdict}")


def as_values(ids, c):
    """the set's row ids (int64) as torch.unique orders the decoded int32 values: c = 32 wraps the upper half below zero"""
    v = ids.to(torch.int32) if c < 32 else ids.to(torch.int64).add(1 << 31).remainder(1 << 32).sub(1 << 31).to(torch.int32)
    return torch.sort(v).values if c == 32 else v


def value_set_case(col, mask, name, gated, extra=None):
    """the distinct values of the selected rows; a shape torch refuses or cannot hold is halved (that case only)"""
    while True:
        n, c = col.n, col.c
        m = 1 << c
        try:
            q = n if mask is None else int(eng.bitmap_count(mask, n).item())
            dense = torch.empty(max(q, 1), dtype=torch.int32, device="cuda")
            sbuf = torch.empty((m + 7) // 8 + 32, dtype=torch.uint8, device="cuda")
            cnt = torch.empty(2, dtype=torch.int64, device="cuda")

            def route():
                if mask is None:
                    return torch.unique(eng.decompress(col, out=dense))
                rowids, k = eng.bitmap_to_rowids(mask, n, max(q, 1))
                return torch.unique(eng.gather(col, rowids, k, out=dense)[:q])

            def call():
                return eng.value_set(col, m, mask=mask, out=sbuf, counts=cnt)

            want = route()
            vset, counts = call()
            d = int(counts[0].item())
            ids, k = eng.bitmap_to_rowids(vset, m, max(min(d, want.numel()), 1))
            same = d == want.numel() and int(counts[1].item()) == 0 and int(k.item()) == d and torch.equal(as_values(ids[:d], c), want)
            del want, ids
            series = {"value_set": (call, args.burst), "route": (route, slow_burst(route))}
            if extra:
                series.update(extra(col))
            t = measure(series)
        except RuntimeError as e:
            say(f"  {name}, {n} rows: torch refuses or runs out of memory ({str(e).splitlines()[0][:100]}); halving this shape")
            torch.cuda.empty_cache()
            half = n // 2 // ALIGN * ALIGN
            col = PackedColumn(col.data, half, col.c)
            mask = None if mask is None else mask[: half // 8]
            continue
        report(name, f"n = {n}, q = {q}, {d} distinct, {value_set_kernel(c, m)}", same, t, gated)
        for other in t:
            if other not in ("value_set", "route"):
                slower = " | **value_set is slower**" if med(t["value_set"]) > med(t[other]) else ""
                say(f"    beside {other} {fmt(t[other])}: value_set / {other} {med(t['value_set']) / med(t[other]):.2f}{slower}")
        return


def beside_lds(col):
    """the LDS tier's neighbours on the same column: histogram (c <= 14: strictly more work per value) and a count-only scan (the bytes)"""
    out = {"count-only scan": (lambda: eng.scan_combine("==", 3, col, count_only=True), args.burst)}
    if col.c <= 14:
        hist = torch.empty(1 << col.c, dtype=torch.int64, device="cuda")
        out["histogram"] = (lambda: eng.histogram(col, out=hist), args.burst)
    return out


def beside_global(col):
    """the global tier's neighbour: semi_join of the same column against a set of the same size, count only -- the same gather, no atomics"""
    m = 1 << col.c
    probe = torch.zeros((m + 7) // 8, dtype=torch.uint8, device="cuda")
    return {"semi_join": (lambda: eng.semi_join(col, probe, m, bitmap=False), args.burst)}


def dense_codes_case(col, name):
    n, c = col.n, col.c
    dense = torch.empty(n, dtype=torch.int32, device="cuda")
    d = eng.count_distinct(col)
    ct = max(1, (d - 1).bit_length())

    def route():
        values, inverse = torch.unique(eng.decompress(col, out=dense), return_inverse=True)
        return eng.compress(inverse.to(torch.int32), ct), values

    def call():
        return eng.dense_codes(col, ct=ct)

    want_codes, want_values = route()
    codes, values, count = call()
    same = (int(count.item()) == d == want_values.numel() and torch.equal(values[:d].to(torch.int32), want_values)
            and torch.equal(codes.data[: (n * ct + 7) // 8], want_codes.data[: (n * ct + 7) // 8]))
    del want_codes, want_values, codes, values
    torch.cuda.empty_cache()
    t = measure({"dense_codes": (call, max(1, args.burst // 2)), "route": (route, slow_burst(route))})
    report(name, f"n = {n}, {d} distinct, codes of {ct} bit; dense_codes here is value_set -> set_ranks -> lookup -> bitmap_to_rowids", same, t, True, call="dense_codes")


say(f"# value_set on {torch.cuda.get_device_name(0)}; scale={args.scale} rounds={args.rounds} burst={args.burst}")
say("# ms per call: median of the rounds [fastest .. slowest]; calls back to back; value_set writes the set (2^c bits) and two counts")
say("# route: decompress -> torch.unique; under a mask bitmap_to_rowids -> gather -> torch.unique; dense_codes: decompress ->")
say("#        torch.unique(return_inverse=True) -> compress at the same width")
say("# gate: the call's median below the route's and its slowest round below the route's fastest")
say()

N1, N4 = int(1_000_000_000 * args.scale) // ALIGN * ALIGN, int(250_000_000 * args.scale) // ALIGN * ALIGN
say("uniform random over the domain 2^c, no mask (gated)")
col9 = eng.generate("splitmix", N1, 9, 42)
value_set_case(col9, None, "1e9 x 9 bit", True, extra=beside_lds)
torch.cuda.empty_cache()
value_set_case(eng.generate("splitmix", N4, 17, 42), None, "2.5e8 x 17 bit", True, extra=beside_lds)
torch.cuda.empty_cache()
col24 = eng.generate("splitmix", N4, 24, 42)
value_set_case(col24, None, "2.5e8 x 24 bit", True, extra=beside_global)
torch.cuda.empty_cache()
say()

say(f"{N1} rows x 9 bit, uniform random, under a random mask of density 1/8 (gated)")
g = torch.Generator(device="cuda").manual_seed(1234)
mask = torch.randint(0, 256, (N1 // 8,), dtype=torch.uint8, generator=g, device="cuda")
for _ in range(2):
    mask &= torch.randint(0, 256, (N1 // 8,), dtype=torch.uint8, generator=g, device="cuda")
value_set_case(col9, mask, "mask 1/8", True)
del mask, col9
torch.cuda.empty_cache()
say()

say(f"dense_codes, {N4} rows x 24 bit, uniform random (gated)")
dense_codes_case(col24, "2.5e8 x 24 bit")
del col24
torch.cuda.empty_cache()
say()

say("reported, not gated")
value_set_case(eng.generate("splitmix", N4, 32, 42), None, "2.5e8 x 32 bit into 2^32 bits", False)
torch.cuda.empty_cache()
for c in (12, 14):
    value_set_case(eng.generate("splitmix", N4, c, 42), None, f"2.5e8 x {c} bit, the LDS tier beside histogram", False, extra=beside_lds)
    torch.cuda.empty_cache()
for c in (9, 24):
    value_set_case(eng.generate("mod", N4, c, 1), None, f"all equal, {c} bit", False)
    asc = (torch.arange(N4, dtype=torch.int64, device="cuda") * (1 << c) // N4).to(torch.int32)
    value_set_case(eng.compress(asc, c), None, f"sorted, {c} bit", False)
    del asc
    zipf = (torch.rand(N4, device="cuda", generator=g).pow_(8.0) * float(1 << c)).to(torch.int32).clamp_(0, (1 << c) - 1)
    value_set_case(eng.compress(zipf, c), None, f"Zipf-like (2^c u^8), {c} bit", False)
    del zipf
    torch.cuda.empty_cache()

print(f"wrote {args.out}")
