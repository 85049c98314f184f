#!/usr/bin/env python3
"""top_k (ScanEngine.top_k: the k largest rows of a packed column, as a bitmap) against the route the library offered before it
-- decompress -> torch.topk (torch.kthvalue for k = n / 2); under a mask bitmap_to_rowids -> gather -> torch.topk / kthvalue --
and against its byte floor, (mi355_top_k_passes(c) + 1) count-only scans of the same column.  HIP events over back-to-back calls,
every shape warmed, all series of a case interleaved in ONE process; every result is compared with the route's before it is
timed.  Writes profiles/r13_top_k.txt.

    python tools/bench_top_k.py [--out profiles/r13_top_k.txt] [--scale 1.0] [--rounds 5] [--burst 10]

Shapes (rows times --scale): uniform random values, 1e9 rows x 9 bit and 2.5e8 rows x 17 / 32 bit, k = 1, 100, 1e6, n / 2, without
a mask and under a random mask of density 1/8 (k = n / 2 then means half of the qualifying rows); one all-equal column (1e9 x 9
bit, k = n / 2) and one sorted column (2.5e8 x 32 bit, value = row id).  The gate (uniform shapes only): the call's median below
the route's, and no round of the call as slow as the route's fastest.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from shared_simd_scan_amd import PackedColumn, ScanEngine, top_k_passes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_top_k.txt"))
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--burst", type=int, default=10)
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
    """series: {name: (callable, burst)}; alternating rounds of `burst` back-to-back calls -> {name: sorted ms per call}.
    burst == 0: a call that takes seconds -- one call a round, three rounds, no call in front of the timed one"""
    times = {k: [] for k in series}
    for fn, burst in series.values():  # every shape warmed
        if burst:
            fn()
    torch.cuda.synchronize()
    for r in range(args.rounds):
        for name, (fn, burst) in series.items():
            if burst == 0 and r >= 3:
                continue
            if burst:
                fn()
            burst = max(burst, 1)
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


def route_of(col, mask, q, k):
    """the route's callable -> the k-th largest value as a device scalar.  c = 32: int32 order is not the values' order, so the
    sign bit is flipped on the way (one more pass; the k-th value is flipped back)"""
    n, c = col.n, col.c
    dense = torch.empty(n if mask is None else max(q, 1), dtype=torch.int32, device="cuda")

    def route():
        if mask is None:
            vals = eng.decompress(col, out=dense)
        else:
            rowids, cnt = eng.bitmap_to_rowids(mask, n, max(q, 1))
            vals = eng.gather(col, rowids, cnt, out=dense)[:q]
        if c == 32:
            vals = vals.bitwise_xor_(-(1 << 31))
        kth = torch.kthvalue(vals, q - k + 1).values if 2 * k >= q else torch.topk(vals, k, sorted=False).values.min()
        return kth.to(torch.int64) + (1 << 31) if c == 32 else kth.to(torch.int64)

    return route


def case(col, mask, k_of, name, gated):
    """one line of the file; a shape torch refuses or cannot hold is halved (that case only) until it runs"""
    passes = top_k_passes(col.c)
    while True:
        n = col.n
        q = n if mask is None else int(eng.bitmap_count(mask, n).item())
        k = k_of(q)
        bitmap, result = eng.alloc_bitmap(n), None
        route = route_of(col, mask, q, k)

        def call():
            return eng.top_k(col, k, largest=True, mask=mask, out=bitmap)

        def count_only():
            return eng.scan_combine("==", 1, col, count_only=True)

        try:
            want = int(route().item())
        except RuntimeError as e:
            say(f"  {name}, {n} rows: torch refuses or runs out of memory ({str(e).splitlines()[0][:100]}); halving this shape")
            del route
            torch.cuda.empty_cache()
            half = n // 2 // ALIGN * ALIGN
            col = PackedColumn(col.data, half, col.c)
            mask = None if mask is None else mask[: half // 8]
            continue
        _, result = call()
        m, T, beyond, ties = (int(x) for x in result.tolist())
        same = m == min(k, q) == int(eng.bitmap_count(bitmap, n).item()) and T == want
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        route()
        e1.record()
        e1.synchronize()
        once = e0.elapsed_time(e1)
        slow = 0 if once > 1000 else (1 if once > 20 else max(1, args.burst // 5))  # a slow route is not called ten times a round
        t = measure({"top_k": (call, args.burst), "route": (route, slow), "scan": (count_only, args.burst)})
        tk, tr, floor = t["top_k"], t["route"], (passes + 1) * med(t["scan"])
        verdict = ""
        if gated:
            verdict = " | gate: ok" if med(tk) < med(tr) and tk[-1] < tr[0] else " | gate: **LOSES**"
        say(f"  {name}: n = {n}, q = {q}, k = {k}, T = {T}, ties {ties}, kept {m - beyond}; results {'agree' if same else 'DIFFER'}")
        say(f"    top_k {fmt(tk)} | route {fmt(tr)} | route / top_k {med(tr) / med(tk):.2f}"
            f" | floor {passes + 1} x {med(t['scan']):.4f} = {floor:.4f} ms, top_k / floor {med(tk) / floor:.2f}{verdict}")
        return


say(f"# top_k on {torch.cuda.get_device_name(0)}; scale={args.scale} rounds={args.rounds} burst={args.burst}")
say("# ms per call: median of the rounds [fastest .. slowest]; calls back to back")
say("# route: decompress -> torch.topk (k-th value = its smallest); 2 k >= q: decompress -> torch.kthvalue; under a mask")
say("#        bitmap_to_rowids -> gather -> the same; c = 32 flips the sign bit in between (int32 order is not the values')")
say("# floor: (mi355_top_k_passes(c) + 1) x a count-only scan of the same column")
say("# gate: top_k's median below the route's and its slowest round below the route's fastest (uniform shapes only)")
say()

N9, N17 = int(1_000_000_000 * args.scale) // ALIGN * ALIGN, int(250_000_000 * args.scale) // ALIGN * ALIGN
KS = [("k = 1", lambda q: 1), ("k = 100", lambda q: 100), ("k = 1e6", lambda q: min(1_000_000, max(q - 1, 1))), ("k = q / 2", lambda q: max(q // 2, 1))]
for n, c in ((N9, 9), (N17, 17), (N17, 32)):
    col = eng.generate("splitmix", n, c, 42)
    g = torch.Generator(device="cuda").manual_seed(1234)
    mask = torch.randint(0, 256, (n // 8,), dtype=torch.uint8, generator=g, device="cuda")
    for _ in range(2):
        mask &= torch.randint(0, 256, (n // 8,), dtype=torch.uint8, generator=g, device="cuda")
    say(f"{n} rows x {c} bit, uniform random; {top_k_passes(c)} histogram pass(es)")
    for mname, mk in (("no mask", None), ("mask 1/8", mask)):
        for kname, k_of in KS:
            case(col, mk, k_of, f"{kname}, {mname}", True)
    say()
    del col, mask
    torch.cuda.empty_cache()

say(f"{N9} rows x 9 bit, all equal (reported, not gated): every LDS atomic of a wave hits one counter, the trim re-reads every chunk behind the cut")
case(eng.generate("mod", N9, 9, 1), None, lambda q: q // 2, "k = n / 2, no mask", False)
torch.cuda.empty_cache()
say()
say(f"{N17} rows x 32 bit, sorted ascending, value = row id (reported, not gated)")
col = eng.generate("index", N17, 32)
for kname, k_of in (KS[1], KS[3]):
    case(col, None, k_of, f"{kname}, no mask", False)

print(f"wrote {args.out}")
