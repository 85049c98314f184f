#!/usr/bin/env python3
"""Grouped aggregates beyond 12-bit keys (ScanEngine.group_aggregate_wide: sum, count, min, max of one packed column per key of a
dense domain of up to 2^26 groups) against the route the call replaces -- decompress both columns, then torch index_add_ /
bincount / scatter_reduce(amin, amax) on the device -- and against a trivial read of the two columns' bytes (torch sums over the
buffers, the stream floor).  Key distributions: uniform over 2^14 / 2^18 / 2^20 / 2^24 groups, Zipf-like over 2^18, one key with
half of the rows, sorted keys, and 4096 groups through both tiers (group_aggregate keeps them in LDS).  HIP events over
back-to-back calls, every shape warmed, all series of a case in alternating rounds in ONE process.  Writes
profiles/r12_group_aggregate_wide.txt.

    python tools/bench_group_aggregate_wide.py [--out profiles/r12_group_aggregate_wide.txt] [--rows 250000000] [--rounds 5] [--burst 10]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from shared_simd_scan_amd import ScanEngine, group_wide_front_slots, lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_group_aggregate_wide.txt"))
ap.add_argument("--rows", type=int, default=250_000_000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--burst", type=int, default=10)
args = ap.parse_args()
assert args.rounds >= 5 and args.burst >= 1 and args.rows % 8 == 0

eng = ScanEngine(0)
L = lib()
n = args.rows
CV = 17
I64_MAX = (1 << 63) - 1
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def measure(series):
    """series: {name: (callable, burst)}; alternating rounds of `burst` back-to-back calls -> {name: sorted ms per call}"""
    times = {k: [] for k in series}
    for fn, _ in series.values():  # every shape warmed
        fn()
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


def spread(t):
    return (t[-1] - t[0]) / med(t)


def fmt(t):
    return f"{med(t):.4f} ms [{t[0]:.4f} .. {t[-1]:.4f}] spread {100 * spread(t):.1f}%"


def kernels():
    return " + ".join(ln.split(" flags=")[0] for ln in L.mi355_ctx_last_launch(eng._ctx).decode().strip().split("\n"))


def keys_of(kind, ck):
    """-> packed key column of n rows over [0, 2^ck)"""
    groups = 1 << ck
    if kind == "uniform":
        return eng.generate("splitmix", n, ck, 42)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1812)
    if kind == "zipf":  # rank = floor(groups^u) - 1 with u uniform: P(rank r) ~ 1 / (r + 1); ranks scattered over the domain
        u = torch.rand(n, device="cuda", generator=gen, dtype=torch.float64)
        rank = (torch.exp(u * torch.log(torch.tensor(float(groups), dtype=torch.float64, device="cuda"))).to(torch.int64) - 1).clamp_(0, groups - 1)
        k = (rank * 2654435761) & (groups - 1)  # an odd multiplier: a bijection of the domain
        del u, rank
    elif kind == "hot":  # one key holds half of the rows, the others are uniform
        k = torch.randint(0, groups, (n,), device="cuda", generator=gen, dtype=torch.int64)
        k[torch.rand(n, device="cuda", generator=gen) < 0.5] = 3001
    elif kind == "sorted":
        k = torch.arange(n, device="cuda", dtype=torch.int64) * groups // n
    else:
        raise ValueError(kind)
    col = eng.compress(k.to(torch.int32), ck)
    del k
    return col


say(f"# grouped aggregates beyond 12-bit keys on {torch.cuda.get_device_name(0)}; rows={n} cv={CV} rounds={args.rounds} burst={args.burst}")
say("# ms per call: median of the rounds [fastest .. slowest]; spread = (slowest - fastest) / median; calls back to back")
say("# wide:   group_aggregate_wide, one call (init launch + aggregation launch); S = slots of a block's LDS front")
say("# route:  decompress(keys), decompress(values) -> int64 -> index_add_ (sum), bincount (count), scatter_reduce_ amin / amax")
say("# stream: torch.sum over both packed buffers as int64.  narrow (4096 groups only): group_aggregate, every group in LDS")
say("# TB/s: algorithmic bytes n*ck/8 + n*cv/8 over the wide median")
say()

CASES = [("uniform", 14), ("uniform", 18), ("uniform", 20), ("uniform", 24), ("zipf", 18), ("hot", 18), ("sorted", 18), ("uniform", 12)]
gates = []
for kind, ck in CASES:
    groups = 1 << ck
    keys = keys_of(kind, ck)
    vals = eng.generate("splitmix", n, CV, 4242)
    out = torch.empty((groups, 4), dtype=torch.int64, device="cuda")
    dropped = torch.empty(1, dtype=torch.int64, device="cuda")
    wide = lambda: eng.group_aggregate_wide(keys, vals, groups, out=out, dropped=dropped)  # noqa: E731
    r_sum = torch.empty(groups, dtype=torch.int64, device="cuda")
    r_min = torch.empty(groups, dtype=torch.int64, device="cuda")
    r_max = torch.empty(groups, dtype=torch.int64, device="cuda")
    r_cnt = [None]

    def route():
        k = eng.decompress(keys).to(torch.int64)
        v = eng.decompress(vals).to(torch.int64)
        r_sum.zero_().index_add_(0, k, v)
        r_cnt[0] = torch.bincount(k, minlength=groups)
        r_min.fill_(I64_MAX).scatter_reduce_(0, k, v, "amin")
        r_max.zero_().scatter_reduce_(0, k, v, "amax")

    kb, vb = keys.data[: keys.data.numel() // 8 * 8].view(torch.int64), vals.data[: vals.data.numel() // 8 * 8].view(torch.int64)
    stream = lambda: (kb.sum(), vb.sum())  # noqa: E731
    series = {"wide": (wide, args.burst), "route": (route, 1), "stream": (stream, args.burst)}
    narrow_out = None
    if ck <= 12:
        narrow_out = torch.empty((groups, 4), dtype=torch.int64, device="cuda")
        series["narrow"] = (lambda: eng.group_aggregate(keys, vals, out=narrow_out), args.burst)
    wide()
    k_wide = kernels()
    t = measure(series)
    tw, tr = t["wide"], t["route"]
    nbytes = n * ck / 8 + n * CV / 8
    say(f"{kind} keys, {groups} groups (ck={ck}), S={group_wide_front_slots(ck, CV)}")
    say(f"    wide         {fmt(tw)}  {nbytes / med(tw) / 1e9:.2f} TB/s   {k_wide}")
    say(f"    route        {fmt(tr)} | route / wide {med(tr) / med(tw):.2f}")
    say(f"    stream floor {fmt(t['stream'])} | wide / stream {med(tw) / med(t['stream']):.2f}")
    if "narrow" in t:
        say(f"    narrow tier  {fmt(t['narrow'])} | wide / narrow {med(tw) / med(t['narrow']):.2f}")
    # the results agree: all four columns with the route's where a group has rows, the empty result where it has none
    wide()
    route()
    torch.cuda.synchronize()
    some = r_cnt[0] > 0
    ok = bool(torch.equal(out[:, 1], r_cnt[0])) and bool(torch.equal(out[:, 0], r_sum)) and bool(torch.equal(out[:, 3], r_max))
    ok = ok and bool(torch.equal(out[:, 2][some], r_min[some])) and bool((out[:, 2][~some] == -1).all()) and int(dropped.item()) == 0
    if narrow_out is not None:
        eng.group_aggregate(keys, vals, out=narrow_out)
        ok = ok and bool(torch.equal(out, narrow_out))
    say(f"    results {'agree' if ok else 'DIFFER'} (all four columns with the route{', and with the narrow tier' if narrow_out is not None else ''}); "
        f"populated groups {int(some.sum().item())} of {groups}, rows counted {int(out[:, 1].sum().item())}, "
        f"largest group {int(out[:, 1].max().item())} rows")
    say()
    if kind == "uniform" and ck in (18, 20):
        gates.append((groups, tw, tr))
    del keys, vals, out, kb, vb, r_sum, r_min, r_max, narrow_out
    r_cnt[0] = None
    torch.cuda.empty_cache()

for groups, tw, tr in gates:
    met = med(tw) * 1.05 < med(tr) and tw[-1] < tr[0]
    say(f"# gate at {groups} uniform groups: wide median more than 5% below the route's, rounds not overlapping: "
        f"{med(tw):.4f} [.. {tw[-1]:.4f}] vs {med(tr):.4f} [{tr[0]:.4f} ..] ms, route / wide {med(tr) / med(tw):.2f}: {'MET' if met else 'MISSED'}")

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
