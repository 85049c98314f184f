"""The scan's Infinity-Cache policy (option "llc_resident_mib") changes which cache policy a tile's loads carry, never a result.

Every case runs with the option off (0), auto (-1) and explicit budgets that make the launcher keep all of the column (D = 1),
every third 64 KiB granule (D = 3) and every ninth (D = 9); each three times back to back on the same buffers, so that the
later launches read what the earlier ones left in the cache; with one and with two blocks per CU, since residency is a
function of the address only.  Every launch is checked against numpy on the CPU, bitmap bytes and hit count, inside guard
bytes; the bitmap is refilled with the guard byte before each launch; and the divisor the launcher chose
(mi355_ctx_last_llc_divisor) is the one the budget was picked for.  At these sizes (20-63 MiB) the whole column fits the auto
budget, and auto never keeps a whole column: it must report D = 0.  test_auto_acts_on_repeats_only runs auto on a 2.5e8-row
column, which does not fit: D = 0 on the first launch, D >= 3 on repeats, D = 0 again after another bitmap, another column or
another kernel came between; every launch against the CPU oracle.
"""
import ctypes as C

import numpy as np
import pytest

from support import Guarded, packbits

MIB = 1 << 20
GRANULE = 64 * 1024
WIDTHS = [5, 9, 12, 17]
MODES = ["eq", "range", "count", "mask"]


def divisor(budget_mib, column_bytes, bitmap_bytes):
    """scan_plan.hpp llc_divisor() for an explicit budget (small bitmaps, nt column loads)"""
    budget = budget_mib * MIB
    if budget_mib <= 0 or budget <= bitmap_bytes:
        return 0
    resident = budget - bitmap_bytes
    if resident >= column_bytes:
        return 1
    return -(-column_bytes // resident) | 1


def cached_bitmap_bytes(n, mode):
    """what the call writes to and reads from bitmaps"""
    return {"eq": 1, "range": 1, "count": 0, "mask": 2}[mode] * ((n + 7) // 8)


def rows_and_budgets(c, mode):
    """a ragged row count of 20+ MiB of column for which whole-MiB budgets give D = 1, 3 and 9"""
    for mib in range(20, 64):
        n = mib * MIB * 8 // c + 77
        col, bm = (n * c + 7) // 8, cached_bitmap_bytes(n, mode)
        got = {}
        for b in range(1, 128):
            got.setdefault(divisor(b, col, bm), b)
        if all(d in got for d in (1, 3, 9)):
            return n, {d: got[d] for d in (1, 3, 9)}
    raise AssertionError(f"no row count found for c={c}, {mode}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", WIDTHS)
def test_budgets_reach_the_divisors(c, mode):
    n, budgets = rows_and_budgets(c, mode)
    col, bm = (n * c + 7) // 8, cached_bitmap_bytes(n, mode)
    assert n % 8192 != 0 and col > 9 * GRANULE
    assert [divisor(budgets[d], col, bm) for d in (1, 3, 9)] == [1, 3, 9]
    assert divisor(0, col, bm) == 0


def run_case(L, O, c, mode, n, options, divisors):
    import torch

    from shared_simd_scan_amd import ScanEngine

    rng = np.random.default_rng(1000 * c + len(mode) + n % 97)
    top = 1 << c
    key = int(rng.integers(0, top))
    vals = rng.integers(0, top, n, dtype=np.uint32)
    vals[rng.random(n) < 0.3] = key
    packed = torch.from_numpy(O.pack(vals, c)).cuda()
    lo, hi = sorted((key, (key * 7 + 5) % top))
    mask_bits = rng.random(n) < 0.5
    mask = torch.from_numpy(packbits(mask_bits)).cuda()
    expect = {"eq": vals == key, "range": (vals >= lo) & (vals <= hi), "count": (vals >= lo) & (vals <= hi),
              "mask": (vals >= lo) & (vals <= hi) & mask_bits}[mode]
    want_bytes, want_hits = packbits(expect), int(expect.sum())
    p = C.c_void_p(packed.data_ptr())
    for bpc in (1, 2):
        for opt, want_d in zip(options, divisors):
            eng = ScanEngine()
            try:
                eng.set_option("max_blocks_per_cu", bpc)
                eng.set_option("llc_resident_mib", opt)
                bm, hits = Guarded((n + 7) // 8), Guarded(8, back=64, front=64)
                for launch in range(3):
                    bm.t.fill_(0xEE)
                    hits.t.fill_(0xEE)
                    if mode == "eq":
                        rc = L.mi355_scan_eq_dev(eng._ctx, p, n, c, key, bm.ptr, hits.ptr)
                    elif mode == "range":
                        rc = L.mi355_scan_range_dev(eng._ctx, p, n, c, lo, hi, bm.ptr, hits.ptr)
                    elif mode == "count":
                        rc = L.mi355_scan_combine_dev(eng._ctx, p, n, c, 6, lo, hi, 0, None, None, hits.ptr)
                    else:
                        rc = L.mi355_scan_combine_dev(eng._ctx, p, n, c, 6, lo, hi, 0, C.c_void_p(mask.data_ptr()), bm.ptr, hits.ptr)
                    assert rc == 0, L.mi355_last_error()
                    eng.synchronize()
                    rec = (L.mi355_ctx_last_launch(eng._ctx) or b"").decode()
                    assert rec.startswith(f"scan_burst_kernel<{c}, "), rec
                    what = f"c={c} {mode} n={n} llc_resident_mib={opt} max_blocks_per_cu={bpc} launch {launch}"
                    assert L.mi355_ctx_last_llc_divisor(eng._ctx) == want_d, f"{what}: divisor"
                    got = bm.fetch()
                    if mode == "count":
                        assert (got == 0xEE).all(), f"{what}: a count-only scan wrote a bitmap"
                    else:
                        assert np.array_equal(got, want_bytes), f"{what}: bitmap differs"
                    assert int(hits.fetch().view(np.uint64)[0]) == want_hits, f"{what}: hit count differs"
            finally:
                eng.close()


# differs from support.L: a missing library is an error here, it is not built
@pytest.fixture(scope="module")
def L():
    from shared_simd_scan_amd import lib

    return lib()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", WIDTHS)
def test_policy_never_changes_a_result(L, O, c, mode):
    """ragged tail, many granules: off, auto, D = 1, 3, 9"""
    n, budgets = rows_and_budgets(c, mode)
    run_case(L, O, c, mode, n, [0, -1, budgets[1], budgets[3], budgets[9]], [0, 0, 1, 3, 9])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", WIDTHS)
def test_column_below_one_granule(L, O, c, mode):
    """the whole column inside granule 0 (resident under every divisor), ragged: off, auto, 1 MiB"""
    n = 3 * 4096 + 77
    assert (n * c + 7) // 8 < GRANULE
    run_case(L, O, c, mode, n, [0, -1, 1], [0, 0, 1])


@pytest.mark.gpu
def test_auto_acts_on_repeats_only(L, O):
    """2.5e8 x 9 bit (268 MiB of column, 30 MiB of bitmap: more than the auto budget holds), default options"""
    import torch

    from shared_simd_scan_amd import ScanEngine

    n, c = 250_000_077, 9
    eng = ScanEngine()
    try:
        cols = [eng.generate("splitmix", n, c, 42 + i) for i in range(2)]
        key = 77
        want = []
        for col in cols:
            obm, ohits = O.scan_eq(col.data.cpu().numpy(), n, c, key)
            want.append((np.asarray(obm)[: (n + 7) // 8].copy(), int(ohits)))
        bms = [Guarded((n + 7) // 8), Guarded((n + 7) // 8)]
        hits = Guarded(8, back=64, front=64)
        small = eng.generate("splitmix", 100_003, c, 7)

        def scan(ci, bi):
            bms[bi].t.fill_(0xEE)
            rc = L.mi355_scan_eq_dev(eng._ctx, C.c_void_p(cols[ci].data.data_ptr()), n, c, key, bms[bi].ptr, hits.ptr)
            assert rc == 0, L.mi355_last_error()
            eng.synchronize()
            d = L.mi355_ctx_last_llc_divisor(eng._ctx)
            assert np.array_equal(bms[bi].fetch(), want[ci][0]), f"column {ci} -> bitmap {bi}: bitmap differs (D = {d})"
            assert int(hits.fetch().view(np.uint64)[0]) == want[ci][1], f"column {ci} -> bitmap {bi}: hit count differs (D = {d})"
            return d

        assert L.mi355_ctx_last_llc_divisor(eng._ctx) == -1  # no scan launched yet
        assert scan(0, 0) == 0          # first scan of the column
        d = scan(0, 0)                  # repeat: the resident granules are loaded with the default policy
        assert d >= 3 and d % 2 == 1, d
        assert scan(0, 0) == d          # repeat: they are read from the cache
        assert scan(0, 1) == 0          # another bitmap
        assert scan(0, 1) == d
        assert scan(1, 1) == 0          # another column
        assert scan(1, 1) == d
        eng.decompress(small)           # another kernel in between
        assert L.mi355_ctx_last_llc_divisor(eng._ctx) == -1
        assert scan(1, 1) == 0
        assert scan(1, 1) == d
        # ... whichever launcher it comes from: the where-scans' own, those of extras.hip, a feature unit's
        small_bits = eng.alloc_bitmap(small.n).zero_()
        others = {
            "shared_scan_where": lambda: eng.shared_scan_where([("<", 5), (">", 100)], small),
            "bitmap_count": lambda: eng.bitmap_count(small_bits, small.n),
            "aggregate": lambda: eng.aggregate(small),
            "histogram": lambda: eng.histogram(small),
            "group_aggregate": lambda: eng.group_aggregate(small, small),
            "generate": lambda: eng.generate("splitmix", small.n, c, 9),
        }
        for name, call in others.items():
            call()
            assert L.mi355_ctx_last_llc_divisor(eng._ctx) == -1, name
            assert scan(1, 1) == 0, name
            assert scan(1, 1) == d, name
        eng.set_option("llc_resident_mib", 0)
        assert scan(1, 1) == 0          # off
    finally:
        eng.close()


@pytest.mark.gpu
def test_option_range(L):
    from shared_simd_scan_amd import Mi355Error, ScanEngine

    eng = ScanEngine()
    try:
        for bad in (-2, 1025):
            with pytest.raises(Mi355Error):
                eng.set_option("llc_resident_mib", bad)
        for good in (-1, 0, 1, 220, 1024):
            eng.set_option("llc_resident_mib", good)
    finally:
        eng.close()
