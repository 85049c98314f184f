"""Scans that compare two packed columns row by row (include/mi355_columns.h, ScanEngine.scan_columns).

CPU: the header is plain C99 and declares exactly what _capi.HEADERS binds for it and the library exports; engine.clamp_diff
keeps every comparison with a difference of two decoded values; scan_columns hands the C ABI what it should (through a
recording stand-in for the library, the idea of tests/test_predicate_constants.py); without a device the entry point fails
with a message.

GPU (-m gpu): every expectation is numpy int64 arithmetic on the values the test generated -- d = v1 - v2 compared with the
Python constants -- packed with the oracle's packer on the way in and np.packbits on the way out; nothing is derived from
engine output.  Output buffers sit inside 0xEE guard bytes (support.Guarded) that must stay untouched.
"""
import ctypes as C
import functools
import operator

import numpy as np
import pytest

import capture
import support
from support import E_INVALID, SENTINEL, Guarded, L, eng, fake, packbits, record  # noqa: F401  (L, eng, fake: fixtures)

HEADER = "mi355_columns.h"
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
OPS = ["==", "!=", "<", "<=", ">", ">=", "between", "not_between"]
CMP = {"==": operator.eq, "!=": operator.ne, "<": operator.lt, "<=": operator.le, ">": operator.gt, ">=": operator.ge}
MASK_OPS = ["and", "or", "xor", "andnot"]

SAME_WIDTHS = [1, 7, 9, 16, 17, 31, 32]
MIXED = [(9, 12), (12, 9), (1, 32), (32, 1), (16, 17), (17, 16), (31, 32), (32, 31), (5, 21), (24, 8)]
# beyond the issue's list: both widths <= 30 and different, column 2 wider than 8 KiB / 3 per tile (its last DMA instruction is a
# partial one at 30 bits), and a 30-bit pair whose difference needs all 31 bits of the 32-bit comparison
EXTRA = [(30, 29), (29, 30), (20, 30)]
PAIRS = [(c, c) for c in SAME_WIDTHS] + MIXED
N_BIG = 8192 * 9 + 1237  # 74965: ten tiles of 8192 rows (37 of 2048) and a ragged tail
GUARD_SIZES = [12365, N_BIG]

gpu = pytest.mark.gpu


def pid(p):
    return f"{p[0]}-{p[1]}"


def constants(c1, c2):
    m1, m2 = (1 << c1) - 1, (1 << c2) - 1
    cs = {0, INT64_MIN, INT64_MAX, (1 << 64) + 5}
    for x in (1, m1, m2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 40):
        cs |= {x, -x}
    return sorted(cs)


def py_pred(d, op, a, b):
    """the predicate on Python ints"""
    if op in CMP:
        return CMP[op](d, a)
    inside = a <= d <= b
    return inside if op == "between" else not inside


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------

def test_columns_header_is_plain_c99():
    support.check_header_is_plain_c99(HEADER)


def test_columns_header_declares_what_python_binds(L):
    names, sigs = support.check_header_binds(L, HEADER)
    assert "mi355_scan_columns_dev" in names


def test_columns_header_carries_its_capture_verdict():
    support.check_capture_verdict(HEADER)


def test_difference_constants_are_int64_arguments():
    from shared_simd_scan_amd import _capi

    sig = {name: args for name, _, args in _capi.HEADERS[HEADER]}["mi355_scan_columns_dev"]
    assert sig[7] is C.c_int64 and sig[8] is C.c_int64
    assert sig[2] is C.c_uint and sig[4] is C.c_uint and sig[5] is C.c_uint64


def difference_edges(c1, c2):
    m1, m2 = (1 << c1) - 1, (1 << c2) - 1
    ds = set()
    for e in (-m2, -1, 0, 1, m1):
        ds |= {e - 1, e, e + 1}
    return sorted(d for d in ds if -m2 <= d <= m1)


@pytest.mark.parametrize("c1", [1, 9, 31, 32])
@pytest.mark.parametrize("c2", [1, 9, 31, 32])
def test_clamp_diff_keeps_every_comparison(c1, c2):
    from shared_simd_scan_amd import clamp_diff, engine

    assert clamp_diff is engine.clamp_diff
    for x in constants(c1, c2):
        y = clamp_diff(x)
        assert -(1 << 32) <= y <= 1 << 32 and C.c_int64(y).value == y
        if -(1 << 32) <= x <= 1 << 32:
            assert y == x
        for d in difference_edges(c1, c2):
            for op in OPS[:6]:
                assert py_pred(d, op, y, 0) == py_pred(d, op, x, 0), (c1, c2, d, op, x, y)
    for a in constants(c1, c2):
        for b in constants(c1, c2):
            for d in difference_edges(c1, c2):
                for op in OPS[6:]:
                    assert py_pred(d, op, clamp_diff(a), clamp_diff(b)) == py_pred(d, op, a, b), (c1, c2, d, op, a, b)


def test_scan_columns_wrapper_passes_what_the_abi_takes(fake):
    import torch

    eng, rec, col = fake
    c1, c2 = col(9, 777), col(12, 777)
    mask, bm, hits = (torch.zeros(128, dtype=torch.uint8) for _ in range(3))
    for x in constants(9, 12):
        want = min(max(x, -(1 << 32)), 1 << 32)
        for k, mop in enumerate(MASK_OPS):
            rec.calls.clear()
            got_bm, got_hits = eng.scan_columns(c1, "between", c2, a=x, b=-x if x != INT64_MIN else x, mask=mask, mask_op=mop, bitmap=bm,
                                                hits=hits.view(torch.int64)[:1])
            (name, a), = rec.calls
            assert name == "mi355_scan_columns_dev"
            assert a[1:6] == [c1.data.data_ptr(), 9, c2.data.data_ptr(), 12, 777] and a[6] == 6
            wb = min(max(-x if x != INT64_MIN else x, -(1 << 32)), 1 << 32)
            assert (a[7], a[8]) == (want, wb), (x, a)
            assert a[9] == k and a[10] == mask.data_ptr() and a[11] == bm.data_ptr() and a[12] == hits.data_ptr()
            assert got_bm is bm
    for code, op in enumerate(OPS):
        rec.calls.clear()
        got_bm, got_hits = eng.scan_columns(c1, op, c2, count_only=True)
        (name, a), = rec.calls
        assert a[6] == code and (a[7], a[8]) == (0, 0) and a[9] == 0 and a[10] is None and a[11] is None and got_bm is None
        assert a[12] == got_hits.data_ptr()
    with pytest.raises(AssertionError):
        eng.scan_columns(c1, "<", col(12, 778))


def test_columns_entry_point_fails_loudly_without_a_gpu(L):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    buf = (C.c_uint8 * 1024)()
    hits = C.c_uint64()
    rc = L.mi355_scan_columns_dev(None, buf, 9, buf, 12, 100, 2, 0, 0, 0, None, buf, C.cast(C.byref(hits), C.c_void_p))
    assert rc != 0 and L.mi355_last_error()


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def values(c1, c2, n, salt=0):
    """the data recipe: v1 uniform; v2 within 3 of v1 on half the rows, uniform on the others; rows 0..7 the corner pairs"""
    rng = np.random.default_rng([c1, c2, salt])
    m1, m2 = (1 << c1) - 1, (1 << c2) - 1
    v1 = rng.integers(0, m1 + 1, n, dtype=np.int64)
    near = rng.random(n) < 0.5
    v2 = np.where(near, np.clip(v1 + rng.integers(-3, 4, n), 0, m2), rng.integers(0, m2 + 1, n, dtype=np.int64))
    m = min(m1, m2)
    corners = [(0, 0), (m1, 0), (0, m2), (m1, m2), (1, 0), (0, 1), (m, m), (m1, m)]
    for i, (x, y) in enumerate(corners[:n]):
        v1[i], v2[i] = x, y
    d = v1 - v2
    for a in (v1, v2, d):
        a.setflags(write=False)
    return v1, v2, d


def expect(d, op, a, b=0):
    """numpy int64 on the generated values.  |d| < 2^32, so a constant saturated at +-2^62 compares like the constant itself;
    numpy cannot compare an int64 array with 2^64 + 5"""
    a, b = (max(min(int(x), 1 << 62), -(1 << 62)) for x in (a, b))
    if op in CMP:
        return CMP[op](d, a)
    inside = (d >= a) & (d <= b)
    return inside if op == "between" else ~inside


def combine(p, m, mask_op):
    return {"and": p & m, "or": p | m, "xor": p ^ m, "andnot": m & ~p}[mask_op]


class Bench:
    """one engine, the uploaded columns of a width pair, guarded outputs that are refilled with 0xEE before every call"""

    def __init__(self, O, eng, c1, c2, n, salt=0):
        import torch

        from shared_simd_scan_amd.engine import PackedColumn

        self.torch, self.eng, self.n, self.nb = torch, eng, n, (n + 7) // 8
        self.v1, self.v2, self.d = values(c1, c2, n, salt)
        self.col1 = PackedColumn(torch.from_numpy(O.pack(self.v1.astype(np.uint32), c1)).cuda(), n, c1)
        self.col2 = PackedColumn(torch.from_numpy(O.pack(self.v2.astype(np.uint32), c2)).cuda(), n, c2)
        self.bm = Guarded(self.nb)
        self.hits = Guarded(8, back=64, front=64)

    def view(self, g, dtype=None):
        t = g.t[g.front: g.front + g.nbytes]
        return t.view(dtype) if dtype is not None else t

    def run(self, op, a=0, b=0, mask_bits=None, mask_op="and", inplace=False, count_only=False, what=""):
        """-> checks bitmap bytes, bits >= n, guard bytes and the hit count against numpy"""
        torch = self.torch
        self.bm.t.fill_(SENTINEL)
        self.hits.t.fill_(SENTINEL)
        want = expect(self.d, op, a, b)
        mask = None
        if mask_bits is not None:
            want = combine(want, mask_bits, mask_op)
            packed_mask = torch.from_numpy(packbits(mask_bits)).cuda()
            if inplace:
                self.view(self.bm).copy_(packed_mask)
                mask = self.view(self.bm)
            else:
                mask = packed_mask
        got_bm, got_hits = self.eng.scan_columns(self.col1, op, self.col2, a=a, b=b, mask=mask, mask_op=mask_op,
                                                 bitmap=None if count_only else self.view(self.bm), hits=self.view(self.hits, torch.int64),
                                                 count_only=count_only)
        self.eng.synchronize()
        body = self.bm.fetch()  # asserts the guard bytes on both sides
        tag = (what, self.col1.c, self.col2.c, self.n, op, a, b, mask_op if mask_bits is not None else None)
        if count_only:
            assert got_bm is None and (body == SENTINEL).all(), tag
        else:
            want_bytes = packbits(want)
            assert len(want_bytes) == self.nb
            if self.n % 8:
                assert body[-1] >> (self.n % 8) == 0, ("bits >= n", tag)
            assert np.array_equal(body, want_bytes), tag
        assert int(self.hits.fetch().view(np.uint64)[0]) == int(want.sum()), tag
        if mask_bits is not None and not inplace:
            assert np.array_equal(mask.cpu().numpy(), packbits(mask_bits)), ("mask written", tag)


@pytest.mark.parametrize("pair", PAIRS + EXTRA, ids=pid)
def test_recipe_is_not_vacuous(pair):
    """(no device needed) every comparison at a = 0 selects some rows and not all, at both sizes, for every width pair"""
    for n in GUARD_SIZES:
        d = values(pair[0], pair[1], n)[2]
        for op in OPS[:6]:
            k = int(expect(d, op, 0).sum())
            assert 0 < k < n, (pair, n, op, k)


@gpu
@pytest.mark.parametrize("pair", [(9, 9), (9, 12), (32, 31), (17, 16)], ids=pid)
def test_sizes_and_tails(L, O, eng, pair):
    for n in (1, 13, 509, 4096, 8192, N_BIG):
        bench = Bench(O, eng, pair[0], pair[1], n)
        for capped in ((False, True) if n == N_BIG else (False,)):
            if capped:  # four waves, each walks several tiles: prefetch, deferred store, tail
                eng.set_option("grid_cus", 1)
                eng.set_option("max_blocks_per_cu", 1)
            try:
                for op in OPS:
                    for a in (0, 1, -1):
                        bench.run(op, a, a + 5, what=f"capped={capped}")
                if capped:
                    (label, grid, _, _), = record(L, eng)
                    assert grid == 1 and label.startswith("scan_columns_kernel<")
            finally:
                if capped:
                    eng.set_option("grid_cus", 0)
                    eng.set_option("max_blocks_per_cu", 0)


@gpu
@pytest.mark.parametrize("pair", PAIRS + EXTRA, ids=pid)
def test_every_pair_every_op(O, eng, pair):
    c1, c2 = pair
    bench = Bench(O, eng, c1, c2, N_BIG)
    for op in OPS[:6]:
        k = int(expect(bench.d, op, 0).sum())
        assert 0 < k < N_BIG, (pair, op, k)
    cs = constants(c1, c2)
    for op in OPS[:6]:
        for a in cs:
            bench.run(op, a)
    rng = np.random.default_rng([c1, c2, 99])
    m1, m2 = (1 << c1) - 1, (1 << c2) - 1
    ranges = [(7, 3), (-3, 3), (-m2, m1), (-m2 - 1, m1 + 1), (m1, m1), (-m2, -m2), (INT64_MIN, INT64_MAX), (INT64_MAX, INT64_MIN), (1, -m2)]
    ranges += [tuple(int(x) if abs(x) < 1 << 63 else x for x in (cs[i], cs[j])) for i, j in rng.integers(0, len(cs), (12, 2))]
    assert any(a > b for a, b in ranges)
    for a, b in ranges:
        for op in OPS[6:]:
            bench.run(op, a, b)


@gpu
@pytest.mark.parametrize("pair", [(31, 31), (31, 32), (32, 32), (32, 1), (1, 32)], ids=pid)
def test_wide_width_boundaries(O, eng, pair):
    """a width of 31 or 32: d - lo spans up to 2^33 - 2, a 32-bit test would alias"""
    bench = Bench(O, eng, pair[0], pair[1], N_BIG)
    edge = [(1 << 31) - 1, 1 << 31, (1 << 32) - 2, (1 << 32) - 1, 1 << 32]
    cs = sorted(edge + [-x for x in edge])
    for op in OPS[:6]:
        for a in cs:
            bench.run(op, a)
    for a in cs:
        for b in cs:
            bench.run("between", a, b)
            bench.run("not_between", a, b)


@gpu
@pytest.mark.parametrize("pair", [(9, 9), (9, 12), (32, 32)], ids=pid)
def test_masks_and_count_only(O, eng, pair):
    bench = Bench(O, eng, pair[0], pair[1], N_BIG)
    mask_bits = np.random.default_rng([pair[0], pair[1], 7]).random(N_BIG) < 0.5
    for mask_op in MASK_OPS:
        for op, a, b in (("<", 0, 0), ("between", -3, 3), ("!=", 0, 0)):
            bench.run(op, a, b, mask_bits=mask_bits, mask_op=mask_op)
            bench.run(op, a, b, mask_bits=mask_bits, mask_op=mask_op, inplace=True)
            bench.run(op, a, b, mask_bits=mask_bits, mask_op=mask_op, count_only=True)  # the 0xEE bitmap is the canary
    bench.run(">=", 1, count_only=True)
    # a ragged size whose tail tile reads the mask byte by byte, in place
    small = Bench(O, eng, pair[0], pair[1], 2048 + 509)
    small_bits = np.random.default_rng(3).random(small.n) < 0.5
    for mask_op in MASK_OPS:
        small.run("<=", 0, mask_bits=small_bits, mask_op=mask_op, inplace=True)
        small.run("<=", 0, mask_bits=small_bits, mask_op=mask_op)


@gpu
@pytest.mark.parametrize("c", [9, 32])
def test_same_buffer(O, eng, c):
    import torch

    from shared_simd_scan_amd.engine import PackedColumn

    n = N_BIG
    v1 = values(c, c, n)[0]
    col = PackedColumn(torch.from_numpy(O.pack(v1.astype(np.uint32), c)).cuda(), n, c)
    bm, hits = eng.scan_columns(col, "==", col)
    assert int(hits.item()) == n and np.array_equal(bm.cpu().numpy(), packbits(np.ones(n, dtype=bool)))
    bm, hits = eng.scan_columns(col, "!=", col)
    assert int(hits.item()) == 0 and not bm.cpu().numpy().any()


@gpu
def test_one_launch_for_any_width_pair(L, O, eng):
    for pair, form in (((9, 12), "scan_columns_kernel<9, 32, false, false>"), ((9, 9), "scan_columns_kernel<9, 128, true, false>"),
                       ((12, 32), "scan_columns_kernel<12, 32, false, true>"), ((32, 32), "scan_columns_kernel<32, 64, true, true>")):
        bench = Bench(O, eng, pair[0], pair[1], N_BIG)
        bench.run("<", 0)
        (label, grid, lds, flags), = record(L, eng)
        assert label == form and grid >= 1 and flags == 0, (pair, label)


@gpu
def test_errors_launch_nothing(L, O, eng):
    import torch

    n = 4096 + 77
    bench = Bench(O, eng, 9, 12, n)
    mask = Guarded(bench.nb)
    p1, p2 = bench.col1.data.data_ptr(), bench.col2.data.data_ptr()

    def call(p2=p2, c2=12, op=2, mask_op=0, mask_ptr=mask.ptr.value, bm=bench.bm.ptr.value, hits=bench.hits.ptr.value, n=n):
        bench.bm.t.fill_(SENTINEL)
        bench.hits.t.fill_(SENTINEL)
        rc = L.mi355_scan_columns_dev(eng._ctx, p1, 9, p2, c2, n, op, 0, 0, mask_op, mask_ptr, bm, hits)
        eng.synchronize()
        return rc

    for what, kw in (("misaligned packed2", dict(p2=p2 + 4)), ("misaligned mask", dict(mask_ptr=mask.ptr.value + 8)),
                     ("misaligned bitmap", dict(bm=bench.bm.ptr.value + 1)), ("c2 = 0", dict(c2=0)), ("c2 = 33", dict(c2=33)),
                     ("op = 8", dict(op=8)), ("mask_op = 4", dict(mask_op=4)), ("both outputs null", dict(bm=None, hits=None))):
        assert call(**kw) == E_INVALID and L.mi355_last_error(), what
        assert record(L, eng) == [], what
        assert (bench.bm.fetch() == SENTINEL).all() and (bench.hits.fetch() == SENTINEL).all() and (mask.fetch() == SENTINEL).all(), what
    assert call(n=0) == 0
    assert record(L, eng) == []
    assert int(bench.hits.fetch().view(np.uint64)[0]) == 0 and (bench.bm.fetch() == SENTINEL).all()
    assert call() == 0 and len(record(L, eng)) == 1  # the same arguments, valid: it does launch


@gpu
def test_graph_capture_and_replay(O):
    """a linear chain on a side stream, as tests/test_graph_capture.py::test_captured_pipeline_through_the_engine: warm up, capture,
    three replays over columns and a mask overwritten in place"""
    import torch

    from shared_simd_scan_amd.engine import PackedColumn

    n, c1, c2 = N_BIG, 9, 12
    versions = []
    for r in range(3):
        v1, v2, d = values(c1, c2, n, salt=r + 1)
        bits = np.random.default_rng(50 + r).random(n) < (0.4, 0.5, 0.6)[r]
        want = expect(d, "<", 0) & bits
        versions.append((O.pack(v1.astype(np.uint32), c1), O.pack(v2.astype(np.uint32), c2), packbits(bits), packbits(want), int(want.sum())))
    assert len({v[4] for v in versions}) == 3  # a stale result cannot pass

    def steps(eng):
        stage = [[torch.from_numpy(x).cuda() for x in v[:3]] for v in versions]
        col1 = PackedColumn(torch.empty_like(stage[0][0]), n, c1)
        col2 = PackedColumn(torch.empty_like(stage[0][1]), n, c2)
        mask = torch.empty_like(stage[0][2])
        bm = Guarded((n + 7) // 8)
        hits = torch.empty(1, dtype=torch.int64, device="cuda")
        out = bm.t[bm.front: bm.front + bm.nbytes]

        def load(r):
            col1.data.copy_(stage[r][0])
            col2.data.copy_(stage[r][1])
            mask.copy_(stage[r][2])
            bm.t.fill_(SENTINEL)
            hits.view(torch.uint8).fill_(SENTINEL)

        def run():
            eng.scan_columns(col1, "<", col2, mask=mask, bitmap=out, hits=hits)

        def check(r, what):
            assert np.array_equal(bm.fetch(), versions[r][3]) and int(hits.item()) == versions[r][4], what

        def untouched():
            assert (bm.fetch() == SENTINEL).all() and (hits.cpu().numpy().view(np.uint8) == SENTINEL).all()

        return capture.Steps(load, run, check, untouched)

    capture.capture_replay(steps, range(3))
