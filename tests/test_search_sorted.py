"""A packed column's positions in a sorted packed table (include/mi355_search.h, ScanEngine.search_sorted and its compositions
bucketize, index_of, is_member, sorted_keys, sparse_lookup): pos_i = the number of table entries < x_i (left) or <= x_i (right),
packed out, the bitmap of the rows whose value occurs in the table, and their number.

CPU: the header is plain C99 and declares exactly what _capi.HEADERS binds for it and the library exports; it carries its
graph-capture verdict; its LDS ceiling is the budget the sources static_assert; mi355_search_sorted_kernel and
mi355_search_sorted_stride (pure arithmetic) name the tier and the sample distance at every boundary; the wrappers hand the C ABI
what they should (through a recording stand-in for the library); without a device the entry point fails with a message; every
__global__ under csrc/search/ is named by the launch record of a GPU case of this file; no source there reads a switch bit or
reaches the context's selection workspace or counter scratch; the data recipes are not vacuous.

GPU (-m gpu): the oracle is numpy.searchsorted on uint64 copies of the values the test generated, and numpy.isin; nothing is
derived from engine output.  Every output lives in a support.Guarded buffer: each of the ceil(n co / 8) position bytes and of the
ceil(n / 8) bitmap bytes (trailing bits included), the counter, and the 0xEE guard bytes on both sides are compared exactly; column
and table must be unchanged after the call.  Column and table stand in hostile surroundings (ones behind the last value and in
the pad).  A tile is 2048 rows and a block four waves.

The issue's list of global-tier table sizes, {L + 1, 2 L + 1, 8 L + 5}, names strides 2, 4 and 16 for them; by the stride's
definition (and the issue's own CPU boundaries, 2 L -> 2 and 2 L + 2 -> 4) those sizes give 2, 2 and 8.  The cases keep the three
sizes and add 2 L + 2 and 8 L + 8, so that the strides 2, 4, 8 and 16 all run.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import capture
import support
from support import (E_INVALID, SENTINEL, Guarded, L, base_name, eng, fake, grouped, header_macro, hostile_pack, packbits, plain_pack,  # noqa: F401
                     record)  # (L, eng, fake: fixtures)

HEADER = "mi355_search.h"

# the kernels of csrc/search/, as the launch record names them: the GPU cases below assert these labels
LDS_KERNEL = "search_lds_kernel"
GLOBAL_KERNEL = "search_global_kernel"

LDS_MAX = header_macro(HEADER, "MI355_SEARCH_LDS_MAX_BYTES")
LMAX = LDS_MAX // 4  # L: the largest table of the LDS tier
R = 2048             # rows per tile: 64 lanes x 32 rows
LEFT, RIGHT = 0, 1
SIDES = (("left", LEFT), ("right", RIGHT))
WIDTHS = (1, 7, 8, 9, 16, 17, 31, 32)

N_BIG = 4 * R + 1237  # 9429: five tiles, so two blocks, and a ragged one; not a multiple of 8
SIZES = [1, 31, 32, 33, 2047, 2048, 2049, 8191, 8192 + 5, 3 * 8192 + 77]
SIZE_CASE = (17, 17, 1000, 10)  # (c, ct, rows, co)
OUTPUT_COMBOS = [(o, f, h) for o in (True, False) for f in (True, False) for h in (True, False) if o or f or h]
# a covering sample: every pair (c, ct) of WIDTHS with co walking through WIDTHS, then every output width in both tiers
WIDTH_CASES = ([(c, ct, WIDTHS[(i + j) % 8]) for i, c in enumerate(WIDTHS) for j, ct in enumerate(WIDTHS)]
               + [(12, 12, co) for co in range(1, 33) if co not in WIDTHS])
GLOBAL_WIDTH_CASES = [(WIDTHS[co % 8], WIDTHS[(co // 2) % 8], co) for co in range(15, 33)]  # rows = L + 1 needs co >= 15
LDS_ROWS = [1, 2, 3, 4, 5, 63, 64, 65, LMAX - 1, LMAX]
GLOBAL_ROWS = [LMAX + 1, 2 * LMAX + 1, 2 * LMAX + 2, 8 * LMAX + 5, 8 * LMAX + 8]
GLOBAL_STRIDES = [2, 2, 4, 8, 16]
ROWS_DEV_CASES = [(rows, have) for rows in (LMAX + 1, 65) for have in (0, 1, 3, rows, 1 << 40)]
OFFSET_CASES = [(24, 17, 3001), (24, 7, 3002), (24, 17, LMAX + 1), (32, 32, LMAX + 3)]  # (c, ct, rows)
VIEW_CASES = [(9, 12, 300), (24, 17, LMAX + 1)]
N_VIEW = 2 * R + 504  # a multiple of 8 (the slice ends on a byte at any width), not of 32: the last lane is ragged
UNSORTED_CASES = [(17, 17, 3001), (24, 24, LMAX + 1), (24, 24, 2 * LMAX + 2)]
LONG_CASES = [(12, 12, 3001), (24, 24, LMAX + 1)]
N_LONG = 40 * R + 77
ERROR_CASE = (9, 12, 300, R + 77)  # (c, ct, rows, n)
CAPTURE_CASES = [(12, 12, 3001), (24, 24, LMAX + 1)]  # one per tier

gpu = pytest.mark.gpu


def pid(p):
    return "-".join(str(x) for x in p) if isinstance(p, tuple) else str(p)


def width_for(rows):
    return max(1, int(rows).bit_length())


def rows_for(co, most=300):
    """a table as long as positions of co bits allow, `most` at the most"""
    return min((1 << co) - 1, most)


def want_family(rows):
    return LDS_KERNEL if rows * 4 <= LDS_MAX else GLOBAL_KERNEL


def want_stride(rows):
    s = 1
    while (rows // s) * 4 > LDS_MAX:
        s *= 2
    return s


def miss_of(co):
    return 1 if co == 1 else 0x5A5A5A5A & ((1 << co) - 1)


def payload(n, c):
    return (n * c + 7) // 8


@functools.lru_cache(maxsize=None)
def table_of(c, ct, rows, kind="plain", salt=0):
    """a sorted table of `rows` entries of ct bits with a pair of equal neighbours in its middle (rows >= 2).
    plain: entries within [1, m - 1], m = min(2^c, 2^ct) - 1, so that a c-bit probe exists below the first and above the last
           (widths of 1 or 2 bits: within [0, m]);
    limit: entries over all of [0, 2^ct - 1], entry 0 = 0 and the last = 2^ct - 1 (one entry: 0);
    above: (c < ct) the upper half of the entries lies above every c-bit probe;
    equal: every entry is the same value."""
    rng = np.random.default_rng([11, c, ct, rows % (1 << 31), rows >> 31, salt, len(kind)])
    top = (1 << ct) - 1
    m = min((1 << c) - 1, top)
    if kind == "plain":
        lo, hi = (1, m - 1) if m >= 3 else (0, m)
        t = rng.integers(lo, hi + 1, rows, dtype=np.uint64)
    elif kind == "limit":
        t = rng.integers(0, top + 1, rows, dtype=np.uint64)
        if rows >= 2:
            t[0], t[-1] = 0, top
        elif rows == 1:
            t[0] = 0
    elif kind == "above":
        assert c < ct
        t = rng.integers(1, m, rows, dtype=np.uint64)
        t[rows // 2:] = rng.integers(m + 1, top + 1, rows - rows // 2, dtype=np.uint64)
    else:
        assert kind == "equal"
        t = np.full(rows, max(1, m // 2), dtype=np.uint64)
    t = np.sort(t)
    if rows >= 4:
        t[rows // 2] = t[rows // 2 - 1]
    t = t.astype(np.uint32)
    t.setflags(write=False)
    return t


def corners_of(c, table):
    """the probes every recipe column carries at its first rows and at its last: 0, 2^c - 1, one below the first entry, one above the
    last, the first and the last entry (clipped to c bits)"""
    top = (1 << c) - 1
    if len(table) == 0:
        return [0, top, 0, top, 0, top]
    first, last = int(table[0]), int(table[-1])
    return [0, top, min(max(first - 1, 0), top), min(last + 1, top), min(first, top), min(last, top)]


@functools.lru_cache(maxsize=None)
def probes_of(c, ct, rows, n, kind="plain", salt=0):
    """a third of the rows an entry of the table (where it fits c bits), a third an entry + 1, a third uniform over [0, 2^c);
    corners_of() at rows 0 .. 5 and, from 12 rows on, at the last six"""
    table = table_of(c, ct, rows, kind, salt)
    rng = np.random.default_rng([13, c, ct, rows % (1 << 31), n, salt, len(kind)])
    top = (1 << c) - 1
    x = rng.integers(0, top + 1, n, dtype=np.uint64)
    if rows:
        pick = table[rng.integers(0, rows, n)].astype(np.uint64)
        how = rng.integers(0, 3, n)
        x = np.where(how == 0, np.minimum(pick, top), np.where(how == 1, np.minimum(pick + 1, top), x))
    cs = corners_of(c, table)
    x[:min(6, n)] = cs[:min(6, n)]
    if n >= 12:
        x[n - 6:] = cs
    x = x.astype(np.uint32)
    x.setflags(write=False)
    return x


def expect(x, table, rows_eff, side):
    """-> (pos int64[n], found bool[n]) by numpy on uint64 copies: the oracle"""
    t = table[:rows_eff].astype(np.uint64)
    pos = np.searchsorted(t, x.astype(np.uint64), side="left" if side == LEFT else "right").astype(np.int64)
    return pos, np.isin(x.astype(np.uint64), t)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------

def test_search_header_is_plain_c99():
    support.check_header_is_plain_c99(HEADER)


def test_search_header_declares_what_python_binds(L):
    names, sigs = support.check_header_binds(L, HEADER)
    assert names == ["mi355_search_sorted_dev", "mi355_search_sorted_kernel", "mi355_search_sorted_stride"]
    sig = sigs["mi355_search_sorted_dev"]
    assert len(sig) == 15 and sig[2] is C.c_uint64 and sig[3] is C.c_uint and sig[5] is C.c_uint and sig[6] is C.c_uint64
    assert sig[8] is C.c_int and sig[9] is C.c_int and sig[10] is C.c_uint32 and sig[12] is C.c_uint
    assert sigs["mi355_search_sorted_kernel"] == [C.c_uint, C.c_uint, C.c_uint, C.c_uint64] and L.mi355_search_sorted_kernel.restype is C.c_char_p
    assert sigs["mi355_search_sorted_stride"] == [C.c_uint64] and L.mi355_search_sorted_stride.restype is C.c_uint64
    text = support.header_text(HEADER)
    assert re.search(r"#define MI355_SEARCH_LEFT\s+0\b", text) and re.search(r"#define MI355_SEARCH_RIGHT\s+1\b", text)


def test_search_names_are_exported():
    import shared_simd_scan_amd as pkg

    for name in ("search_sorted_kernel", "search_sorted_stride"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    for name in ("search_sorted", "bucketize", "index_of", "is_member", "sorted_keys", "sparse_lookup"):
        assert callable(getattr(pkg.ScanEngine, name))


def test_search_header_carries_its_capture_verdict():
    support.check_capture_verdict(HEADER, r"read at\s+\*?\s*every replay", r"needs no warm-up call", r"zeroing of hits_dev", r"whatever its arguments")


def test_header_limit_is_the_budget_the_sources_assert():
    """160 KiB minus four waves' two 8 KiB input images and 64 bytes, in whole 16 bytes; the sources derive it from the same parts and
    static_assert both the budget and the header's number"""
    assert LDS_MAX == (160 * 1024 - 4 * 2 * 8192 - 64) // 16 * 16 and LDS_MAX % 4 == 0
    hpp = open(os.path.join(support.CSRC, "search", "search.hpp")).read()
    hip = open(os.path.join(support.CSRC, "search", "search_sorted.hip")).read()
    assert "kSearchLdsMaxBytes = (kCuLdsBytes - kWavesPerBlock * 2u * rt_image(32) - kSearchLdsSlack) & ~15u" in hpp
    assert re.search(r"kSearchLdsSlack = 64;", hpp)
    assert 'static_assert(search_images_lds(32) + kSearchLdsMaxBytes <= kCuLdsBytes, "LDS budget")' in hpp
    assert "static_assert(kSearchLdsMaxBytes == MI355_SEARCH_LDS_MAX_BYTES" in hip


def test_kernel_and_stride_at_the_boundaries(L):
    """both need neither a device nor a context"""
    from shared_simd_scan_amd import search_sorted_kernel, search_sorted_stride

    k, s = L.mi355_search_sorted_kernel, L.mi355_search_sorted_stride
    lds, glob_ = LDS_KERNEL.encode(), GLOBAL_KERNEL.encode()
    for c, ct, co in ((1, 1, 1), (9, 12, 17), (32, 32, 32), (32, 1, 16)):
        assert [k(c, ct, co, rows) for rows in (0, 1, LMAX - 1, LMAX)] == [lds] * 4
        assert [k(c, ct, co, rows) for rows in (LMAX + 1, 2 * LMAX, (1 << 32) - 1)] == [glob_] * 3
        assert k(c, ct, co, 1 << 32) is None
    assert [s(rows) for rows in (0, 1, LMAX - 1, LMAX)] == [1] * 4
    assert s(LMAX + 1) == 2 and s(2 * LMAX) == 2 and s(2 * LMAX + 1) == 2 and s(2 * LMAX + 2) == 4
    assert [s(rows) for rows in GLOBAL_ROWS] == GLOBAL_STRIDES == [want_stride(rows) for rows in GLOBAL_ROWS]
    big = (1 << 32) - 1
    S = s(big)
    assert S & (S - 1) == 0 and (big // S) * 4 <= LDS_MAX < (big // (S // 2)) * 4, "the largest table's samples fit, and no closer ones would"
    for rows in (0, 1, 3001, LMAX + 1):
        for bad in ((0, 8, 8), (33, 8, 8), (8, 0, 8), (8, 33, 8), (8, 8, 0), (8, 8, 33)):
            assert k(*bad, rows) is None, (bad, rows)
    assert search_sorted_kernel(9, 12, 12, 3001) == LDS_KERNEL and search_sorted_kernel(32, 32, 32, LMAX + 1) == GLOBAL_KERNEL
    assert search_sorted_stride(LMAX) == 1 and search_sorted_stride(8 * LMAX + 8) == 16
    for bad in ((0, 8, 8, 5), (8, 33, 8, 5), (8, 8, 0, 5), (8, 8, 8, 1 << 32), (8, 8, 8, -1), (-1, 8, 8, 5)):
        with pytest.raises(ValueError):
            search_sorted_kernel(*bad)
    for bad in (-1, 1 << 32):
        with pytest.raises(ValueError):
            search_sorted_stride(bad)


def test_cases_reach_both_tiers_and_every_output_width(L):
    """(no device needed) the arithmetic of this file is the library's, and the width cases launch every instance of both kernels"""
    for rows in LDS_ROWS + GLOBAL_ROWS + [0, 300, 3001]:
        assert L.mi355_search_sorted_kernel(9, 9, 32, rows).decode() == want_family(rows) and L.mi355_search_sorted_stride(rows) == want_stride(rows)
    assert all(want_family(rows) == LDS_KERNEL for rows in LDS_ROWS) and all(want_family(rows) == GLOBAL_KERNEL for rows in GLOBAL_ROWS)
    assert {co for _, _, co in WIDTH_CASES} == set(range(1, 33)) and {co for _, _, co in GLOBAL_WIDTH_CASES} == set(range(15, 33))
    for slot in range(3):
        assert {case[slot] for case in WIDTH_CASES} >= set(WIDTHS)
    assert {(c, ct) for c, ct, _ in WIDTH_CASES} >= {(c, ct) for c in WIDTHS for ct in WIDTHS}
    assert all(LMAX + 1 <= (1 << co) - 1 for _, _, co in GLOBAL_WIDTH_CASES)


def test_search_wrappers_pass_what_the_abi_takes(fake, L):
    import torch

    eng, rec, col = fake
    fact, table = col(17, 777), col(12, 4001)

    def one():
        (name, a), = rec.calls
        rec.calls.clear()
        assert name == "mi355_search_sorted_dev"
        return a

    # defaults: left, every entry, not exact, the width that holds the row count, positions only
    pos, found, hits = eng.search_sorted(fact, table)
    a = one()
    assert a[1:11] == [fact.data.data_ptr(), 777, 17, table.data.data_ptr(), 12, 4001, None, LEFT, 0, 0] and a[12:] == [12, None, None]
    assert (pos.n, pos.c) == (777, 12) and a[11] == pos.data.data_ptr() and pos.data.numel() == L.mi355_compressed_buffer_size(12, 777)
    assert found is None and hits is None
    # everything named
    out, bitmap, count, rows_dev = torch.zeros(payload(777, 20), dtype=torch.uint8), torch.zeros(98, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64)
    pos, found, hits = eng.search_sorted(fact, table, side="right", rows=rows_dev, exact=True, miss=77, co=20, out=out, found=bitmap, hits=count)
    a = one()
    assert a[1:] == [fact.data.data_ptr(), 777, 17, table.data.data_ptr(), 12, 4001, rows_dev.data_ptr(), RIGHT, 1, 77, out.data_ptr(), 20, bitmap.data_ptr(),
                     count.data_ptr()]
    assert pos.data is out and found is bitmap and hits is count
    # an int row bound below the table's length; exact widens co to hold miss
    pos, _, _ = eng.search_sorted(fact, table, rows=100, exact=True, miss=4001)
    a = one()
    assert a[6:8] == [100, None] and a[9:11] == [1, 4001] and a[12] == 12 and pos.c == 12
    pos, _, _ = eng.search_sorted(fact, table, rows=100)
    assert one()[12] == 7 and pos.c == 7
    # allocated bitmap and counter; no positions
    pos, found, hits = eng.search_sorted(fact, table, out=False, found=True, hits=True)
    a = one()
    assert pos is None and a[11] is None and a[13] == found.data_ptr() and found.numel() == 98 and a[14] == hits.data_ptr() and hits.dtype == torch.int64
    # the empty table needs no buffer
    eng.search_sorted(fact, col(9, 0))
    a = one()
    assert a[4:7] == [None, 9, 0] and a[12] == 1
    # an empty column: every result asked for still travels as its pointer (the call decides that n == 0 launches nothing)
    empty = col(17, 0)
    pos, found, hits = eng.search_sorted(empty, table)
    a = one()
    assert a[1:4] == [None, 0, 17] and a[11] == pos.data.data_ptr() and a[12:] == [12, None, None] and (pos.n, pos.c) == (0, 12)
    assert pos.data.numel() == L.mi355_compressed_buffer_size(12, 0)
    pos, found, hits = eng.search_sorted(empty, table, out=False, found=True, hits=True)
    a = one()
    assert pos is None and a[2] == 0 and a[11] is None and found.numel() == 0 and a[13] == found.data_ptr() and a[14] == hits.data_ptr()
    # refusals of the wrapper
    for kw in (dict(side="middle"), dict(rows=4002), dict(rows=-1), dict(co=0), dict(co=33), dict(co=11), dict(exact=True, miss=1 << 12, co=12), dict(miss=-1),
               dict(miss=1 << 32)):
        with pytest.raises(ValueError):
            eng.search_sorted(fact, table, **kw)
    with pytest.raises(AssertionError):
        eng.search_sorted(fact, table, out=False)  # nothing asked for
    with pytest.raises(AssertionError):
        eng.search_sorted(fact, table, out=torch.zeros(payload(777, 12) - 1, dtype=torch.uint8))
    with pytest.raises(AssertionError):
        eng.search_sorted(fact, table, found=torch.zeros(97, dtype=torch.uint8))
    assert rec.calls == []


def test_compositions_are_the_calls_they_name(fake, L):
    import torch

    eng, rec, col = fake
    fact, table = col(17, 777), col(12, 4001)

    def calls():
        got = list(rec.calls)
        rec.calls.clear()
        return got

    bins = eng.bucketize(fact, col(17, 40))
    (name, a), = calls()
    assert name == "mi355_search_sorted_dev" and a[5:11] == [17, 40, None, RIGHT, 0, 0] and a[12:] == [6, None, None] and (bins.n, bins.c) == (777, 6)
    idx = eng.index_of(fact, table, miss=4001)
    (name, a), = calls()
    assert name == "mi355_search_sorted_dev" and a[5:11] == [12, 4001, None, LEFT, 1, 4001] and a[12:] == [12, None, None] and (idx.n, idx.c) == (777, 12)
    bitmap, hits = eng.is_member(fact, table)
    (name, a), = calls()
    assert name == "mi355_search_sorted_dev" and a[5:11] == [12, 4001, None, LEFT, 0, 0] and a[11] is None
    assert a[13] == bitmap.data_ptr() and a[14] == hits.data_ptr() and bitmap.numel() == 98
    # ... and on an empty column: the same calls, n = 0, every pointer as it is
    empty = col(17, 0)
    bins, idx = eng.bucketize(empty, col(17, 40)), eng.index_of(empty, table, miss=4001)
    (n1, a1), (n2, a2) = calls()
    assert n1 == n2 == "mi355_search_sorted_dev" and a1[2] == a2[2] == 0 and a1[11] == bins.data.data_ptr() and a2[11] == idx.data.data_ptr()
    assert (bins.n, bins.c, idx.n, idx.c) == (0, 6, 0, 12)
    bitmap, hits = eng.is_member(empty, table)
    (name, a), = calls()
    assert a[2] == 0 and a[11] is None and a[13] == bitmap.data_ptr() and a[14] == hits.data_ptr() and bitmap.numel() == 0
    keys = col(32, 500)
    mask = torch.zeros(63, dtype=torch.uint8)
    sorted_col, rowids, count = eng.sorted_keys(keys, mask)
    (n1, a1), (n2, a2) = calls()
    assert n1 == "mi355_sort_rows_dev" and a1[1:7] == [keys.data.data_ptr(), 500, 32, mask.data_ptr(), 0, 0] and a1[7] == rowids.data_ptr() and a1[9:] == [500, count.data_ptr()]
    assert n2 == "mi355_pack_u32_dev" and a2[1] == a1[8] and a2[2:4] == [500, 32] and a2[4] == sorted_col.data.data_ptr() and (sorted_col.n, sorted_col.c) == (500, 32)
    attr = col(9, 500)
    res = eng.sparse_lookup(fact, keys, attr, miss=5, mask=mask)
    got = calls()
    assert [n for n, _ in got] == ["mi355_sort_rows_dev", "mi355_pack_u32_dev", "mi355_gather_dev", "mi355_pack_u32_dev", "mi355_search_sorted_dev", "mi355_lookup_dev"]
    sort_a, pack_a, gather_a, pack2_a, search_a, lookup_a = (a for _, a in got)
    assert gather_a[1:4] == [attr.data.data_ptr(), 500, 9] and gather_a[5] == sort_a[7] and gather_a[6] == sort_a[10] and gather_a[7] == 500
    assert pack2_a[1] == gather_a[8] and pack2_a[2:4] == [500, 9]
    # the search: the fact column against the sorted keys, the row count read on the device, exact, its miss the dimension's row count
    assert search_a[1:4] == [fact.data.data_ptr(), 777, 17] and search_a[4] == pack_a[4] and search_a[5:7] == [32, 500] and search_a[7] == sort_a[10]
    assert search_a[8:11] == [LEFT, 1, 500] and search_a[12:] == [9, None, None]
    # the lookup: the positions through the attributes in key order
    assert lookup_a[1] == search_a[11] and lookup_a[2:4] == [777, 9] and lookup_a[4] == pack2_a[4] and lookup_a[5:8] == [500, 9, 5] and (res.n, res.c) == (777, 9)
    res = eng.sparse_lookup(col(17, 0), keys, attr, miss=5)
    got = calls()
    assert [n for n, _ in got][-2:] == ["mi355_search_sorted_dev", "mi355_lookup_dev"] and got[-2][1][2] == 0 and got[-1][1][2] == 0 and (res.n, res.c) == (0, 9)


def test_search_entry_point_fails_loudly_without_a_gpu(L):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    buf = (C.c_uint8 * 1024)()
    tab = (C.c_uint8 * 1024)()
    out = (C.c_uint8 * 1024)()
    rc = L.mi355_search_sorted_dev(None, buf, 100, 9, tab, 12, 300, None, LEFT, 0, 0, out, 9, None, None)
    assert rc != 0 and L.mi355_last_error()


def test_every_search_kernel_has_a_case():
    """every __global__ under csrc/search/ is asserted from the launch record by a GPU case of this file, and the file names no
    kernel that does not exist"""
    kernels = support.global_kernels_of("search")
    assert kernels == {LDS_KERNEL, GLOBAL_KERNEL}, kernels
    support.check_gpu_part_asserts(__file__, "LDS_KERNEL", "GLOBAL_KERNEL")  # test_table_sizes names each from the record, per tier
    assert {want_family(rows_for(co)) for _, _, co in WIDTH_CASES} == {LDS_KERNEL} and want_family(LMAX + 1) == GLOBAL_KERNEL


def test_search_sources_read_no_flag_bits_and_no_context_state():
    assert [os.path.basename(p) for p in support.feature_sources("search")] == ["search.hpp", "search_sorted.hip"]
    support.check_sources_read_no_flag_bits("search")
    mine = {name for name, path, _ in support.hip_functions() if path.startswith("search" + os.sep)}
    assert {"mi355_search_sorted_dev", "mi355_search_sorted_kernel", "mi355_search_sorted_stride"} <= mine
    assert not mine & set(support.entry_points_reaching("rowid_ws_get("))
    assert not mine & set(support.entry_points_reaching("kernel_scratch"))
    for path in support.feature_sources("search"):
        text = open(path).read()
        assert "rowid_ws_get(" not in text and "kernel_scratch" not in text and "pool_get(" not in text, path


def descent_model(table, R, top, lg, x, side):
    """search.hpp's descent, statement by statement, on numpy arrays: the samples t[(k + 1) S - 1], the steps >= S through them with
    the clamped sample index, the steps below S through the table with the clamped entry index -> (pos, found, every table index
    read)"""
    t = table.astype(np.int64)
    x = x.astype(np.int64)
    pos = np.zeros(len(x), dtype=np.int64)
    if R == 0:
        return pos, np.zeros(len(x), dtype=bool), []
    ns = R >> lg
    samples = np.array([t[((k + 1) << lg) - 1] for k in range(ns)] + [-7], dtype=np.int64)  # (-7: the dword behind, never a value)
    read = [((k + 1) << lg) - 1 for k in range(ns)]
    last = np.zeros(len(x), dtype=np.int64)
    s = top
    while s:
        cand = pos + s
        if s >> lg:
            kk = np.minimum(cand >> lg, ns)
            e = samples[np.where(kk > 0, kk - 1, 0)]
        else:
            j = np.minimum(cand, R) - 1
            read += j.tolist()
            e = t[j]
        ok = (cand <= R) & ((e <= x) if side == RIGHT else (e < x))
        pos = np.where(ok, cand, pos)
        last = np.where(ok, e, last)
        s >>= 1
    if side == RIGHT:
        return pos, (pos != 0) & (last == x), read
    j = np.minimum(pos, R - 1)
    read += j.tolist()
    return pos, (pos < R) & (t[j] == x), read


def test_descent_model_against_numpy():
    """(no device needed) the descent as the kernels spell it, sample stride 1, 4 and 16, a device row count below the host's bound
    included: numpy.searchsorted's positions, numpy.isin's members, and no index outside [0, R)"""
    rng = np.random.default_rng(3)
    for trial in range(1500):
        rows = int(rng.integers(0, 70))
        lg = int(rng.integers(0, 3)) * 2
        R = rows if trial % 3 else int(rng.integers(0, rows + 1))
        top = 0 if rows == 0 else 1 << (rows.bit_length() - 1)
        hi = [4, 40, 1 << 32][trial % 3]
        table = np.sort(rng.integers(0, hi, rows, dtype=np.uint64)).astype(np.uint32)
        if rows and trial % 5 == 0:
            table[-1] = (1 << 32) - 1
        x = np.concatenate([rng.integers(0, hi, 40, dtype=np.uint64), table[:R].astype(np.uint64), [0, (1 << 32) - 1]]).astype(np.uint32)
        for side in (LEFT, RIGHT):
            pos, found, read = descent_model(table, R, top, lg, x, side)
            want_pos, want_found = expect(x, table, R, side)
            assert (pos == want_pos).all() and (found == want_found).all(), (trial, rows, R, lg, side)
            assert all(0 <= j < R for j in read), (trial, rows, R, lg, side)


def gpu_shapes():
    """every (c, ct, rows, n, kind) the GPU tests below run on recipe data"""
    c, ct, rows, _ = SIZE_CASE
    shapes = {(c, ct, rows, n, "plain") for n in SIZES}
    shapes |= {(c, ct, rows, N_BIG, "plain")}
    shapes |= {(c, ct, rows_for(co), N_BIG, "limit") for c, ct, co in WIDTH_CASES}
    shapes |= {(c, ct, LMAX + 1, N_BIG, "limit") for c, ct, co in GLOBAL_WIDTH_CASES}
    shapes |= {(9, 17, 3001, N_BIG, "above"), (9, 17, LMAX + 1, N_BIG, "above"), (17, 9, 300, N_BIG, "limit"), (24, 9, LMAX + 1, N_BIG, "limit")}
    shapes |= {(32, 32, 3001, N_BIG, "limit"), (32, 32, LMAX + 1, N_BIG, "limit")}
    shapes |= {(24, 24, rows, N_BIG, "plain") for rows in LDS_ROWS + GLOBAL_ROWS}
    shapes |= {(17, 17, 3001, N_BIG, "equal"), (24, 24, LMAX + 1, N_BIG, "equal")}
    shapes |= {(24, 24, rows, N_BIG, "plain") for rows, _ in ROWS_DEV_CASES}
    shapes |= {(c, ct, rows, N_BIG, "plain") for c, ct, rows in OFFSET_CASES}
    shapes |= {(c, ct, rows, N_VIEW, "plain") for c, ct, rows in VIEW_CASES}
    shapes |= {(c, ct, rows, N_LONG, "plain") for c, ct, rows in LONG_CASES}
    shapes |= {ERROR_CASE[:3] + (ERROR_CASE[3], "plain")}
    return sorted(shapes)


@pytest.mark.parametrize("shape", [s for s in gpu_shapes() if s[3] >= 12], ids=pid)
def test_recipe_is_not_vacuous(shape):
    """(no device needed) what every case must exercise: found rows and, unless the table holds every value of c bits, rows that are
    not found; duplicate entries from four entries on; the limits in the `limit` recipe.  A position of 0 (of R) is asked for under each side where a c-bit probe
    can have it -- left: 0 always, R when the last entry is below 2^c - 1; right: 0 when the first entry is above 0, R when the
    last entry is at most 2^c - 1 -- and under at least one side anyway, except R where the table's last entry lies above every
    probe (the `above` recipe: that is its point)."""
    c, ct, rows, n, kind = shape
    table, x = table_of(c, ct, rows, kind), probes_of(c, ct, rows, n, kind)
    top = (1 << c) - 1
    assert len(table) == rows and len(x) == n and (np.diff(table.astype(np.int64)) >= 0).all() and int(x.max()) <= top
    assert int(table.max()) <= (1 << ct) - 1
    first, last = int(table[0]), int(table[-1])
    seen0 = seenR = False
    for _, side in SIDES:
        pos, found = expect(x, table, rows, side)
        assert found.any(), "found rows"
        assert not found.all() or len(np.unique(table[table <= top])) == top + 1, "not-found rows (unless the table holds every c-bit value)"
        can0 = side == LEFT or first > 0
        canR = last < top if side == LEFT else last <= top
        assert not can0 or (pos == 0).any(), ("no row with position 0", side)
        assert not canR or (pos == rows).any(), ("no row with position R", side)
        seen0, seenR = seen0 or (pos == 0).any(), seenR or (pos == rows).any()
        if rows >= 3 and kind != "equal":
            assert ((pos > 0) & (pos < rows)).any(), "no row lands inside the table"
    assert seen0 and (seenR or last > top)
    if rows >= 4:
        assert (np.diff(table.astype(np.int64)) == 0).any(), "duplicate table entries"
    if kind == "limit":
        assert (x == 0).any() and (x == top).any()
        if rows >= 2:
            assert first == 0 and last == (1 << ct) - 1
    if kind == "above":
        assert last > top and (table.astype(np.int64) > top).sum() >= rows // 2 and first <= top
    if kind == "equal":
        for _, side in SIDES:
            pos, found = expect(x, table, rows, side)
            assert set(np.unique(pos)) == {0, rows} and (x == first).any() and (x < first).any() and (x > first).any()


@pytest.mark.parametrize("shape", [s for s in gpu_shapes() if s[3] < 12], ids=pid)
def test_one_row_shapes_probe_zero(shape):
    """(no device needed) n = 1 holds one row, value 0: it cannot carry the properties above, but its position is 0 and it is not found"""
    c, ct, rows, n, kind = shape
    assert n == 1 and kind == "plain"
    pos, found = expect(probes_of(c, ct, rows, n), table_of(c, ct, rows), rows, LEFT)
    assert int(pos[0]) == 0 and not found[0]


def test_wrap_case_is_in_the_data():
    """c = ct = 32 under RIGHT with x = 2^32 - 1 and an entry 2^32 - 1: `t < x + 1` would wrap"""
    for rows in (3001, LMAX + 1):
        table, x = table_of(32, 32, rows, "limit"), probes_of(32, 32, rows, N_BIG, "limit")
        assert int(table[-1]) == (1 << 32) - 1 and (x == (1 << 32) - 1).any()
        pos, found = expect(x, table, rows, RIGHT)
        assert (pos[x == (1 << 32) - 1] == rows).all() and found[x == (1 << 32) - 1].all()


@functools.lru_cache(maxsize=None)
def sparse_data():
    """32-bit keys drawn from all of 2^32: a dimension of 5000 rows with repeated keys and a filter, 9-bit attributes, a fact column
    half of whose keys occur in the dimension"""
    rng = np.random.default_rng(31)
    dim = rng.integers(0, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32)
    dim[100:400] = dim[1000:1300]  # repeats: the lower row wins
    dim[7], dim[8] = 0, (1 << 32) - 1
    attr = rng.integers(0, 1 << 9, 5000, dtype=np.uint64).astype(np.uint32)
    sel = rng.random(5000) < 0.7
    sel[100:250] = False           # ... unless the filter drops it
    fk = rng.integers(0, 1 << 32, N_BIG, dtype=np.uint64).astype(np.uint32)
    take = rng.random(N_BIG) < 0.5
    fk[take] = dim[rng.integers(0, 5000, int(take.sum()))]
    for a in (dim, attr, sel, fk):
        a.setflags(write=False)
    return dim, attr, sel, fk


def sparse_want(dim, attr, sel, fk, miss):
    first = {}
    for row in np.nonzero(sel)[0]:
        first.setdefault(int(dim[row]), int(row))
    return np.array([attr[first[int(k)]] if int(k) in first else miss for k in fk], dtype=np.uint32)


def test_chain_data_is_not_vacuous():
    dim, attr, sel, fk = sparse_data()
    want = sparse_want(dim, attr, sel, fk, 511)
    hit = np.isin(fk, dim[sel])
    assert hit.sum() * 4 >= len(fk) and (~hit).sum() * 4 >= len(fk)
    assert len(np.unique(dim)) < len(dim) and np.isin(fk, dim[~sel]).any() and int(dim.max()) >= 1 << 31
    # a key whose lower row is filtered out resolves to its upper row; one whose rows both pass, to the lower
    both = [k for k in range(250, 400) if sel[k] and sel[k + 900]]
    upper = [k for k in range(100, 250) if sel[k + 900]]
    assert both and upper
    assert sparse_want(dim, attr, sel, dim[both], 511).tolist() == attr[both].tolist()
    assert sparse_want(dim, attr, sel, dim[upper], 511).tolist() == attr[[k + 900 for k in upper]].tolist()
    assert (want[~hit] == 511).all()


@functools.lru_cache(maxsize=None)
def capture_data(c, ct, rows):
    """three versions of column, table and device row count: version 1 changes all three, version 2 only the count"""
    cols = [probes_of(c, ct, rows, N_BIG, "plain", salt=v) for v in (0, 1, 0)]
    tables = [table_of(c, ct, rows, "plain", salt=v) for v in (0, 1, 0)]
    return cols, tables, [rows, rows - 3, rows // 2]


@pytest.mark.parametrize("case", CAPTURE_CASES, ids=pid)
def test_capture_data_is_not_vacuous(case):
    c, ct, rows = case
    cols, tables, counts = capture_data(c, ct, rows)
    res = [expect(cols[v], tables[v], counts[v], LEFT) for v in range(3)]
    for a, b in ((0, 1), (1, 2), (0, 2)):
        assert (res[a][0] != res[b][0]).any() and (res[a][1] != res[b][1]).any(), "a stale result could pass"
    assert (cols[0] != cols[1]).any() and (tables[0] != tables[1]).any() and len(set(counts)) == 3


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

class Search:
    """one engine, an uploaded column and table (both in hostile surroundings), guarded outputs refilled with 0xEE before every call"""

    def __init__(self, O, eng, c, ct, rows, n, kind="plain", x=None, table=None, table_offset=0, co=None):
        from shared_simd_scan_amd.engine import PackedColumn

        self.O, self.eng, self.c, self.ct, self.rows, self.n = O, eng, c, ct, rows, n
        if x is None:
            x, table = probes_of(c, ct, rows, n, kind), table_of(c, ct, rows, kind)
        self.x, self.table_vals = x, table
        self.co = width_for(rows) if co is None else co
        self.col = PackedColumn(hostile_pack(O, x, c), n, c)
        self.table = PackedColumn(hostile_pack(O, table, ct, table_offset), rows, ct)
        self.out, self.found, self.hits = Guarded(payload(n, self.co)), Guarded((n + 7) // 8), Guarded(8, back=64, front=64)
        self.rows_word = None

    def outputs(self):
        return (self.out, self.found, self.hits)

    def refill(self):
        for g in self.outputs():
            g.t.fill_(SENTINEL)

    def call(self, L, side=LEFT, exact=False, miss=None, with_out=True, with_found=True, with_hits=True, have=None, table_ptr="mine", **kw):
        """the raw entry point -> status; `have`: the value of *rows_dev (None: no rows_dev)"""
        import torch

        rows_dev = None
        if have is not None:
            self.rows_word = torch.tensor([have], dtype=torch.int64, device="cuda")
            rows_dev = self.rows_word.data_ptr()
        a = dict(cp=self.col.data.data_ptr(), n=self.n, c=self.c, tp=self.table.data.data_ptr() if table_ptr == "mine" else table_ptr, ct=self.ct,
                 rows=self.rows, rows_dev=rows_dev, side=side, exact=1 if exact else 0, miss=(miss_of(self.co) if exact else 0) if miss is None else miss,
                 op=self.out.ptr if with_out else None, co=self.co, fp=self.found.ptr if with_found else None, hp=self.hits.ptr if with_hits else None)
        a.update(kw)
        self.refill()
        rc = L.mi355_search_sorted_dev(self.eng._ctx, a["cp"], a["n"], a["c"], a["tp"], a["ct"], a["rows"], a["rows_dev"], a["side"], a["exact"], a["miss"],
                                       a["op"], a["co"], a["fp"], a["hp"])
        self.eng.synchronize()
        return rc

    def run(self, L, side=LEFT, exact=False, with_out=True, with_found=True, with_hits=True, have=None, what="", **kw):
        """-> checks every output byte, the trailing bits, the guards, the inputs and the launch record; returns the record"""
        import torch

        tag = (what, self.c, self.ct, self.co, self.rows, self.n, side, exact, have)
        rows_eff = self.rows if have is None else min(self.rows, have)
        pos, found = expect(self.x, self.table_vals, rows_eff, side)
        miss = miss_of(self.co)
        col_before, table_before = self.col.data.clone(), self.table.data.clone()
        assert self.call(L, side, exact, None, with_out, with_found, with_hits, have, **kw) == 0, (tag, L.mi355_last_error())
        want_out = np.where(found, pos, miss) if exact else pos
        images = ((self.out, with_out, self.O.pack(want_out.astype(np.uint32), self.co)[: self.out.nbytes], "positions"),
                  (self.found, with_found, packbits(found), "found bitmap"),
                  (self.hits, with_hits, np.frombuffer(np.uint64(found.sum()).tobytes(), dtype=np.uint8), "hits"))
        for g, given, want, name in images:
            have_bytes = g.fetch()  # asserts the guard bytes on both sides
            if not given:
                assert (have_bytes == SENTINEL).all(), (tag, name, "written though not asked for")
                continue
            assert len(want) == g.nbytes
            bad = np.nonzero(have_bytes != want)[0]
            assert bad.size == 0, (tag, name, "byte", int(bad[0]), "of", g.nbytes, "have", int(have_bytes[bad[0]]), "want", int(want[bad[0]]), "wrong", int(bad.size))
        if with_out and (self.n * self.co) % 8:
            assert int(self.out.fetch()[-1]) >> ((self.n * self.co) % 8) == 0, (tag, "bits behind the last position are not zero")
        if with_found and self.n % 8:
            assert int(self.found.fetch()[-1]) >> (self.n % 8) == 0, (tag, "bits behind the last row are not zero")
        assert torch.equal(self.col.data, col_before), (tag, "column written")
        assert torch.equal(self.table.data, table_before), (tag, "table written")
        if have is not None:
            assert int(self.rows_word.item()) == have, (tag, "*rows_dev written")
        rec = record(L, self.eng)
        (label, grid, lds, flags), = rec
        fam = want_family(self.rows)
        assert base_name(label) == fam == L.mi355_search_sorted_kernel(self.c, self.ct, self.co, self.rows).decode() and label.startswith(f"{fam}<{self.co}>"), (tag, label)
        assert flags == 0 and lds >= 4 * 2 * 256 * self.c + 4 * (self.rows // want_stride(self.rows)), (tag, lds)
        return rec

    def both_sides(self, L, **kw):
        for _, side in SIDES:
            for exact in (False, True):
                self.run(L, side=side, exact=exact, **kw)


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_tails(L, O, eng, n):
    c, ct, rows, co = SIZE_CASE
    Search(O, eng, c, ct, rows, n, co=co).both_sides(L)


@gpu
@pytest.mark.parametrize("combo", OUTPUT_COMBOS, ids=lambda p: "".join("ofh"[i] if p[i] else "-" for i in range(3)))
def test_output_combinations(L, O, eng, combo):
    with_out, with_found, with_hits = combo
    for rows in (1000, LMAX + 1):
        s = Search(O, eng, 17, 17, rows, N_BIG)
        s.both_sides(L, with_out=with_out, with_found=with_found, with_hits=with_hits)


@gpu
@pytest.mark.parametrize("case", WIDTH_CASES, ids=pid)
def test_widths(L, O, eng, case):
    c, ct, co = case
    Search(O, eng, c, ct, rows_for(co), N_BIG, kind="limit", co=co).both_sides(L)


@gpu
@pytest.mark.parametrize("case", GLOBAL_WIDTH_CASES, ids=pid)
def test_widths_global_tier(L, O, eng, case):
    c, ct, co = case
    Search(O, eng, c, ct, LMAX + 1, N_BIG, kind="limit", co=co).both_sides(L)


@gpu
@pytest.mark.parametrize("case", [(9, 17, 3001, "above"), (9, 17, LMAX + 1, "above"), (17, 9, 300, "limit"), (24, 9, LMAX + 1, "limit"),
                                  (32, 32, 3001, "limit"), (32, 32, LMAX + 1, "limit")], ids=pid)
def test_unequal_widths_and_the_wrap(L, O, eng, case):
    """c < ct with entries above every probe, c > ct with probes above every entry, c = ct = 32 with x = 2^32 - 1 under RIGHT"""
    c, ct, rows, kind = case
    s = Search(O, eng, c, ct, rows, N_BIG, kind=kind)
    if c > ct:
        assert int(s.x.max()) > int(s.table_vals.max())
    s.both_sides(L)


@gpu
@pytest.mark.parametrize("rows", LDS_ROWS + GLOBAL_ROWS)
def test_table_sizes(L, O, eng, rows):
    s = Search(O, eng, 24, 24, rows, N_BIG)
    for _, side in SIDES:
        (label, grid, lds, flags), = s.run(L, side=side, exact=side == LEFT)
        if rows in LDS_ROWS:
            assert base_name(label) == LDS_KERNEL
        else:
            assert base_name(label) == GLOBAL_KERNEL
        if rows in GLOBAL_ROWS:
            assert lds <= 4 * 2 * 256 * 24 + 16 + LDS_MAX + 16 and L.mi355_search_sorted_stride(rows) == GLOBAL_STRIDES[GLOBAL_ROWS.index(rows)]


@gpu
@pytest.mark.parametrize("with_buffer", [False, True], ids=["null", "buffer"])
def test_empty_table(L, O, eng, with_buffer):
    """rows == 0: position 0 everywhere, nothing found, with no table pointer at all or with one whose bytes are all ones"""
    s = Search(O, eng, 24, 17, 0, N_BIG, co=5)
    for _, side in SIDES:
        for exact in (False, True):
            rec = s.run(L, side=side, exact=exact, **({} if with_buffer else dict(tp=None)))
            assert base_name(rec[0][0]) == want_family(0) == LDS_KERNEL


@gpu
@pytest.mark.parametrize("rows", [3001, LMAX + 1])
def test_all_equal_table(L, O, eng, rows):
    c = 17 if rows == 3001 else 24
    s = Search(O, eng, c, c, rows, N_BIG, kind="equal")
    s.both_sides(L)
    v = int(s.table_vals[0])
    pos_l, pos_r = expect(s.x, s.table_vals, rows, LEFT)[0], expect(s.x, s.table_vals, rows, RIGHT)[0]
    assert (pos_l[s.x <= v] == 0).all() and (pos_l[s.x > v] == rows).all() and (pos_r[s.x >= v] == rows).all() and (pos_r[s.x < v] == 0).all()


@gpu
@pytest.mark.parametrize("case", ROWS_DEV_CASES, ids=pid)
def test_rows_dev(L, O, eng, case):
    """R = min(rows, *rows_dev), read on the device; the tier follows the host's bound"""
    rows, have = case
    s = Search(O, eng, 24, 24, rows, N_BIG)
    for _, side in SIDES:
        rec = s.run(L, side=side, exact=side == RIGHT, have=have)
        assert base_name(rec[0][0]) == want_family(rows)


@gpu
@pytest.mark.parametrize("case", OFFSET_CASES, ids=pid)
def test_table_at_four_byte_offsets(L, O, eng, case):
    """the table is a view at a 4-byte-aligned, not 16-byte-aligned offset inside a buffer of 0xff, ones behind entry R - 1"""
    c, ct, rows = case
    for offset in (4, 12, 8):
        s = Search(O, eng, c, ct, rows, N_BIG, table_offset=offset)
        assert s.table.data.data_ptr() % 16 == offset
        s.both_sides(L, what=f"table at +{offset}")
    # ... and with the entries behind R hostile too: the device row count cuts the table in front of an entry of all ones
    s = Search(O, eng, c, ct, rows, N_BIG, table_offset=4)
    cut = rows - 7
    hostile = s.table_vals.copy()
    hostile[cut:] = (1 << ct) - 1
    from shared_simd_scan_amd.engine import PackedColumn
    s.table = PackedColumn(hostile_pack(O, hostile, ct, 4), rows, ct)
    for _, side in SIDES:
        s.run(L, side=side, have=cut, what="hostile entries behind R")


@gpu
@pytest.mark.parametrize("case", VIEW_CASES, ids=pid)
def test_row_range_views(L, O, eng, case):
    """rows [lead, lead + n) of a longer column searched into rows [lead_out, lead_out + n) of a longer output column and of a longer
    bitmap: exactly the slices' bytes change, and nothing of the foreign rows reaches them"""
    from shared_simd_scan_amd.engine import PackedColumn

    c, ct, rows = case
    co = width_for(rows)
    n, lead, trail, lead_out = N_VIEW, 2 * R + 128, 4096, 384
    assert n % 8 == 0 and n % 32 and lead % 128 == 0 and lead_out % 128 == 0
    x, table = probes_of(c, ct, rows, n), table_of(c, ct, rows)
    rng = np.random.default_rng([c, ct, 13])
    top = (1 << c) - 1
    junk = rng.integers(0, top + 1, lead, dtype=np.uint64).astype(np.uint32)
    whole = PackedColumn(plain_pack(O, np.concatenate([junk, x, np.full(trail, top, dtype=np.uint32)]), c), lead + n + trail, c)
    col = eng.slice_rows(whole, lead, lead + n)
    assert col.n == n and col.data.data_ptr() % 16 == 0
    n_out = lead_out + n + 1000
    before = rng.integers(0, 1 << co, n_out, dtype=np.uint64).astype(np.uint32)
    before_bits = rng.random(n_out) < 0.5
    tab = PackedColumn(hostile_pack(O, table, ct), rows, ct)
    for name, side in SIDES:
        out_whole = PackedColumn(plain_pack(O, before, co), n_out, co)
        out_slice = eng.slice_rows(out_whole, lead_out, lead_out + n)
        bits_whole = plain_pack(O, before_bits.astype(np.uint32), 1)
        bits_slice = bits_whole[lead_out // 8:]
        res, found, hits = eng.search_sorted(col, tab, side=name, out=out_slice.data, found=bits_slice, hits=True)
        eng.synchronize()
        (label, _, _, _), = record(L, eng)
        assert base_name(label) == want_family(rows) and res.data.data_ptr() == out_slice.data.data_ptr()
        pos, fnd = expect(x, table, rows, side)
        after, after_bits = before.copy(), before_bits.copy()
        after[lead_out: lead_out + n], after_bits[lead_out: lead_out + n] = pos, fnd
        assert (out_whole.data.cpu().numpy() == O.pack(after, co)).all(), "positions: rows outside the slice changed, or wrong inside"
        assert (bits_whole.cpu().numpy() == O.pack(after_bits.astype(np.uint32), 1)).all(), "bitmap: rows outside the slice changed, or wrong inside"
        assert int(hits.item()) == int(fnd.sum())


@gpu
@pytest.mark.parametrize("case", UNSORTED_CASES, ids=pid)
def test_unsorted_table_keeps_the_contract(L, O, eng, case):
    """a shuffled table: every position lies in [0, R], found is set exactly where the named entry equals the row's value, the
    counter is the bitmap's, and the guards stand"""
    c, ct, rows = case
    rng = np.random.default_rng([5, rows])
    table = table_of(c, ct, rows).copy()
    rng.shuffle(table)
    assert (np.diff(table.astype(np.int64)) < 0).any()
    x = probes_of(c, ct, rows, N_BIG)
    s = Search(O, eng, c, ct, rows, N_BIG, x=x, table=table)
    t64, x64 = table.astype(np.int64), x.astype(np.int64)
    for _, side in SIDES:
        assert s.call(L, side=side) == 0
        (label, _, _, _), = record(L, eng)
        assert base_name(label) == want_family(rows)
        pos = O.decompress(s.out.fetch(), N_BIG, s.co).view(np.uint32).astype(np.int64)
        found = np.unpackbits(s.found.fetch(), bitorder="little")[:N_BIG].astype(bool)
        hits = int(np.frombuffer(s.hits.fetch().tobytes(), dtype=np.uint64)[0])
        assert (pos >= 0).all() and (pos <= rows).all()
        if side == LEFT:
            named = (pos < rows) & (t64[np.minimum(pos, rows - 1)] == x64)
        else:
            named = (pos > 0) & (t64[np.maximum(pos, 1) - 1] == x64)
        assert (found == named).all() and hits == int(found.sum())
        assert (np.packbits(found, bitorder="little") == s.found.fetch()).all()  # bits >= n are zero


@gpu
@pytest.mark.parametrize("case", LONG_CASES, ids=pid)
def test_one_block_walks_many_tiles(L, O, eng, case):
    """grid_cus = 1, max_blocks_per_cu = 1: one block, its four waves walk ten tiles each -- the alternating images, the deferred
    stores, the ragged tail"""
    c, ct, rows = case
    s = Search(O, eng, c, ct, rows, N_LONG)
    eng.set_option("grid_cus", 1)
    eng.set_option("max_blocks_per_cu", 1)
    try:
        for _, side in SIDES:
            (label, grid, lds, flags), = s.run(L, side=side, exact=side == LEFT, what="one block")
            assert grid == 1 and base_name(label) == want_family(rows)
    finally:
        eng.set_option("grid_cus", 0)
        eng.set_option("max_blocks_per_cu", 0)
    (label, grid, lds, flags), = s.run(L, what="whole chip")
    assert grid > 1


@gpu
def test_errors_launch_nothing(L, O, eng):
    c, ct, rows, n = ERROR_CASE
    s = Search(O, eng, c, ct, rows, n)
    co = s.co
    big = Guarded(8192)  # a buffer that can stand for an input and an output at once
    cp, tp, op, fp, hp = s.col.data.data_ptr(), s.table.data.data_ptr(), s.out.ptr.value, s.found.ptr.value, s.hits.ptr.value

    def call(**kw):
        big.t.fill_(SENTINEL)
        return s.call(L, have=7 if kw.pop("with_rows_dev", False) else None, **kw)

    assert call() == 0 and base_name(record(L, eng)[0][0]) == want_family(rows)
    valid = record(L, eng)
    nb_out, nb_col, nb_found, nb_tab = payload(n, co), payload(n, c), (n + 7) // 8, (rows * ct + 31) // 32 * 4
    assert max(nb_out, nb_col, nb_tab) + 1024 <= 8192
    b = big.ptr.value
    s.call(L, have=7)
    rd = s.rows_word.data_ptr()
    errors = (("c = 0", dict(c=0), b"32"), ("c = 33", dict(c=33), b"32"), ("ct = 0", dict(ct=0), b"ct"), ("ct = 33", dict(ct=33), b"ct"),
              ("co = 0", dict(co=0), b"co"), ("co = 33", dict(co=33), b"co"), ("side = 2", dict(side=2), b"side"), ("side = -1", dict(side=-1), b"side"),
              ("rows = 2^32", dict(rows=1 << 32), b"2^32"), ("rows = 2^co", dict(rows=1 << co), b"co"), ("rows beyond co = 1", dict(rows=2, co=1), b"co"),
              ("miss = 2^co", dict(miss=1 << co), b"miss"), ("miss = 2^co without exact", dict(miss=1 << co, exact=0), b"miss"),
              ("no output", dict(with_out=False, with_found=False, with_hits=False), b"nothing to compute"),
              ("null column", dict(cp=None), b"packed_dev"), ("null table", dict(tp=None), b"table_dev"),
              ("column at +4", dict(cp=cp + 4), b"aligned"), ("table at +2", dict(tp=tp + 2), b"aligned"), ("rows_dev at +4", dict(rows_dev=rd + 4), b"aligned"),
              ("positions at +4", dict(op=op + 4), b"aligned"), ("bitmap at +2", dict(fp=fp + 2), b"aligned"), ("counter at +4", dict(hp=hp + 4), b"aligned"),
              ("positions are the column", dict(cp=b, op=b), b"out_dev overlaps packed_dev"),
              ("positions start in the column's last byte", dict(cp=b, op=b + (nb_col - 1) // 16 * 16), b"out_dev overlaps packed_dev"),
              ("column starts inside the positions", dict(cp=b + 256, op=b), b"out_dev overlaps packed_dev"),
              ("positions are the table", dict(tp=b, op=b), b"out_dev overlaps table_dev"),
              ("table starts inside the positions", dict(tp=b + 64, op=b), b"out_dev overlaps table_dev"),
              ("positions start in the table's last dword", dict(tp=b, op=b + (nb_tab - 1) // 16 * 16), b"out_dev overlaps table_dev"),
              ("bitmap is the column", dict(cp=b, fp=b), b"found_dev overlaps packed_dev"),
              ("bitmap starts in the column's last byte", dict(cp=b, fp=b + (nb_col - 1) // 4 * 4), b"found_dev overlaps packed_dev"),
              ("bitmap is the table", dict(tp=b, fp=b), b"found_dev overlaps table_dev"),
              ("bitmap starts in the table's last dword", dict(tp=b, fp=b + nb_tab - 4), b"found_dev overlaps table_dev"),
              ("counter inside the column", dict(cp=b, hp=b + 8), b"hits_dev overlaps packed_dev"),
              ("counter in the table's last dword", dict(tp=b, hp=b + (nb_tab - 1) // 8 * 8), b"hits_dev overlaps table_dev"),
              ("counter is the row count", dict(rows_dev=rd, hp=rd), b"hits_dev overlaps rows_dev"),
              ("counter inside the positions", dict(op=b, hp=b + 16), b"hits_dev overlaps out_dev"),
              ("counter in the bitmap's last byte", dict(fp=b, hp=b + (nb_found - 1) // 8 * 8), b"hits_dev overlaps found_dev"),
              ("row count inside the positions", dict(op=b, rows_dev=b + 8), b"out_dev overlaps rows_dev"),
              ("row count inside the bitmap", dict(fp=b, rows_dev=b + 8), b"found_dev overlaps rows_dev"),
              ("bitmap is the positions", dict(op=b, fp=b), b"out_dev overlaps found_dev"),
              ("bitmap starts in the positions' last byte", dict(op=b, fp=b + (nb_out - 1) // 4 * 4), b"out_dev overlaps found_dev"),
              ("positions start in the bitmap's last byte", dict(fp=b, op=b + (nb_found - 1) // 16 * 16), b"out_dev overlaps found_dev"))
    for what, kw, word in errors:
        assert call(**kw) == E_INVALID, what
        assert word in L.mi355_last_error(), (what, L.mi355_last_error())
        assert record(L, eng) == [], what  # a refused call leaves an empty record and launches nothing
        for g in s.outputs() + (big,):
            assert (g.fetch() == SENTINEL).all(), what
    # without positions neither the row bound nor miss is held against co
    assert call(with_out=False, co=1, miss=5) == 0 and record(L, eng)[0][0].startswith(f"{LDS_KERNEL}<1>") and record(L, eng)[0][1:] == valid[0][1:]
    # neighbours that do not overlap are fine: the bitmap begins where the positions' bytes end, the positions where the table's do
    import torch

    at_out = (nb_tab + 15) // 16 * 16
    at_found = at_out + (nb_out + 3) // 4 * 4
    big.t.fill_(SENTINEL)
    big.t[big.front: big.front + nb_tab] = torch.from_numpy(O.pack(s.table_vals, ct)[:nb_tab].copy()).cuda()
    rc = L.mi355_search_sorted_dev(eng._ctx, cp, n, c, b, ct, rows, None, LEFT, 0, 0, b + at_out, co, b + at_found, None)
    eng.synchronize()
    assert rc == 0 and record(L, eng) == valid
    got = big.fetch()
    pos, fnd = expect(s.x, s.table_vals, rows, LEFT)
    assert (got[at_out: at_out + nb_out] == O.pack(pos.astype(np.uint32), co)[:nb_out]).all() and (got[at_found: at_found + nb_found] == packbits(fnd)).all()
    assert (got[at_out + nb_out: at_found] == SENTINEL).all() and (got[at_found + nb_found:] == SENTINEL).all()
    # n == 0: nothing launched, nothing written but the counter's zero, and no column needed
    assert call(n=0, cp=None) == 0 and record(L, eng) == []
    assert (s.out.fetch() == SENTINEL).all() and (s.found.fetch() == SENTINEL).all() and (s.hits.fetch() == 0).all()
    # ... and no result either: an empty column has an empty answer
    assert call(n=0, cp=None, with_out=False, with_found=False, with_hits=False) == 0 and record(L, eng) == []
    for g in s.outputs():
        assert (g.fetch() == SENTINEL).all()


@gpu
def test_empty_column_through_the_wrapper(L, O, eng):
    """an empty shard, or what a filter left: every wrapper returns its empty result, nothing is launched, a counter asked for is zero"""
    from shared_simd_scan_amd.engine import PackedColumn

    table = PackedColumn(plain_pack(O, table_of(17, 17, 3001), 17), 3001, 17)
    attr = PackedColumn(plain_pack(O, probes_of(9, 9, 300, 3001), 9), 3001, 9)
    empty = eng.alloc_packed(0, 17)
    for side, _ in SIDES:
        pos, found, hits = eng.search_sorted(empty, table, side=side)
        assert (pos.n, pos.c) == (0, 12) and found is None and hits is None and record(L, eng) == []
    pos, found, hits = eng.search_sorted(empty, table, exact=True, miss=3001, found=True, hits=True)
    eng.synchronize()
    assert (pos.n, pos.c) == (0, 12) and found.numel() == 0 and int(hits.item()) == 0 and record(L, eng) == []
    bitmap, hits = eng.is_member(empty, table)
    eng.synchronize()
    assert bitmap.numel() == 0 and int(hits.item()) == 0 and record(L, eng) == []
    bins, idx = eng.bucketize(empty, table), eng.index_of(empty, table, miss=3001)
    assert (bins.n, bins.c, idx.n, idx.c) == (0, 12, 0, 12) and record(L, eng) == []
    res = eng.sparse_lookup(empty, table, attr, miss=7)
    eng.synchronize()
    assert (res.n, res.c) == (0, 9)


@gpu
def test_sparse_lookup_against_numpy(L, O, eng):
    """the join on 32-bit surrogate keys: sort_rows(dim.pk, filter) -> search_sorted(fk, exact) -> lookup, nothing on the host"""
    from shared_simd_scan_amd.engine import PackedColumn
    import torch

    dim, attr, sel, fk = sparse_data()
    dim_keys, dim_attr = PackedColumn(plain_pack(O, dim, 32), len(dim), 32), PackedColumn(plain_pack(O, attr, 9), len(attr), 9)
    fact = PackedColumn(plain_pack(O, fk, 32), len(fk), 32)
    mask = torch.from_numpy(packbits(sel)).cuda()
    res = eng.sparse_lookup(fact, dim_keys, dim_attr, miss=511, mask=mask)
    eng.synchronize()
    assert (res.n, res.c) == (len(fk), 9)
    assert (O.decompress(res.data.cpu().numpy(), res.n, 9).view(np.uint32) == sparse_want(dim, attr, sel, fk, 511)).all()
    # the search inside it ran against the sorted, filtered keys, its row count read on the device
    table, rowids, count = eng.sorted_keys(dim_keys, mask)
    idx = eng.index_of(fact, table, miss=len(dim), rows=count)
    (label, _, _, _), = record(L, eng)
    eng.synchronize()
    assert base_name(label) == want_family(len(dim)) and int(count.item()) == int(sel.sum())
    kept = np.sort(dim[sel], kind="stable")
    pos, found = expect(fk, kept, len(kept), LEFT)
    assert (O.decompress(idx.data.cpu().numpy(), idx.n, idx.c).view(np.uint32) == np.where(found, pos, len(dim))).all()
    # ... and without a filter
    res = eng.sparse_lookup(fact, dim_keys, dim_attr, miss=0)
    eng.synchronize()
    assert (O.decompress(res.data.cpu().numpy(), res.n, 9).view(np.uint32) == sparse_want(dim, attr, np.ones(len(dim), dtype=bool), fk, 0)).all()


@gpu
def test_bucketize_then_group_aggregate(L, O, eng):
    """a histogram with uneven bins: SELECT width_bucket(v, edges), sum(w), count(*), min(w), max(w) ... GROUP BY 1"""
    from shared_simd_scan_amd.engine import PackedColumn

    rng = np.random.default_rng(41)
    edges = np.sort(np.concatenate([[10, 250, 250], rng.integers(0, 1 << 12, 37)])).astype(np.uint32)
    v = rng.integers(0, 1 << 12, N_BIG, dtype=np.uint64).astype(np.uint32)
    w = rng.integers(0, 1 << 17, N_BIG, dtype=np.uint64).astype(np.uint32)
    bins = eng.bucketize(PackedColumn(plain_pack(O, v, 12), N_BIG, 12), PackedColumn(plain_pack(O, edges, 12), len(edges), 12))
    (label, _, _, _), = record(L, eng)
    assert base_name(label) == want_family(len(edges)) and (bins.n, bins.c) == (N_BIG, 6)
    agg = eng.group_aggregate(bins, PackedColumn(plain_pack(O, w, 17), N_BIG, 17))
    eng.synchronize()
    keys = np.searchsorted(edges.astype(np.uint64), v.astype(np.uint64), side="right")
    assert len(np.unique(keys)) >= 30 and (keys == 0).any() and (keys == len(edges)).any()
    assert (agg.cpu().numpy().view(np.uint64) == grouped(keys, w, 64)).all()


@gpu
def test_search_of_row_numbers_is_run_decode(L, O, eng):
    """search_sorted(arange, ends, right) -> lookup(values) is run_decode on the same runs: run_decode's j(i) is the special case
    where the probe is the row number"""
    from shared_simd_scan_amd.engine import PackedColumn

    rng = np.random.default_rng(43)
    n = N_BIG
    lengths = rng.integers(0, 40, 400)  # runs of length zero among them
    ends = np.minimum(np.cumsum(lengths), n - 100).astype(np.uint32)  # the last rows are behind every run
    values = rng.integers(0, 1 << 9, len(ends), dtype=np.uint64).astype(np.uint32)
    ce = width_for(n)
    ends_col, values_col = PackedColumn(plain_pack(O, ends, ce), len(ends), ce), PackedColumn(plain_pack(O, values, 9), len(values), 9)
    rows = PackedColumn(plain_pack(O, np.arange(n, dtype=np.uint32), ce), n, ce)
    pos, _, _ = eng.search_sorted(rows, ends_col, side="right")
    (label, _, _, _), = record(L, eng)
    assert base_name(label) == want_family(len(ends))
    via_search = eng.lookup(pos, values_col, miss=77)
    via_decode = eng.run_decode(values_col, ends_col, n, miss=77)
    eng.synchronize()
    j = np.searchsorted(ends.astype(np.uint64), np.arange(n, dtype=np.uint64), side="right")
    want = np.where(j < len(ends), values[np.minimum(j, len(ends) - 1)], 77).astype(np.uint32)
    assert (j == len(ends)).any() and (np.diff(ends.astype(np.int64)) == 0).any()
    nb = payload(n, 9)
    assert (via_search.data.cpu().numpy()[:nb] == O.pack(want, 9)[:nb]).all()
    assert (via_search.data.cpu().numpy()[:nb] == via_decode.data.cpu().numpy()[:nb]).all()


@gpu
def test_is_member_is_semi_join_on_a_dense_domain(L, O, eng):
    from shared_simd_scan_amd.engine import PackedColumn
    import torch

    rng = np.random.default_rng(47)
    members = rng.random(1 << 12) < 0.3
    fk = rng.integers(0, 1 << 12, N_BIG, dtype=np.uint64).astype(np.uint32)
    fact = PackedColumn(plain_pack(O, fk, 12), N_BIG, 12)
    table = np.nonzero(members)[0].astype(np.uint32)
    bitmap, hits = eng.is_member(fact, PackedColumn(plain_pack(O, table, 12), len(table), 12))
    (label, _, _, _), = record(L, eng)
    assert base_name(label) == want_family(len(table))
    semi_bitmap, semi_hits = eng.semi_join(fact, torch.from_numpy(packbits(members)).cuda(), 1 << 12)
    eng.synchronize()
    nb = (N_BIG + 7) // 8
    assert (bitmap.cpu().numpy()[:nb] == packbits(members[fk])).all() and int(hits.item()) == int(members[fk].sum())
    assert torch.equal(bitmap[:nb], semi_bitmap[:nb]) and int(hits.item()) == int(semi_hits.item())


@gpu
@pytest.mark.parametrize("case", CAPTURE_CASES, ids=pid)
def test_graph_capture_and_replay(O, case):
    """one search per graph, a linear chain on a side stream: column, table and *rows_dev are overwritten between the replays and
    every replay follows them.  No warm-up call of the test's own: the protocol's eager run is the first call the context sees."""
    import torch

    from shared_simd_scan_amd.engine import PackedColumn

    c, ct, rows = case
    n, co = N_BIG, width_for(rows)
    fam = want_family(rows)
    miss = miss_of(co)
    cols, tables, counts = capture_data(c, ct, rows)
    wants = [expect(cols[v], tables[v], counts[v], LEFT) for v in range(3)]

    def steps(eng):
        col_stage, table_stage = [plain_pack(O, x, c) for x in cols], [plain_pack(O, t, ct) for t in tables]
        col, table = PackedColumn(torch.empty_like(col_stage[0]), n, c), PackedColumn(torch.empty_like(table_stage[0]), rows, ct)
        rows_dev = torch.zeros(1, dtype=torch.int64, device="cuda")
        out, found, hits = Guarded(payload(n, co)), Guarded((n + 7) // 8), Guarded(8, back=64, front=64)
        view = lambda g, dtype=torch.uint8: g.t[g.front: g.front + g.nbytes].view(dtype)
        launched = []

        def load(r):
            col.data.copy_(col_stage[r])
            table.data.copy_(table_stage[r])
            rows_dev.fill_(counts[r])
            for g in (out, found, hits):
                g.t.fill_(SENTINEL)

        def run():
            eng.search_sorted(col, table, rows=rows_dev, exact=True, miss=miss, co=co, out=view(out), found=view(found), hits=view(hits, torch.int64))
            launched[:] = capture.last_record(eng)

        def check(r, what):
            pos, fnd = wants[r]
            assert (out.fetch() == O.pack(np.where(fnd, pos, miss).astype(np.uint32), co)[: out.nbytes]).all(), what
            assert (found.fetch() == packbits(fnd)).all(), what
            assert int(np.frombuffer(hits.fetch().tobytes(), dtype=np.uint64)[0]) == int(fnd.sum()), what

        def untouched():
            for g in (out, found, hits):
                assert (g.fetch() == SENTINEL).all()

        def warmed(_):
            assert [base_name(x[0]) for x in launched] == [fam]

        return capture.Steps(load, run, check, untouched, warmed)

    capture.capture_replay(steps, (0, 1, 2, 0))
