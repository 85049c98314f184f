"""A packed column mapped through a device-resident packed table (include/mi355_lookup.h, ScanEngine.lookup):
out[i] = table[v_i] if v_i < table_rows else miss, packed in and packed out.

CPU: the header is plain C99 and declares exactly what _capi.HEADERS binds for it and the library exports; it carries its
graph-capture verdict; mi355_lookup_kernel (pure arithmetic) names the tier at every boundary; lookup hands the C ABI what it
should (through a recording stand-in for the library); without a device the entry point fails with a message; every __global__
under csrc/lookup/ is named by the launch record of a GPU case of this file; no source there reads a switch bit; the data
recipe is not vacuous.

GPU (-m gpu): every expectation is numpy on the values and the table the test generated --
where(v < T, table[minimum(v, T - 1)], miss) -- packed with the oracle's packer; nothing is derived from engine output.  Every
one of the ceil(n ct / 8) payload bytes (trailing bits of the last one included) and the 0xEE guard bytes on both sides of the
output (support.Guarded) are compared exactly; column and table must be unchanged after the call.  Every case runs in
hostile surroundings: ones in the column's bits behind row n - 1 and in its pad, ones in the table's last-byte bits behind value
T - 1 and in its pad, ones in the table rows no value can reach (T > 2^c).  A tile is R = 2048 rows, so the sizes below are
the smallest that reach one lane, one partial tile, one full tile, a full tile plus one row and many tiles with a ragged tail.
"""
import ctypes as C
import functools
import os
import types

import numpy as np
import pytest

import capture
import support
from support import (E_INVALID, SENTINEL, Guarded, L, base_name, corner_rows, eng, fake, grouped, header_macro, hostile_pack, packbits, plain_pack,  # noqa: F401
                     record)  # (L, eng, fake: fixtures)

HEADER = "mi355_lookup.h"

# the kernels of csrc/lookup/, as the launch record names them: the GPU cases below assert these labels
LDS_KERNEL = "lookup_lds_kernel"
GLOBAL_KERNEL = "lookup_global_kernel"


LDS_MAX = header_macro(HEADER, "MI355_LOOKUP_LDS_MAX_BYTES")
R = 2048  # rows per tile: 64 lanes x 32 rows


def entry_bytes(ct):
    return 1 if ct <= 8 else (2 if ct <= 16 else 4)


def ceiling(ct):
    """the largest reachable table the LDS tier holds at output width ct: reach + 1 entries within LDS_MAX bytes"""
    return LDS_MAX // entry_bytes(ct) - 1


N_BIG = 9 * R + 1237  # 19669: nine tiles and a ragged one; not a multiple of 8
SIZES = [1, 13, R - 1, R, R + 1, N_BIG]
SIZE_CASES = [(9, 5, 512), (9, 12, 300), (17, 17, 100003), (32, 32, 5000)]  # (c, ct, T)
# every input width, every output width in the LDS tier, and every output width one row past its class's ceiling: every
# instantiation of both kernels runs
WIDTH_CASES = ([(c, 12, min(1 << c, 3001)) for c in range(1, 33)] + [(12, ct, 3001) for ct in range(1, 33)]
               + [(24, ct, ceiling(ct) + 1) for ct in range(1, 33)])
TABLE_CTS = (8, 16, 17)
TABLE_SIZE_CASES = ([(24, ct, T) for ct in TABLE_CTS for T in (0, 1, 2, 31, 32, 33, 509, ceiling(ct) - 1, ceiling(ct), ceiling(ct) + 1, (1 << 22) + 5)]
                    + [(5, ct, 1000) for ct in TABLE_CTS])
OFFSET_CASES = [(24, 17, 3001), (24, 7, 3002), (24, 17, ceiling(17) + 1), (24, 8, ceiling(8) + 3), (5, 12, 1000)]
VIEW_CASES = [(9, 12, 300), (12, 7, 3001), (24, 17, ceiling(17) + 1)]
N_VIEW = 2 * R + 504  # a multiple of 8 (the slice ends on a byte at any width), not of 32: the last lane is ragged
ERROR_CASE = (9, 12, 300, R + 77)
LONG_CASES = [(12, 8, 3001), (24, 8, ceiling(8) + 1), (24, 21, ceiling(21) + 1)]
N_LONG = 64 * R + 1237  # one block's four waves walk sixteen tiles each
CHAIN_T, CHAIN_N = 3001, N_BIG
CAPTURE_CASES = [(12, 6, 3001), (24, 6, ceiling(6) + 1)]  # one per tier; 6 bits: group_aggregate's keys

gpu = pytest.mark.gpu


def pid(p):
    return "-".join(str(x) for x in p)


def reach_of(c, T):
    """what a c-bit value can address of a T-row table"""
    return min(T, 1 << c)


def miss_of(ct):
    return 1 if ct == 1 else 0x5A5A5A5A & ((1 << ct) - 1)


def want_family(c, ct, T):
    return LDS_KERNEL if (reach_of(c, T) + 1) * entry_bytes(ct) <= LDS_MAX else GLOBAL_KERNEL


@functools.lru_cache(maxsize=None)
def table_of(c, ct, T):
    """the table's entries: uniform over [0, 2^ct), entry 0 = 2^ct - 1, entry reach - 1 = 0, the rows no c-bit value reaches all ones"""
    rng = np.random.default_rng([7, c, ct, T % (1 << 31), T >> 31])
    reach = reach_of(c, T)
    table = rng.integers(0, 1 << ct, T, dtype=np.uint64)
    if reach >= 1:
        table[0] = (1 << ct) - 1
    if reach >= 2:
        table[reach - 1] = 0
    table[reach:] = (1 << ct) - 1
    table = table.astype(np.uint32)
    table.setflags(write=False)
    return table


@functools.lru_cache(maxsize=None)
def values_of(c, T, n, salt=0):
    """half of the values uniform below reach, half uniform over [0, 2^c), then the corner values 0, reach - 1, min(T, 2^c - 1)
    and 2^c - 1 at corner_rows()"""
    rng = np.random.default_rng([c, T % (1 << 31), T >> 31, n, salt])
    top = (1 << c) - 1
    reach = reach_of(c, T)
    vals = rng.integers(0, top + 1, n, dtype=np.uint64)
    if reach:
        low = rng.random(n) < 0.5
        vals[low] = rng.integers(0, reach, int(low.sum()), dtype=np.uint64)
    corners = [0, max(reach - 1, 0), min(T, top), top]
    for rows in corner_rows(n):
        for r, v in zip(rows, corners):
            vals[r] = v
    vals = vals.astype(np.uint32)
    vals.setflags(write=False)
    return vals


def data(c, ct, T, n):
    return values_of(c, T, n), table_of(c, ct, T)


def expect(vals, table, T, miss):
    """the expectation, as the issue words it: where(v < T, table[minimum(v, T - 1)], miss)"""
    v = vals.astype(np.int64)
    if T == 0:
        return np.full(len(v), miss, dtype=np.uint32)
    return np.where(v < T, table[np.minimum(v, T - 1)], np.uint32(miss)).astype(np.uint32)


def payload(n, c):
    return (n * c + 7) // 8


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------

def test_lookup_header_is_plain_c99():
    support.check_header_is_plain_c99(HEADER)


def test_lookup_header_declares_what_python_binds(L):
    names, sigs = support.check_header_binds(L, HEADER)
    assert names == ["mi355_lookup_dev", "mi355_lookup_kernel"]
    sig = sigs["mi355_lookup_dev"]
    assert sig[2] is C.c_uint64 and sig[3] is C.c_uint and sig[5] is C.c_uint64 and sig[6] is C.c_uint and sig[7] is C.c_uint32 and len(sig) == 9
    assert sigs["mi355_lookup_kernel"] == [C.c_uint, C.c_uint64, C.c_uint] and L.mi355_lookup_kernel.restype is C.c_char_p


def test_lookup_header_carries_its_capture_verdict():
    support.check_capture_verdict(HEADER, r"read at every replay")


def test_header_limit_is_the_budget_it_describes(L):
    """160 KiB minus four waves' two 8 KiB input images and 64 bytes, in whole 16 bytes"""
    assert LDS_MAX == (160 * 1024 - 4 * 2 * 8192 - 64) // 16 * 16
    assert LDS_MAX >= 4 * ((1 << 12) + 1), "a 12-bit key column's whole table must fit at any output width"


def test_kernel_choice_at_the_boundaries(L):
    """mi355_lookup_kernel needs neither a device nor a context; the tier follows (min(table_rows, 2^c) + 1) entries of the width
    class against MI355_LOOKUP_LDS_MAX_BYTES"""
    from shared_simd_scan_amd import lookup_kernel

    k = L.mi355_lookup_kernel
    lds, glob_ = LDS_KERNEL.encode(), GLOBAL_KERNEL.encode()
    for ct, eb in ((1, 1), (8, 1), (9, 2), (16, 2), (17, 4), (32, 4)):
        assert entry_bytes(ct) == eb
        top = LDS_MAX // eb - 1  # reach + 1 entries exactly at the ceiling
        assert (top + 1) * eb <= LDS_MAX < (top + 2) * eb
        for c in (24, 32):
            assert [k(c, T, ct) for T in (0, 1, top - 1, top)] == [lds] * 4, (c, ct)
            assert k(c, top + 1, ct) == glob_ and k(c, 1 << 32, ct) == glob_, (c, ct)
            assert k(c, (1 << 32) + 1, ct) is None, (c, ct)
    # the class boundaries themselves: the same table changes tier between ct = 8 and 9, and between 16 and 17
    assert k(24, ceiling(8), 8) == lds and k(24, ceiling(8), 9) == glob_
    assert k(24, ceiling(16), 16) == lds and k(24, ceiling(16), 17) == glob_
    # a narrow column reaches only the first 2^c rows, however large the table is
    for c in (1, 5, 9, 12, 14):
        for ct in (1, 8, 16, 32):
            assert ((1 << c) + 1) * entry_bytes(ct) <= LDS_MAX and k(c, 1 << 32, ct) == lds and k(c, (1 << c) + 1, ct) == lds, (c, ct)
    assert k(16, 1 << 32, 8) == lds and k(17, 1 << 32, 8) == glob_ and k(17, ceiling(8), 8) == lds
    assert k(15, 1 << 32, 16) == lds and k(16, 1 << 32, 16) == glob_
    assert k(14, 1 << 32, 32) == lds and k(15, 1 << 32, 32) == glob_
    for T in (0, 1, 3001, 1 << 32):
        assert k(0, T, 8) is None and k(33, T, 8) is None and k(9, T, 0) is None and k(9, T, 33) is None, T
    assert lookup_kernel(12, 3001, 8) == LDS_KERNEL and lookup_kernel(24, ceiling(8) + 1, 8) == GLOBAL_KERNEL
    for bad in ((0, 5, 8), (33, 5, 8), (9, 5, 0), (9, 5, 33), (9, (1 << 32) + 1, 8), (9, -1, 8), (9, (1 << 64) + 3, 8)):
        with pytest.raises(ValueError):
            lookup_kernel(*bad)


def test_width_cases_reach_both_tiers(L):
    """(no device needed) what test_every_width runs launches both kernels at every output width, the LDS one at every input
    width too, and the arithmetic of this file is the library's"""
    fam = {case: L.mi355_lookup_kernel(case[0], case[2], case[1]).decode() for case in WIDTH_CASES}
    assert {ct for (c, ct, T), f in fam.items() if f == LDS_KERNEL} == set(range(1, 33))
    assert {ct for (c, ct, T), f in fam.items() if f == GLOBAL_KERNEL} == set(range(1, 33))
    assert {c for (c, ct, T), f in fam.items() if f == LDS_KERNEL} == set(range(1, 33))
    for case in WIDTH_CASES + TABLE_SIZE_CASES + SIZE_CASES + OFFSET_CASES + VIEW_CASES + LONG_CASES + CAPTURE_CASES:
        c, ct, T = case
        assert L.mi355_lookup_kernel(c, T, ct).decode() == want_family(c, ct, T), case


def test_lookup_wrapper_passes_what_the_abi_takes(fake, L):
    import torch

    eng, rec, col = fake
    fact, table = col(17, 777), col(12, 4001)
    out = torch.zeros(1166, dtype=torch.uint8)  # ceil(777 * 12 / 8): a slice of a longer column needs no more
    res = eng.lookup(fact, table, miss=77, out=out)
    (name, a), = rec.calls
    assert name == "mi355_lookup_dev" and res.data is out and (res.n, res.c) == (777, 12)
    assert a[1:] == [fact.data.data_ptr(), 777, 17, table.data.data_ptr(), 4001, 12, 77, out.data_ptr()]
    rec.calls.clear()
    res = eng.lookup(fact, table)  # defaults: miss 0, a fresh buffer that a consumer can take as a column
    (name, a), = rec.calls
    assert a[1:8] == [fact.data.data_ptr(), 777, 17, table.data.data_ptr(), 4001, 12, 0]
    assert res.data.dtype == torch.uint8 and res.data.numel() == L.mi355_compressed_buffer_size(12, 777) and a[8] == res.data.data_ptr()
    assert (res.n, res.c) == (777, 12)
    rec.calls.clear()
    eng.lookup(fact, col(9, 0), miss=5)  # the empty table needs no buffer
    assert rec.calls[0][1][4:8] == [None, 0, 9, 5]
    rec.calls.clear()
    huge = types.SimpleNamespace(data=types.SimpleNamespace(data_ptr=lambda: 1 << 20), n=1 << 32, c=32)  # 16 GiB, never touched
    eng.lookup(col(32, 5), huge, miss=(1 << 32) - 1)  # 2^32 rows and the largest miss do not wrap on the way
    assert rec.calls[0][1][4:8] == [1 << 20, 1 << 32, 32, (1 << 32) - 1]
    rec.calls.clear()
    for bad in (-1, 1 << 12, 1 << 40):
        with pytest.raises(ValueError):
            eng.lookup(fact, table, miss=bad)
    with pytest.raises(AssertionError):
        eng.lookup(fact, table, out=torch.zeros(1165, dtype=torch.uint8))  # shorter than the payload
    assert rec.calls == []


def test_lookup_entry_point_fails_loudly_without_a_gpu(L):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    buf = (C.c_uint8 * 1024)()
    tab = (C.c_uint8 * 1024)()
    out = (C.c_uint8 * 1024)()
    rc = L.mi355_lookup_dev(None, buf, 100, 9, tab, 300, 12, 0, out)
    assert rc != 0 and L.mi355_last_error()


def test_every_lookup_kernel_has_a_case():
    """every __global__ under csrc/lookup/ is asserted from the launch record by a GPU case of this file, and the file names no
    kernel that does not exist"""
    kernels = support.global_kernels_of("lookup")
    assert kernels == {LDS_KERNEL, GLOBAL_KERNEL}, kernels
    support.check_gpu_part_asserts(__file__, r"want_family\(")  # (not the constants: the GPU cases assert the predicted kernel)
    assert {want_family(*case) for case in WIDTH_CASES} == kernels


def test_lookup_sources_read_no_flag_bits():
    assert [os.path.basename(p) for p in support.feature_sources("lookup")] == ["lookup.hip", "lookup.hpp"]
    support.check_sources_read_no_flag_bits("lookup")


def gpu_shapes():
    """every (c, ct, T, n) the GPU tests below run on recipe data"""
    shapes = {(c, ct, T, n) for c, ct, T in SIZE_CASES for n in SIZES}
    shapes |= {(c, ct, T, N_BIG) for c, ct, T in WIDTH_CASES + TABLE_SIZE_CASES + OFFSET_CASES}
    shapes |= {(c, ct, T, N_VIEW) for c, ct, T in VIEW_CASES}
    shapes |= {(c, ct, T, N_LONG) for c, ct, T in LONG_CASES}
    shapes |= {ERROR_CASE}
    return sorted(shapes)


@pytest.mark.parametrize("shape", [s for s in gpu_shapes() if s[3] >= 13], ids=pid)
def test_recipe_is_not_vacuous(shape):
    """(no device needed) what every case must exercise; n = 1 holds one row and is left out (see below)"""
    c, ct, T, n = shape
    vals, table = data(c, ct, T, n)
    v = vals.astype(np.int64)
    reach, top, miss = reach_of(c, T), (1 << c) - 1, miss_of(ct)
    assert len(table) == T and miss < 1 << ct
    want = expect(vals, table, T, miss)
    hit = v < T
    if 0 < reach < 1 << c:
        assert hit.sum() * 10 >= n and (~hit).sum() * 10 >= n, "a tenth of the rows must hit and a tenth must miss"
        assert (v == T).any() and (want[v == T] == miss).all(), "a value equal to T must exist and miss"
    if reach:
        assert (table[:reach] != miss).any(), "miss must differ from a table entry"
        assert int(table[0]) == (1 << ct) - 1 and (reach < 2 or int(table[reach - 1]) == 0)
        assert (v == 0).any() and (v == reach - 1).any(), "no row addresses entry 0 / entry reach - 1"
        assert (want[v == 0] == table[0]).all() and (want[v == reach - 1] == table[reach - 1]).all()
        assert len(np.unique(want)) >= 2 or ct == 1 and reach == 1, "the expected column is constant"
    else:
        assert (want == miss).all()
    if T > 1 << c:
        assert (table[1 << c:] == (1 << ct) - 1).all() and reach == 1 << c
    # the corner values sit at fixed rows of the first tile, the last full tile and the ragged tail
    corners = [0, max(reach - 1, 0), min(T, top), top]
    groups = corner_rows(n)
    assert groups[0][0] == 0
    if n >= R:
        assert any(rows[-1] == n // R * R - 1 for rows in groups), "no corner rows in the last full tile"
    if n % R >= 4 and n > 4:
        assert groups[-1][-1] == n - 1 and groups[-1][0] >= n // R * R, "no corner rows in the ragged tail"
    for rows in groups:
        assert [int(v[r]) for r in rows] == corners[:len(rows)], rows


@pytest.mark.parametrize("shape", [s for s in gpu_shapes() if s[3] < 13], ids=pid)
def test_one_row_shapes_look_up_entry_zero(shape):
    """(no device needed) n = 1 holds one row, value 0: it cannot carry the properties above, but it addresses entry 0, which is
    all ones and differs from miss"""
    c, ct, T, n = shape
    assert n == 1 and T >= 1
    vals, table = data(c, ct, T, n)
    assert int(vals[0]) == 0 and int(expect(vals, table, T, miss_of(ct))[0]) == (1 << ct) - 1 != miss_of(ct)


@functools.lru_cache(maxsize=None)
def chain_data():
    """the star query's tables -> (dim kind uint32[T] at 5 bits, dim year at 6 bits, fact fk at 12 bits, amount at 17), read-only"""
    rng = np.random.default_rng(2025)
    kind = rng.integers(0, 32, CHAIN_T, dtype=np.uint64).astype(np.uint32)
    year = rng.integers(0, 64, CHAIN_T, dtype=np.uint64).astype(np.uint32)
    fk = rng.integers(0, 1 << 12, CHAIN_N, dtype=np.uint64).astype(np.uint32)
    amount = rng.integers(0, 1 << 17, CHAIN_N, dtype=np.uint64).astype(np.uint32)
    for a in (kind, year, fk, amount):
        a.setflags(write=False)
    return kind, year, fk, amount


def test_chain_data_is_not_vacuous():
    kind, year, fk, amount = chain_data()
    f = fk.astype(np.int64)
    assert (f >= CHAIN_T).any() and (f < CHAIN_T).any()
    by = expect(fk, year, CHAIN_T, 63)
    assert len(np.unique(by)) == 64 and (by[f >= CHAIN_T] == 63).all()
    sel = (f < CHAIN_T) & (kind[np.minimum(f, CHAIN_T - 1)] == 3)
    assert sel.any() and not sel.all() and len(np.unique(by[sel])) >= 2


@functools.lru_cache(maxsize=None)
def capture_data(c, ct, T):
    """the capture test's tables -> (fact fk uint32[N_BIG] at c bits, amount at 17 bits, two versions of the T-row table)"""
    rng = np.random.default_rng([c, ct, 99])
    fk = rng.integers(0, min(1 << c, T + T // 8 + 8), N_BIG, dtype=np.uint64).astype(np.uint32)
    fk[:4] = [0, T - 1, T, min(T + 1, (1 << c) - 1)]
    amount = rng.integers(0, 1 << 17, N_BIG, dtype=np.uint64).astype(np.uint32)
    tables = []
    for r in range(2):
        t = np.random.default_rng([c, ct, 100 + r]).integers(0, 1 << ct, T, dtype=np.uint64).astype(np.uint32)
        t[0] = 3 if r == 0 else 4
        t.setflags(write=False)
        tables.append(t)
    for a in (fk, amount):
        a.setflags(write=False)
    return fk, amount, tables


@pytest.mark.parametrize("case", CAPTURE_CASES, ids=pid)
def test_capture_data_is_not_vacuous(case):
    c, ct, T = case
    fk, amount, tables = capture_data(c, ct, T)
    f = fk.astype(np.int64)
    assert (f >= T).any() and (f == T).any() and (f == T - 1).any() and (f == 0).any()
    wants = [grouped(expect(fk, t, T, miss_of(ct)), amount, 1 << ct) for t in tables]
    assert (wants[0] != wants[1]).any(), "a stale result could pass"
    assert tables[0][0] != tables[1][0], "row 0 (key 0) changes group between the versions"


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

class Look:
    """one engine, an uploaded column and table (both in hostile surroundings), a guarded output refilled with 0xEE before every call"""

    def __init__(self, O, eng, c, ct, T, n, vals=None, table=None, table_offset=0):
        from shared_simd_scan_amd.engine import PackedColumn

        self.O, self.eng, self.c, self.ct, self.T, self.n = O, eng, c, ct, T, n
        if vals is None:
            vals, table = data(c, ct, T, n)
        self.vals, self.table_vals, self.miss = vals, table, miss_of(ct)
        self.col = PackedColumn(hostile_pack(O, vals, c), n, c)
        self.table = PackedColumn(hostile_pack(O, table, ct, table_offset), T, ct)
        self.nbytes = payload(n, ct)
        self.out = Guarded(self.nbytes)

    def out_view(self):
        return self.out.t[self.out.front: self.out.front + self.nbytes]

    def run(self, L, what=""):
        """-> checks every payload byte, the trailing bits, the guards, the inputs and the launch record; returns the record"""
        import torch

        tag = (what, self.c, self.ct, self.T, self.n)
        want = expect(self.vals, self.table_vals, self.T, self.miss)
        wb = self.O.pack(want, self.ct)[: self.nbytes]
        self.out.t.fill_(SENTINEL)
        col_before, table_before = self.col.data.clone(), self.table.data.clone()
        res = self.eng.lookup(self.col, self.table, miss=self.miss, out=self.out_view())
        self.eng.synchronize()
        have = self.out.fetch()  # asserts the guard bytes on both sides
        assert res.data.data_ptr() == self.out_view().data_ptr() and (res.n, res.c) == (self.n, self.ct)
        bad = np.nonzero(have != wb)[0]
        assert bad.size == 0, (tag, "byte", int(bad[0]), "of", self.nbytes, "have", int(have[bad[0]]), "want", int(wb[bad[0]]))
        if (self.n * self.ct) % 8:
            assert int(have[-1]) >> ((self.n * self.ct) % 8) == 0, (tag, "bits behind the last value are not zero")
        assert torch.equal(self.col.data, col_before), (tag, "column written")
        assert torch.equal(self.table.data, table_before), (tag, "table written")
        rec = record(L, self.eng)
        (label, grid, lds, flags), = rec
        fam = want_family(self.c, self.ct, self.T)
        assert base_name(label) == fam == L.mi355_lookup_kernel(self.c, self.T, self.ct).decode() and label.startswith(f"{fam}<{self.ct}>"), (tag, label)
        assert flags == 0 and lds >= 4 * 2 * 256 * self.c + (fam == LDS_KERNEL) * (reach_of(self.c, self.T) + 1) * entry_bytes(self.ct), (tag, lds)
        return rec


@gpu
@pytest.mark.parametrize("case", SIZE_CASES, ids=pid)
def test_sizes_and_tails(L, O, eng, case):
    c, ct, T = case
    for n in SIZES:
        Look(O, eng, c, ct, T, n).run(L)


@gpu
@pytest.mark.parametrize("case", WIDTH_CASES, ids=pid)
def test_every_width(L, O, eng, case):
    c, ct, T = case
    Look(O, eng, c, ct, T, N_BIG).run(L)


@gpu
@pytest.mark.parametrize("case", TABLE_SIZE_CASES, ids=pid)
def test_table_sizes(L, O, eng, case):
    c, ct, T = case
    look = Look(O, eng, c, ct, T, N_BIG)
    (label, grid, lds, flags), = look.run(L)
    # the tier switches between ceiling and ceiling + 1 reachable rows, and nowhere else
    if T in (ceiling(ct) - 1, ceiling(ct)):
        assert base_name(label) == LDS_KERNEL and lds >= (T + 1) * entry_bytes(ct)
    if T == ceiling(ct) + 1:
        assert base_name(label) == GLOBAL_KERNEL and lds <= 4 * 2 * 8192 + 16
    if T > 1 << c:
        assert base_name(label) == LDS_KERNEL and (look.table_vals[1 << c:] == (1 << ct) - 1).all()


@gpu
@pytest.mark.parametrize("with_buffer", [False, True], ids=["null", "buffer"])
def test_empty_table(L, O, eng, with_buffer):
    """table_rows == 0: every row gets miss, with no table pointer at all or with one whose bytes are all ones"""
    import torch

    from shared_simd_scan_amd import lib

    c, ct, n = 24, 17, N_BIG
    look = Look(O, eng, c, ct, 0, n)
    if not with_buffer:
        look.run(L, what="empty")  # ScanEngine.lookup hands a NULL table to the ABI when table.n == 0
        return
    junk = torch.full((64,), 0xFF, dtype=torch.uint8, device="cuda")
    look.out.t.fill_(SENTINEL)
    rc = lib().mi355_lookup_dev(eng._ctx, look.col.data.data_ptr(), n, c, junk.data_ptr(), 0, ct, look.miss, look.out.ptr)
    eng.synchronize()
    assert rc == 0 and base_name(record(L, eng)[0][0]) == LDS_KERNEL
    assert (look.out.fetch() == O.pack(np.full(n, look.miss, dtype=np.uint32), ct)[: look.nbytes]).all() and (junk == 0xFF).all()


@gpu
@pytest.mark.parametrize("case", OFFSET_CASES, ids=pid)
def test_table_at_four_byte_offsets(L, O, eng, case):
    """the table is a view at a 4-byte-aligned, not 16-byte-aligned offset inside a buffer of 0xff: nothing around it reaches a
    result (a value equal to T gets miss)"""
    c, ct, T = case
    for offset in (4, 12, 8):
        look = Look(O, eng, c, ct, T, N_BIG, table_offset=offset)
        assert look.table.data.data_ptr() % 16 == offset
        look.run(L, what=f"table at +{offset}")


@gpu
@pytest.mark.parametrize("case", VIEW_CASES, ids=pid)
def test_row_range_views(L, O, eng, case):
    """rows [lead, lead + n) of a longer column looked up into rows [lead_out, lead_out + n) of a longer output column: exactly the
    slice's bytes change, and nothing of the foreign rows reaches them"""
    import torch

    from shared_simd_scan_amd.engine import PackedColumn

    c, ct, T = case
    n, lead, trail, lead_out = N_VIEW, 2 * R + 128, 4096, 384
    assert n % 8 == 0 and n % 32 and lead % 128 == 0 and lead_out % 128 == 0
    vals, table = data(c, ct, T, n)
    rng = np.random.default_rng([c, ct, 13])
    top = (1 << c) - 1
    junk = rng.integers(0, top + 1, lead, dtype=np.uint64).astype(np.uint32)
    whole = PackedColumn(plain_pack(O, np.concatenate([junk, vals, np.full(trail, top, dtype=np.uint32)]), c), lead + n + trail, c)
    col = eng.slice_rows(whole, lead, lead + n)
    assert col.n == n and col.data.data_ptr() % 16 == 0
    n_out = lead_out + n + 1000
    before = rng.integers(0, 1 << ct, n_out, dtype=np.uint64).astype(np.uint32)
    out_whole = PackedColumn(plain_pack(O, before, ct), n_out, ct)
    out_bytes_before = out_whole.data.cpu().numpy().copy()
    out_slice = eng.slice_rows(out_whole, lead_out, lead_out + n)
    tab = PackedColumn(hostile_pack(O, table, ct), T, ct)
    miss = miss_of(ct)
    res = eng.lookup(col, tab, miss=miss, out=out_slice.data)
    eng.synchronize()
    (label, _, _, _), = record(L, eng)
    assert base_name(label) == want_family(c, ct, T) and res.data.data_ptr() == out_slice.data.data_ptr()
    after = before.copy()
    after[lead_out: lead_out + n] = expect(vals, table, T, miss)
    want_bytes = O.pack(after, ct)
    have = out_whole.data.cpu().numpy()
    first, last = lead_out * ct // 8, (lead_out + n) * ct // 8
    assert (have[:first] == out_bytes_before[:first]).all(), "rows in front of the slice changed"
    assert (have[last:] == out_bytes_before[last:]).all(), "rows behind the slice changed"
    assert (have == want_bytes).all()
    assert (O.decompress(have, n_out, ct).view(np.uint32) == after).all()


@gpu
def test_errors_launch_nothing(L, O, eng):
    c, ct, T, n = ERROR_CASE
    look = Look(O, eng, c, ct, T, n)
    big = Guarded(8192)  # a buffer that can stand for an input and the output at once
    cp, tp, op = look.col.data.data_ptr(), look.table.data.data_ptr(), look.out.ptr.value
    miss = look.miss

    def call(cp=cp, n=n, c=c, tp=tp, T=T, ct=ct, miss=miss, op=op):
        for g in (look.out, big):
            g.t.fill_(SENTINEL)
        rc = L.mi355_lookup_dev(eng._ctx, cp, n, c, tp, T, ct, miss, op)
        eng.synchronize()
        return rc

    assert call() == 0 and base_name(record(L, eng)[0][0]) == LDS_KERNEL
    valid = record(L, eng)
    nb_out, nb_col = payload(n, ct), payload(n, c)
    assert nb_out + 512 <= 8192 and nb_col + 512 <= 8192
    errors = (("c = 0", dict(c=0), b"32"), ("c = 33", dict(c=33), b"32"), ("ct = 0", dict(ct=0), b"ct"), ("ct = 33", dict(ct=33), b"ct"),
              ("table_rows = 2^32 + 1", dict(T=(1 << 32) + 1), b"2^32"), ("miss = 2^ct", dict(miss=1 << ct), b"miss"),
              ("miss = 2^32 - 1", dict(miss=(1 << 32) - 1), b"miss"),
              ("null column", dict(cp=None), b"packed_dev"), ("null table", dict(tp=None), b"table_dev"), ("null output", dict(op=None), b"out_dev"),
              ("column at +4", dict(cp=cp + 4), b"aligned"), ("table at +2", dict(tp=tp + 2), b"aligned"), ("output at +4", dict(op=op + 4), b"aligned"),
              ("output is the column", dict(cp=big.ptr.value, op=big.ptr.value), b"overlaps packed_dev"),
              ("output starts in the column's last byte", dict(cp=big.ptr.value, op=big.ptr.value + (nb_col - 1) // 16 * 16), b"overlaps packed_dev"),
              ("column starts inside the output", dict(cp=big.ptr.value + 256, op=big.ptr.value), b"overlaps packed_dev"),
              ("output is the table", dict(tp=big.ptr.value, op=big.ptr.value), b"overlaps table_dev"),
              ("table starts inside the output", dict(tp=big.ptr.value + 64, op=big.ptr.value), b"overlaps table_dev"),
              ("output starts in the table's last bytes", dict(tp=big.ptr.value, T=2048, op=big.ptr.value + 2048 * ct // 8 - 16), b"overlaps table_dev"))
    for what, kw, word in errors:
        assert call(**kw) == E_INVALID, what
        assert word in L.mi355_last_error(), (what, L.mi355_last_error())
        assert record(L, eng) == [], what  # a refused call leaves an empty record and launches nothing
        for g in (look.out, big):
            assert (g.fetch() == SENTINEL).all(), what
    # neighbours that do not overlap are fine: the output begins where the table's bytes end
    import torch

    tb = payload(T, ct)
    at = (tb + 15) // 16 * 16
    big.t.fill_(SENTINEL)
    big.t[big.front: big.front + tb] = torch.from_numpy(O.pack(look.table_vals, ct)[:tb].copy()).cuda()
    rc = L.mi355_lookup_dev(eng._ctx, cp, n, c, big.ptr.value, T, ct, miss, big.ptr.value + at)
    eng.synchronize()
    assert rc == 0 and record(L, eng) == valid
    got = big.fetch()
    assert (got[at: at + nb_out] == O.pack(expect(look.vals, look.table_vals, T, miss), ct)[:nb_out]).all()
    assert (got[tb: at] == SENTINEL).all() and (got[at + nb_out:] == SENTINEL).all()
    # n == 0: nothing launched, nothing written, and no column needed
    assert call(n=0, cp=None) == 0 and record(L, eng) == []
    assert (look.out.fetch() == SENTINEL).all()


@gpu
@pytest.mark.parametrize("case", LONG_CASES, ids=pid)
def test_one_block_walks_many_tiles(L, O, eng, case):
    """grid_cus = 1, max_blocks_per_cu = 1: one block, its four waves walk sixteen tiles each -- the alternating images, the
    deferred stores, the ragged tail"""
    c, ct, T = case
    look = Look(O, eng, c, ct, T, N_LONG)
    eng.set_option("grid_cus", 1)
    eng.set_option("max_blocks_per_cu", 1)
    try:
        (label, grid, lds, flags), = look.run(L, what="one block")
        assert grid == 1 and base_name(label) == want_family(c, ct, T)
    finally:
        eng.set_option("grid_cus", 0)
        eng.set_option("max_blocks_per_cu", 0)
    (label, grid, lds, flags), = look.run(L, what="whole chip")
    assert grid > 1


@gpu
def test_lookup_then_group_aggregate(L, O, eng):
    """SELECT d.year, sum(f.amount), count(*), min, max FROM fact f JOIN dim d ON f.fk = d.pk GROUP BY d.year"""
    from shared_simd_scan_amd.engine import PackedColumn

    kind, year, fk, amount = chain_data()
    fact_fk = PackedColumn(plain_pack(O, fk, 12), CHAIN_N, 12)
    by_year = eng.lookup(fact_fk, PackedColumn(plain_pack(O, year, 6), CHAIN_T, 6), miss=63)
    (label, _, _, _), = record(L, eng)
    assert base_name(label) == want_family(12, 6, CHAIN_T) == LDS_KERNEL and (by_year.n, by_year.c) == (CHAIN_N, 6)
    agg = eng.group_aggregate(by_year, PackedColumn(plain_pack(O, amount, 17), CHAIN_N, 17))
    eng.synchronize()
    assert (agg.cpu().numpy().view(np.uint64) == grouped(expect(fk, year, CHAIN_T, 63), amount, 64)).all()


@gpu
@pytest.mark.parametrize("op", ["==", "<", ">="])
def test_lookup_then_scan_where(L, O, eng, op):
    """a predicate on a dimension attribute, evaluated per fact row: table[fk] OP a"""
    from shared_simd_scan_amd.engine import PackedColumn

    kind, year, fk, amount = chain_data()
    fact_fk = PackedColumn(plain_pack(O, fk, 12), CHAIN_N, 12)
    by_kind = eng.lookup(fact_fk, PackedColumn(plain_pack(O, kind, 5), CHAIN_T, 5), miss=31)
    bitmap, hits = eng.scan_where(op, 17, by_kind)
    eng.synchronize()
    attr = expect(fk, kind, CHAIN_T, 31).astype(np.int64)
    want = {"==": attr == 17, "<": attr < 17, ">=": attr >= 17}[op]
    assert want.any() and not want.all()
    assert (bitmap.cpu().numpy()[: (CHAIN_N + 7) // 8] == packbits(want)).all() and int(hits.item()) == int(want.sum())


@gpu
def test_whole_star_query(L, O, eng):
    """SELECT d.year, sum(f.amount), ... FROM fact f JOIN dim d ON f.fk = d.pk WHERE d.kind = 3 GROUP BY d.year:
    scan_where(dim) -> semi_join -> lookup -> group_aggregate(mask), no host round trip"""
    from shared_simd_scan_amd.engine import PackedColumn

    kind, year, fk, amount = chain_data()
    T, n = CHAIN_T, CHAIN_N
    dim_kind, dim_year = PackedColumn(plain_pack(O, kind, 5), T, 5), PackedColumn(plain_pack(O, year, 6), T, 6)
    fact_fk, fact_amount = PackedColumn(plain_pack(O, fk, 12), n, 12), PackedColumn(plain_pack(O, amount, 17), n, 17)
    dim_bitmap, _ = eng.scan_where("==", 3, dim_kind)
    bitmap, hits = eng.semi_join(fact_fk, dim_bitmap, T)
    by_year = eng.lookup(fact_fk, dim_year, miss=63)
    (label, _, _, _), = record(L, eng)
    assert base_name(label) == want_family(12, 6, T)
    agg = eng.group_aggregate(by_year, fact_amount, mask=bitmap)
    eng.synchronize()
    f = fk.astype(np.int64)
    sel = (f < T) & (kind[np.minimum(f, T - 1)] == 3)
    assert int(hits.item()) == int(sel.sum())
    assert (agg.cpu().numpy().view(np.uint64) == grouped(expect(fk, year, T, 63), amount, 64, sel)).all()


@gpu
@pytest.mark.parametrize("case", CAPTURE_CASES, ids=pid)
def test_graph_capture_and_replay(O, case):
    """lookup + group_aggregate in one graph, a linear chain on a side stream: after the table's contents change the replay
    follows the new table"""
    import torch

    from shared_simd_scan_amd.engine import PackedColumn

    c, ct, T = case
    n = N_BIG
    fam = want_family(c, ct, T)
    miss = miss_of(ct)
    fk, amount, tables = capture_data(c, ct, T)
    wants = [grouped(expect(fk, t, T, miss), amount, 1 << ct) for t in tables]

    def steps(eng):
        stage = [plain_pack(O, t, ct) for t in tables]
        table = PackedColumn(torch.empty_like(stage[0]), T, ct)
        fact, values = PackedColumn(plain_pack(O, fk, c), n, c), PackedColumn(plain_pack(O, amount, 17), n, 17)
        keys = Guarded(payload(n, ct), back=4096)  # the looked-up column; the guard behind stands for the column's pad
        keys_view = keys.t[keys.front: keys.front + keys.nbytes]
        agg = torch.empty((1 << ct, 4), dtype=torch.int64, device="cuda")
        launched = []

        def load(r):
            table.data.copy_(stage[r])
            keys.t.fill_(SENTINEL)
            agg.fill_(-7)

        def run():
            by = eng.lookup(fact, table, miss=miss, out=keys_view)
            launched[:] = capture.last_record(eng)  # the lookup's: the chain's last call is the aggregate
            eng.group_aggregate(by, values, out=agg)

        def check(r, what):
            assert (keys.fetch() == O.pack(expect(fk, tables[r], T, miss), ct)[: keys.nbytes]).all(), what
            assert (agg.cpu().numpy().view(np.uint64) == wants[r]).all(), what

        def untouched():
            assert (keys.fetch() == SENTINEL).all() and (agg == -7).all()

        def warmed(_):
            assert [base_name(x[0]) for x in launched] == [fam]

        return capture.Steps(load, run, check, untouched, warmed)

    capture.capture_replay(steps, (0, 1, 0))
