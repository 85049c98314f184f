"""The row ids of a packed column in value order (include/mi355_sort.h, ScanEngine.sort_rows).

CPU: the header is plain C99 and declares exactly what _capi.HEADERS binds for it and the library exports; it carries its
graph-capture verdict; mi355_sort_rows_passes (pure arithmetic) is 1 / 2 / 3 / 4 by width; mi355_sort_rows_workspace_words is
monotone in the capacity and needs no item buffer at one-pass widths; sort_rows hands the C ABI what it should (through a
recording stand-in for the library); without a device the entry point fails with a message; every __global__ under csrc/sort/
is named by the launch record of a GPU case of this file; no source there reads a switch bit; the data recipes are not vacuous.

GPU (-m gpu): every expectation is numpy on the values and the mask the test generated -- np.lexsort((row id, key)) over the
qualifying rows, key = ~v for a descending sort; nothing is derived from engine output.  Every one of the q row ids, the q values
where asked, the count word and the 0xEE guard bytes on both sides of each output (the guard behind begins at entry q) are
compared exactly; column and mask must be unchanged after the call.  Every case runs in hostile surroundings: ones in the
column's bits behind row n - 1 and in its pad, 0xFF bytes directly behind byte ceil(n / 8) of the mask.  A span is S = 16384
rows (one wave's work at a time), a scan group 1024 counters; a digit is 8 bits, so widths 8 | 9, 16 | 17 and 24 | 25 are the
two sides of a digit boundary.  A scatter ranks a tile of 2048 rows inside an LDS stage from 1024 qualifying rows and 16 buckets
on, and writes the rows straight to their places below: both sides of both thresholds have their cases.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import capture
import support
from support import E_INVALID, SENTINEL, Guarded, L, base_name, eng, fake, hostile_bitmap, hostile_pack, packbits, plain_pack, record  # noqa: F401  (L, eng, fake: fixtures)

HEADER = "mi355_sort.h"

# the kernels of csrc/sort/, as the launch record names them: the GPU cases below assert these labels
COUNT_KERNEL = "sort_count_kernel"
SCATTER_KERNEL = "sort_scatter_kernel"
ITEM_COUNT_KERNEL = "sort_item_count_kernel"
ITEM_SCATTER_KERNEL = "sort_item_scatter_kernel"
OFFSETS_KERNEL = "sort_offsets_kernel"
SCAN_KERNEL = "rowid_scan_kernel"  # kernels/bitmap.hpp, launched between a count and sort_offsets_kernel

S = 16384  # rows per span
GROUP = 1024  # counters per scan group
DIGIT = 8

N_PAT = 5 * S + 77
N_LONG = 40 * S + 1237
N_GROUPS = 6 * S + 3
SIZES = [1, 63, 64, 65, 2047, 2048, 2049, S - 1, S, S + 1, 3 * S + 5]
SIZE_WIDTHS = [1, 8, 9, 16, 17, 24, 25, 32]
PATTERN_WIDTHS = [2, 9, 17, 32]
PATTERNS = ["all-equal", "two-values", "ascending", "descending", "lowest-digit", "top-digit", "extremes"]
MASKS = ["none", "random-1/2", "random-1/64", "empty", "first", "last"]
MASK_WIDTHS = [9, 25]
LONG_WIDTHS = [9, 24]
CAPTURE_WIDTHS = [9, 17]
GUARD64 = int.from_bytes(bytes([SENTINEL]) * 8, "little")
GUARD32 = int.from_bytes(bytes([SENTINEL]) * 4, "little")

gpu = pytest.mark.gpu


def passes(c):
    return (c + DIGIT - 1) // DIGIT


def want_record(c, writes=True):
    """the kernels of a call at width c, in launch order; writes = False: capacity 0, the call only counts"""
    names = [COUNT_KERNEL, SCAN_KERNEL, OFFSETS_KERNEL]
    if writes:
        names += [SCATTER_KERNEL] + [ITEM_COUNT_KERNEL, SCAN_KERNEL, OFFSETS_KERNEL, ITEM_SCATTER_KERNEL] * (passes(c) - 1)
    return names


# values_of and mask_of differ from test_compact's and test_top_k's in the seeds ([.., 17] and [.., 19] here), mask_of also in the kinds it knows:
# the "not vacuous" tests pin each file's data
@functools.lru_cache(maxsize=None)
def values_of(c, n, salt=0):
    rng = np.random.default_rng([c, n, salt, 17])
    vals = rng.integers(0, 1 << c, n, dtype=np.uint64).astype(np.uint32)
    vals.setflags(write=False)
    return vals


@functools.lru_cache(maxsize=None)
def mask_of(kind, n, salt=0):
    """the qualifying rows as a bool array of n rows; None = no mask at all"""
    if kind == "none":
        return None
    rng = np.random.default_rng([n, salt, len(kind), 19])
    bits = np.zeros(n, dtype=bool)
    if kind.startswith("random-"):
        num, _, den = kind[7:].partition("/")
        bits = rng.random(n) < float(num) / float(den)
    elif kind == "first":
        bits[0] = True
    elif kind == "last":
        bits[n - 1] = True
    else:
        assert kind == "empty", kind
    bits.setflags(write=False)
    return bits


def expect(vals, descending, qual=None):
    """-> (the qualifying rows in the call's order, their values): numpy's lexsort by (key, row id)"""
    n = len(vals)
    rows = np.arange(n, dtype=np.int64) if qual is None else np.nonzero(qual)[0].astype(np.int64)
    v = vals[rows]
    key = ~v if descending else v  # the complement of an unsigned value reverses the order
    order = np.lexsort((rows, key))
    return rows[order], v[order]


@functools.lru_cache(maxsize=None)
def pattern(name, c):
    """the values of a pattern at n = N_PAT, or None where the pattern needs more digits than c has"""
    n, top = N_PAT, (1 << c) - 1
    rng = np.random.default_rng([c, len(name), 5])
    low = DIGIT * (passes(c) - 1)  # where the top digit begins
    if name == "all-equal":
        vals = np.full(n, top // 3, dtype=np.uint32)
    elif name == "two-values":
        vals = np.where(rng.random(n) < 0.3, top // 5 + max(1, top // 2), top // 5).astype(np.uint32)
    elif name == "ascending":
        vals = (np.arange(n, dtype=np.uint64) * (top + 1) // n).astype(np.uint32)
    elif name == "descending":
        vals = (np.arange(n, dtype=np.uint64)[::-1] * (top + 1) // n).astype(np.uint32)
    elif name == "lowest-digit":  # every value shares what lies above its lowest digit
        if passes(c) < 2:
            return None
        vals = ((top >> DIGIT) // 3 << DIGIT | rng.integers(0, 1 << DIGIT, n, dtype=np.uint64)).astype(np.uint32)
    elif name == "top-digit":  # every value shares what lies below its top digit
        if passes(c) < 2:
            return None
        vals = (rng.integers(0, 1 << (c - low), n, dtype=np.uint64) << low | (0x5A5A5A & ((1 << low) - 1))).astype(np.uint32)
    else:
        assert name == "extremes", name
        vals = np.where(rng.random(n) < 0.4, top, 0).astype(np.uint32)
    vals.setflags(write=False)
    return vals


PATTERN_CASES = [(c, name) for c in PATTERN_WIDTHS for name in PATTERNS if pattern(name, c) is not None]


@functools.lru_cache(maxsize=None)
def capture_data(c):
    """two versions of a column and of a mask over N_PAT rows"""
    return [(values_of(c, N_PAT, salt=50 + r), mask_of("random-1/2", N_PAT, salt=60 + r)) for r in range(2)]


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------

def test_sort_rows_header_is_plain_c99():
    support.check_header_is_plain_c99(HEADER)


def test_sort_rows_header_declares_what_python_binds(L):
    from shared_simd_scan_amd import _capi

    names, sigs = support.check_header_binds(L, HEADER)
    assert names == ["mi355_sort_rows_dev", "mi355_sort_rows_passes", "mi355_sort_rows_workspace_words"]
    sig = sigs["mi355_sort_rows_dev"]
    assert len(sig) == 11 and sig[2] is C.c_uint64 and sig[3] is C.c_uint and sig[5] is C.c_int and sig[6] is C.c_uint64 and sig[9] is C.c_uint64
    assert sigs["mi355_sort_rows_passes"] == [C.c_uint] and L.mi355_sort_rows_passes.restype is C.c_uint
    assert sigs["mi355_sort_rows_workspace_words"] == [C.c_uint64, C.c_uint64, C.c_uint] and L.mi355_sort_rows_workspace_words.restype is C.c_uint64
    text = support.header_text(HEADER)
    assert '#include "mi355_scan.h"' in text and text.count("#include") == 1
    assert list(_capi.HEADERS)[-1] == HEADER
    assert f"spans of {S} rows" in text, "the header names the span"


def test_sort_rows_header_carries_its_capture_verdict():
    support.check_capture_verdict(HEADER, r"capturable after a warm-up call", r"read at every replay")


def test_sort_rows_passes_by_width(L):
    """mi355_sort_rows_passes needs neither a device nor a context"""
    from shared_simd_scan_amd import sort_rows_passes

    for c in range(1, 33):
        assert L.mi355_sort_rows_passes(c) == sort_rows_passes(c) == passes(c), c
    assert [L.mi355_sort_rows_passes(c) for c in (8, 9, 16, 17, 24, 25)] == [1, 2, 2, 3, 3, 4]
    assert L.mi355_sort_rows_passes(0) == 0 and L.mi355_sort_rows_passes(33) == 0
    for bad in (0, 33, -1, 1 << 32):
        with pytest.raises(ValueError):
            sort_rows_passes(bad)


def test_sort_rows_workspace_words(L):
    """pure arithmetic: monotone in the capacity, sized by it and not by n beyond the counters, no item buffer at one-pass widths"""
    W = L.mi355_sort_rows_workspace_words
    n = 10**9
    for c in (1, 5, 8):
        assert W(n, 0, c) == W(n, 10**6, c) == W(n, n, c) > 0, c
    for c in (9, 16, 17, 24, 25, 32):
        buffers = min(passes(c) - 1, 2)
        caps = [0, 1, 1000, 10**6, n, n + 5, 1 << 63]
        words = [W(n, cap, c) for cap in caps]
        assert words == sorted(words) and words[-1] == words[-2] == words[-3], (c, words)  # a capacity beyond n asks for n
        assert W(n, 10**6, c) - W(n, 0, c) == buffers * 10**6, c
        assert W(n, 10**6, c) * 8 < 200 << 20, "the survivors of a 1e9-row top_k must not take gigabytes"
    assert W(0, 5, 9) == 0 and W(100, 5, 0) == 0 and W(100, 5, 33) == 0 and W((1 << 32) + 1, 5, 9) == 0
    assert W(1 << 32, 5, 9) > 0


def test_sort_rows_wrapper_passes_what_the_abi_takes(fake):
    import torch

    eng, rec, col = fake
    fact = col(17, 777)
    rowids, count = eng.sort_rows(fact)  # defaults: ascending, no mask, capacity = n, no values
    (name, a), = rec.calls
    assert name == "mi355_sort_rows_dev" and a[1:7] == [fact.data.data_ptr(), 777, 17, None, 0, 0]
    assert rowids.dtype == torch.int64 and rowids.numel() == 777 and a[7] == rowids.data_ptr() and a[8] is None and a[9] == 777
    assert count.dtype == torch.int64 and count.numel() == 1 and a[10] == count.data_ptr()
    rec.calls.clear()
    mask = torch.zeros(98, dtype=torch.uint8)
    rowids, count, values = eng.sort_rows(fact, descending=True, mask=mask, capacity=50, first_row=(1 << 40) + 3, with_values=True)
    (name, a), = rec.calls
    assert a[1:7] == [fact.data.data_ptr(), 777, 17, mask.data_ptr(), 1, (1 << 40) + 3] and a[9] == 50
    assert rowids.numel() == 50 and values.numel() == 50 and values.dtype == torch.int32 and a[7] == rowids.data_ptr() and a[8] == values.data_ptr()
    rec.calls.clear()
    rowids, count, values = eng.sort_rows(fact, capacity=0, with_values=True)  # only the count: no output pointer
    assert rec.calls[0][1][7:10] == [None, None, 0] and rowids.numel() == 0 and values.numel() == 0
    rec.calls.clear()
    eng.sort_rows(col(9, 0), mask=mask)  # an empty column: no pointer but the count's
    assert rec.calls[0][1][1:5] == [None, 0, 9, None] and rec.calls[0][1][7] is None
    rec.calls.clear()
    for bad in (dict(capacity=-1), dict(capacity=1 << 64), dict(first_row=-1), dict(first_row=1 << 64)):
        with pytest.raises(ValueError):
            eng.sort_rows(fact, **bad)
    with pytest.raises(AssertionError):
        eng.sort_rows(fact, mask=torch.zeros(97, dtype=torch.uint8))  # a mask shorter than the column
    assert rec.calls == []


def test_sort_rows_entry_point_fails_loudly_without_a_gpu(L):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    buf = (C.c_uint8 * 1024)()
    ids, cnt = (C.c_uint64 * 128)(), (C.c_uint64 * 1)()
    rc = L.mi355_sort_rows_dev(None, buf, 100, 9, None, 0, 0, ids, None, 100, cnt)
    assert rc != 0 and L.mi355_last_error()


def test_every_sort_rows_kernel_has_a_case():
    """every __global__ under csrc/sort/ is asserted from the launch record by a GPU case of this file, and the file names no
    kernel that does not exist"""
    kernels = support.global_kernels_of("sort")
    assert kernels == {COUNT_KERNEL, SCATTER_KERNEL, ITEM_COUNT_KERNEL, ITEM_SCATTER_KERNEL, OFFSETS_KERNEL}, kernels
    support.check_gpu_part_asserts(__file__, "COUNT_KERNEL", "SCATTER_KERNEL", "ITEM_COUNT_KERNEL", "ITEM_SCATTER_KERNEL", "OFFSETS_KERNEL")


def test_sort_rows_sources_read_no_flag_bits():
    assert [os.path.basename(p) for p in support.feature_sources("sort")] == ["sort_rows.hip", "sort_rows.hpp"]
    support.check_sources_read_no_flag_bits("sort")


def test_expectation_orders_by_value_then_row():
    vals = np.array([5, 9, 5, 1, 9, 5, 0, 5], dtype=np.uint32)
    rows, v = expect(vals, False)
    assert rows.tolist() == [6, 3, 0, 2, 5, 7, 1, 4] and v.tolist() == [0, 1, 5, 5, 5, 5, 9, 9]
    rows, v = expect(vals, True)
    assert rows.tolist() == [1, 4, 0, 2, 5, 7, 3, 6] and v.tolist() == [9, 9, 5, 5, 5, 5, 1, 0]
    rows, v = expect(vals, True, qual=np.array([1, 0, 1, 0, 1, 1, 1, 0], dtype=bool))
    assert rows.tolist() == [4, 0, 2, 5, 6]
    wide = np.array([1 << 31, 3, (1 << 32) - 1, 1 << 31], dtype=np.uint32)
    assert expect(wide, True)[0].tolist() == [2, 0, 3, 1] and expect(wide, False)[0].tolist() == [1, 0, 3, 2]
    assert want_record(8) == [COUNT_KERNEL, SCAN_KERNEL, OFFSETS_KERNEL, SCATTER_KERNEL] and len(want_record(32)) == 16


@pytest.mark.parametrize("case", PATTERN_CASES, ids=lambda s: f"{s[0]}-{s[1]}")
def test_patterns_are_not_vacuous(case):
    c, name = case
    vals = pattern(name, c)
    assert len(vals) == N_PAT and int(vals.max()) < 1 << c
    low = DIGIT * (passes(c) - 1)
    distinct = len(np.unique(vals))
    if name == "all-equal":
        assert distinct == 1
    if name in ("two-values", "extremes"):
        assert distinct == 2 and min(np.bincount((vals == vals[0]).astype(np.int64))) > S # thousands of ties per bucket, in every span
    if name == "extremes":
        assert sorted(np.unique(vals).tolist()) == [0, (1 << c) - 1]
    if name in ("ascending", "descending"):
        d = np.diff(vals.astype(np.int64))
        assert ((d >= 0).all() if name == "ascending" else (d <= 0).all()) and distinct >= min(1 << c, 1000)
    if name == "lowest-digit":
        assert len(np.unique(vals >> DIGIT)) == 1 and len(np.unique(vals & 0xFF)) == 256
    if name == "top-digit":
        assert len(np.unique(vals & ((1 << low) - 1))) == 1 and len(np.unique(vals >> low)) == min(1 << (c - low), 256)
    if c == 2:  # the stability test: every bucket holds thousands of ties
        assert name in ("all-equal", "two-values", "extremes") or min(np.bincount(vals, minlength=4)) > 1000


@pytest.mark.parametrize("kind", [m for m in MASKS if m.startswith("random")])
def test_random_masks_are_neither_empty_nor_full(kind):
    bits = mask_of(kind, N_PAT)
    assert bits.any() and not bits.all() and len(bits) == N_PAT


def test_shapes_cross_what_they_should():
    assert 256 * ((N_GROUPS + S - 1) // S) > GROUP and 256 * ((N_LONG + S - 1) // S) > GROUP  # more than one scan group of counters
    assert (N_LONG + S - 1) // S > 2 * 4 * 4  # one block of four waves walks several spans per wave
    for c in CAPTURE_WIDTHS:
        (v0, m0), (v1, m1) = capture_data(c)
        a, b = expect(v0, False, m0), expect(v1, False, m1)
        assert len(a[0]) != len(b[0]) and (a[0][:1000] != b[0][:1000]).any(), "a stale result could pass"


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

class Sort:
    """one engine, an uploaded column and mask (both in hostile surroundings); every run gets guarded outputs full of 0xEE"""

    def __init__(self, O, eng, c, vals, qual=None, col=None, mask=None):
        from shared_simd_scan_amd.engine import PackedColumn

        self.eng, self.c, self.n, self.vals, self.qual = eng, c, len(vals), vals, qual
        self.col = PackedColumn(hostile_pack(O, vals, c), self.n, c) if col is None else col
        if mask is not None:
            self.mask, self.mask_buf = mask
        elif qual is not None:
            self.mask, self.mask_buf = hostile_bitmap(qual)
        else:
            self.mask = self.mask_buf = None

    def run(self, L, descending=False, capacity=None, first_row=0, with_values=True, what="", pre=None, raw=False):
        """-> checks every row id and value, the guards, the count, the inputs and the launch record; returns the record
        (raw: the outputs' bytes as well)"""
        import torch

        tag = (what, self.c, self.n, descending, capacity, first_row)
        rows, v = pre or expect(self.vals, descending, self.qual)
        q = len(rows)
        cap = self.n if capacity is None else capacity
        ids, vals = Guarded(cap * 8), Guarded(cap * 4)
        count = torch.full((1,), -0x1112, dtype=torch.int64, device="cuda")
        col_before = self.col.data.clone()
        mask_before = None if self.mask_buf is None else self.mask_buf.clone()
        rc = L.mi355_sort_rows_dev(self.eng._ctx, self.col.data.data_ptr(), self.n, self.c, None if self.mask is None else self.mask.data_ptr(),
                                   1 if descending else 0, first_row, ids.ptr if cap else None, vals.ptr if with_values and cap else None, cap,
                                   count.data_ptr())
        assert rc == 0, (tag, L.mi355_last_error())
        self.eng.synchronize()
        have_ids, have_vals = ids.fetch().view(np.uint64), vals.fetch().view(np.uint32)  # (fetch asserts the guard bytes on both sides)
        assert count.tolist() == [q], (tag, count.tolist(), q)
        m = q if q <= cap else 0  # all or nothing
        want_ids = (rows[:m].astype(np.uint64) + np.uint64(first_row)).astype(np.uint64)
        bad = np.nonzero(have_ids[:m] != want_ids)[0]
        assert bad.size == 0, (tag, "row id", int(bad[0]), "of", m, "have", int(have_ids[bad[0]]), "want", int(want_ids[bad[0]]), "wrong", bad.size)
        assert (have_ids[m:] == GUARD64).all(), (tag, "row ids written at or behind entry", m)
        if with_values:
            bad = np.nonzero(have_vals[:m] != v[:m])[0]
            assert bad.size == 0, (tag, "value", int(bad[0]), "of", m, "have", int(have_vals[bad[0]]), "want", int(v[bad[0]]), "wrong", bad.size)
            assert (have_vals[m:] == GUARD32).all(), (tag, "values written at or behind entry", m)
        else:
            assert (have_vals == GUARD32).all(), (tag, "values written without being asked for")
        assert torch.equal(self.col.data, col_before), (tag, "column written")
        assert mask_before is None or torch.equal(self.mask_buf, mask_before), (tag, "mask written")
        rec = record(L, self.eng)
        names = [base_name(x[0]) for x in rec]
        assert names == want_record(self.c, writes=cap > 0), (tag, names)
        assert rec[0][0] == COUNT_KERNEL and rec[2] == (OFFSETS_KERNEL, 1, 0, 0) and all(x[3] == 0 for x in rec), (tag, rec)
        if cap > 0:
            assert rec[3][0] == SCATTER_KERNEL and rec[3][2] > rec[0][2] > 0, (tag, rec)  # (dynamic LDS: the images; the scatter's stage)
        if cap > 0 and passes(self.c) > 1:
            assert rec[4][0] == ITEM_COUNT_KERNEL and rec[-1][0] == ITEM_SCATTER_KERNEL and rec[-1][2] > rec[4][2] == 0, (tag, rec)
        return (rec, have_ids.tobytes(), have_vals.tobytes()) if raw else rec


@gpu
@pytest.mark.parametrize("c", SIZE_WIDTHS)
def test_sizes_and_tails(L, O, eng, c):
    for n in SIZES:
        Sort(O, eng, c, values_of(c, n)).run(L, False)
        Sort(O, eng, c, values_of(c, n, salt=1), mask_of("random-1/2", n, salt=n)).run(L, True)


@gpu
@pytest.mark.parametrize("c", LONG_WIDTHS)
def test_one_block_walks_many_spans(L, O, eng, c):
    """grid_cus = 1, max_blocks_per_cu = 1: one block per launch, every wave walks ten spans and their tiles"""
    look = Sort(O, eng, c, values_of(c, N_LONG, salt=4), mask_of("random-1/2", N_LONG))
    eng.set_option("grid_cus", 1)
    eng.set_option("max_blocks_per_cu", 1)
    try:
        for descending in (False, True):
            rec = look.run(L, descending, what="one block")
            assert all(x[1] == 1 for x in rec if base_name(x[0]) != SCAN_KERNEL) and base_name(rec[0][0]) == COUNT_KERNEL, rec
    finally:
        eng.set_option("grid_cus", 0)
        eng.set_option("max_blocks_per_cu", 0)
    assert look.run(L, False, what="whole chip")[0][1] > 1


@gpu
@pytest.mark.parametrize("c", LONG_WIDTHS)
def test_prefix_across_scan_groups(L, O, eng, c):
    """7 spans x 256 digits: the counters fill two scan groups of 1024, a rank adds its group's prefix"""
    look = Sort(O, eng, c, values_of(c, N_GROUPS, salt=6))
    for descending in (False, True):
        rec = look.run(L, descending, what="scan groups")
        assert rec[1][0] == SCAN_KERNEL and rec[1][1] == 2 and rec[2][0] == OFFSETS_KERNEL, rec


@gpu
@pytest.mark.parametrize("case", PATTERN_CASES, ids=lambda s: f"{s[0]}-{s[1]}")
def test_value_patterns(L, O, eng, case):
    c, name = case
    look = Sort(O, eng, c, pattern(name, c))
    for descending in (False, True):
        look.run(L, descending, what=name)


@gpu
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("c", MASK_WIDTHS)
def test_masks(L, O, eng, c, kind):
    n = N_PAT
    look = Sort(O, eng, c, values_of(c, n, salt=3), mask_of(kind, n))
    for descending in (False, True):
        look.run(L, descending, what=kind)
    if kind == "empty":
        assert len(expect(look.vals, False, look.qual)[0]) == 0  # (run() found every output byte a guard byte)


@gpu
@pytest.mark.parametrize("c", (8, 12, 16))
def test_tiles_on_both_sides_of_the_stage_threshold(L, O, eng, c):
    """a scatter ranks a tile inside an LDS stage from 1024 qualifying rows on and writes every row straight to its place below:
    tiles of 1023, 1024, 1025, 0, 2048 and 1 qualifying rows follow each other inside one span, at widths whose passes have 256
    and 16 buckets (the stage) and at 8 + 4 bit's second pass"""
    n = S + 2048 + 77
    rng = np.random.default_rng([c, 29])
    qual = np.zeros(n, dtype=bool)
    for t, rows in enumerate((1023, 1024, 1025, 0, 2048, 1, 1024, 700, 2048)):
        qual[t * 2048 + rng.choice(2048, rows, replace=False)] = True
    qual[S + 2048:] = True
    assert [int(qual[t * 2048: (t + 1) * 2048].sum()) for t in range(3)] == [1023, 1024, 1025]
    look = Sort(O, eng, c, values_of(c, n, salt=14), qual)
    for descending in (False, True):
        rec = look.run(L, descending, what="stage threshold")
        assert rec[3][0] == SCATTER_KERNEL, rec
    for n in (2048 + 1023, 2048 + 1024, 2048 + 1025):  # the item passes' last stage: 1023, 1024, 1025 items
        rec = Sort(O, eng, c, values_of(c, n, salt=15)).run(L, False, what="the last stage of items")
        assert c == 8 or rec[-1][0] == ITEM_SCATTER_KERNEL, rec


@gpu
def test_capacity(L, O, eng):
    """all or nothing: q == capacity writes q entries, q == capacity + 1 writes none; capacity 0 only counts"""
    n = N_PAT
    for c in (8, 9, 17):
        vals, qual = values_of(c, n, salt=7), mask_of("random-1/2", n, salt=7)
        q = int(qual.sum())
        look = Sort(O, eng, c, vals, qual)
        for descending in (False, True):
            pre = expect(vals, descending, qual)
            look.run(L, descending, capacity=q, what="q == capacity", pre=pre)
            look.run(L, descending, capacity=q - 1, what="q == capacity + 1", pre=pre)
            look.run(L, descending, capacity=8 * n, what="a capacity far above q", pre=pre)
        rec = look.run(L, False, capacity=0, what="capacity 0, null row ids")
        assert [base_name(x[0]) for x in rec] == [COUNT_KERNEL, SCAN_KERNEL, OFFSETS_KERNEL]
        look.run(L, False, capacity=1, what="capacity 1")
    one = Sort(O, eng, 9, values_of(9, n, salt=7), mask_of("first", n))
    one.run(L, False, capacity=1, what="q == capacity == 1")


@gpu
def test_other_arguments(L, O, eng):
    n = 3 * S + 5
    for c in (9, 32):
        vals, qual = values_of(c, n, salt=8), mask_of("random-1/2", n, salt=8)
        look = Sort(O, eng, c, vals, qual)
        for first_row in (0, (1 << 32) + 12345, (1 << 64) - n):
            look.run(L, True, first_row=first_row, what="first_row")
        look.run(L, False, with_values=False, what="no values")


@gpu
@pytest.mark.parametrize("c", (9, 17))
def test_row_range_views(L, O, eng, c):
    """rows [lead, lead + n) of a longer column, lead = 128 rows (the least slice_rows admits), with the mask's bytes of exactly
    those rows inside a longer bitmap that begins 4 bytes behind a 16-byte boundary: nothing of the rows in front or behind
    reaches the result"""
    from shared_simd_scan_amd.engine import PackedColumn

    n, lead, trail = N_PAT, 128, 4096
    vals, qual = values_of(c, n, salt=9), mask_of("random-1/2", n, salt=9)
    rng = np.random.default_rng([c, 23])
    junk = np.full(lead, (1 << c) - 1, dtype=np.uint32)
    whole = PackedColumn(plain_pack(O, np.concatenate([junk, vals, np.zeros(trail, dtype=np.uint32)]), c), lead + n + trail, c)
    col = eng.slice_rows(whole, lead, lead + n)
    assert col.n == n and col.data.data_ptr() % 16 == 0
    front = np.concatenate([np.full(4, 0xFF, dtype=np.uint8), rng.integers(0, 256, lead // 8, dtype=np.uint8)])
    mask = hostile_bitmap(qual, offset=4, front=front)
    assert mask[0].data_ptr() % 16 == 4
    look = Sort(O, eng, c, vals, qual, col=col, mask=mask)
    for descending in (False, True):
        look.run(L, descending, first_row=lead, what="view")


@gpu
def test_same_bytes_whatever_the_grid(L, O, eng):
    n = N_LONG
    for c in (9, 25):
        look = Sort(O, eng, c, values_of(c, n, salt=10) % np.uint32(min(1 << c, 5000)), mask_of("random-1/2", n, salt=10))
        pre = expect(look.vals, True, look.qual)
        runs = []
        for grid_cus, bpc in ((0, 0), (3, 1), (64, 2)):
            eng.set_option("grid_cus", grid_cus)
            eng.set_option("max_blocks_per_cu", bpc)
            try:
                runs.append(look.run(L, True, capacity=n + 100, what=f"grid_cus {grid_cus}", pre=pre, raw=True))
            finally:
                eng.set_option("grid_cus", 0)
                eng.set_option("max_blocks_per_cu", 0)
        assert runs[0][0][0][1] != runs[1][0][0][1], "the grids do not differ"
        assert base_name(runs[0][0][0][0]) == COUNT_KERNEL and all(r[1:] == runs[0][1:] for r in runs[1:]), c


@gpu
def test_top_k_sort_rows_gather(L, O, eng):
    """ORDER BY v DESC LIMIT 1000: top_k, then sort_rows under its bitmap with capacity = k, then gather on the ids"""
    from shared_simd_scan_amd.engine import PackedColumn

    n, c, k = 3 * S + 5, 9, 1000
    vals = values_of(c, n, salt=11)
    col = PackedColumn(plain_pack(O, vals, c), n, c)
    top, result = eng.top_k(col, k, largest=True)
    rowids, count, values = eng.sort_rows(col, descending=True, mask=top, capacity=k, with_values=True)
    assert [base_name(x[0]) for x in record(L, eng)] == [COUNT_KERNEL, SCAN_KERNEL, OFFSETS_KERNEL, SCATTER_KERNEL, ITEM_COUNT_KERNEL, SCAN_KERNEL,
                                                         OFFSETS_KERNEL, ITEM_SCATTER_KERNEL]
    taken = eng.gather(col, rowids, count)
    eng.synchronize()
    rows, v = expect(vals, True)
    assert count.tolist() == [k] and result.tolist()[0] == k
    assert rowids.tolist() == rows[:k].tolist()
    assert (values.cpu().numpy().view(np.uint32) == v[:k]).all() and (taken.cpu().numpy()[:k].view(np.uint32) == v[:k]).all()
    assert len(np.unique(v[:k])) < k // 10, "no ties among the survivors"


@gpu
def test_errors_launch_nothing(L, O, eng):
    import torch

    c, n = 9, S + 77
    vals, qual = values_of(c, n, salt=12), mask_of("random-1/2", n, salt=12)
    look = Sort(O, eng, c, vals, qual)
    nb_col, nb = (n * c + 7) // 8, (n + 7) // 8
    ids, out_vals = Guarded(n * 8), Guarded(n * 4)
    big = Guarded(1 << 18)  # a buffer that can stand for an input and an output at once
    cnt = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    cp, mp, ip, vp, np_ = look.col.data.data_ptr(), look.mask.data_ptr(), ids.ptr.value, out_vals.ptr.value, cnt.data_ptr()

    def call(cp=cp, n=n, c=c, mp=mp, ip=ip, vp=vp, cap=n, np_=np_):
        for g in (ids, out_vals, big):
            g.t.fill_(SENTINEL)
        cnt.fill_(-7)
        rc = L.mi355_sort_rows_dev(eng._ctx, cp, n, c, mp, 0, 0, ip, vp, cap, np_)
        eng.synchronize()
        return rc

    rows, v = expect(vals, False, qual)
    q = len(rows)
    assert call() == 0 and cnt.tolist() == [q, -7] and (ids.fetch().view(np.uint64)[:q] == rows.astype(np.uint64)).all()
    valid = record(L, eng)
    assert [base_name(x[0]) for x in valid] == want_record(c)
    assert nb_col + 8 * n + 512 <= 1 << 18
    b = big.ptr.value
    errors = (("c = 0", dict(c=0), b"32"), ("c = 33", dict(c=33), b"32"), ("n = 2^32 + 1", dict(n=(1 << 32) + 1), b"2^32"),
              ("null row ids", dict(ip=None), b"rowids_dev"), ("null count", dict(np_=None), b"count_dev"), ("null column", dict(cp=None), b"packed_dev"),
              ("column at +4", dict(cp=cp + 4), b"aligned"), ("mask at +2", dict(mp=mp + 2), b"aligned"), ("row ids at +4", dict(ip=ip + 4), b"aligned"),
              ("values at +2", dict(vp=vp + 2), b"aligned"), ("count at +4", dict(np_=np_ + 4), b"aligned"),
              ("row ids are the column", dict(cp=b, ip=b), b"rowids_dev overlaps packed_dev"),
              ("row ids start in the column's last byte", dict(cp=b, ip=b + (nb_col - 1) // 8 * 8), b"rowids_dev overlaps packed_dev"),
              ("column starts inside the row ids", dict(cp=b + 256, ip=b), b"rowids_dev overlaps packed_dev"),
              ("row ids start in the mask's last byte", dict(mp=b, ip=b + (nb - 1) // 8 * 8), b"rowids_dev overlaps mask_dev"),
              ("values are the column", dict(cp=b, vp=b), b"values_dev overlaps packed_dev"),
              ("values start 4 bytes into the mask", dict(mp=b, vp=b + 4), b"values_dev overlaps mask_dev"),
              ("count inside the column", dict(cp=b, np_=b + 64), b"count_dev overlaps packed_dev"),
              ("count inside the mask", dict(mp=b, np_=b + 8), b"count_dev overlaps mask_dev"),
              ("values inside the row ids", dict(ip=b, vp=b + 8 * n - 4), b"rowids_dev overlaps values_dev"),
              ("count inside the row ids", dict(ip=b, np_=b + 8), b"count_dev overlaps rowids_dev"),
              ("count inside the values", dict(vp=b, np_=b + 8), b"count_dev overlaps values_dev"))
    for what, kw, word in errors:
        assert call(**kw) == E_INVALID, what
        assert word in L.mi355_last_error(), (what, L.mi355_last_error())
        assert record(L, eng) == [], what  # a refused call leaves an empty record and launches nothing
        for g in (ids, out_vals, big):
            assert (g.fetch() == SENTINEL).all(), what
        assert cnt.tolist() == [-7, -7], what
    # n == 0: the count zeroed, nothing launched, nothing else written, and no other pointer needed
    assert call(n=0, cp=None, mp=None, ip=None, vp=None) == 0 and record(L, eng) == [] and cnt.tolist() == [0, -7]
    assert (ids.fetch() == SENTINEL).all() and (out_vals.fetch() == SENTINEL).all()
    assert call() == 0 and record(L, eng) == valid and cnt.tolist() == [q, -7]


@gpu
@pytest.mark.parametrize("c", CAPTURE_WIDTHS)
def test_graph_capture_and_replay(O, c):
    """one sort_rows in a graph on a side stream, after a warm-up call of the same size: after column and mask are rewritten in
    place the replay follows them"""
    import torch

    from shared_simd_scan_amd import lib

    n = N_PAT
    versions = capture_data(c)

    def steps(eng):
        stage = [(plain_pack(O, v, c), torch.from_numpy(packbits(m)).cuda()) for v, m in versions]
        col, mask = torch.empty_like(stage[0][0]), torch.empty_like(stage[0][1])
        ids, vals = Guarded(n * 8), Guarded(n * 4)
        cnt = torch.empty(1, dtype=torch.int64, device="cuda")

        def load(r):
            col.copy_(stage[r][0])
            mask.copy_(stage[r][1])
            ids.t.fill_(SENTINEL)
            vals.t.fill_(SENTINEL)
            cnt.fill_(-7)

        def run():
            rc = lib().mi355_sort_rows_dev(eng._ctx, col.data_ptr(), n, c, mask.data_ptr(), 0, 0, ids.ptr, vals.ptr, n, cnt.data_ptr())
            assert rc == 0, lib().mi355_last_error()

        def check(r, what):
            rows, v = expect(versions[r][0], False, versions[r][1])
            q = len(rows)
            have_ids, have_vals = ids.fetch().view(np.uint64), vals.fetch().view(np.uint32)
            assert cnt.tolist() == [q], what
            assert (have_ids[:q] == rows.astype(np.uint64)).all() and (have_ids[q:] == GUARD64).all(), what
            assert (have_vals[:q] == v).all() and (have_vals[q:] == GUARD32).all(), what

        def untouched():
            assert (ids.fetch() == SENTINEL).all() and (vals.fetch() == SENTINEL).all() and cnt.tolist() == [-7]

        def warmed(launched):
            assert [base_name(x[0]) for x in launched] == want_record(c)

        return capture.Steps(load, run, check, untouched, warmed)

    capture.capture_replay(steps, (0, 1, 0))


@gpu
def test_capture_refuses_to_grow_the_workspace(O):
    """a fresh context that has seen a small column only: under capture a larger one is refused (MI355_E_INVALID, the message
    names graph capture), nothing is enqueued for it and the capture stays intact -- the small call around it replays"""
    import torch

    from shared_simd_scan_amd import lib

    c, small_n, big_n = 9, S + 77, 40 * S
    vals = values_of(c, small_n, salt=13)

    def setup(eng):
        col, big_col = plain_pack(O, vals, c), plain_pack(O, values_of(c, big_n), c)
        ids, refused = Guarded(small_n * 8), Guarded(big_n * 8)
        cnt = torch.full((2,), -7, dtype=torch.int64, device="cuda")

        def small():
            assert lib().mi355_sort_rows_dev(eng._ctx, col.data_ptr(), small_n, c, None, 1, 0, ids.ptr, None, small_n, cnt.data_ptr()) == 0

        def big():
            return lib().mi355_sort_rows_dev(eng._ctx, big_col.data_ptr(), big_n, c, None, 1, 0, refused.ptr, None, big_n, cnt.data_ptr() + 8)

        def reset():
            ids.t.fill_(SENTINEL)
            cnt.fill_(-7)

        def check_small():
            rows, _ = expect(vals, True)
            assert cnt.tolist() == [small_n, -7] and (ids.fetch().view(np.uint64) == rows.astype(np.uint64)).all()

        return small, big, reset, check_small, refused

    capture.refused_under_capture(setup)
