"""The k largest or smallest rows of a packed column, as a bitmap (include/mi355_topk.h, ScanEngine.top_k / kth_value).

CPU: the header is plain C99 and declares exactly what _capi.HEADERS binds for it and the library exports; it carries its
graph-capture verdict; mi355_top_k_passes (pure arithmetic) is 1 / 2 / 3 by width; top_k and kth_value hand the C ABI what they
should (through a recording stand-in for the library); without a device the entry point fails with a message; every __global__
under csrc/topk/ is named by the launch record of a GPU case of this file; no source there reads a switch bit; the data recipes
are not vacuous.

GPU (-m gpu): every expectation is numpy on the values and the mask the test generated -- np.lexsort((row id, key)) over the
qualifying rows, the first m = min(k, q) of them set in a bitmap, the four result words computed alongside; nothing is derived
from engine output.  Every one of the ceil(n / 8) bitmap bytes and the 0xEE guard bytes on both sides of it (the guard behind
begins at the very next byte) are compared exactly, and the four result words; column and mask must be unchanged after the call
(unless the mask is the output).  Every case runs in hostile surroundings: ones in the column's bits behind row n - 1 and in its
pad, 0xFF bytes directly behind byte ceil(n / 8) of the mask.  A chunk is K = 16384 rows (one wave's work in the trim), a scan
group 1024 chunks; a digit is 12 bits, so widths 12 | 13 and 24 | 25 are the two sides of a digit boundary.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import capture
import support
from support import E_INVALID, SENTINEL, Guarded, L, base_name, eng, fake, hostile_bitmap, hostile_pack, packbits, plain_pack, record  # noqa: F401  (L, eng, fake: fixtures)

HEADER = "mi355_topk.h"

# the kernels of csrc/topk/, as the launch record names them: the GPU cases below assert these labels
HIST_KERNEL = "topk_hist_kernel"
PICK_KERNEL = "topk_pick_kernel"
EMIT_KERNEL = "topk_emit_kernel"
TRIM_KERNEL = "topk_trim_kernel"
SCAN_KERNEL = "rowid_scan_kernel"  # kernels/bitmap.hpp, launched between the last two

K = 16384  # rows per chunk
GROUP = 1024  # chunks per scan group
DIGIT = 12

N_WIDTH = 20011
N_PAT = 5 * K + 77
N_LONG = 40 * K + 1237
N_GROUPS = (GROUP + 1) * K + 1237
SIZES = [1, 31, 63, 64, 4095, 4096, 8191, 8192, 8193, K, K + 1, 3 * K + 5]
SIZE_WIDTHS = [1, 9, 12, 13, 17, 24, 25, 32]
PATTERN_WIDTHS = [9, 17, 32]
PATTERNS = ["all-equal", "all-equal-early", "all-equal-late", "two-values", "ascending", "descending", "extremes", "top-digit", "top-two-digits", "exact-bucket"]
MASKS = ["none", "random-1/2", "random-1/64", "empty", "first", "last", "in-place"]
MASK_WIDTHS = [9, 25]
LONG_WIDTHS = [9, 24]
VIEW_WIDTHS = [9, 17]
CAPTURE_WIDTHS = [9, 17]

gpu = pytest.mark.gpu


def passes(c):
    return (c + DIGIT - 1) // DIGIT


def digits_of(x, c):
    """the digits of a value's key (largest: the value itself), most significant first: the top one takes what 12-bit digits leave"""
    D = passes(c)
    return [(int(x) >> (DIGIT * (D - 1 - d))) & ((1 << DIGIT) - 1 if d else (1 << (c - DIGIT * (D - 1))) - 1) for d in range(D)]


# values_of and mask_of differ from test_compact's and test_sort_rows' in the seeds ([.., 7] and [.., 11] here), mask_of also in its "in-place" and "ones"
# kinds: the "not vacuous" tests pin each file's data
@functools.lru_cache(maxsize=None)
def values_of(c, n, salt=0):
    rng = np.random.default_rng([c, n, salt, 7])
    vals = rng.integers(0, 1 << c, n, dtype=np.uint64).astype(np.uint32)
    vals.setflags(write=False)
    return vals


@functools.lru_cache(maxsize=None)
def mask_of(kind, n, salt=0):
    """the qualifying rows as a bool array of n rows; None = no mask at all"""
    if kind in ("none",):
        return None
    rng = np.random.default_rng([n, salt, len(kind), 11])
    bits = np.zeros(n, dtype=bool)
    if kind.startswith("random-"):
        num, _, den = kind[7:].partition("/")
        bits = rng.random(n) < float(num) / float(den)
    elif kind == "first":
        bits[0] = True
    elif kind == "last":
        bits[n - 1] = True
    elif kind in ("in-place", "ones"):
        bits = rng.random(n) < 0.5 if kind == "in-place" else np.ones(n, dtype=bool)
    else:
        assert kind == "empty", kind
    bits.setflags(write=False)
    return bits


def expect(vals, k, largest, qual=None):
    """-> (the selected rows as a bool array, [m, T, beyond, ties]): numpy's lexsort over the qualifying rows by (key, row id)"""
    n = len(vals)
    rows = np.arange(n, dtype=np.int64) if qual is None else np.nonzero(qual)[0].astype(np.int64)
    v = vals[rows]
    if int(vals.max(initial=0)) < 1 << 16:
        v = v.astype(np.uint16)  # (the same order; numpy sorts 16-bit keys by radix)
    key = ~v if largest else v  # the complement of an unsigned value reverses the order
    order = np.lexsort((rows, key))
    m = min(int(k), len(rows))
    bits = np.zeros(n, dtype=bool)
    bits[rows[order[:m]]] = True
    if m == 0:
        return bits, [0, 0, 0, 0]
    T = int(v[order[m - 1]])
    beyond = int((v[order[:m]] != T).sum())
    return bits, [m, T, beyond, int((v == T).sum())]


def cut_of(vals, k, largest, qual=None, pre=None):
    """-> (T, ties per chunk among the qualifying rows, r = ties the call keeps); pre: expect's answer, where it is at hand"""
    bits, (m, T, beyond, ties) = pre or expect(vals, k, largest, qual)
    tie = (vals == T) if qual is None else ((vals == T) & qual)
    nch = (len(vals) + K - 1) // K
    per_chunk = np.array([int(tie[ch * K: (ch + 1) * K].sum()) for ch in range(nch)])
    return T, per_chunk, m - beyond


@functools.lru_cache(maxsize=None)
def pattern(name, c):
    """-> (values, k, largest) of a value pattern at n = N_PAT, or None where the pattern needs more digits than c has"""
    n, top = N_PAT, (1 << c) - 1
    rng = np.random.default_rng([c, len(name), 3])
    D, low = passes(c), DIGIT * (passes(c) - 1)
    if name.startswith("all-equal"):  # k in the middle of the third chunk; -early: of the second, -late: of the fourth
        first = {"all-equal": 2, "all-equal-early": 1, "all-equal-late": 3}[name]
        vals, k, largest = np.full(n, top // 3, dtype=np.uint32), first * K + K // 2 + 3, True
    elif name == "two-values":
        a, b = top // 5, top // 5 + max(1, top // 2)
        vals = np.where(rng.random(n) < 0.3, b, a).astype(np.uint32)
        k, largest = int((vals == b).sum()) + int((vals == a).sum()) // 2, True
    elif name == "ascending":
        vals, k, largest = (np.arange(n, dtype=np.uint64) * (top + 1) // n).astype(np.uint32), n // 3, False
    elif name == "descending":
        vals, k, largest = (np.arange(n, dtype=np.uint64)[::-1] * (top + 1) // n).astype(np.uint32), n // 3, False
    elif name == "extremes":
        vals = np.where(rng.random(n) < 0.4, top, 0).astype(np.uint32)
        k, largest = int((vals == top).sum()) + int((vals[: 2 * K + K // 2] == 0).sum()) + 1, True
    elif name == "top-digit":  # every value shares its top digit; the lower ones are random
        if D < 2:
            return None
        vals = ((3 << low) | rng.integers(0, 1 << low, n, dtype=np.uint64)).astype(np.uint32)
        k, largest = 1000, True
    elif name == "top-two-digits":
        if D < 3:
            return None
        vals = ((0x5A << 24) | (0x123 << 12) | rng.integers(0, 1 << 12, n, dtype=np.uint64)).astype(np.uint32)
        k, largest = 1000, False
    else:  # the threshold's bucket holds exactly what is left of k, in every pass
        assert name == "exact-bucket", name
        vals = values_of(c, n, salt=5).copy()
        d0 = (1 << (c - low)) * 2 // 3  # a top digit; k = the rows at or above its bucket
        k, largest = int((vals >= (d0 << low)).sum()), True
    vals.setflags(write=False)
    return vals, k, largest


PATTERN_CASES = [(c, name) for c in PATTERN_WIDTHS for name in PATTERNS if pattern(name, c) is not None]


@functools.lru_cache(maxsize=None)
def k_cases():
    """a random 9-bit column under a random 1/2 mask -> (values, mask, {what: k}); the last k ends on a chunk boundary of the ties"""
    vals, qual = values_of(9, N_PAT, salt=1), mask_of("random-1/2", N_PAT, salt=1)
    q = int(qual.sum())
    T = 300
    tie = (vals == T) & qual
    above = int(((vals > T) & qual).sum())
    return vals, qual, {"0": 0, "1": 1, "q-1": q - 1, "q": q, "q+1": q + 1, "2^63": 1 << 63, "chunk-boundary": above + int(tie[: 3 * K].sum()),
                        "chunk-boundary-early": above + int(tie[:K].sum())}


@functools.lru_cache(maxsize=None)
def group_case():
    """more than 1024 chunks of random 9-bit values -> (values, [k]): cuts whose straddling chunk lies in the first scan group
    (every chunk of the second clears its ties) and in the second (its ties before come from the first group's total)"""
    vals = values_of(9, N_GROUPS, salt=2)
    T = 200
    tie = vals == T
    above = int((vals > T).sum())
    ks = [above + int(tie[: 500 * K].sum()) + 3, above + int(tie[: GROUP * K].sum()) + 5]
    return vals, ks, [expect(vals, k, True) for k in ks]


@functools.lru_cache(maxsize=None)
def chain_data():
    rng = np.random.default_rng(2027)
    a = rng.integers(0, 1 << 9, N_PAT, dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 1 << 17, N_PAT, dtype=np.uint64).astype(np.uint32)
    b[::5] = 130000  # ties in the ordering column, high enough for the cut to go through them
    for x in (a, b):
        x.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def capture_data(c):
    """two versions of a column and of a mask over N_PAT rows"""
    return [(values_of(c, N_PAT, salt=50 + r), mask_of("random-1/2", N_PAT, salt=60 + r)) for r in range(2)]


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------

def test_top_k_header_is_plain_c99():
    support.check_header_is_plain_c99(HEADER)


def test_top_k_header_declares_what_python_binds(L):
    from shared_simd_scan_amd import _capi

    names, sigs = support.check_header_binds(L, HEADER)
    assert names == ["mi355_top_k_dev", "mi355_top_k_passes"]
    sig = sigs["mi355_top_k_dev"]
    assert sig[2] is C.c_uint64 and sig[3] is C.c_uint and sig[5] is C.c_uint64 and sig[6] is C.c_int and len(sig) == 9
    assert sigs["mi355_top_k_passes"] == [C.c_uint] and L.mi355_top_k_passes.restype is C.c_uint
    text = support.header_text(HEADER)
    assert '#include "mi355_scan.h"' in text and text.count("#include") == 1
    assert "mi355_topk.h" in _capi.HEADERS  # (the module's docstring points at HEADERS; it names no header of its own)


def test_top_k_header_carries_its_capture_verdict():
    support.check_capture_verdict(HEADER, r"capturable after a warm-up call", r"read at every replay")


def test_top_k_passes_by_width(L):
    """mi355_top_k_passes needs neither a device nor a context"""
    from shared_simd_scan_amd import top_k_passes

    for c in range(1, 33):
        want = 1 if c <= 12 else (2 if c <= 24 else 3)
        assert L.mi355_top_k_passes(c) == want == top_k_passes(c) == passes(c), c
    assert L.mi355_top_k_passes(0) == 0 and L.mi355_top_k_passes(33) == 0
    for bad in (0, 33, -1, 1 << 32):
        with pytest.raises(ValueError):
            top_k_passes(bad)


def test_top_k_wrapper_passes_what_the_abi_takes(fake, monkeypatch):
    import torch

    eng, rec, col = fake
    fact = col(17, 777)
    bitmap, result = eng.top_k(fact, 10)  # defaults: the largest, no mask, a fresh bitmap of ceil(777 / 8) bytes
    (name, a), = rec.calls
    assert name == "mi355_top_k_dev" and a[1:7] == [fact.data.data_ptr(), 777, 17, None, 10, 1]
    assert bitmap.dtype == torch.uint8 and bitmap.numel() == 98 and a[7] == bitmap.data_ptr()
    assert result.dtype == torch.int64 and result.numel() == 4 and a[8] == result.data_ptr()
    rec.calls.clear()
    mask, mine = torch.zeros(98, dtype=torch.uint8), torch.zeros(98, dtype=torch.uint8)
    bitmap, _ = eng.top_k(fact, 1 << 63, largest=False, mask=mask, out=mine)
    (name, a), = rec.calls
    assert bitmap is mine and a[1:8] == [fact.data.data_ptr(), 777, 17, mask.data_ptr(), 1 << 63, 0, mine.data_ptr()]
    rec.calls.clear()
    bitmap, _ = eng.top_k(fact, 5, mask=mask, out=mask)  # in place
    assert bitmap is mask and rec.calls[0][1][4] == rec.calls[0][1][7] == mask.data_ptr()
    rec.calls.clear()
    eng.top_k(col(9, 0), 5)  # an empty column: no pointer but the result's
    assert rec.calls[0][1][1:5] == [None, 0, 9, None] and rec.calls[0][1][7] is None
    rec.calls.clear()
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError):
            eng.top_k(fact, bad)
    with pytest.raises(AssertionError):
        eng.top_k(fact, 5, mask=torch.zeros(97, dtype=torch.uint8))  # a mask shorter than the column
    with pytest.raises(AssertionError):
        eng.top_k(fact, 5, out=torch.zeros(97, dtype=torch.uint8))
    with pytest.raises(AssertionError):
        eng.top_k(fact, 5, out=torch.zeros(98, dtype=torch.int8))
    assert rec.calls == []
    # kth_value: one top_k, then the threshold read on the host; fewer than k qualifying rows is an error
    zeros = torch.zeros
    monkeypatch.setattr(torch, "empty", lambda size, **kw: zeros(size, **kw) + 7 if kw.get("dtype") is torch.int64 else zeros(size, **kw))
    assert eng.kth_value(fact, 7, largest=False, mask=mask) == 7
    (name, a), = rec.calls
    assert name == "mi355_top_k_dev" and a[4:7] == [mask.data_ptr(), 7, 0]
    with pytest.raises(ValueError):
        eng.kth_value(fact, 8)  # the stand-in's m is 7
    with pytest.raises(ValueError):
        eng.kth_value(fact, 0)


def test_top_k_entry_point_fails_loudly_without_a_gpu(L):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    buf, bm = (C.c_uint8 * 1024)(), (C.c_uint8 * 1024)()
    res = (C.c_uint64 * 4)()
    rc = L.mi355_top_k_dev(None, buf, 100, 9, None, 5, 1, bm, res)
    assert rc != 0 and L.mi355_last_error()


def test_every_top_k_kernel_has_a_case():
    """every __global__ under csrc/topk/ is asserted from the launch record by a GPU case of this file, and the file names no
    kernel that does not exist"""
    kernels = support.global_kernels_of("topk")
    assert kernels == {HIST_KERNEL, PICK_KERNEL, EMIT_KERNEL, TRIM_KERNEL}, kernels
    support.check_gpu_part_asserts(__file__, "HIST_KERNEL", "PICK_KERNEL", "EMIT_KERNEL", "TRIM_KERNEL")


def test_top_k_sources_read_no_flag_bits():
    assert [os.path.basename(p) for p in support.feature_sources("topk")] == ["top_k.hip", "top_k.hpp"]
    support.check_sources_read_no_flag_bits("topk")


def test_expectation_orders_by_value_then_row():
    vals = np.array([5, 9, 5, 1, 9, 5, 0, 5], dtype=np.uint32)
    bits, res = expect(vals, 4, True)
    assert np.nonzero(bits)[0].tolist() == [0, 1, 2, 4] and res == [4, 5, 2, 4]  # two 9s, then the two lowest rows of the four 5s
    bits, res = expect(vals, 3, False, qual=np.array([1, 1, 1, 0, 1, 1, 1, 1], dtype=bool))
    assert np.nonzero(bits)[0].tolist() == [0, 2, 6] and res == [3, 5, 1, 4]
    assert expect(vals, 0, True)[1] == [0, 0, 0, 0] and expect(vals, 99, True)[0].all()
    wide = np.array([1 << 31, 3, (1 << 32) - 1, 1 << 31], dtype=np.uint32)
    assert np.nonzero(expect(wide, 2, True)[0])[0].tolist() == [0, 2] and expect(wide, 2, True)[1] == [2, 1 << 31, 1, 2]


@pytest.mark.parametrize("case", PATTERN_CASES, ids=lambda s: f"{s[0]}-{s[1]}")
def test_patterns_are_not_vacuous(case):
    c, name = case
    vals, k, largest = pattern(name, c)
    assert len(vals) == N_PAT and int(vals.max()) < 1 << c and 0 < k < N_PAT
    T, per_chunk, r = cut_of(vals, k, largest)
    ties = int(per_chunk.sum())
    assert 1 <= r <= ties
    if name.startswith("all-equal") or name in ("two-values", "extremes"):  # the cut goes through ties
        assert 0 < r < ties, (r, ties)
        before = np.concatenate([[0], np.cumsum(per_chunk)])
        straddle = [ch for ch in range(len(per_chunk)) if before[ch] < r < before[ch + 1]]
        assert len(straddle) == 1 and 0 < straddle[0] < len(per_chunk) - 1, straddle  # neither the first nor the last chunk
        assert per_chunk[0] > 0 and before[1] <= r, "no chunk lies wholly before the cut"
        assert per_chunk[-1] > 0 and before[-2] >= r, "no chunk lies wholly behind the cut"
    if name.startswith("all-equal"):
        assert len(np.unique(vals)) == 1 and (name != "all-equal" or 2 * K < k < 3 * K)
    # fewer than half of the ties kept: the trim adds them; more: it takes the others away -- both happen, with a cut inside the column
    if name == "all-equal-early":
        assert 2 * r < ties
    if name == "all-equal-late":
        assert 2 * r > ties
    if name == "two-values":
        assert len(np.unique(vals)) == 2
    if name in ("ascending", "descending"):
        d = np.diff(vals.astype(np.int64))
        assert ((d >= 0).all() if name == "ascending" else (d <= 0).all()) and len(np.unique(vals)) >= min(1 << c, 1000)
    if name == "extremes":
        assert sorted(np.unique(vals).tolist()) == [0, (1 << c) - 1]
    if name == "top-digit":  # the prefix collision: every row survives the first pass, the threshold's top digit is everyone's
        assert {digits_of(x, c)[0] for x in vals[:2000]} == {digits_of(T, c)[0]} and len({digits_of(x, c)[1] for x in vals}) > 100
    if name == "top-two-digits":
        assert {tuple(digits_of(x, c)[:2]) for x in vals[:2000]} == {tuple(digits_of(T, c)[:2])} and len(np.unique(vals)) > 1000
    if name == "exact-bucket":  # in every pass the rows at or beyond the threshold's bucket are exactly what is left of k
        assert r == ties
        key = vals.astype(np.int64)
        for d in range(passes(c)):
            sh = DIGIT * (passes(c) - 1 - d)
            assert int((key >> sh >= T >> sh).sum()) == k, d


def test_k_cases_are_not_vacuous():
    vals, qual, ks = k_cases()
    q = int(qual.sum())
    assert 0 < q < N_PAT and ks["q-1"] == q - 1 and ks["q+1"] == q + 1
    T, per_chunk, r = cut_of(vals, ks["chunk-boundary"], True, qual)
    before = np.cumsum(per_chunk)
    assert T == 300 and r == before[2] and per_chunk[2] > 0 and per_chunk[3] > 0 and 0 < r < per_chunk.sum() < 2 * r
    T, per_chunk, r = cut_of(vals, ks["chunk-boundary-early"], True, qual)
    assert T == 300 and r == per_chunk[0] > 0 and per_chunk[1] > 0 and 2 * r < per_chunk.sum()
    T, per_chunk, r = cut_of(vals, ks["q-1"], True, qual)
    assert r == per_chunk.sum() - 1 > 0  # all but the last row of the smallest value


def test_group_case_is_not_vacuous():
    vals, ks, pre = group_case()
    assert len(vals) > GROUP * K and len(ks) == 2
    for k, want, (lo, hi) in zip(ks, pre, ((1, GROUP - 1), (GROUP, GROUP))):
        T, per_chunk, r = cut_of(vals, k, True, pre=want)
        before = np.concatenate([[0], np.cumsum(per_chunk)])
        straddle = [ch for ch in range(len(per_chunk)) if before[ch] < r < before[ch + 1]]
        assert T == 200 and len(straddle) == 1 and lo <= straddle[0] <= hi, straddle
        assert per_chunk[:GROUP].sum() > 0 and per_chunk[GROUP:].sum() > 0, "no ties on one side of the group boundary"


@pytest.mark.parametrize("kind", [m for m in MASKS if m.startswith("random") or m == "in-place"])
def test_random_masks_are_neither_empty_nor_full(kind):
    for n in (N_PAT, N_WIDTH):
        bits = mask_of(kind, n)
        assert bits.any() and not bits.all() and len(bits) == n
    for n in SIZES:
        if n >= 63:
            bits = mask_of("random-1/2", n, salt=n)
            assert bits.any() and not bits.all()


@pytest.mark.parametrize("c", CAPTURE_WIDTHS)
def test_capture_data_is_not_vacuous(c):
    (v0, m0), (v1, m1) = capture_data(c)
    a, b = expect(v0, 1000, True, m0), expect(v1, 1000, True, m1)
    assert (a[0] != b[0]).any() and a[1] != b[1], "a stale result could pass"


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

class Top:
    """one engine, an uploaded column and mask (both in hostile surroundings); every run gets a guarded bitmap full of 0xEE"""

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

    def run(self, L, k, largest=True, in_place=False, what="", pre=None):
        """-> checks every bitmap byte, the guards, the result words, the inputs and the launch record; returns the record"""
        import torch

        tag = (what, self.c, self.n, k, largest)
        nbytes = (self.n + 7) // 8
        bits, res = pre or expect(self.vals, k, largest, self.qual)
        g = Guarded(nbytes)
        view = g.t[g.front: g.front + nbytes]
        mask = self.mask
        if in_place:
            view.copy_(self.mask)
            mask = view
        result = torch.full((4,), -0x1112, dtype=torch.int64, device="cuda")
        col_before = self.col.data.clone()
        mask_before = None if self.mask_buf is None else self.mask_buf.clone()
        rc = L.mi355_top_k_dev(self.eng._ctx, self.col.data.data_ptr(), self.n, self.c, None if mask is None else mask.data_ptr(), k,
                               1 if largest else 0, view.data_ptr(), result.data_ptr())
        assert rc == 0, (tag, L.mi355_last_error())
        self.eng.synchronize()
        have = g.fetch()  # asserts the guard bytes on both sides
        assert [x & 0xFFFFFFFFFFFFFFFF for x in result.tolist()] == res, (tag, result.tolist(), res)
        want = packbits(bits)
        bad = np.nonzero(have != want)[0]
        assert bad.size == 0, (tag, "byte", int(bad[0]), "of", nbytes, "have", int(have[bad[0]]), "want", int(want[bad[0]]), "wrong bytes", bad.size)
        assert torch.equal(self.col.data, col_before), (tag, "column written")
        assert mask_before is None or torch.equal(self.mask_buf, mask_before), (tag, "mask written")
        rec = record(L, self.eng)
        names = [base_name(x[0]) for x in rec]
        assert names == [HIST_KERNEL, PICK_KERNEL] * passes(self.c) + [EMIT_KERNEL, SCAN_KERNEL, TRIM_KERNEL], (tag, names)
        assert rec[0][0] == f"{HIST_KERNEL}<{self.c}>" and rec[-3][0] == f"{EMIT_KERNEL}<{self.c}>" and rec[-1][0] == f"{TRIM_KERNEL}<{self.c}>", tag
        assert rec[1] == (PICK_KERNEL, 1, 0, 0) and all(x[3] == 0 for x in rec), (tag, rec)
        return rec


@gpu
@pytest.mark.parametrize("c", range(1, 33))
def test_every_width(L, O, eng, c):
    look = Top(O, eng, c, values_of(c, N_WIDTH))
    for largest in (True, False):
        look.run(L, 257, largest)


@gpu
@pytest.mark.parametrize("c", SIZE_WIDTHS)
def test_sizes_and_tails(L, O, eng, c):
    for n in SIZES:
        Top(O, eng, c, values_of(c, n)).run(L, max(1, n // 3), True)
        Top(O, eng, c, values_of(c, n, salt=1), mask_of("random-1/2", n, salt=n)).run(L, max(1, n // 5), False)


@gpu
def test_k(L, O, eng):
    vals, qual, ks = k_cases()
    look = Top(O, eng, 9, vals, qual)
    for what, k in ks.items():
        for largest in (True, False) if not what.startswith("chunk-boundary") else (True,):
            look.run(L, k, largest, what="k = " + what)
    unmasked = Top(O, eng, 17, values_of(17, N_PAT))
    for k in (0, 1, N_PAT - 1, N_PAT, N_PAT + 1, 1 << 63, (1 << 64) - 1):
        unmasked.run(L, k, False, what="no mask")


@gpu
@pytest.mark.parametrize("case", PATTERN_CASES, ids=lambda s: f"{s[0]}-{s[1]}")
def test_value_patterns(L, O, eng, case):
    c, name = case
    vals, k, largest = pattern(name, c)
    look = Top(O, eng, c, vals)
    look.run(L, k, largest, what=name)
    look.run(L, k, not largest, what=name + ", the other way")


@gpu
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("c", MASK_WIDTHS)
def test_masks(L, O, eng, c, kind):
    n = N_PAT
    look = Top(O, eng, c, values_of(c, n, salt=3), mask_of(kind, n))
    for largest in (True, False):
        look.run(L, 257, largest, in_place=kind == "in-place", what=kind)
    if kind == "empty":
        assert expect(look.vals, 257, True, look.qual)[1] == [0, 0, 0, 0]


@gpu
@pytest.mark.parametrize("c", LONG_WIDTHS)
def test_one_block_walks_many_tiles(L, O, eng, c):
    """grid_cus = 1, max_blocks_per_cu = 1: one block per launch -- the LDS counters accumulate over the block's tiles and flush
    once, the trim's waves walk ten chunks each"""
    look = Top(O, eng, c, values_of(c, N_LONG, salt=4) % np.uint32(min(1 << c, 1000)), mask_of("random-1/2", N_LONG))
    eng.set_option("grid_cus", 1)
    eng.set_option("max_blocks_per_cu", 1)
    try:
        rec = look.run(L, N_LONG // 4, True, what="one block")
        assert all(x[1] == 1 for x in rec) and base_name(rec[0][0]) == HIST_KERNEL and base_name(rec[-1][0]) == TRIM_KERNEL
    finally:
        eng.set_option("grid_cus", 0)
        eng.set_option("max_blocks_per_cu", 0)
    assert look.run(L, N_LONG // 4, True, what="whole chip")[0][1] > 1


@gpu
def test_across_a_scan_group(L, O, eng):
    """1025 chunks and a ragged one, ties on both sides of the group boundary: the second scan group's chunks add the first group's total"""
    vals, ks, pre = group_case()
    look = Top(O, eng, 9, vals)
    for k, want in zip(ks, pre):
        look.run(L, k, True, what="scan groups", pre=want)


@gpu
@pytest.mark.parametrize("c", VIEW_WIDTHS)
def test_row_range_views(L, O, eng, c):
    """rows [lead, lead + n) of a longer column, lead a multiple of 8192, with the mask's bytes of exactly those rows inside a
    longer bitmap: nothing of the rows in front or behind reaches the result"""
    from shared_simd_scan_amd.engine import PackedColumn

    n, lead, trail = N_PAT, 8192, 4096
    vals, qual = values_of(c, n, salt=8), mask_of("random-1/2", n, salt=8)
    rng = np.random.default_rng([c, 13])
    top = (1 << c) - 1
    junk = np.full(lead, top, dtype=np.uint32)  # rows that would win every top-k
    whole = PackedColumn(plain_pack(O, np.concatenate([junk, vals, np.zeros(trail, dtype=np.uint32)]), c), lead + n + trail, c)
    col = eng.slice_rows(whole, lead, lead + n)
    assert col.n == n and col.data.data_ptr() % 16 == 0
    # the longer bitmap begins 4 bytes behind a 16-byte boundary; the view's rows begin lead / 8 bytes into it
    front = np.concatenate([np.full(4, 0xFF, dtype=np.uint8), rng.integers(0, 256, lead // 8, dtype=np.uint8)])
    mask = hostile_bitmap(qual, offset=4, front=front)
    assert mask[0].data_ptr() % 16 == 4
    look = Top(O, eng, c, vals, qual, col=col, mask=mask)
    for largest in (True, False):
        look.run(L, 1000, largest, what="view")


@gpu
def test_errors_launch_nothing(L, O, eng):
    import torch

    c, n = 9, K + 77
    vals, qual = values_of(c, n, salt=9), mask_of("random-1/2", n, salt=9)
    look = Top(O, eng, c, vals, qual)
    nb_col, nb = (n * c + 7) // 8, (n + 7) // 8
    out = Guarded(nb)
    big = Guarded(65536)  # a buffer that can stand for an input and the output at once
    res = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    cp, mp, op, rp = look.col.data.data_ptr(), look.mask.data_ptr(), out.ptr.value, res.data_ptr()

    def call(cp=cp, n=n, c=c, mp=mp, k=100, op=op, rp=rp):
        for g in (out, big):
            g.t.fill_(SENTINEL)
        res.fill_(-7)
        rc = L.mi355_top_k_dev(eng._ctx, cp, n, c, mp, k, 1, op, rp)
        eng.synchronize()
        return rc

    bits, want = expect(vals, 100, True, qual)
    assert call() == 0 and res.tolist() == want and (out.fetch() == packbits(bits)).all()
    valid = record(L, eng)
    assert [base_name(x[0]) for x in valid] == [HIST_KERNEL, PICK_KERNEL, EMIT_KERNEL, SCAN_KERNEL, TRIM_KERNEL]
    assert nb_col + 512 <= 65536
    b = big.ptr.value
    errors = (("c = 0", dict(c=0), b"32"), ("c = 33", dict(c=33), b"32"), ("null result", dict(rp=None), b"result_dev"),
              ("null bitmap", dict(op=None), b"bitmap_dev"), ("null column", dict(cp=None), b"packed_dev"),
              ("column at +4", dict(cp=cp + 4), b"aligned"), ("mask at +2", dict(mp=mp + 2), b"aligned"), ("bitmap at +2", dict(op=op + 2), b"aligned"),
              ("result at +4", dict(rp=rp + 4), b"aligned"),
              ("bitmap is the column", dict(cp=b, op=b), b"overlaps packed_dev"),
              ("bitmap starts in the column's last byte", dict(cp=b, op=b + (nb_col - 1) // 16 * 16), b"overlaps packed_dev"),
              ("column starts inside the bitmap", dict(cp=b + 256, op=b), b"overlaps packed_dev"),
              ("bitmap starts 4 bytes into the mask", dict(mp=b, op=b + 4), b"overlaps mask_dev"),
              ("bitmap starts in the mask's last byte", dict(mp=b, op=b + (nb - 1) // 4 * 4), b"overlaps mask_dev"),
              ("mask starts inside the bitmap", dict(mp=b + 64, op=b), b"overlaps mask_dev"),
              ("result inside the bitmap", dict(op=b, rp=b + 8), b"result_dev overlaps"))
    for what, kw, word in errors:
        assert call(**kw) == E_INVALID, what
        assert word in L.mi355_last_error(), (what, L.mi355_last_error())
        assert record(L, eng) == [], what  # a refused call leaves an empty record and launches nothing
        for g in (out, big):
            assert (g.fetch() == SENTINEL).all(), what
        assert res.tolist() == [-7] * 4, what
    # n == 0: the result words zeroed, nothing launched, nothing else written, and no other pointer needed
    assert call(n=0, cp=None, mp=None, op=None) == 0 and record(L, eng) == [] and res.tolist() == [0, 0, 0, 0]
    assert (out.fetch() == SENTINEL).all()
    assert call() == 0 and record(L, eng) == valid and res.tolist() == want


@gpu
def test_scan_top_k_compact(L, O, eng):
    """SELECT a, b WHERE a < 100 ORDER BY b DESC LIMIT 500: filter on a, the top 500 of b under that bitmap, compact both columns"""
    from shared_simd_scan_amd.engine import PackedColumn

    a, b = chain_data()
    n = N_PAT
    col_a, col_b = PackedColumn(plain_pack(O, a, 9), n, 9), PackedColumn(plain_pack(O, b, 17), n, 17)
    where, _ = eng.scan_where("<", 100, col_a)
    top, result = eng.top_k(col_b, 500, largest=True, mask=where)
    assert [base_name(x[0]) for x in record(L, eng)] == [HIST_KERNEL, PICK_KERNEL] * 2 + [EMIT_KERNEL, SCAN_KERNEL, TRIM_KERNEL]
    small_a, small_b = eng.compact_column(col_a, top), eng.compact_column(col_b, top)
    eng.synchronize()
    bits, res = expect(b, 500, True, a < 100)
    assert res[0] == 500 and res[3] > res[0] - res[2] > 0, "the cut does not go through ties"
    assert result.tolist() == res and (small_a.n, small_b.n) == (500, 500)
    for have, want, c in ((small_a, a[bits], 9), (small_b, b[bits], 17)):
        wb = O.pack(np.ascontiguousarray(want), c)[: (500 * c + 7) // 8]
        assert (have.data.cpu().numpy()[: len(wb)] == wb).all(), c
    # the order statistics: the k-th largest / smallest of the qualifying rows, and the median of the whole column
    sel = np.sort(b[a < 100])
    assert eng.kth_value(col_b, 500, largest=True, mask=where) == int(sel[len(sel) - 500]) == res[1]
    assert eng.kth_value(col_b, 77, largest=False, mask=where) == int(np.partition(b[a < 100], 76)[76])
    assert eng.kth_value(col_b, n // 2, largest=False) == int(np.partition(b, n // 2 - 1)[n // 2 - 1])
    with pytest.raises(ValueError):
        eng.kth_value(col_b, len(sel) + 1, mask=where)


@gpu
@pytest.mark.parametrize("c", CAPTURE_WIDTHS)
def test_graph_capture_and_replay(O, c):
    """one top_k in a graph on a side stream, after a warm-up call of the same size: after column and mask are rewritten in
    place the replay follows them"""
    import torch

    from shared_simd_scan_amd import lib

    n, k = N_PAT, 1000
    versions = capture_data(c)
    nb = (n + 7) // 8

    def steps(eng):
        stage = [(plain_pack(O, v, c), torch.from_numpy(packbits(m)).cuda()) for v, m in versions]
        col, mask = torch.empty_like(stage[0][0]), torch.empty_like(stage[0][1])
        out = Guarded(nb)
        res = torch.empty(4, dtype=torch.int64, device="cuda")

        def load(r):
            col.copy_(stage[r][0])
            mask.copy_(stage[r][1])
            out.t.fill_(SENTINEL)
            res.fill_(-7)

        def run():
            rc = lib().mi355_top_k_dev(eng._ctx, col.data_ptr(), n, c, mask.data_ptr(), k, 1, out.ptr, res.data_ptr())
            assert rc == 0, lib().mi355_last_error()

        def check(r, what):
            bits, want = expect(versions[r][0], k, True, versions[r][1])
            assert res.tolist() == want, what
            assert (out.fetch() == packbits(bits)).all(), what

        def untouched():
            assert (out.fetch() == SENTINEL).all() and res.tolist() == [-7] * 4

        def warmed(launched):
            assert [base_name(x[0]) for x in launched] == [HIST_KERNEL, PICK_KERNEL] * passes(c) + [EMIT_KERNEL, SCAN_KERNEL, TRIM_KERNEL]

        return capture.Steps(load, run, check, untouched, warmed)

    capture.capture_replay(steps, (0, 1, 0))


@gpu
def test_capture_refuses_to_grow_the_workspace(O):
    """a fresh context that has seen a small column only: under capture a larger one is refused (MI355_E_INVALID, the message
    names graph capture), nothing is enqueued for it and the capture stays intact -- the small call around it replays"""
    import torch

    from shared_simd_scan_amd import lib

    c, small_n, big_n, k = 9, K + 77, 40 * K, 100
    vals = values_of(c, small_n, salt=9)

    def setup(eng):
        col, big_col = plain_pack(O, vals, c), plain_pack(O, values_of(c, big_n), c)
        out, refused = Guarded((small_n + 7) // 8), Guarded((big_n + 7) // 8)
        res = torch.full((8,), -7, dtype=torch.int64, device="cuda")

        def small():
            assert lib().mi355_top_k_dev(eng._ctx, col.data_ptr(), small_n, c, None, k, 1, out.ptr, res.data_ptr()) == 0

        def big():
            return lib().mi355_top_k_dev(eng._ctx, big_col.data_ptr(), big_n, c, None, k, 1, refused.ptr, res.data_ptr() + 32)

        def reset():
            out.t.fill_(SENTINEL)
            res.fill_(-7)

        def check_small():
            bits, want = expect(vals, k, True)
            assert res.tolist() == want + [-7] * 4 and (out.fetch() == packbits(bits)).all()

        return small, big, reset, check_small, refused

    capture.refused_under_capture(setup)
