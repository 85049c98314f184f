"""The rows a bitmap selects, as a packed column (include/mi355_compact.h, ScanEngine.compact / compact_column).

CPU: the header is plain C99 and declares exactly what _capi.HEADERS binds for it and the library exports; it carries its
graph-capture verdict; mi355_compact_kernel (pure arithmetic) answers for c = 1..32; compact and compact_column hand the C ABI
what they should (through a recording stand-in for the library); without a device the entry point fails with a message; every
__global__ under csrc/compact/ is named by the launch record of a GPU case of this file; no source there reads a switch bit; the
data recipe is not vacuous.

GPU (-m gpu): every expectation is numpy on the values and the bitmap the test generated --
vals[np.unpackbits(bitmap, bitorder="little")[:n].astype(bool)], cut at the capacity and packed with the oracle's packer; the
count is int(bits.sum()); nothing is derived from engine output.  Every one of the ceil(m c / 8) payload bytes (trailing bits of
the last one included) and the 0xEE guard bytes on both sides of the output (support.Guarded) are compared exactly --
the guard behind the payload begins at the very next byte --; column and bitmap must be unchanged after the call.  Every case
runs in hostile surroundings: ones in the column's bits behind row n - 1 and in its pad, 0xFF bytes directly behind byte
ceil(n / 8) of the bitmap.  A tile is R = 2048 rows, a chunk K = 16384 rows (one wave's work), a scan group 1024 chunks.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import capture
import support
from support import E_INVALID, SENTINEL, Guarded, L, base_name, eng, fake, hostile_bitmap, hostile_pack, packbits, plain_pack, record  # noqa: F401  (L, eng, fake: fixtures)

HEADER = "mi355_compact.h"

# the kernels of csrc/compact/, as the launch record names them: the GPU cases below assert these labels
EDGES_KERNEL = "compact_edges_kernel"
COMPACT_KERNEL = "compact_kernel"
PREFIX_KERNELS = ["rowid_count_kernel", "rowid_scan_kernel"]  # kernels/bitmap.hpp, launched in front of them

R = 2048  # rows per tile: 64 lanes x 32 rows
K = 16384  # rows per chunk: 8 tiles
GROUP = 1024  # chunks per scan group

N_BIG = 5 * K + 1237
N_WIDTH = 2 * K + 1237
N_SPARSE = 80 * K
N_LONG = 40 * K + 1237
N_GROUPS = (GROUP + 1) * K + 1237
SIZES = [1, 13, 31, 32, 33, R - 1, R, R + 1, K - 1, K, K + 1, N_BIG]
SIZE_WIDTHS = [9, 17, 32, 1]
PATTERNS = ["zeros", "ones", "first", "last", "alternating", "random-1/512", "random-1/8", "random-0.97", "clustered"]
PATTERN_WIDTHS = [9, 17]
SPARSE_WIDTHS = [1, 3]
LONG_WIDTHS = [9, 24]
CAPACITY_WIDTHS = [9, 17]
VIEW_WIDTHS = [9, 17]
CAPTURE_WIDTHS = [9, 17]

gpu = pytest.mark.gpu


def payload(n, c):
    return (n * c + 7) // 8


def dword_bytes(n, c):
    """what the call may write of `n` values: whole dwords"""
    return (n * c + 31) // 32 * 4


# differs from test_top_k's and test_sort_rows' values_of in the seed only ([c, n, salt], theirs end in 7 and 17): the "not vacuous" tests pin each file's data
@functools.lru_cache(maxsize=None)
def values_of(c, n, salt=0):
    rng = np.random.default_rng([c, n, salt])
    vals = rng.integers(0, 1 << c, n, dtype=np.uint64).astype(np.uint32)
    vals.setflags(write=False)
    return vals


@functools.lru_cache(maxsize=None)
def bits_of(pattern, n, salt=0):
    """the selection as a bool array of n rows"""
    rng = np.random.default_rng([n, salt, len(pattern)])
    bits = np.zeros(n, dtype=bool)
    if pattern == "ones":
        bits[:] = True
    elif pattern == "first":
        bits[0] = True
    elif pattern == "last":
        bits[n - 1] = True
    elif pattern == "alternating":
        bits[::2] = True
    elif pattern.startswith("random-"):
        num, _, den = pattern[7:].partition("/")
        bits = rng.random(n) < (float(num) / float(den) if den else float(num))
    elif pattern == "clustered":
        # chunk 0 full, chunk 1 empty, chunk 2: only tiles 1 and 6 (one full, one random), chunk 3 empty, the rest random 1/8
        bits[:K] = True
        bits[2 * K + R: 2 * K + 2 * R] = True
        bits[2 * K + 6 * R: 2 * K + 7 * R] = rng.random(R) < 0.5
        bits[4 * K:] = rng.random(n - 4 * K) < 0.125
    elif pattern == "one-per-chunk":
        for ch in range((n + K - 1) // K):
            bits[min(ch * K + int(rng.integers(0, K)), n - 1)] = True
    else:
        assert pattern == "zeros", pattern
    bits.setflags(write=False)
    return bits


def expect(vals, bits, capacity=None):
    """-> (the values the call writes, the count it reports)"""
    want = vals[bits]
    return (want if capacity is None else want[:capacity]), int(bits.sum())


def shapes():
    """every (c, n, pattern) the GPU cases below run on recipe data"""
    s = {(c, n, "random-1/2") for c in SIZE_WIDTHS for n in SIZES}
    s |= {(c, N_WIDTH, "random-1/3") for c in range(1, 33)}
    s |= {(c, N_BIG, p) for c in PATTERN_WIDTHS for p in PATTERNS}
    s |= {(c, N_SPARSE, "one-per-chunk") for c in SPARSE_WIDTHS}
    s |= {(c, N_LONG, "random-1/2") for c in LONG_WIDTHS}
    s |= {(9, N_GROUPS, "random-1/8")}
    s |= {(c, N_BIG, "random-1/2") for c in CAPACITY_WIDTHS + VIEW_WIDTHS}
    return sorted(s)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------

def test_compact_header_is_plain_c99():
    support.check_header_is_plain_c99(HEADER)


def test_compact_header_declares_what_python_binds(L):
    names, sigs = support.check_header_binds(L, HEADER)
    assert names == ["mi355_compact_dev", "mi355_compact_kernel"]
    sig = sigs["mi355_compact_dev"]
    assert sig[2] is C.c_uint64 and sig[3] is C.c_uint and sig[6] is C.c_uint64 and len(sig) == 8
    assert sigs["mi355_compact_kernel"] == [C.c_uint] and L.mi355_compact_kernel.restype is C.c_char_p
    text = support.header_text(HEADER)
    assert '#include "mi355_scan.h"' in text and text.count("#include") == 1


def test_compact_header_carries_its_capture_verdict():
    support.check_capture_verdict(HEADER, r"capturable after a warm-up call", r"read at every replay")


def test_compact_kernel_answers_for_every_width(L):
    """mi355_compact_kernel needs neither a device nor a context"""
    from shared_simd_scan_amd import compact_kernel

    for c in range(1, 33):
        assert L.mi355_compact_kernel(c) == COMPACT_KERNEL.encode() and compact_kernel(c) == COMPACT_KERNEL
    assert L.mi355_compact_kernel(0) is None and L.mi355_compact_kernel(33) is None
    for bad in (0, 33, -1, 1 << 32):
        with pytest.raises(ValueError):
            compact_kernel(bad)


def test_compact_wrapper_passes_what_the_abi_takes(fake, L, monkeypatch):
    import torch

    eng, rec, col = fake
    fact = col(17, 777)
    bitmap = torch.zeros(98, dtype=torch.uint8)  # ceil(777 / 8)
    out, count = eng.compact(fact, bitmap)  # defaults: capacity col.n, a fresh buffer that a consumer can take as a column
    (name, a), = rec.calls
    assert name == "mi355_compact_dev" and a[1:5] == [fact.data.data_ptr(), 777, 17, bitmap.data_ptr()] and a[6] == 777
    assert out.dtype == torch.uint8 and out.numel() == L.mi355_compressed_buffer_size(17, 777) and a[5] == out.data_ptr()
    assert count.dtype == torch.int64 and count.numel() == 1 and a[7] == count.data_ptr()
    rec.calls.clear()
    mine = torch.zeros(216, dtype=torch.uint8)  # 100 values of 17 bits in whole dwords: ceil(1700 / 32) * 4
    out, count = eng.compact(fact, bitmap, capacity=100, out=mine)
    (name, a), = rec.calls
    assert out is mine and a[1:7] == [fact.data.data_ptr(), 777, 17, bitmap.data_ptr(), mine.data_ptr(), 100]
    rec.calls.clear()
    eng.compact(fact, bitmap, capacity=0)  # count-only: no output pointer at all
    assert rec.calls[0][1][5:7] == [None, 0]
    rec.calls.clear()
    with pytest.raises(AssertionError):
        eng.compact(fact, bitmap, capacity=100, out=torch.zeros(215, dtype=torch.uint8))  # a byte short
    with pytest.raises(AssertionError):
        eng.compact(fact, bitmap, out=torch.zeros(216, dtype=torch.uint8))  # fits 100 values, not the default 777
    with pytest.raises(AssertionError):
        eng.compact(fact, bitmap, capacity=100, out=torch.zeros(216, dtype=torch.int8))
    with pytest.raises(AssertionError):
        eng.compact(fact, torch.zeros(97, dtype=torch.uint8))  # a bitmap shorter than the column
    assert rec.calls == []
    # compact_column: one compact at full capacity, then the count read on the host is the new column's row count
    zeros = torch.zeros
    monkeypatch.setattr(torch, "empty", lambda size, **kw: zeros(size, **kw) + 5 if kw.get("dtype") is torch.int64 else zeros(size, **kw))
    res = eng.compact_column(fact, bitmap)
    (name, a), = rec.calls
    assert name == "mi355_compact_dev" and a[6] == 777 and a[5] == res.data.data_ptr() and (res.n, res.c) == (5, 17)


def test_compact_entry_point_fails_loudly_without_a_gpu(L):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    buf, bm, out = (C.c_uint8 * 1024)(), (C.c_uint8 * 1024)(), (C.c_uint8 * 1024)()
    cnt = C.c_uint64(0)
    rc = L.mi355_compact_dev(None, buf, 100, 9, bm, out, 100, C.byref(cnt))
    assert rc != 0 and L.mi355_last_error()


def test_every_compact_kernel_has_a_case():
    """every __global__ under csrc/compact/ is asserted from the launch record by a GPU case of this file, and the file names no
    kernel that does not exist"""
    kernels = support.global_kernels_of("compact")
    assert kernels == {EDGES_KERNEL, COMPACT_KERNEL}, kernels
    support.check_gpu_part_asserts(__file__, "EDGES_KERNEL", "COMPACT_KERNEL")


def test_compact_sources_read_no_flag_bits():
    assert [os.path.basename(p) for p in support.feature_sources("compact")] == ["compact.hip", "compact.hpp"]
    support.check_sources_read_no_flag_bits("compact")


@pytest.mark.parametrize("shape", [s for s in shapes() if s[2].startswith("random") and s[1] >= 33], ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
def test_random_bitmaps_are_not_vacuous(shape):
    """(no device needed) at every size with >= 33 rows the random bitmaps have both set and clear bits, and the selected values
    are not all alike"""
    c, n, pattern = shape
    bits = bits_of(pattern, n)
    vals = values_of(c, n)
    assert bits.any() and not bits.all() and len(bits) == n == len(vals)
    want, count = expect(vals, bits)
    assert count == len(want) and (c == 1 or n < 64 or len(np.unique(want)) >= 2)
    assert (np.unpackbits(packbits(bits), bitorder="little")[:n].astype(bool) == bits).all()
    assert (packbits(bits)[-1] >> ((n - 1) % 8 + 1)) == 0, "the recipe's bitmap is not canonical"


def test_patterns_reach_what_they_name():
    n = N_BIG
    assert not bits_of("zeros", n).any() and bits_of("ones", n).all()
    assert list(np.nonzero(bits_of("first", n))[0]) == [0] and list(np.nonzero(bits_of("last", n))[0]) == [n - 1]
    assert bits_of("alternating", n)[:4].tolist() == [True, False, True, False]
    assert 0 < bits_of("random-1/512", n).sum() < n // 256 and bits_of("random-0.97", n).sum() > 0.95 * n
    cl = bits_of("clustered", n)
    per_chunk = [int(cl[k * K: (k + 1) * K].sum()) for k in range(6)]
    assert per_chunk[0] == K and per_chunk[1] == 0 and per_chunk[3] == 0 and 0 < per_chunk[4] < K, per_chunk
    per_tile = [int(cl[2 * K + t * R: 2 * K + (t + 1) * R].sum()) for t in range(8)]
    assert per_tile[1] == R and 0 < per_tile[6] < R and sum(per_tile) == per_tile[1] + per_tile[6], per_tile


def test_sparse_pattern_shares_dwords_between_many_chunks():
    """one set bit per chunk at a varying row: at c = 1 every output dword is filled by 32 different chunks (a dword holds 32
    one-bit values, so 32 is the most there can be), at c = 3 by 11 or 12"""
    bits = bits_of("one-per-chunk", N_SPARSE)
    rows = np.nonzero(bits)[0]
    assert len(rows) == N_SPARSE // K == 80 and (rows // K == np.arange(80)).all()
    assert len(set(rows % K)) > 40, "the row inside the chunk does not vary"
    for c, most in ((1, 32), (3, 12)):
        dwords = [set() for _ in range(payload(80, c) // 4 + 1)]
        for i, row in enumerate(rows):
            for bit in (i * c, i * c + c - 1):
                dwords[bit // 32].add(int(row // K))
        assert max(len(d) for d in dwords) == most and most >= (32 if c == 1 else 11), (c, [len(d) for d in dwords])


@functools.lru_cache(maxsize=None)
def chain_data():
    """two fact columns (9 and 17 bits) and a 12-bit key column with its 6-bit dimension attribute, read-only"""
    rng = np.random.default_rng(2026)
    a = rng.integers(0, 1 << 9, N_BIG, dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 1 << 17, N_BIG, dtype=np.uint64).astype(np.uint32)
    b[::3] = a[::3]  # rows where the two columns compare equal
    fk = rng.integers(0, 1 << 12, N_BIG, dtype=np.uint64).astype(np.uint32)
    attr = rng.integers(0, 64, 3001, dtype=np.uint64).astype(np.uint32)
    for x in (a, b, fk, attr):
        x.setflags(write=False)
    return a, b, fk, attr


def test_chain_data_is_not_vacuous():
    a, b, fk, attr = chain_data()
    sel = a < 100
    assert sel.any() and not sel.all()
    lt = a[sel].astype(np.int64) < b[sel].astype(np.int64)
    assert lt.any() and not lt.all()
    assert (fk[sel] >= 3001).any() and (fk[sel] < 3001).any()


@functools.lru_cache(maxsize=None)
def capture_data(c):
    """two versions of a column and of a bitmap over N_BIG rows whose compacted images and counts differ"""
    out = []
    for r in range(2):
        out.append((values_of(c, N_BIG, salt=50 + r), bits_of("random-1/3" if r == 0 else "random-1/8", N_BIG, salt=60 + r)))
    return out


@pytest.mark.parametrize("c", CAPTURE_WIDTHS)
def test_capture_data_is_not_vacuous(c):
    (v0, b0), (v1, b1) = capture_data(c)
    assert b0.sum() != b1.sum() and (v0 != v1).any(), "a stale result could pass"


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

def want_record(c, writes=True):
    return PREFIX_KERNELS + [EDGES_KERNEL] + ([COMPACT_KERNEL] if writes else [])


class Comp:
    """one engine, an uploaded column and bitmap (both in hostile surroundings); every run gets a guarded output full of 0xEE"""

    def __init__(self, O, eng, c, n, bits, vals=None, col=None, bitmap=None):
        from shared_simd_scan_amd.engine import PackedColumn

        self.O, self.eng, self.c, self.n, self.bits = O, eng, c, n, bits
        self.vals = values_of(c, n) if vals is None else vals
        self.col = PackedColumn(hostile_pack(O, self.vals, c), n, c) if col is None else col
        self.bitmap, self.bitmap_buf = hostile_bitmap(bits) if bitmap is None else bitmap

    def image(self, want):
        return self.O.pack(np.ascontiguousarray(want, dtype=np.uint32), self.c)[: payload(len(want), self.c)] if len(want) else np.zeros(0, dtype=np.uint8)

    def run(self, L, capacity=None, what=""):
        """-> checks every payload byte, the trailing bits, the guards (the one behind begins right behind the payload), the count,
        the inputs and the launch record; returns the record"""
        import torch

        cap = self.n if capacity is None else capacity
        tag = (what, self.c, self.n, cap)
        want, count = expect(self.vals, self.bits, cap)
        m = len(want)
        assert m == min(count, cap)
        wb = self.image(want)
        g = Guarded(payload(m, self.c), back=max(4096, dword_bytes(cap, self.c) + 64))
        view = g.t[g.front: g.front + max(dword_bytes(cap, self.c), 4)]  # writable in whole dwords, as the contract asks
        col_before, bitmap_before = self.col.data.clone(), self.bitmap_buf.clone()
        out, cnt = self.eng.compact(self.col, self.bitmap, capacity=capacity, out=view)
        self.eng.synchronize()
        have = g.fetch()  # asserts the guard bytes on both sides
        assert out.data_ptr() == view.data_ptr() and int(cnt.item()) == count, (tag, int(cnt.item()), count)
        bad = np.nonzero(have != wb)[0]
        assert bad.size == 0, (tag, "byte", int(bad[0]), "of", len(wb), "have", int(have[bad[0]]), "want", int(wb[bad[0]]))
        if (m * self.c) % 8:
            assert int(have[-1]) >> ((m * self.c) % 8) == 0, (tag, "bits behind the last value are not zero")
        assert torch.equal(self.col.data, col_before), (tag, "column written")
        assert torch.equal(self.bitmap_buf, bitmap_before), (tag, "bitmap written")
        rec = record(L, self.eng)
        names = [base_name(x[0]) for x in rec]
        assert names == PREFIX_KERNELS + [EDGES_KERNEL] + [COMPACT_KERNEL] * (cap > 0), (tag, names)
        if cap > 0:
            label, grid, lds, flags = rec[-1]
            assert label == f"{COMPACT_KERNEL}<{self.c}>" and L.mi355_compact_kernel(self.c) == COMPACT_KERNEL.encode(), (tag, label)
            assert flags == 0 and lds >= 4 * (2 * 256 * self.c + 256 * self.c) and grid >= 1, (tag, lds)
        return rec


def comp(O, eng, c, n, pattern):
    return Comp(O, eng, c, n, bits_of(pattern, n))


@gpu
@pytest.mark.parametrize("c", SIZE_WIDTHS)
def test_sizes_and_tails(L, O, eng, c):
    for n in SIZES:
        comp(O, eng, c, n, "random-1/2").run(L)


@gpu
@pytest.mark.parametrize("c", range(1, 33))
def test_every_width(L, O, eng, c):
    rec = comp(O, eng, c, N_WIDTH, "random-1/3").run(L)
    assert rec[-1][0] == f"{COMPACT_KERNEL}<{c}>"


@gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("c", PATTERN_WIDTHS)
def test_densities_and_patterns(L, O, eng, c, pattern):
    n = N_BIG
    look = comp(O, eng, c, n, pattern)
    look.run(L, what=pattern)
    if pattern == "ones":  # the identity: the output's payload is the input's, trailing bits zeroed
        want, count = expect(look.vals, look.bits)
        assert count == n and (look.image(want) == O.pack(look.vals, c)[: payload(n, c)]).all()
    if pattern == "zeros":
        assert expect(look.vals, look.bits)[1] == 0


@gpu
@pytest.mark.parametrize("c", SPARSE_WIDTHS)
def test_many_chunks_in_one_dword(L, O, eng, c):
    comp(O, eng, c, N_SPARSE, "one-per-chunk").run(L)


@gpu
@pytest.mark.parametrize("c", LONG_WIDTHS)
def test_one_block_walks_many_chunks(L, O, eng, c):
    """grid_cus = 1, max_blocks_per_cu = 1: one block, its four waves walk ten chunks each -- the stage's carry across tiles and
    chunks, the alternating images"""
    look = comp(O, eng, c, N_LONG, "random-1/2")
    eng.set_option("grid_cus", 1)
    eng.set_option("max_blocks_per_cu", 1)
    try:
        rec = look.run(L, what="one block")
        assert rec[-1][1] == 1 and base_name(rec[-1][0]) == COMPACT_KERNEL
    finally:
        eng.set_option("grid_cus", 0)
        eng.set_option("max_blocks_per_cu", 0)
    assert look.run(L, what="whole chip")[-1][1] > 1


@gpu
def test_across_a_scan_group(L, O, eng):
    """1025 chunks and a ragged one: the second scan group's chunks add the first group's total"""
    comp(O, eng, 9, N_GROUPS, "random-1/8").run(L)


@gpu
@pytest.mark.parametrize("c", CAPACITY_WIDTHS)
def test_capacity(L, O, eng, c):
    import torch

    from shared_simd_scan_amd import lib

    look = comp(O, eng, c, N_BIG, "random-1/2")
    count = int(look.bits.sum())
    for cap in (0, 1, 31, 32, 33, count - 1, count, count + 1):
        look.run(L, capacity=cap, what=f"capacity {cap}")
    # capacity == 0 with no output pointer at all: the count alone
    cnt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    rc = lib().mi355_compact_dev(eng._ctx, look.col.data.data_ptr(), look.n, c, look.bitmap.data_ptr(), None, 0, cnt.data_ptr())
    eng.synchronize()
    assert rc == 0 and int(cnt.item()) == count
    assert [base_name(x[0]) for x in record(L, eng)] == PREFIX_KERNELS + [EDGES_KERNEL]


@gpu
@pytest.mark.parametrize("c", VIEW_WIDTHS)
def test_row_range_views(L, O, eng, c):
    """rows [lead, lead + n) of a longer column with the bitmap's bytes of exactly those rows, at an address that is a multiple
    of 4 and not of 16: nothing of the rows in front or behind reaches the result"""
    from shared_simd_scan_amd.engine import PackedColumn

    n, lead, trail = N_BIG, 2 * R + 128, 4096
    vals, bits = values_of(c, n), bits_of("random-1/2", n)
    rng = np.random.default_rng([c, 13])
    top = (1 << c) - 1
    junk = rng.integers(0, top + 1, lead, dtype=np.uint64).astype(np.uint32)
    whole = PackedColumn(plain_pack(O, np.concatenate([junk, vals, np.full(trail, top, dtype=np.uint32)]), c), lead + n + trail, c)
    col = eng.slice_rows(whole, lead, lead + n)
    assert col.n == n and col.data.data_ptr() % 16 == 0
    # the longer bitmap begins 4 bytes behind a 16-byte boundary; the view's rows begin lead / 8 bytes into it
    front = np.concatenate([np.full(4, 0xFF, dtype=np.uint8), rng.integers(0, 256, lead // 8, dtype=np.uint8)])
    bitmap = hostile_bitmap(bits, offset=4, front=front)
    assert bitmap[0].data_ptr() % 4 == 0 and bitmap[0].data_ptr() % 16 == 4
    Comp(O, eng, c, n, bits, vals=vals, col=col, bitmap=bitmap).run(L, what="view")


@gpu
def test_errors_launch_nothing(L, O, eng):
    import torch

    c, n = 9, K + 77
    look = comp(O, eng, c, n, "random-1/2")
    count = int(look.bits.sum())
    out = Guarded(payload(n, c))
    big = Guarded(65536)  # a buffer that can stand for an input and the output at once
    cnt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    cp, bp, op, kp = look.col.data.data_ptr(), look.bitmap.data_ptr(), out.ptr.value, cnt.data_ptr()

    def call(cp=cp, n=n, c=c, bp=bp, op=op, cap=n, kp=kp):
        for g in (out, big):
            g.t.fill_(SENTINEL)
        cnt.fill_(-1)
        rc = L.mi355_compact_dev(eng._ctx, cp, n, c, bp, op, cap, kp)
        eng.synchronize()
        return rc

    assert call() == 0 and int(cnt.item()) == count
    valid = record(L, eng)
    assert [base_name(x[0]) for x in valid] == PREFIX_KERNELS + [EDGES_KERNEL, COMPACT_KERNEL]
    nb_col, nb_bm = payload(n, c), (n + 7) // 8
    assert nb_col + 512 <= 65536
    b = big.ptr.value
    errors = (("c = 0", dict(c=0), b"32"), ("c = 33", dict(c=33), b"32"), ("null count", dict(kp=None), b"count_dev"),
              ("null column", dict(cp=None), b"packed_dev"), ("null bitmap", dict(bp=None), b"bitmap_dev"), ("null output", dict(op=None), b"out_dev"),
              ("column at +4", dict(cp=cp + 4), b"aligned"), ("output at +4", dict(op=op + 4), b"aligned"), ("bitmap at +2", dict(bp=bp + 2), b"aligned"),
              ("output is the column", dict(cp=b, op=b), b"overlaps packed_dev"),
              ("output starts in the column's last byte", dict(cp=b, op=b + (nb_col - 1) // 16 * 16), b"overlaps packed_dev"),
              ("column starts inside the output", dict(cp=b + 256, op=b), b"overlaps packed_dev"),
              ("output is the bitmap", dict(bp=b, op=b), b"overlaps bitmap_dev"),
              ("output starts in the bitmap's last byte", dict(bp=b, op=b + (nb_bm - 1) // 16 * 16), b"overlaps bitmap_dev"),
              ("bitmap starts inside the output", dict(bp=b + 64, op=b), b"overlaps bitmap_dev"))
    for what, kw, word in errors:
        assert call(**kw) == E_INVALID, what
        assert word in L.mi355_last_error(), (what, L.mi355_last_error())
        assert record(L, eng) == [], what  # a refused call leaves an empty record and launches nothing
        for g in (out, big):
            assert (g.fetch() == SENTINEL).all(), what
        assert int(cnt.item()) == -1, what
    # n == 0: count 0, nothing launched, nothing written, and neither column nor bitmap needed
    assert call(n=0, cp=None, bp=None) == 0 and record(L, eng) == [] and int(cnt.item()) == 0
    assert (out.fetch() == SENTINEL).all()
    assert call() == 0 and record(L, eng) == valid and int(cnt.item()) == count


@gpu
def test_scan_compact_scan_columns(L, O, eng):
    """SELECT ... WHERE a < 100 AND a < b: filter on a, compact a and b with the one bitmap, compare the compacted pair"""
    from shared_simd_scan_amd.engine import PackedColumn

    a, b, fk, attr = chain_data()
    n = N_BIG
    col_a, col_b = PackedColumn(plain_pack(O, a, 9), n, 9), PackedColumn(plain_pack(O, b, 17), n, 17)
    bitmap, hits = eng.scan_where("<", 100, col_a)
    small_a, small_b = eng.compact_column(col_a, bitmap), eng.compact_column(col_b, bitmap)
    assert base_name(record(L, eng)[-1][0]) == COMPACT_KERNEL
    sel = a < 100
    m = int(sel.sum())
    assert (small_a.n, small_a.c, small_b.n, small_b.c) == (m, 9, m, 17) and int(hits.item()) == m
    for op, want in (("<", a[sel].astype(np.int64) < b[sel]), ("==", a[sel] == b[sel])):
        got, got_hits = eng.scan_columns(small_a, op, small_b)
        eng.synchronize()
        assert want.any() and not want.all()
        assert (got.cpu().numpy()[: (m + 7) // 8] == packbits(want)).all() and int(got_hits.item()) == int(want.sum()), op


@gpu
def test_compact_and_lookup_commute(L, O, eng):
    """compact_column -> lookup equals lookup -> compact_column, and both equal numpy"""
    from shared_simd_scan_amd.engine import PackedColumn

    a, b, fk, attr = chain_data()
    n, T = N_BIG, len(attr)
    col_a, col_fk, dim = PackedColumn(plain_pack(O, a, 9), n, 9), PackedColumn(plain_pack(O, fk, 12), n, 12), PackedColumn(plain_pack(O, attr, 6), T, 6)
    bitmap, _ = eng.scan_where("<", 100, col_a)
    one = eng.lookup(eng.compact_column(col_fk, bitmap), dim, miss=63)
    two = eng.compact_column(eng.lookup(col_fk, dim, miss=63), bitmap)
    assert base_name(record(L, eng)[-1][0]) == COMPACT_KERNEL
    eng.synchronize()
    sel = a < 100
    m = int(sel.sum())
    f = fk[sel].astype(np.int64)
    want = np.where(f < T, attr[np.minimum(f, T - 1)], 63).astype(np.uint32)
    wb = O.pack(want, 6)[: payload(m, 6)]
    assert (one.n, one.c, two.n, two.c) == (m, 6, m, 6)
    assert (one.data.cpu().numpy()[: len(wb)] == wb).all() and (two.data.cpu().numpy()[: len(wb)] == wb).all()


@gpu
@pytest.mark.parametrize("c", CAPTURE_WIDTHS)
def test_graph_capture_and_replay(O, c):
    """one compact in a graph on a side stream, after a warm-up call of the same size: after column and bitmap are rewritten in
    place the replay follows them"""
    import torch

    from shared_simd_scan_amd import lib
    from shared_simd_scan_amd.engine import PackedColumn

    n = N_BIG
    versions = capture_data(c)

    def steps(eng):
        stage = [(plain_pack(O, v, c), torch.from_numpy(packbits(b)).cuda()) for v, b in versions]
        col = PackedColumn(torch.empty_like(stage[0][0]), n, c)
        bitmap = torch.empty_like(stage[0][1])
        out = Guarded(dword_bytes(n, c), back=4096)
        view = out.t[out.front: out.front + out.nbytes]
        cnt = torch.empty(1, dtype=torch.int64, device="cuda")

        def load(r):
            col.data.copy_(stage[r][0])
            bitmap.copy_(stage[r][1])
            out.t.fill_(SENTINEL)
            cnt.fill_(-7)

        def run():
            rc = lib().mi355_compact_dev(eng._ctx, col.data.data_ptr(), n, c, bitmap.data_ptr(), view.data_ptr(), n, cnt.data_ptr())
            assert rc == 0, lib().mi355_last_error()

        def check(r, what):
            want, count = expect(*versions[r])
            wb = O.pack(np.ascontiguousarray(want), c)[: payload(count, c)]
            have = out.fetch()
            assert int(cnt.item()) == count, what
            assert (have[: len(wb)] == wb).all() and (have[len(wb):] == SENTINEL).all(), what

        def untouched():
            assert (out.fetch() == SENTINEL).all() and int(cnt.item()) == -7

        def warmed(launched):
            assert [base_name(x[0]) for x in launched] == PREFIX_KERNELS + [EDGES_KERNEL, COMPACT_KERNEL]

        return capture.Steps(load, run, check, untouched, warmed)

    capture.capture_replay(steps, (0, 1, 0))


@gpu
def test_capture_refuses_to_grow_the_workspace(O):
    """a fresh context that has seen a small column only: under capture a larger one is refused (MI355_E_INVALID, the message
    names graph capture), nothing is enqueued for it and the capture stays intact -- the small call around it replays"""
    import torch

    from shared_simd_scan_amd import lib
    from shared_simd_scan_amd.engine import PackedColumn

    c, small_n, big_n = 9, K + 77, 40 * K
    vals, bits = values_of(c, small_n), bits_of("random-1/2", small_n)

    def setup(eng):
        col, bitmap = PackedColumn(plain_pack(O, vals, c), small_n, c), torch.from_numpy(packbits(bits)).cuda()
        big_col = PackedColumn(plain_pack(O, values_of(c, big_n), c), big_n, c)
        big_bitmap = torch.from_numpy(packbits(bits_of("random-1/2", big_n))).cuda()
        out, refused = Guarded(dword_bytes(small_n, c)), Guarded(dword_bytes(big_n, c))
        cnt = torch.full((2,), -7, dtype=torch.int64, device="cuda")

        def small():
            assert lib().mi355_compact_dev(eng._ctx, col.data.data_ptr(), small_n, c, bitmap.data_ptr(), out.ptr, small_n, cnt.data_ptr()) == 0

        def big():
            return lib().mi355_compact_dev(eng._ctx, big_col.data.data_ptr(), big_n, c, big_bitmap.data_ptr(), refused.ptr, big_n, cnt.data_ptr() + 8)

        def reset():
            out.t.fill_(SENTINEL)
            cnt.fill_(-7)

        def check_small():
            want, count = expect(vals, bits)
            wb = O.pack(np.ascontiguousarray(want), c)[: payload(count, c)]
            assert cnt.tolist() == [count, -7] and (out.fetch()[: len(wb)] == wb).all()

        return small, big, reset, check_small, refused

    capture.refused_under_capture(setup)
