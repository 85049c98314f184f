"""The runs of a packed column, and back (include/mi355_runs.h, ScanEngine.run_encode / run_decode): row i is a tail when
i == n - 1 or x_i != x_{i+1}; run j ends at the j-th tail, its value is that row's and its end the row behind it.  run_decode gives
out_i = values[j(i)] with j(i) the number of ends <= i, `miss` behind the last run.

CPU: the header is plain C99 and declares exactly what _capi.HEADERS binds for it; it carries both graph-capture verdicts; the
kernel-name functions answer on both sides of every refusal; the workspace formula; the n <= 2^ce - 1 rule; the engine wrappers hand
the C ABI what they should (through a recording stand-in for the library); every __global__ under csrc/runs/ is asserted from the
launch record by a GPU case of this file; no source there reads a switch bit or reaches the context's workspace or scratch; the
data recipes are not vacuous.

GPU (-m gpu): every expectation is numpy on data the test generated (np.nonzero of the neighbours' inequality, np.searchsorted),
packed with the oracle's packer; nothing is derived from engine output.  Outputs, count words and the workspace sit in
support.Guarded buffers full of SENTINEL; payload bytes and both guards are compared exactly.  Columns and tables are uploaded in
hostile surroundings: ones in the bits behind the last row and in the pad.

A lane owns 32 rows, a tile is 2048, a chunk (one word of the workspace) 16384, a scan group 1024 chunks: the sizes are the smallest
on both sides of each.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import capture
import support
from support import E_INVALID, SENTINEL, Guarded, L, base_name, eng, fake, hostile_pack, plain_pack, record  # noqa: F401  (L, eng, fake: fixtures)

HEADER = "mi355_runs.h"

# the kernels of a call, as the launch record names them
COUNT_KERNEL = "run_count_kernel"
EMIT_KERNEL = "run_emit_kernel"
DECODE_KERNEL = "run_decode_kernel"
SCAN_KERNEL = "rowid_scan_kernel"      # kernels/bitmap.hpp, as it stands
EDGES_KERNEL = "compact_edges_kernel"  # compact/compact.hpp, as it stands

LANE, R, CHUNK, GROUP = 32, 2048, 16384, 1024
N_BIG = 9 * 8192 + 1237          # five chunks, the last ragged in tile, lane and byte
N_GROUPS = 1025 * CHUNK + 77     # a second scan group
N_CROSS = CHUNK + R + 100        # the crossings' case: a chunk boundary, tile and lane boundaries
N_ONE_BLOCK = 9 * CHUNK + 123    # ten chunks for the four waves of a one-block grid
SIZES = [1, 7, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 16383, 16384, 16385, N_BIG]
WIDTH_PAIRS = [(c, ce) for c in (1, 8, 17, 32) for ce in (17, 24, 32)]

gpu = pytest.mark.gpu


def top(c):
    return (1 << c) - 1


def payload(n, c):
    return (n * c + 7) // 8


def dwords(n, c):
    """bytes of n values of c bits in the whole dwords the encoder stores"""
    return (n * c + 31) // 32 * 4


def miss_of(c):
    return 1 if c == 1 else 0x5A5A5A5A & top(c)


def words_of(n):
    nchunks = -(-n // CHUNK)
    return nchunks + 1 + -(-nchunks // GROUP)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---- the definition, in numpy ---------------------------------------------------------------------------------------------------

def tails_of(x):
    """bool[n]: row i is a tail"""
    t = np.ones(len(x), dtype=bool)
    t[:-1] = x[1:] != x[:-1]
    return t


def runs_of(x):
    """-> (values uint32[r], ends uint32[r]) of the column x"""
    at = np.nonzero(tails_of(x))[0] if len(x) else np.zeros(0, dtype=np.int64)
    return x[at].astype(np.uint32), (at + 1).astype(np.uint32)


def expand(values, ends, R_, n, miss):
    """-> (out uint32[n], rows behind the last run): j(i) = the number of j < R with end_j <= i, for non-decreasing ends"""
    e = np.asarray(ends[:R_], dtype=np.int64)
    assert (np.diff(e) >= 0).all()
    j = np.searchsorted(e, np.arange(n, dtype=np.int64), side="right")
    out = np.where(j < R_, np.asarray(values, dtype=np.uint32)[np.minimum(j, max(R_ - 1, 0))] if R_ else miss, miss).astype(np.uint32)
    return out, int((j == R_).sum())


# ---- recipes --------------------------------------------------------------------------------------------------------------------

def column_of_tails(tails, c):
    """the column whose tails are exactly `tails` (its last row aside): cumsum(head marks) mod 2^c, so neighbours across a mark
    differ by one mod 2^c -- at every width, c = 1 included"""
    head = np.zeros(len(tails), dtype=np.int64)
    head[1:] = tails[:-1]
    return (np.cumsum(head) % (1 << c)).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def heads(c, n, mean=8, seed=0):
    """runs of geometric length around `mean`"""
    rng = np.random.default_rng([c, n, mean, seed, 31])
    return frozen(column_of_tails(rng.random(n) < 1.0 / mean, c))


# forced marks of the crossings column: (row, is a tail)
CROSS_RUNS_ACROSS = (5 * LANE - 1, R - 1)                 # no tail at a lane's and a tile's last row: the run goes on in the next
CROSS_TAILS_AT = (3 * LANE - 1, 2 * R - 1)                # a tail exactly at a lane's and a tile's last row
CROSS_ONE_ROW_RUNS = (7 * LANE, 9 * LANE + LANE - 1, CHUNK + 3 * LANE, CHUNK + R + LANE - 1)  # at a lane's first row, at a lane's last row; in both chunks


@functools.lru_cache(maxsize=None)
def crossings(c, across_chunk, seed=0):
    """N_CROSS rows, tails at random (1 / 16) under the forced marks; across_chunk: a run crosses the chunk boundary, else a tail sits
    exactly at the chunk's last row"""
    n = N_CROSS
    t = np.random.default_rng([c, seed, 41]).random(n) < 1 / 16
    for row in CROSS_RUNS_ACROSS:
        t[row] = False
    for row in CROSS_TAILS_AT:
        t[row] = True
    for row in CROSS_ONE_ROW_RUNS:
        t[row - 1] = t[row] = True
    t[CHUNK - 1] = not across_chunk
    return frozen(column_of_tails(t, c))


@functools.lru_cache(maxsize=None)
def long_runs(n=N_BIG, about=20000):
    """c = 1: runs of about 20000 rows -- a chunk with no tail at all, several chunks whose slots share one output dword"""
    t = np.zeros(n, dtype=bool)
    row = about + 123
    while row < n:
        t[row - 1] = True
        row += about - 77
    return frozen(column_of_tails(t, 1))


@functools.lru_cache(maxsize=None)
def dense(c, n):
    assert c >= 2
    return frozen((np.arange(n, dtype=np.uint64) % (1 << c)).astype(np.uint32))


@functools.lru_cache(maxsize=None)
def decode_table(cv, n, last, seed=0):
    """-> (values, ends) with two and three zero-length runs in a row, a run longer than a chunk, one that covers a whole tile
    exactly, short runs that cross lane boundaries; last: 'below' n, 'at' n or 'above' n"""
    rng = np.random.default_rng([cv, n, seed, 43])
    lengths = [5, 0, 0, 27, R - 32, R, 0, 0, 0, 1, 1, CHUNK + 700]  # rows 0 .. 2048: ragged; [2048, 4096): exactly a tile
    assert sum(lengths[:5]) == R
    while sum(lengths) < n - 3000:
        lengths.append(int(rng.integers(0, 90)))
    ends = np.cumsum(lengths)
    assert ends[-1] < n
    if last == "at":
        ends = np.append(ends, n)
    elif last == "above":
        ends = np.append(ends, min(n + 5000, top(32)))
    values = rng.integers(0, 1 << cv, len(ends), dtype=np.uint64).astype(np.uint32)
    if cv > 1:
        values[1:] = np.where(values[1:] == values[:-1], values[1:] ^ 1, values[1:])
    return frozen(values, ends.astype(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------


def test_runs_header_is_plain_c99():
    support.check_header_is_plain_c99(HEADER)


def test_runs_header_declares_what_python_binds(L):
    names, sigs = support.check_header_binds(L, HEADER)
    assert names == ["mi355_run_decode_dev", "mi355_run_decode_kernel", "mi355_run_encode_dev", "mi355_run_encode_kernel", "mi355_run_encode_workspace_words"]
    sig = sigs["mi355_run_encode_dev"]
    assert sig[2] is C.c_uint64 and sig[3] is C.c_uint and sig[4] is C.c_uint and sig[7] is C.c_uint64 and len(sig) == 10
    sig = sigs["mi355_run_decode_dev"]
    assert sig[2] is C.c_uint and sig[4] is C.c_uint and sig[5] is C.c_uint64 and sig[7] is C.c_uint64 and sig[8] is C.c_uint32 and len(sig) == 11
    assert sigs["mi355_run_encode_kernel"] == [C.c_uint, C.c_uint] == sigs["mi355_run_decode_kernel"]
    assert L.mi355_run_encode_kernel.restype is C.c_char_p and L.mi355_run_decode_kernel.restype is C.c_char_p
    assert L.mi355_run_encode_workspace_words.restype is C.c_uint64
    text = support.header_text(HEADER)
    assert '#include "mi355_scan.h"' in text and text.count("#include") == 1
    from shared_simd_scan_amd._capi import HEADERS

    assert list(HEADERS)[-2:] == [HEADER, "mi355_sort.h"]


def test_runs_names_are_exported():
    import shared_simd_scan_amd as pkg

    for name in ("run_encode_kernel", "run_decode_kernel", "run_encode_workspace_words"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    for name in ("run_encode", "count_runs", "run_lengths", "run_decode", "repeat", "runs_column"):
        assert callable(getattr(pkg.ScanEngine, name))


def test_runs_header_carries_both_capture_verdicts():
    text = support.header_text(HEADER)
    assert len(re.findall(r"graph capture: capturable\b", text)) == 2
    support.check_capture_verdict(HEADER, r"needs no warm-up call, whatever its arguments", r"caller's workspace", r"zeroing of uncovered_dev",
                                  r"zeroing of count_dev", r"read at every\s+\*?\s*replay")


def test_kernel_names_on_both_sides_of_every_refusal(L):
    from shared_simd_scan_amd import run_decode_kernel, run_encode_kernel

    for f, name in ((L.mi355_run_encode_kernel, EMIT_KERNEL), (L.mi355_run_decode_kernel, DECODE_KERNEL)):
        for a in (1, 2, 9, 31, 32):
            for b in (1, 14, 32):
                assert f(a, b) == name.encode(), (a, b)
        for bad in (0, 33, 1 << 31):
            assert f(bad, 9) is None and f(9, bad) is None and f(bad, bad) is None, bad
    assert run_encode_kernel(9, 17) == EMIT_KERNEL and run_decode_kernel(1, 32) == DECODE_KERNEL
    for bad in ((0, 9), (9, 0), (33, 9), (9, 33), (-1, 9), (9, 1 << 32)):
        with pytest.raises(ValueError):
            run_encode_kernel(*bad)
        with pytest.raises(ValueError):
            run_decode_kernel(*bad)


def test_workspace_words_are_the_chunk_prefix(L):
    from shared_simd_scan_amd import run_encode_workspace_words

    for n, want in ((0, 1), (1, 3), (16384, 3), (16385, 4), (1 << 24, 1024 + 1 + 1), ((1 << 24) + 1, 1025 + 1 + 2)):
        assert L.mi355_run_encode_workspace_words(n) == want == words_of(n) == run_encode_workspace_words(n), n
    assert words_of(N_GROUPS) == 1026 + 1 + 2


def test_ends_must_hold_n(fake):
    """n <= 2^ce - 1, at ce = 1, 14, 15, 32: the wrapper refuses what the call would (the GPU part asserts the call's own refusal)"""
    eng, rec, col = fake
    rec.mi355_run_encode_workspace_words = lambda n: words_of(n)
    for ce in (1, 14, 15, 32):
        eng.run_encode(col(9, top(ce)), capacity=0, ends_width=ce, values=False, ends=False)
        (name, a), = rec.calls
        rec.calls.clear()
        assert a[2:5] == [top(ce), 9, ce]
        with pytest.raises(ValueError):
            eng.run_encode(col(9, top(ce) + 1), capacity=0, ends_width=ce, values=False, ends=False)
        assert rec.calls == []
        # ends_width=None picks the width that holds n
        eng.run_encode(col(9, top(ce)), capacity=0, values=False, ends=False)
        assert rec.calls.pop()[1][4] == ce
        if ce < 32:
            eng.run_encode(col(9, top(ce) + 1), capacity=0, values=False, ends=False)
            assert rec.calls.pop()[1][4] == ce + 1


def test_wrappers_pass_what_the_abi_takes(fake, L):
    import torch

    eng, rec, col = fake
    rec.mi355_run_encode_workspace_words = lambda n: words_of(n)
    rec.mi355_running_sum_workspace_words = lambda n: words_of(n)

    def last():
        (name, a), = rec.calls
        rec.calls.clear()
        return name, a

    c1 = col(9, 777)
    values, ends, count = eng.run_encode(c1)  # defaults: capacity n, the width that holds 777, fresh buffers, the engine's workspace
    name, a = last()
    assert name == "mi355_run_encode_dev" and a[1:5] == [c1.data.data_ptr(), 777, 9, 10] and a[5:9] == [values.data_ptr(), ends.data_ptr(), 777, count.data_ptr()]
    assert values.numel() == L.mi355_compressed_buffer_size(9, 777) and ends.numel() == L.mi355_compressed_buffer_size(10, 777)
    assert count.dtype == torch.int64 and count.numel() == 1
    ws = eng._running_ws[-1]
    assert a[9] == ws.data_ptr() and ws.numel() >= words_of(777)
    v = torch.zeros(dwords(100, 9), dtype=torch.uint8)
    e = torch.zeros(dwords(100, 32), dtype=torch.uint8)
    cnt = torch.zeros(1, dtype=torch.int64)
    mine = torch.zeros(words_of(777), dtype=torch.int64)
    got = eng.run_encode(c1, capacity=100, ends_width=32, values=v, ends=e, count=cnt, workspace=mine)
    name, a = last()
    assert a[1:] == [c1.data.data_ptr(), 777, 9, 32, v.data_ptr(), e.data_ptr(), 100, cnt.data_ptr(), mine.data_ptr()]
    assert got[0] is v and got[1] is e and got[2] is cnt
    got = eng.run_encode(c1, values=False)  # ends only
    name, a = last()
    assert a[5] is None and a[6] == got[1].data_ptr() and got[0] is None
    got = eng.run_encode(c1, ends=False)  # values only
    name, a = last()
    assert a[6] is None and a[5] == got[0].data_ptr() and got[1] is None
    count = eng.count_runs(c1)
    name, a = last()
    assert name == "mi355_run_encode_dev" and a[5:8] == [None, None, 0] and a[8] == count.data_ptr()
    for bad in (dict(ends_width=0), dict(ends_width=33), dict(ends_width=9), dict(capacity=-1), dict(values=False, ends=False)):
        with pytest.raises(ValueError):
            eng.run_encode(c1, **bad)
    for bad in (dict(values=torch.zeros(dwords(777, 9) - 1, dtype=torch.uint8)), dict(ends=torch.zeros(dwords(777, 10) - 1, dtype=torch.uint8)),
                dict(count=torch.zeros(1, dtype=torch.int32)), dict(workspace=torch.zeros(words_of(777) - 1, dtype=torch.int64))):
        with pytest.raises(AssertionError):
            eng.run_encode(c1, **bad)
    assert rec.calls == []
    # run_lengths is delta(first = 0) at the ends' width
    e1 = col(10, 55)
    res = eng.run_lengths(e1)
    name, a = last()
    assert name == "mi355_delta_dev" and a[1:8] == [e1.data.data_ptr(), 55, 10, 0, 0, 10, 0] and (res.n, res.c) == (55, 10)
    eng.run_lengths(e1, co=7)
    assert last()[1][6] == 7
    # run_decode: runs as nothing, an int, a device tensor
    v1 = col(9, 60)
    res = eng.run_decode(v1, e1, 777)
    name, a = last()
    assert name == "mi355_run_decode_dev" and a[1:10] == [v1.data.data_ptr(), 9, e1.data.data_ptr(), 10, 55, None, 777, 0, res.data.data_ptr()] and a[10] is None
    assert (res.n, res.c) == (777, 9) and res.data.numel() == L.mi355_compressed_buffer_size(9, 777)
    unc = torch.zeros(1, dtype=torch.int64)
    out = torch.zeros(payload(777, 9), dtype=torch.uint8)
    res = eng.run_decode(v1, e1, 777, runs=13, miss=511, out=out, uncovered=unc)
    name, a = last()
    assert a[5:] == [13, None, 777, 511, out.data_ptr(), unc.data_ptr()] and res.data is out
    res = eng.run_decode(v1, e1, 777, runs=cnt)
    name, a = last()
    assert a[5:7] == [55, cnt.data_ptr()]
    res = eng.run_decode(v1, e1, 777, runs=0)
    name, a = last()
    assert a[1] is None and a[3] is None and a[5] == 0
    for bad in (dict(runs=56), dict(runs=-1), dict(miss=512), dict(miss=-1)):
        with pytest.raises(ValueError):
            eng.run_decode(v1, e1, 777, **bad)
    for bad in (dict(out=torch.zeros(payload(777, 9) - 1, dtype=torch.uint8)), dict(uncovered=torch.zeros(1, dtype=torch.int32)),
                dict(runs=torch.zeros(1, dtype=torch.int32))):
        with pytest.raises(AssertionError):
            eng.run_decode(v1, e1, 777, **bad)
    assert rec.calls == []
    # repeat: running_sum(counts) at the width that holds every sum, then run_decode on its output
    counts = col(4, 60)
    res = eng.repeat(v1, counts, 777, miss=3)
    (n1, a1), (n2, a2) = rec.calls
    rec.calls.clear()
    assert n1 == "mi355_running_sum_dev" and a1[1:10] == [counts.data.data_ptr(), 60, 4, None, 0, 0, 0, 10, 0]
    assert n2 == "mi355_run_decode_dev" and a2[1:9] == [v1.data.data_ptr(), 9, a1[10], 10, 60, None, 777, 3] and (res.n, res.c) == (777, 9)


def test_every_runs_kernel_has_a_case():
    kernels = support.global_kernels_of("runs")
    assert kernels == {COUNT_KERNEL, EMIT_KERNEL, DECODE_KERNEL}, kernels
    support.check_gpu_part_asserts(__file__, "COUNT_KERNEL", "EMIT_KERNEL", "DECODE_KERNEL", "SCAN_KERNEL", "EDGES_KERNEL")


def test_runs_sources_read_no_flag_bits_and_no_context_state():
    assert [os.path.basename(p) for p in support.feature_sources("runs")] == ["run_decode.hip", "run_encode.hip", "runs.hpp"]
    support.check_sources_read_no_flag_bits("runs")
    mine = {name for name, path, _ in support.hip_functions() if path.startswith("runs" + os.sep)}
    assert {"mi355_run_encode_dev", "mi355_run_decode_dev", "mi355_run_encode_kernel", "mi355_run_decode_kernel", "mi355_run_encode_workspace_words"} <= mine
    assert not mine & set(support.entry_points_reaching("rowid_ws_get("))
    assert not mine & set(support.entry_points_reaching("kernel_scratch"))
    for path in support.feature_sources("runs"):
        text = open(path).read()
        assert "rowid_ws_get(" not in text and "kernel_scratch" not in text and "pool_get(" not in text, path


def chunk_slots(x):
    """-> (tails per chunk, first slot per chunk)"""
    t = tails_of(x)
    per = np.add.reduceat(t.astype(np.int64), np.arange(0, len(x), CHUNK))
    return per, np.cumsum(per) - per


def test_recipes_are_not_vacuous():
    for c in range(1, 33):  # neighbours across a mark differ at every width, c = 1 included: the marks ARE the tails
        rng = np.random.default_rng(c)
        t = rng.random(5000) < 1 / 4
        x = column_of_tails(t, c)
        assert (tails_of(x)[:-1] == t[:-1]).all() and int(x.max()) <= top(c), c
        assert len(runs_of(heads(c, 2049))[0]) > 150, c
    for across in (True, False):
        x = crossings(9, across)
        t = tails_of(x)
        assert len(x) == N_CROSS == CHUNK + R + 100
        # a run across a lane boundary, a tile boundary (and the chunk boundary); a tail exactly at the last row of each
        assert not t[5 * LANE - 1] and (5 * LANE) % LANE == 0 and not t[R - 1]
        assert t[3 * LANE - 1] and t[2 * R - 1]
        assert bool(t[CHUNK - 1]) == (not across) and (x[CHUNK - 1] == x[CHUNK]) == across
        for row in CROSS_ONE_ROW_RUNS:  # a one-row run at a lane's first row and at a lane's last row
            assert t[row - 1] and t[row]
        assert [row % LANE for row in CROSS_ONE_ROW_RUNS] == [0, LANE - 1, 0, LANE - 1]
        assert t[-1] and 800 < t.sum() < 1500
    x = long_runs()
    per, first = chunk_slots(x)
    v, e = runs_of(x)
    assert int(x.max()) == 1 and len(per) == 5 and (per == 0).any() and per[0] == 0, per  # a chunk with no tail at all
    assert len(v) == 4 and (np.diff(np.r_[0, e.astype(np.int64)])[:3] > CHUNK).all()
    assert (per > 0).sum() >= 3 and (first[per > 0] * 1 // 32 == 0).all()                # their slots share values dword 0
    assert len({int(f) * 17 // 32 for f in first[per > 0]}) < (per > 0).sum()            # and a dword of the ends at 17 bits
    for c in (2, 9, 32):
        x = dense(c, 2049 if c > 2 else N_BIG)
        assert tails_of(x).all()  # every row is a tail: r == n
    for last in ("below", "at", "above"):
        values, ends = decode_table(9, N_BIG, last)
        lengths = np.diff(np.r_[0, ends.astype(np.int64)])
        zero = lengths == 0
        assert (zero[1:] & zero[:-1]).any() and (zero[2:] & zero[1:-1] & zero[:-2]).any()  # two and three zero-length runs in a row
        assert (lengths > CHUNK).any()
        whole = np.nonzero(lengths == R)[0]
        assert any((ends[j] - R) % R == 0 for j in whole)                                  # one covers a whole tile exactly
        assert (np.diff(ends.astype(np.int64)) >= 0).all()
        assert {"below": ends[-1] < N_BIG, "at": ends[-1] == N_BIG, "above": ends[-1] > N_BIG}[last]
        want, uncovered = expand(values, ends, len(ends), N_BIG, miss_of(9))
        assert (uncovered > 0) == (last == "below")
    # the two paths of the decoder, named by their data
    one, several = tile_paths(*runs_of(long_runs()), N_BIG)
    assert one >= 30 and 1 <= several <= 4, (one, several)          # long_runs: the one-run-per-tile path (and the four tiles a run ends in)
    one, several = tile_paths(*runs_of(heads(9, N_BIG)), N_BIG)
    assert one == 0 and several == -(-N_BIG // R)              # heads: the walk path in every tile


def tile_paths(values, ends, n):
    """-> (tiles whose first and last row lie in one run, tiles that hold several)"""
    e = ends.astype(np.int64)
    first = np.arange(0, n, R)
    last = np.minimum(first + R - 1, n - 1)
    same = np.searchsorted(e, first, side="right") == np.searchsorted(e, last, side="right")
    return int(same.sum()), int((~same).sum())


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

class Enc:
    """one run_encode call through the C ABI: the column in hostile surroundings; both outputs (in the whole dwords the call may
    store), the count word and the workspace each in a Guarded buffer full of SENTINEL"""

    def __init__(self, O, eng, x, c, ce, capacity=None, values=True, ends=True, ws=None, col=None):
        self.O, self.eng, self.x, self.c, self.ce = O, eng, x, c, ce
        self.n = n = len(x)
        self.capacity = n if capacity is None else capacity
        self.with_values, self.with_ends = values, ends
        self.col = col if col is not None else (hostile_pack(O, x, c) if n else None)
        most = min(self.capacity, n)
        self.values = Guarded(dwords(most, c))
        self.ends = Guarded(dwords(most, ce))
        self.count = Guarded(8, back=64, front=64)
        self.ws = ws if ws is not None else Guarded(8 * words_of(n))
        assert self.ws.nbytes >= 8 * words_of(n)

    def call(self, L, **kw):
        a = dict(col=self.col.data_ptr() if self.n else None, n=self.n, c=self.c, ce=self.ce, values=self.values.ptr if self.with_values else None,
                 ends=self.ends.ptr if self.with_ends else None, capacity=self.capacity, count=self.count.ptr, ws=self.ws.ptr)
        a.update(kw)
        rc = L.mi355_run_encode_dev(self.eng._ctx, a["col"], a["n"], a["c"], a["ce"], a["values"], a["ends"], a["capacity"], a["count"], a["ws"])
        self.eng.synchronize()
        return rc

    def check_output(self, g, want, width, m, tag):
        have = g.fetch()  # asserts the guard bytes on both sides
        nb = payload(m, width)
        wb = self.O.pack(np.ascontiguousarray(want[:m], dtype=np.uint32), width)[:nb] if m else np.zeros(0, dtype=np.uint8)
        bad = np.nonzero(have[:nb] != wb)[0]
        assert bad.size == 0, (tag, width, "byte", int(bad[0]), "of", nb, "have", int(have[bad[0]]), "want", int(wb[bad[0]]), "wrong bytes", int(bad.size))
        assert (have[nb:] == SENTINEL).all(), (tag, width, "a byte behind the payload was written")  # (trailing bits of byte nb - 1 are the packer's zeros)

    def run(self, L, what=""):
        """-> the launch record, after every byte, the count, the guards and the input have been checked"""
        tag = (what, self.n, self.c, self.ce, self.capacity)
        want_v, want_e = runs_of(self.x)
        r = len(want_v)
        m = min(r, self.capacity)
        for g in (self.values, self.ends, self.count):
            g.t.fill_(SENTINEL)
        before = self.col.clone()
        assert self.call(L) == 0, (tag, L.mi355_last_error())
        got = int(self.count.fetch().view(np.int64)[0])
        assert got == r, (tag, "count", got, "want", r)
        self.check_output(self.values, want_v, self.c, m if self.with_values else 0, tag)
        self.check_output(self.ends, want_e, self.ce, m if self.with_ends else 0, tag)
        self.ws.fetch()  # its guards
        assert bool((self.col == before).all()), (tag, "the column was written")
        rec = record(L, self.eng)
        names = [base_name(x[0]) for x in rec]
        if self.capacity == 0:
            assert names == [COUNT_KERNEL, SCAN_KERNEL], (tag, rec)  # count-only: no emitting kernel
        else:
            assert names == [COUNT_KERNEL, SCAN_KERNEL] + [EDGES_KERNEL] * (int(self.with_values) + int(self.with_ends)) + [EMIT_KERNEL], (tag, rec)
            assert rec[-1][0].startswith(f"{EMIT_KERNEL}<{self.c}>"), (tag, rec)
            assert rec[-1][2] >= 4 * (2 * 256 * self.c + 4 * (64 * self.c + 4) + 4 * (64 * self.ce + 4)), (tag, rec)
        assert all(x[3] == 0 for x in rec) and rec[1][1] == -(-(-(-self.n // CHUNK)) // GROUP) and rec[0][2] >= 4 * 2 * 256 * self.c, (tag, rec)
        return rec


class Dec:
    """one run_decode call through the C ABI: both tables in hostile surroundings, the output and the counter Guarded"""

    def __init__(self, O, eng, values, ends, cv, ce, n, runs=None, runs_dev=None, miss=None, counter=True):
        import torch

        self.O, self.eng, self.values, self.ends, self.cv, self.ce, self.n = O, eng, values, ends, cv, ce, n
        self.runs = len(ends) if runs is None else runs
        self.runs_dev = None if runs_dev is None else torch.tensor([runs_dev], dtype=torch.int64, device="cuda")
        self.R = self.runs if runs_dev is None else min(self.runs, runs_dev)
        self.miss = miss_of(cv) if miss is None else miss
        self.vt = hostile_pack(O, values, cv) if len(values) else None
        self.et = hostile_pack(O, ends, ce) if len(ends) else None
        self.out = Guarded(payload(n, cv))
        self.counter = Guarded(8, back=64, front=64) if counter else None

    def call(self, L, **kw):
        a = dict(values=self.vt.data_ptr() if self.vt is not None else None, cv=self.cv, ends=self.et.data_ptr() if self.et is not None else None, ce=self.ce,
                 runs=self.runs, runs_dev=self.runs_dev.data_ptr() if self.runs_dev is not None else None, n=self.n, miss=self.miss, out=self.out.ptr,
                 counter=self.counter.ptr if self.counter else None)
        a.update(kw)
        rc = L.mi355_run_decode_dev(self.eng._ctx, a["values"], a["cv"], a["ends"], a["ce"], a["runs"], a["runs_dev"], a["n"], a["miss"], a["out"], a["counter"])
        self.eng.synchronize()
        return rc

    def fetch_checked(self, L, what=""):
        """the call, the guards, the trailing bits, the record -> the payload bytes"""
        self.tag = (what, self.n, self.cv, self.ce, self.R)
        self.out.t.fill_(SENTINEL)
        if self.counter:
            self.counter.t.fill_(SENTINEL)
        assert self.call(L) == 0, (self.tag, L.mi355_last_error())
        have = self.out.fetch()
        if (self.n * self.cv) % 8:
            assert int(have[-1]) >> ((self.n * self.cv) % 8) == 0, (self.tag, "bits behind the last value are not zero")
        (label, grid, lds, flags), = rec = record(L, self.eng)
        assert label.startswith(f"{DECODE_KERNEL}<{self.cv}>") and flags == 0 and lds == 0, (self.tag, rec)
        self.grid = grid
        return have

    def run(self, L, what=""):
        want, uncovered = expand(self.values, self.ends, self.R, self.n, self.miss)
        wb = self.O.pack(want, self.cv)[: self.out.nbytes]
        have = self.fetch_checked(L, what)
        bad = np.nonzero(have != wb)[0]
        assert bad.size == 0, (self.tag, "byte", int(bad[0]), "of", len(wb), "have", int(have[bad[0]]), "want", int(wb[bad[0]]), "wrong bytes", int(bad.size))
        if self.counter:
            got = int(self.counter.fetch().view(np.int64)[0])
            assert got == uncovered, (self.tag, "counter", got, "want", uncovered)
        return uncovered


def one_block(eng):
    """a context manager: one block of four waves, so that a wave walks several chunks (run_encode) or strides over tiles (run_decode)"""
    import contextlib

    @contextlib.contextmanager
    def cm():
        eng.set_option("grid_cus", 1)
        eng.set_option("max_blocks_per_cu", 1)
        try:
            yield
        finally:
            eng.set_option("grid_cus", 0)
            eng.set_option("max_blocks_per_cu", 0)

    return cm()


# ---- run_encode ----

@gpu
@pytest.mark.parametrize("n", SIZES)
def test_encode_sizes_and_tails(L, O, eng, n):
    x = heads(9, n)
    for ce in (n.bit_length(), 32):
        rec = Enc(O, eng, x, 9, ce).run(L)
        assert base_name(rec[0][0]) == COUNT_KERNEL and base_name(rec[1][0]) == SCAN_KERNEL and base_name(rec[2][0]) == EDGES_KERNEL
        assert base_name(rec[-1][0]) == EMIT_KERNEL


@gpu
@pytest.mark.parametrize("c", range(1, 33))
def test_encode_every_width(L, O, eng, c):
    rec = Enc(O, eng, heads(c, 2049, mean=4), c, 12).run(L)
    assert rec[-1][0].startswith(f"{EMIT_KERNEL}<{c}>")
    Enc(O, eng, heads(9, 2049, mean=4), 9, c if c >= 12 else 12 + c).run(L)  # ... and the ends' widths that hold 2049


@gpu
@pytest.mark.parametrize("c,ce", WIDTH_PAIRS)
def test_encode_width_pairs(L, O, eng, c, ce):
    Enc(O, eng, heads(c, N_BIG), c, ce).run(L)


@gpu
@pytest.mark.parametrize("recipe", ["across", "tail at the chunk's end", "long runs", "dense c=2", "dense c=9", "dense c=32", "one run", "alternating bits"])
def test_encode_recipes(L, O, eng, recipe):
    x, c = {"across": (crossings(9, True), 9), "tail at the chunk's end": (crossings(9, False), 9), "long runs": (long_runs(), 1),
            "dense c=2": (dense(2, N_BIG), 2), "dense c=9": (dense(9, N_BIG), 9), "dense c=32": (dense(32, N_BIG), 32),
            "one run": (np.full(N_BIG, 5, dtype=np.uint32), 3), "alternating bits": ((np.arange(N_BIG) & 1).astype(np.uint32), 1)}[recipe]
    for ce in (len(x).bit_length(), 32):
        rec = Enc(O, eng, x, c, ce).run(L, what=recipe)
        assert base_name(rec[-1][0]) == EMIT_KERNEL


@gpu
def test_encode_second_scan_group(L, O, eng):
    """1025 chunks, mean run 64: the last chunks' first slots come from group_totals"""
    x = heads(9, N_GROUPS, mean=64)
    rec = Enc(O, eng, x, 9, 25).run(L)
    assert rec[1][1] == 2 and base_name(rec[-1][0]) == EMIT_KERNEL


@gpu
def test_encode_capacities(L, O, eng):
    """compact's capacity rule: the first min(r, capacity) runs, the count always r, nothing behind them written"""
    x = heads(9, N_BIG)
    per, first = chunk_slots(x)
    r = int(per.sum())
    assert per[2] > 10
    inside, at_first = int(first[2]) + int(per[2]) // 2, int(first[3])
    for capacity in (r, r - 1, inside, at_first, 1, r + 1000):
        rec = Enc(O, eng, x, 9, 17, capacity=capacity).run(L, what="capacity")
        assert base_name(rec[-1][0]) == EMIT_KERNEL
    for x1 in (x, long_runs()):
        rec = Enc(O, eng, x1, 9 if x1 is x else 1, 17, capacity=0).run(L, what="count only")
        assert [base_name(k[0]) for k in rec] == [COUNT_KERNEL, SCAN_KERNEL]
        rec = Enc(O, eng, x1, 9 if x1 is x else 1, 17, capacity=0, values=False, ends=False).run(L, what="count only, no outputs")
        assert EMIT_KERNEL not in [base_name(k[0]) for k in rec]


@gpu
def test_encode_one_output(L, O, eng):
    for x, c in ((heads(9, N_BIG), 9), (long_runs(), 1), (crossings(9, True), 9)):
        rec = Enc(O, eng, x, c, 17, ends=False).run(L, what="values only")
        assert [base_name(k[0]) for k in rec].count(EDGES_KERNEL) == 1
        rec = Enc(O, eng, x, c, 17, values=False).run(L, what="ends only")
        assert [base_name(k[0]) for k in rec].count(EDGES_KERNEL) == 1 and base_name(rec[-1][0]) == EMIT_KERNEL


@gpu
def test_encode_row_range_view(L, O, eng):
    """rows [lead, lead + n) of a longer column whose row lead + n equals row lead + n - 1: the view's last row is still a tail, and
    the rows in front of the view reach nothing"""
    for n in (2 * R + 504, R, 3 * LANE, CHUNK):
        lead = 2 * R + 128
        x = heads(9, n, mean=8, seed=5)
        whole = np.concatenate([heads(9, lead, seed=6), x, np.full(4096, x[-1], dtype=np.uint32)])
        assert whole[lead + n] == whole[lead + n - 1] and (lead * 9) % 128 == 0
        col = hostile_pack(O, whole, 9)[lead * 9 // 8:]
        assert col.data_ptr() % 16 == 0
        Enc(O, eng, x, 9, 17, col=col).run(L, what="view")


@gpu
def test_encode_one_block_walks_many_chunks(L, O, eng):
    x = heads(9, N_ONE_BLOCK, mean=16)
    with one_block(eng):
        for e in (Enc(O, eng, x, 9, 18), Enc(O, eng, x, 9, 32, capacity=3000), Enc(O, eng, dense(9, N_ONE_BLOCK), 9, 18)):
            rec = e.run(L, what="one block")
            assert rec[0][1] == rec[-1][1] == 1 and base_name(rec[0][0]) == COUNT_KERNEL
    assert Enc(O, eng, x, 9, 18).run(L)[-1][1] > 1


@gpu
def test_encode_workspace_holds_leftovers(L, O, eng):
    """the workspace of a larger call, as that call left it, under a smaller one: nothing stale is read"""
    big = Enc(O, eng, heads(9, N_ONE_BLOCK), 9, 18)
    big.run(L, what="the larger call")
    for n in (3 * CHUNK + 5, CHUNK, 77):
        Enc(O, eng, heads(9, n, seed=7), 9, 17, ws=big.ws).run(L, what="leftovers")
        Enc(O, eng, heads(1, n, mean=3000, seed=7), 1, 17, ws=big.ws).run(L, what="leftovers")
    assert not (big.ws.fetch() == SENTINEL).all()


@gpu
def test_empty_column(L, O, eng):
    x = np.zeros(0, dtype=np.uint32)
    e = Enc(O, eng, x, 9, 1)
    for kw in ({}, dict(values=None, ends=None, ws=None, capacity=0), dict(ws=None, capacity=5)):
        e.count.t.fill_(SENTINEL)
        assert e.call(L, **kw) == 0 and record(L, eng) == []
        assert int(e.count.fetch().view(np.int64)[0]) == 0
    d = Dec(O, eng, *decode_table(9, N_BIG, "at"), 9, 17, 0)
    d.counter.t.fill_(SENTINEL)
    assert d.call(L) == 0 and record(L, eng) == [] and int(d.counter.fetch().view(np.int64)[0]) == 0
    assert d.call(L, out=None, counter=None, values=None, ends=None) == 0


# ---- run_decode ----

@gpu
@pytest.mark.parametrize("n", SIZES)
def test_decode_sizes_and_tails(L, O, eng, n):
    x = heads(9, n)
    values, ends = runs_of(x)
    for ce in (n.bit_length(), 32):
        d = Dec(O, eng, values, ends, 9, ce, n)
        assert d.run(L) == 0
        assert (d.out.fetch() == O.pack(x, 9)[: payload(n, 9)]).all()  # the column itself
    if len(ends) > 1:  # without the last run: its rows get `miss` and are counted
        d = Dec(O, eng, values, ends, 9, 32, n, runs=len(ends) - 1)
        assert d.run(L) == n - int(ends[-2])


@gpu
@pytest.mark.parametrize("w", range(1, 33))
def test_decode_every_width(L, O, eng, w):
    values, ends = runs_of(heads(w, 2049, mean=4))
    Dec(O, eng, values, ends, w, 12, 2049).run(L)
    values, ends = runs_of(heads(9, 2049, mean=4))
    Dec(O, eng, values, ends, 9, w if w >= 12 else 12 + w, 2049).run(L)


@gpu
@pytest.mark.parametrize("cv,ce", WIDTH_PAIRS)
def test_decode_width_pairs(L, O, eng, cv, ce):
    values, ends = runs_of(heads(cv, N_BIG))
    Dec(O, eng, values, ends, cv, ce, N_BIG).run(L)
    values, ends = decode_table(cv, N_BIG, "below")
    assert Dec(O, eng, values, ends, cv, ce, N_BIG, miss=top(cv)).run(L) > 0  # miss at 2^cv - 1


@gpu
@pytest.mark.parametrize("last", ["below", "at", "above"])
def test_decode_tables(L, O, eng, last):
    """zero-length runs in a row, a run longer than a chunk, one that covers a tile exactly; the last end below, at and above n"""
    values, ends = decode_table(9, N_BIG, last)
    uncovered = Dec(O, eng, values, ends, 9, 32 if last == "above" else 17, N_BIG).run(L, what=last)
    assert (uncovered > 0) == (last == "below")
    Dec(O, eng, values, ends, 9, 32, N_BIG, counter=False).run(L, what="no counter")


@gpu
def test_decode_both_paths(L, O, eng):
    """long_runs: one run per tile (the splat); heads: several runs in every tile (the walk) -- asserted of the data in the CPU part"""
    for x, c in ((long_runs(), 1), (heads(9, N_BIG), 9), (crossings(9, True), 9), (crossings(9, False), 9), (dense(9, N_BIG), 9)):
        values, ends = runs_of(x)
        d = Dec(O, eng, values, ends, c, 17, len(x))
        assert d.run(L) == 0
        assert (d.out.fetch() == O.pack(x, c)[: payload(len(x), c)]).all()


@gpu
def test_decode_run_counts(L, O, eng):
    """R = 0, R = 1, runs_dev below and above runs: entries at and behind R are not read as runs"""
    values, ends = decode_table(9, N_BIG, "at")
    nt = len(ends)
    assert Dec(O, eng, values, ends, 9, 17, N_BIG, runs=0).run(L, what="R = 0") == N_BIG
    assert Dec(O, eng, values[:0], ends[:0], 9, 17, N_BIG, runs=0).run(L, what="R = 0, no tables") == N_BIG
    assert Dec(O, eng, values, ends, 9, 17, N_BIG, runs=1).run(L, what="R = 1") == N_BIG - int(ends[0])
    assert Dec(O, eng, values, np.full(nt, N_BIG, dtype=np.uint32), 9, 17, N_BIG, runs=1).run(L, what="R = 1, all rows") == 0
    assert Dec(O, eng, values, ends, 9, 17, N_BIG, runs=nt, runs_dev=nt // 2).run(L, what="runs_dev below runs") == N_BIG - int(ends[nt // 2 - 1])
    assert Dec(O, eng, values, ends, 9, 17, N_BIG, runs=nt // 2, runs_dev=nt + 1000).run(L, what="runs_dev above runs") == N_BIG - int(ends[nt // 2 - 1])
    assert Dec(O, eng, values, ends, 9, 17, N_BIG, runs=nt, runs_dev=0).run(L, what="runs_dev = 0") == N_BIG
    assert Dec(O, eng, values, ends, 9, 17, N_BIG, runs=nt, runs_dev=nt).run(L, what="runs_dev = runs") == 0


@gpu
def test_decode_bitmap_over_runs_to_bitmap_over_rows(L, O, eng):
    """cv = 1 into a buffer of exactly ceil(n / 8) bytes: a scan's result over the runs, expanded, is the result over the rows"""
    for n in (N_BIG, 2049, 63):
        x = heads(9, n, mean=40)
        values, ends = runs_of(x)
        bits = (values > 255).astype(np.uint32)
        d = Dec(O, eng, bits, ends, 1, 32, n)
        assert d.out.nbytes == -(-n // 8)
        d.run(L, what="bitmap")
        assert (d.out.fetch() == support.packbits(x > 255)).all()


@gpu
def test_decode_second_scan_group_sized_column_and_one_block(L, O, eng):
    x = heads(9, N_GROUPS, mean=64)
    values, ends = runs_of(x)
    d = Dec(O, eng, values, ends, 9, 25, N_GROUPS)
    assert d.run(L) == 0 and d.grid > 1
    with one_block(eng):
        for x in (heads(9, N_ONE_BLOCK, mean=16), heads(1, N_ONE_BLOCK, mean=3000)):
            values, ends = runs_of(x)
            d = Dec(O, eng, values, ends, 9, 18, N_ONE_BLOCK)
            d.run(L, what="one block")
            assert d.grid == 1


@gpu
def test_decode_unsorted_ends(L, O, eng):
    """ends in no order: every output value is one of the R values, or miss -- no stronger claim"""
    rng = np.random.default_rng(77)
    for nt, R_ in ((500, 400), (40000, 40000), (3, 2)):
        ends = rng.integers(0, N_BIG + 1000, nt, dtype=np.uint64).astype(np.uint32)
        values = (np.arange(nt, dtype=np.uint32) * 5 + 2) & top(17)  # none is the sentinel below
        values[R_:] = 1  # behind R: must not appear
        miss = 3
        assert miss not in set(values[:R_].tolist()) and 1 not in set(values[:R_].tolist())
        d = Dec(O, eng, values, ends, 17, 32, N_BIG, runs=R_, miss=miss)
        have = d.fetch_checked(L, what="unsorted")
        got = O.decompress(np.concatenate([have, np.zeros(4096, dtype=np.uint8)]), N_BIG, 17).view(np.uint32)[:N_BIG]
        assert np.isin(got, np.append(values[:R_], miss)).all()
        assert int(d.counter.fetch().view(np.int64)[0]) == int((got == miss).sum())


# ---- round trips through existing calls ----

def column(O, x, c):
    from shared_simd_scan_amd.engine import PackedColumn

    return PackedColumn(hostile_pack(O, x, c), len(x), c)


def bytes_of(col, n=None):
    n = col.n if n is None else n
    return col.data.cpu().numpy()[: payload(n, col.c)]


@gpu
@pytest.mark.parametrize("c", range(1, 33))
def test_round_trip_gives_the_bytes_back(L, O, eng, c):
    """run_decode(run_encode(x)) with the count read on the device: nothing touches the host in between"""
    n = 2049
    x = heads(c, n, mean=5, seed=c)
    values, ends, count = eng.run_encode(column(O, x, c))
    assert [base_name(k[0]) for k in record(L, eng)] == [COUNT_KERNEL, SCAN_KERNEL, EDGES_KERNEL, EDGES_KERNEL, EMIT_KERNEL]
    from shared_simd_scan_amd.engine import PackedColumn

    back = eng.run_decode(PackedColumn(values, n, c), PackedColumn(ends, n, 12), n, runs=count)
    eng.synchronize()
    assert base_name(record(L, eng)[0][0]) == DECODE_KERNEL
    assert (bytes_of(back) == O.pack(x, c)[: payload(n, c)]).all() and int(count.item()) == len(runs_of(x)[0])


@gpu
def test_lengths_and_ends_through_delta_and_running_sum(L, O, eng):
    x = heads(9, N_BIG, mean=30)
    want_v, want_e = runs_of(x)
    vcol, ecol = eng.runs_column(column(O, x, 9))
    r = len(want_e)
    assert (vcol.n, vcol.c, ecol.n, ecol.c) == (r, 9, r, 17)
    assert (bytes_of(vcol) == O.pack(want_v, 9)[: payload(r, 9)]).all() and (bytes_of(ecol) == O.pack(want_e, 17)[: payload(r, 17)]).all()
    lengths = eng.run_lengths(ecol)
    want_l = np.diff(np.r_[0, want_e.astype(np.int64)]).astype(np.uint32)
    assert (bytes_of(lengths) == O.pack(want_l, 17)[: payload(r, 17)]).all()
    again, _ = eng.running_sum(lengths, co=17)
    assert (bytes_of(again) == O.pack(want_e, 17)[: payload(r, 17)]).all()
    # repeat: the values, each its length times, are the column
    back = eng.repeat(vcol, lengths, N_BIG)
    assert (bytes_of(back) == O.pack(x, 9)[: payload(N_BIG, 9)]).all()
    assert int(eng.count_runs(column(O, x, 9)).item()) == r
    assert [base_name(k[0]) for k in record(L, eng)] == [COUNT_KERNEL, SCAN_KERNEL]


@gpu
def test_sort_then_runs_is_unique_with_counts(L, O, eng):
    """sort_rows(with_values) -> compress -> run_encode: the third step of the sort-based GROUP BY, against np.unique"""
    n, c = N_BIG, 11
    x = np.random.default_rng(5).integers(0, 1500, n, dtype=np.uint64).astype(np.uint32)
    rowids, count, values = eng.sort_rows(column(O, x, c), with_values=True)
    sorted_col = eng.compress(values, c)
    vcol, ecol = eng.runs_column(sorted_col)
    lengths = eng.run_lengths(ecol)
    eng.synchronize()
    want_u, want_n = np.unique(x, return_counts=True)
    r = len(want_u)
    assert vcol.n == r and (bytes_of(vcol) == O.pack(want_u.astype(np.uint32), c)[: payload(r, c)]).all()
    assert (bytes_of(lengths) == O.pack(want_n.astype(np.uint32), 17)[: payload(r, 17)]).all()


@gpu
def test_per_run_sums_through_existing_calls(L, O, eng):
    """lookup(arith(ends - 1), running_sum(y)) -> delta is sum(y) per run, against np.add.reduceat"""
    n = N_BIG
    x = heads(9, n, mean=25, seed=3)
    y = np.random.default_rng(9).integers(0, 1 << 9, n, dtype=np.uint64).astype(np.uint32)
    want_v, want_e = runs_of(x)
    r = len(want_e)
    starts = np.r_[0, want_e[:-1].astype(np.int64)]
    want = np.add.reduceat(y.astype(np.int64), starts)
    assert int(y.sum()) < 1 << 32
    vcol, ecol = eng.runs_column(column(O, x, 9))
    last_rows = eng.arith("linear", ecol, ecol, a=1, b=0, k=-1, co=17)
    sums, _ = eng.running_sum(column(O, y, 9), co=32)
    at_ends = eng.lookup(last_rows, sums)
    per_run = eng.delta(at_ends, first=0, co=32)
    eng.synchronize()
    assert (bytes_of(per_run) == O.pack(want.astype(np.uint32), 32)[: payload(r, 32)]).all()


# ---- refusals ----

@gpu
def test_errors_launch_nothing(L, O, eng):
    n = R + 77
    x = heads(9, n)
    e = Enc(O, eng, x, 9, 12)
    e.run(L)
    valid = record(L, eng)
    big = Guarded(16384)  # stands for an input and an output at once
    col, ws, vp, ep = e.col.data_ptr(), e.ws.ptr.value, e.values.ptr.value, e.ends.ptr.value
    errors = (("c = 0", dict(c=0), b"width"), ("c = 33", dict(c=33), b"width"), ("ce = 0", dict(ce=0), b"width"), ("ce = 33", dict(ce=33), b"width"),
              ("n beyond 2^ce - 1", dict(ce=11), b"ce"), ("n = 2^ce", dict(n=2048, ce=11), b"ce"),
              ("null count", dict(count=None), b"count_dev"), ("count at +4", dict(count=e.count.ptr.value + 4), b"count_dev"),
              ("null column", dict(col=None), b"packed_dev"), ("column at +4", dict(col=col + 4), b"aligned"),
              ("null workspace", dict(ws=None), b"ws_dev"), ("workspace at +4", dict(ws=ws + 4), b"aligned"),
              ("both outputs null", dict(values=None, ends=None), b"both null"),
              ("values at +8", dict(values=vp + 8), b"values_dev"), ("ends at +4", dict(ends=ep + 4), b"ends_dev"),
              ("values are the column", dict(col=big.ptr.value, values=big.ptr.value), b"values_dev overlaps packed_dev"),
              ("ends start in the column's last byte", dict(col=big.ptr.value, ends=big.ptr.value + (payload(n, 9) - 1) // 16 * 16), b"ends_dev overlaps packed_dev"),
              ("values are the ends", dict(values=big.ptr.value, ends=big.ptr.value), b"values_dev overlaps ends_dev"),
              ("ends start inside the values", dict(values=big.ptr.value, ends=big.ptr.value + 1024), b"values_dev overlaps ends_dev"),
              ("values are the workspace", dict(ws=big.ptr.value, values=big.ptr.value), b"values_dev overlaps ws_dev"),
              ("ends start in the workspace's last word", dict(ws=big.ptr.value, ends=big.ptr.value + 16), b"ends_dev overlaps ws_dev"))
    assert n > top(11) and 2048 > top(11)
    buffers = (e.values, e.ends, e.count, e.ws, big)
    for what, kw, word in errors:
        for g in buffers:
            g.t.fill_(SENTINEL)
        assert e.call(L, **kw) == E_INVALID, what
        assert word in L.mi355_last_error(), (what, L.mi355_last_error())
        assert record(L, eng) == [], what
        for g in buffers:
            assert (g.fetch() == SENTINEL).all(), what
    # the rule's other side: n = 2^ce - 1 is fine
    Enc(O, eng, heads(9, 2047), 9, 11).run(L)
    Enc(O, eng, np.zeros(1, dtype=np.uint32), 9, 1).run(L)
    e.run(L)
    assert record(L, eng) == valid
    # run_decode
    values, ends = runs_of(x)
    d = Dec(O, eng, values, ends, 9, 12, n, runs_dev=len(ends))
    d.run(L)
    vt, et, out = d.vt.data_ptr(), d.et.data_ptr(), d.out.ptr.value
    errors = (("cv = 0", dict(cv=0), b"width"), ("cv = 33", dict(cv=33), b"width"), ("ce = 0", dict(ce=0), b"width"), ("ce = 33", dict(ce=33), b"width"),
              ("miss = 2^cv", dict(miss=512), b"miss"), ("runs = 2^32", dict(runs=1 << 32), b"runs"),
              ("runs_dev at +4", dict(runs_dev=d.runs_dev.data_ptr() + 4), b"runs_dev"), ("counter at +4", dict(counter=d.counter.ptr.value + 4), b"uncovered_dev"),
              ("values at +2", dict(values=vt + 2), b"values_dev"), ("ends at +1", dict(ends=et + 1), b"ends_dev"),
              ("null output", dict(out=None), b"out_dev"), ("output at +8", dict(out=out + 8), b"out_dev"),
              ("null values", dict(values=None), b"values_dev"), ("null ends", dict(ends=None), b"ends_dev"),
              ("output is the values", dict(values=big.ptr.value, out=big.ptr.value), b"out_dev overlaps values_dev"),
              ("ends start inside the output", dict(ends=big.ptr.value + (payload(n, 9) - 1) // 4 * 4, out=big.ptr.value), b"out_dev overlaps ends_dev"))
    buffers = (d.out, d.counter, big)
    for what, kw, word in errors:
        for g in buffers:
            g.t.fill_(SENTINEL)
        assert d.call(L, **kw) == E_INVALID, what
        assert word in L.mi355_last_error(), (what, L.mi355_last_error())
        assert record(L, eng) == [], what
        for g in buffers:
            assert (g.fetch() == SENTINEL).all(), what
    d.run(L)


# ---- graph capture ----

N_CAP = 3 * CHUNK + 1237


@functools.lru_cache(maxsize=None)
def capture_versions():
    """two columns of other runs, other values (the second counts its runs from 100) and another number of runs"""
    return [frozen(((heads(9, N_CAP, mean=mean, seed=salt) + from_) & 511).astype(np.uint32)) for mean, salt, from_ in ((12, 11, 0), (300, 12, 100))]


def test_capture_data_is_not_vacuous():
    (v0, e0), (v1, e1) = (runs_of(x) for x in capture_versions())
    assert len(e1) * 8 < len(e0) and (v0[: len(v1)] != v1).any() and (e0[: len(e1)] != e1).any(), "a stale result could pass"


@gpu
@pytest.mark.parametrize("chain", [False, True], ids=["run_encode", "run_encode-then-run_decode"])
def test_graph_capture_and_replay(O, chain):
    """the caller's workspace full of SENTINEL and no larger call in front; replays follow the column overwritten in place -- another
    number of runs, which run_decode reads from the device word run_encode left"""
    import torch

    versions = capture_versions()
    n, c, ce = N_CAP, 9, 16
    wants = [runs_of(x) for x in versions]

    def steps(eng):
        from shared_simd_scan_amd.engine import PackedColumn

        stage = [plain_pack(O, x, c) for x in versions]
        col = PackedColumn(torch.empty_like(stage[0]), n, c)
        values, ends, count, ws, back = Guarded(dwords(n, c)), Guarded(dwords(n, ce)), Guarded(8, back=64, front=64), Guarded(8 * words_of(n)), Guarded(payload(n, c))
        guarded = (values, ends, count, ws, back)
        views = [g.t[g.front: g.front + g.nbytes] for g in guarded]

        def load(v):
            col.data.copy_(stage[v])
            for g in guarded:
                g.t.fill_(SENTINEL)

        def run():
            eng.run_encode(col, ends_width=ce, values=views[0], ends=views[1], count=views[2].view(torch.int64), workspace=views[3].view(torch.int64))
            if chain:
                eng.run_decode(PackedColumn(views[0], n, c), PackedColumn(views[1], n, ce), n, runs=views[2].view(torch.int64), out=views[4])

        def check(v, what):
            want_v, want_e = wants[v]
            r = len(want_e)
            assert int(count.fetch().view(np.int64)[0]) == r, what
            hv, he = values.fetch(), ends.fetch()
            assert (hv[: payload(r, c)] == O.pack(want_v, c)[: payload(r, c)]).all() and (hv[payload(r, c):] == SENTINEL).all(), what
            assert (he[: payload(r, ce)] == O.pack(want_e, ce)[: payload(r, ce)]).all() and (he[payload(r, ce):] == SENTINEL).all(), what
            ws.fetch()
            if chain:
                assert (back.fetch() == O.pack(versions[v], c)[: payload(n, c)]).all(), what
            else:
                assert (back.fetch() == SENTINEL).all(), what

        def untouched():
            for g in guarded:
                assert (g.fetch() == SENTINEL).all()

        def warmed(launched):
            names = [base_name(x[0]) for x in launched]
            if chain:
                assert names == [DECODE_KERNEL]
            else:
                assert names == [COUNT_KERNEL, SCAN_KERNEL, EDGES_KERNEL, EDGES_KERNEL, EMIT_KERNEL]

        return capture.Steps(load, run, check, untouched, warmed)

    capture.capture_replay(steps, (0, 1, 0))
