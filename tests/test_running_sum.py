"""Prefix sums and differences of a packed column (include/mi355_running.h, ScanEngine.running_sum / delta):
out[i] = r_i if 0 <= r_i < 2^co else miss, with r_i = k + the terms x_j + b of the selected rows j <= i (exclusive: j < i), or
r_i = x_i - x_{i-1} + k; packed in and out.

CPU: the header is plain C99 and declares exactly what _capi.HEADERS binds for it and the library exports; it carries both
graph-capture verdicts; mi355_running_sum_kernel and mi355_delta_kernel (pure arithmetic) name the family on both sides of every
boundary of their rules and refuse what the range rule refuses; the workspace formula; the engine wrappers hand the C ABI what they
should (through a recording stand-in for the library); every __global__ under csrc/running/ is asserted from the launch record by a
GPU case of this file; no source there reads a switch bit or reaches the context's workspace or scratch; the data recipes are not
vacuous.

GPU (-m gpu): every expectation is numpy on data the test generated -- np.cumsum in int64 (exact under the range rule), Python
integers for word 0 of the 64-bit cases, np.diff for delta -- packed with the oracle's packer; nothing is derived from engine
output.  Every output (column, result words, counter) and the workspace sit in support.Guarded buffers full of SENTINEL; the
ceil(n co / 8) payload bytes (trailing bits of the last one included) and the guards on both sides are compared exactly.  Every
column is uploaded in hostile surroundings: ones in the bits behind row n - 1 and in the pad.

A lane owns 32 rows, a tile is 2048, a chunk (one word of the workspace) 16384, a scan group 1024 chunks: the sizes are the smallest
on both sides of each.

The recipes of the checked kernels (walk, delta_values) keep at least an eighth of the rows on either side of the range; the
64-bit carry columns (carry_cases) are the fixed ones their test names: all rows, only the last rows, or none are in range.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import capture
import support
from support import E_INVALID, SENTINEL, Guarded, L, base_name, eng, fake, hostile_bitmap, hostile_pack, packbits, plain_pack, record  # noqa: F401  (L, eng, fake: fixtures)

HEADER = "mi355_running.h"
INCLUSIVE, EXCLUSIVE = 0, 1
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)

# the kernels of csrc/running/, as the launch record names them
TOTALS_KERNEL = "running_sum_totals_kernel"
EXACT_KERNEL = "running_sum_exact_kernel"
CHECKED_KERNEL = "running_sum_checked_kernel"
DELTA_EXACT_KERNEL = "delta_exact_kernel"
DELTA_CHECKED_KERNEL = "delta_checked_kernel"
SCAN_KERNEL = "rowid_scan_kernel"  # kernels/bitmap.hpp, as it stands

LANE, R, CHUNK, GROUP = 32, 2048, 16384, 1024
N_BIG = 9 * 8192 + 1237          # five chunks, the last ragged in tile, lane and byte
N_GROUPS = 1025 * CHUNK + 77     # a second scan group: the carry comes from group_totals
N_CARRY = 2 * CHUNK + 77
N_WALK = CHUNK + R + 100         # the crossings' case: a chunk boundary, tile and lane boundaries
N_ONE_BLOCK = 9 * CHUNK + 123    # ten chunks for the four waves of a one-block grid
SIZES = [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 16383, 16384, 16385, N_BIG]

gpu = pytest.mark.gpu


def top(c):
    return (1 << c) - 1


def payload(n, c):
    return (n * c + 7) // 8


def miss_of(co):
    return 1 if co == 1 else 0x5A5A5A5A & top(co)


def words_of(n):
    """mi355_compact.h's chunk prefix: ceil(n / 16384) + 1 + ceil(n / 16777216)"""
    nchunks = -(-n // CHUNK)
    return nchunks + 1 + -(-nchunks // GROUP)


def rule(c, n, b, k):
    """the issue's range rule, in Python ints"""
    return k + n * min(0, b), k + n * max(0, top(c) + b)


def want_family(c, n, b, k, co):
    lo, hi = rule(c, n, b, k)
    assert INT64_MIN <= lo and hi <= INT64_MAX
    return EXACT_KERNEL if lo >= 0 and hi <= top(co) else CHECKED_KERNEL


def want_delta_family(c, k, co):
    return DELTA_EXACT_KERNEL if k >= top(c) and k + top(c) < 1 << co else DELTA_CHECKED_KERNEL


# ---- recipes ------------------------------------------------------------------------------------------------------------------

def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def walk(c, co, n, seed=0, bottom=False, forced=()):
    """-> (x uint32[n], b, k): a column whose running sum crosses one edge of [0, 2^co) again and again.  c >= 2: b = -s with
    s = (2^c - 1) // 2, so a term lies in [-s, s]; the sum is 2^co + w_i (bottom: w_i) with w_i drawn per row on the side a two-state
    chain names (it flips with probability 1/16; `forced`: (row, inside) pairs laid over it), |w_i| small enough for any two to be
    one term apart.  c == 1 admits no negative term: the sum climbs and crosses 2^co once, at row n // 2."""
    rng = np.random.default_rng([c, co, n, seed, int(bottom)])
    A = 1 << co
    if c == 1:
        assert not bottom and not forced
        m = min(A, max(n // 4, 1))  # ones among the rows 0 .. n // 2, the last of them AT n // 2
        x = np.zeros(n, dtype=np.uint32)
        if n // 2 > 0:
            x[rng.choice(n // 2, size=min(m - 1, n // 2), replace=False)] = 1
        x[n // 2] = 1
        x[n // 2 + 1:] = rng.integers(0, 2, n - n // 2 - 1)
        return frozen(x), 0, A - int(x[: n // 2 + 1].sum())
    s = top(c) // 2
    J = (s - 1) // 2
    inside = (np.cumsum(rng.random(n) < 1 / 16) & 1) == 0
    for row, state in forced:
        if row < n:
            inside[row] = state
    u = rng.integers(0, min(J, A - 1) + 1, n, dtype=np.int64)
    v = rng.integers(0, J + 1, n, dtype=np.int64)
    if bottom:
        r, k = np.where(inside, u, -1 - v), 0
    else:
        r, k = A + np.where(inside, -1 - u, v), A - 1
    x = np.diff(r, prepend=k) + s
    assert x.min() >= 0 and x.max() <= top(c)
    return frozen(x.astype(np.uint32)), -s, k


@functools.lru_cache(maxsize=None)
def uniform(c, n, seed=0):
    return frozen(np.random.default_rng([c, n, seed, 77]).integers(0, 1 << c, n, dtype=np.uint64).astype(np.uint32))


@functools.lru_cache(maxsize=None)
def mask_bits(kind, n, seed=0):
    rng = np.random.default_rng([n, seed, 99])
    if kind == "zero":
        m = np.zeros(n, dtype=bool)
    elif kind == "one":
        m = np.ones(n, dtype=bool)
    elif kind == "coin":
        m = rng.random(n) < 1 / 8
    elif kind == "half":
        m = rng.random(n) < 1 / 2
    else:
        assert kind == "ends"
        m = np.zeros(n, dtype=bool)
        m[0] = m[n - 1] = True
    return frozen(m)


@functools.lru_cache(maxsize=None)
def walk_under(c, co, n, kind, seed=0):
    """walk() laid on the rows a mask selects, uniform junk on the others -> (x, b, k, selected)"""
    sel = mask_bits(kind, n, seed)
    x = uniform(c, n, seed + 1).copy()
    b, k = -(top(c) // 2), (1 << co) - 1
    if sel.any():
        forced = ((0, True), (1, False)) if kind == "ends" else ()
        xs, b, k = walk(c, co, int(sel.sum()), seed, False, forced)
        x[sel] = xs
    return frozen(x), b, k, sel


def expect_sum(x, b, k, co, miss, sel=None, exclusive=False):
    """-> (the co-bit values the call writes, word 0, word 1): np.cumsum in int64, exact under the range rule"""
    t = x.astype(np.int64) + np.int64(b)
    if sel is not None:
        t = np.where(sel, t, 0)
    incl = np.int64(k) + np.cumsum(t, dtype=np.int64)
    r = incl - t if exclusive else incl
    inside = (r >= 0) & (r < (1 << co))
    word0 = int(k) + int(t.sum(dtype=np.int64))  # a Python int
    return np.where(inside, r, miss).astype(np.uint32), word0, int((~inside).sum())


@functools.lru_cache(maxsize=None)
def delta_values(c, co, n, seed=0):
    """a column for delta with k = 0: three quarters of the rows below 2^min(c, co) (half of their differences are descents, the
    others in range), a quarter anywhere (differences of either sign beyond 2^co)"""
    rng = np.random.default_rng([c, co, n, seed, 5])
    x = rng.integers(0, 1 << min(c, co), n, dtype=np.uint64)
    wide = rng.random(n) < 1 / 4
    x[wide] = rng.integers(0, 1 << c, int(wide.sum()), dtype=np.uint64)
    return frozen(x.astype(np.uint32))


def expect_delta(x, first, k, co, miss):
    """-> (values, rows replaced): np.diff in int64"""
    d = np.diff(x.astype(np.int64), prepend=np.int64(first)) + np.int64(k)
    inside = (d >= 0) & (d < (1 << co))
    return np.where(inside, d, miss).astype(np.uint32), int((~inside).sum())


def lead_rows(c):
    """the fewest rows in front of a row-range view of c bits that starts 16 bytes behind a 32-byte boundary"""
    return next(r for r in range(1, 4096) if (r * c) % 8 == 0 and (r * c // 8) % 32 == 16)


def exact_case(co):
    """-> (c, n): sums of uniform rows with b = k = 0 that the rule keeps inside co bits at N_BIG rows, or at the most rows it admits"""
    if co >= 18:
        return min(co - 17, 15), N_BIG  # N_BIG < 2^17
    return 1, min(N_BIG, top(co))


CROSSINGS = tuple((row, True) for row in (40, 3 * R + LANE - 1, R - 1, CHUNK - 1, 70, 5 * R + LANE, 2 * R, CHUNK + R)) + \
    tuple((row, False) for row in (41, 3 * R + LANE, R, CHUNK, 69, 5 * R + LANE - 1, 2 * R - 1, CHUNK + R - 1))
C_SWEEP_CO = 20
CO_SWEEP_C = 9

# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------


def test_running_header_is_plain_c99():
    support.check_header_is_plain_c99(HEADER)


def test_running_header_declares_what_python_binds(L):
    names, sigs = support.check_header_binds(L, HEADER)
    assert names == ["mi355_delta_dev", "mi355_delta_kernel", "mi355_running_sum_dev", "mi355_running_sum_kernel", "mi355_running_sum_workspace_words"]
    sig = sigs["mi355_running_sum_dev"]
    assert sig[2] is C.c_uint64 and sig[3] is C.c_uint and sig[5] is C.c_int64 and sig[6] is C.c_int64 and sig[7] is C.c_uint and sig[8] is C.c_uint
    assert sig[9] is C.c_uint32 and len(sig) == 13
    sig = sigs["mi355_delta_dev"]
    assert sig[2] is C.c_uint64 and sig[3] is C.c_uint and sig[4] is C.c_uint32 and sig[5] is C.c_int64 and sig[6] is C.c_uint and sig[7] is C.c_uint32 and len(sig) == 10
    assert sigs["mi355_running_sum_kernel"] == [C.c_uint, C.c_uint64, C.c_int64, C.c_int64, C.c_uint]
    assert sigs["mi355_delta_kernel"] == [C.c_uint, C.c_int64, C.c_uint]
    assert L.mi355_running_sum_kernel.restype is C.c_char_p and L.mi355_delta_kernel.restype is C.c_char_p
    assert L.mi355_running_sum_workspace_words.restype is C.c_uint64
    text = support.header_text(HEADER)
    assert '#include "mi355_scan.h"' in text and text.count("#include") == 1
    assert support.header_macro(HEADER, "MI355_RUNNING_INCLUSIVE") == INCLUSIVE and support.header_macro(HEADER, "MI355_RUNNING_EXCLUSIVE") == EXCLUSIVE


def test_running_names_are_exported():
    import shared_simd_scan_amd as pkg

    for name in ("running_sum_kernel", "delta_kernel", "running_sum_workspace_words"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    for name in ("running_sum", "delta", "delta_decode", "row_positions", "is_sorted"):
        assert callable(getattr(pkg.ScanEngine, name))


def test_running_header_carries_both_capture_verdicts():
    text = support.header_text(HEADER)
    assert len(re.findall(r"graph capture: capturable\b", text)) == 2
    support.check_capture_verdict(HEADER, r"needs no warm-up call, whatever its arguments", r"caller's workspace", r"zeroing of out_of_range_dev",
                                  r"read at every\s+\*?\s*replay")


def test_running_sum_kernel_at_the_boundaries(L):
    """needs neither a device nor a context; the family follows [k + n lo_t, k + n hi_t] against [0, 2^co - 1]"""
    from shared_simd_scan_amd import running_sum_kernel

    f = L.mi355_running_sum_kernel
    exact, checked = EXACT_KERNEL.encode(), CHECKED_KERNEL.encode()
    # hi == 2^co - 1 against 2^co: n rows of 9 bits, hi = 511 n + k = 65408 + k
    assert f(9, 100, 0, 0, 16) == exact and f(9, 128, 0, 127, 16) == exact and f(9, 128, 0, 128, 16) == checked
    assert f(9, 128, 0, 128, 17) == exact and f(9, 128, 0, 127, 15) == checked
    # lo == 0 against -1
    assert f(9, 100, -3, 300, 16) == exact and f(9, 100, -3, 299, 16) == checked
    assert f(9, 100, 0, 0, 16) == exact and f(9, 100, 0, -1, 16) == checked
    # hi_t = max(0, 2^c - 1 + b): a b below -(2^c - 1) only lowers lo
    assert f(9, 100, -511, 51100, 16) == exact and f(9, 100, -512, 51200, 16) == exact and f(9, 100, -512, 51199, 16) == checked
    assert f(9, 100, -512, 65535, 16) == exact and f(9, 100, -512, 65536, 16) == checked
    # the position case: the bitmap as the column, n < 2^32 rows into 32 bits; n = 2^32 no longer
    assert f(1, top(32), 0, 0, 32) == exact and f(1, 1 << 32, 0, 0, 32) == checked
    for co in range(1, 33):  # the widest exact sum at every width, and one beyond it
        assert f(1, top(co), 0, 0, co) == exact and f(1, top(co), 0, 1, co) == checked, co
        assert f(co, 1, 0, 0, co) == exact and f(co, 2, 0, 0, co) == checked, co
    # n == 0: the interval is [k, k]
    assert f(9, 0, -5, 7, 3) == exact and f(9, 0, -5, 8, 3) == checked and f(9, 0, INT64_MIN, INT64_MAX, 3) == checked
    # NULL for a bad width
    for bad in (0, 33, 1 << 31):
        assert f(bad, 10, 0, 0, 10) is None and f(9, 10, 0, 0, bad) is None, bad
    # the range rule at INT64_MAX and one beyond, for hi_t = 511, 1 and 2^32 - 1, and on the INT64_MIN side
    for c, n in ((9, 1000), (1, 12345), (32, 1 << 20), (9, 1)):
        edge = INT64_MAX - n * top(c)
        assert f(c, n, 0, edge, 32) == checked and f(c, n, 0, edge + 1, 32) is None, (c, n)
        assert f(c, n, 5, edge - 5 * n, 32) == checked and f(c, n, 5, edge - 5 * n + 1, 32) is None, (c, n)
        low = INT64_MIN + 7 * n
        assert f(c, n, -7, low, 32) == checked and f(c, n, -7, low - 1, 32) is None, (c, n)
    assert f(9, 1 << 40, INT64_MIN, 0, 32) is None and f(9, 1 << 40, INT64_MAX, 0, 32) is None
    assert f(9, 1, INT64_MIN, 0, 32) == checked and f(9, 1, INT64_MIN, -1, 32) is None
    assert f(9, 1, INT64_MAX - 511, 0, 32) == checked and f(9, 1, INT64_MAX - 510, 0, 32) is None
    assert f(1, 1 << 63, 0, 0, 32) is None  # n beyond 2^62
    # the Python face: the same answers, and ValueError for what the call would refuse or ctypes would wrap
    assert running_sum_kernel(9, 128, 0, 127, 16) == EXACT_KERNEL and running_sum_kernel(9, 128, 0, 128, 16) == CHECKED_KERNEL
    assert running_sum_kernel(9, 128) == EXACT_KERNEL and running_sum_kernel(9, 128, 0, 511) == EXACT_KERNEL  # co=None: the width that holds hi
    for bad in ((0, 10, 0, 0, 10), (9, 10, 0, 0, 33), (9, 10, 0, 0, -1), (9, 10, 0, 0, (1 << 32) + 10), (9, 10, 1 << 63, 0, 10), (9, 10, 0, -(1 << 63) - 1, 10),
                (9, 1000, 0, INT64_MAX - 1000 * 511 + 1, 32), (9, 10, 0, -1), (9, 10, -1, 0), (32, 2, 0, 0), (9, -1, 0, 0, 10)):
        with pytest.raises(ValueError):
            running_sum_kernel(*bad)


def test_delta_kernel_at_the_boundaries(L):
    from shared_simd_scan_amd import delta_kernel

    f = L.mi355_delta_kernel
    exact, checked = DELTA_EXACT_KERNEL.encode(), DELTA_CHECKED_KERNEL.encode()
    for c in range(1, 32):  # k >= 2^c - 1, and k + 2^c - 1 < 2^co
        assert f(c, top(c), c + 1) == exact and f(c, top(c) - 1, c + 1) == checked and f(c, top(c), c) == checked, c
        assert f(c, top(c) + 1, c + 1) == exact and f(c, top(c) + 2, c + 1) == checked, c
        assert f(c, top(32) - top(c), 32) == exact and f(c, top(32) - top(c) + 1, 32) == checked, c
    assert f(32, top(32), 32) == checked and f(32, 0, 32) == checked and f(9, 0, 9) == checked and f(9, -1, 32) == checked
    assert f(9, INT64_MAX, 32) == checked and f(9, INT64_MIN, 32) == checked  # no range rule: the wrapped result is out of range too
    for bad in (0, 33, 1 << 31):
        assert f(bad, 0, 10) is None and f(9, 0, bad) is None, bad
    assert delta_kernel(9, 511, 10) == DELTA_EXACT_KERNEL and delta_kernel(9, 511) == DELTA_EXACT_KERNEL and delta_kernel(9) == DELTA_CHECKED_KERNEL
    for bad in ((0, 0, 9), (9, 0, 33), (9, 1 << 63, 9), (9, 0, -1), (9, 0, 1 << 32), (32, 1)):
        with pytest.raises(ValueError):
            delta_kernel(*bad)


def test_workspace_words_are_the_chunk_prefix(L):
    from shared_simd_scan_amd import running_sum_workspace_words

    for n, want in ((0, 1), (1, 3), (16384, 3), (16385, 4), (1 << 24, 1024 + 1 + 1), ((1 << 24) + 1, 1025 + 1 + 2)):
        assert L.mi355_running_sum_workspace_words(n) == want == words_of(n) == running_sum_workspace_words(n), n
    assert words_of(N_GROUPS) == 1026 + 1 + 2  # 1025 full chunks and a ragged one, in two scan groups


def test_wrappers_pass_what_the_abi_takes(fake, L):
    import torch

    eng, rec, col = fake
    rec.mi355_running_sum_workspace_words = lambda n: words_of(n)  # (the stand-in answers 0 to everything it records)

    def last():
        (name, a), = rec.calls
        rec.calls.clear()
        return name, a

    c1 = col(9, 777)
    res, result = eng.running_sum(c1)  # defaults: no mask, b = k = 0, inclusive, the width that holds 777 * 511, miss 0, fresh buffers, the engine's workspace
    name, a = last()
    assert name == "mi355_running_sum_dev" and a[1:10] == [c1.data.data_ptr(), 777, 9, None, 0, 0, INCLUSIVE, 19, 0]
    assert res.data.numel() == L.mi355_compressed_buffer_size(19, 777) and a[10] == res.data.data_ptr() and (res.n, res.c) == (777, 19)
    assert result.dtype == torch.int64 and result.numel() == 2 and a[11] == result.data_ptr()
    ws = eng._running_ws[-1]
    assert a[12] == ws.data_ptr() and ws.dtype == torch.int64 and ws.numel() >= words_of(777)
    eng.running_sum(c1)
    assert last()[1][12] == ws.data_ptr() and len(eng._running_ws) == 1  # kept between calls
    eng.running_sum(col(9, 5 * CHUNK))
    assert len(eng._running_ws) == 2 and eng._running_ws[0] is ws and eng._running_ws[1].numel() >= words_of(5 * CHUNK)  # grown, the old one kept alive
    rec.calls.clear()
    mask = torch.zeros(98, dtype=torch.uint8)
    out = torch.zeros(payload(777, 13), dtype=torch.uint8)
    result = torch.zeros(2, dtype=torch.int64)
    mine = torch.zeros(words_of(777), dtype=torch.int64)
    res, got = eng.running_sum(c1, mask=mask, b=-(1 << 40), k=INT64_MIN + (1 << 60), exclusive=True, co=13, miss=8191, out=out, result=result, workspace=mine)
    name, a = last()
    assert a[1:] == [c1.data.data_ptr(), 777, 9, mask.data_ptr(), -(1 << 40), INT64_MIN + (1 << 60), EXCLUSIVE, 13, 8191, out.data_ptr(), result.data_ptr(),
                     mine.data_ptr()]
    assert res.data is out and got is result and (res.n, res.c) == (777, 13)
    for bad in (dict(miss=-1), dict(miss=1 << 13), dict(co=0), dict(co=33), dict(b=1 << 63), dict(k=-(1 << 63) - 1)):
        with pytest.raises(ValueError):  # what ctypes would wrap silently
            eng.running_sum(c1, **{"co": 13, **bad})
    for bad in (dict(k=-1), dict(b=-1), dict(k=1 << 32), dict(b=1 << 23)):  # co=None: lo < 0, or hi >= 2^32
        with pytest.raises(ValueError):
            eng.running_sum(c1, **bad)
    for bad in (dict(out=torch.zeros(payload(777, 13) - 1, dtype=torch.uint8)), dict(mask=torch.zeros(97, dtype=torch.uint8)),
                dict(result=torch.zeros(2, dtype=torch.int32)), dict(result=torch.zeros(1, dtype=torch.int64)),
                dict(workspace=torch.zeros(words_of(777) - 1, dtype=torch.int64)), dict(workspace=torch.zeros(64, dtype=torch.int32))):
        with pytest.raises(AssertionError):
            eng.running_sum(c1, co=13, **bad)
    assert rec.calls == []
    # delta
    res = eng.delta(c1)  # defaults: first = k = 0, co = c, miss 0, no counter
    name, a = last()
    assert name == "mi355_delta_dev" and a[1:8] == [c1.data.data_ptr(), 777, 9, 0, 0, 9, 0] and a[8] == res.data.data_ptr() and a[9] is None
    assert (res.n, res.c) == (777, 9) and res.data.numel() == L.mi355_compressed_buffer_size(9, 777)
    cnt = torch.zeros(1, dtype=torch.int64)
    res = eng.delta(c1, first=511, k=511, miss=1023, out_of_range=cnt)  # co=None: the width that holds k + 2^c - 1
    name, a = last()
    assert a[4:8] == [511, 511, 10, 1023] and a[9] == cnt.data_ptr() and res.c == 10
    for bad in (dict(first=512), dict(first=-1), dict(miss=512), dict(co=0), dict(co=33), dict(k=1 << 63), dict(k=top(32))):
        with pytest.raises(ValueError):
            eng.delta(c1, **bad)
    with pytest.raises(AssertionError):
        eng.delta(c1, out_of_range=torch.zeros(1, dtype=torch.int32))
    assert rec.calls == []
    # the conveniences
    res, result = eng.delta_decode(c1, 1000, min_delta=-3)
    name, a = last()
    assert name == "mi355_running_sum_dev" and a[4:10] == [None, -3, 1000, INCLUSIVE, 32, 0] and res.c == 32
    eng.delta_decode(c1, 5, co=21)
    assert last()[1][5:9] == [0, 5, INCLUSIVE, 21]
    bitmap = torch.zeros(payload(777, 1) + 32, dtype=torch.uint8)
    res, result = eng.row_positions(bitmap, 777)
    name, a = last()
    assert name == "mi355_running_sum_dev" and a[1:10] == [bitmap.data_ptr(), 777, 1, None, 0, 0, EXCLUSIVE, 10, 0] and (res.n, res.c) == (777, 10)
    eng.row_positions(bitmap, 1023)
    assert last()[1][8] == 10
    eng.row_positions(torch.zeros(128 + 32, dtype=torch.uint8), 1024)  # position 1024 itself is word 0's, and must fit
    assert last()[1][8] == 11
    counter = eng.is_sorted(c1)
    name, a = last()
    assert name == "mi355_delta_dev" and a[2:8] == [777, 9, 0, 0, 9, 0] and a[9] == counter.data_ptr() and counter.dtype == torch.int64


def test_every_running_kernel_has_a_case():
    kernels = support.global_kernels_of("running")
    assert kernels == {TOTALS_KERNEL, EXACT_KERNEL, CHECKED_KERNEL, DELTA_EXACT_KERNEL, DELTA_CHECKED_KERNEL}, kernels
    support.check_gpu_part_asserts(__file__, "TOTALS_KERNEL", "EXACT_KERNEL", "CHECKED_KERNEL", "DELTA_EXACT_KERNEL", "DELTA_CHECKED_KERNEL")
    # all 4 x 32 instantiations run
    for co in range(1, 33):
        c, n = exact_case(co)
        assert want_family(c, n, 0, 0, co) == EXACT_KERNEL and n >= 1, co
        x, b, k = walk(CO_SWEEP_C, co, N_BIG)
        assert want_family(CO_SWEEP_C, N_BIG, b, k, co) == CHECKED_KERNEL, co
        assert want_delta_family(min(co - 1, 9), top(min(co - 1, 9)), co) == DELTA_EXACT_KERNEL or co == 1
        assert want_delta_family(CO_SWEEP_C, 0, co) == DELTA_CHECKED_KERNEL
    assert want_delta_family(1, 0, 1) == DELTA_CHECKED_KERNEL  # co = 1 admits no exact delta: k >= 1 and k + 1 < 2 exclude each other


def test_running_sources_read_no_flag_bits_and_no_context_state():
    assert [os.path.basename(p) for p in support.feature_sources("running")] == ["delta.hip", "running.hpp", "running_sum.hip"]
    support.check_sources_read_no_flag_bits("running")
    mine = {name for name, path, _ in support.hip_functions() if path.startswith("running" + os.sep)}
    assert {"mi355_running_sum_dev", "mi355_delta_dev", "mi355_running_sum_kernel", "mi355_delta_kernel", "mi355_running_sum_workspace_words"} <= mine
    assert not mine & set(support.entry_points_reaching("rowid_ws_get("))
    assert not mine & set(support.entry_points_reaching("kernel_scratch"))
    for path in support.feature_sources("running"):
        text = open(path).read()
        assert "rowid_ws_get(" not in text and "kernel_scratch" not in text and "pool_get(" not in text, path


def test_library_agrees_with_this_files_rule(L):
    """(no device needed) the families the GPU cases assert are the library's"""
    f, g = L.mi355_running_sum_kernel, L.mi355_delta_kernel
    for co in range(1, 33):
        c, n = exact_case(co)
        assert f(c, n, 0, 0, co).decode() == EXACT_KERNEL
        x, b, k = walk(CO_SWEEP_C, co, N_BIG)
        assert f(CO_SWEEP_C, N_BIG, b, k, co).decode() == CHECKED_KERNEL
        assert g(CO_SWEEP_C, 0, co).decode() == want_delta_family(CO_SWEEP_C, 0, co)
    for c in range(1, 33):
        x, b, k = walk(c, C_SWEEP_CO, N_BIG)
        assert f(c, N_BIG, b, k, C_SWEEP_CO).decode() == want_family(c, N_BIG, b, k, C_SWEEP_CO) == CHECKED_KERNEL, c


def fractions(want_inside):
    return want_inside.mean(), 1 - want_inside.mean()


def checked_recipes():
    """(label, c, x, b, k, co, selected or None) of every walk() a GPU case runs on"""
    for co in range(1, 33):
        yield (f"co{co}", CO_SWEEP_C) + walk(CO_SWEEP_C, co, N_BIG) + (co, None)
    for c in range(1, 33):
        yield (f"c{c}", c) + walk(c, C_SWEEP_CO, N_BIG) + (C_SWEEP_CO, None)
    for n in SIZES:
        if n >= 64:
            yield (f"n{n}", 9) + walk(9, 12, n) + (12, None)
    yield ("groups", 9) + walk(9, 12, N_GROUPS) + (12, None)
    yield ("one block", 9) + walk(9, 12, N_ONE_BLOCK) + (12, None)
    for bottom in (False, True):
        yield (f"crossings{int(bottom)}", 9) + walk(9, 12, N_WALK, 3, bottom, CROSSINGS) + (12, None)
    for kind in ("one", "coin", "half"):
        x, b, k, sel = walk_under(9, 12, N_BIG, kind)
        yield (kind, 9, x, b, k, 12, sel)


def test_recipes_are_not_vacuous():
    """(no device needed) every recipe of the checked kernel keeps at least an eighth of the rows in range and at least an eighth
    replaced; where the column admits negative terms the replaced rows are no suffix; the forced crossings sit where they should"""
    seen = 0
    for label, c, x, b, k, co, sel in checked_recipes():
        want, word0, outside = expect_sum(x, b, k, co, miss_of(co), sel)
        n = len(x)
        assert int(x.max()) <= top(c) and (c < 6 or int(x.max()) >> (c - 2)), label  # inside the width, and using its top bits
        assert outside >= n / 8 and n - outside >= n / 8, (label, outside, n)
        t = x.astype(np.int64) + b
        r = k + np.cumsum(t if sel is None else np.where(sel, t, 0))
        inside = (r >= 0) & (r < (1 << co))
        if b < 0:  # non-monotone: rows are in range again behind replaced ones
            first_out = int(np.argmax(~inside))
            assert inside[first_out:].any(), label
            assert (np.diff(r) < 0).any() and (np.diff(r) > 0).any(), label
        seen += 1
    assert seen == 32 + 32 + 9 + 2 + 2 + 3
    for bottom in (False, True):
        x, b, k = walk(9, 12, N_WALK, 3, bottom, CROSSINGS)
        r = k + np.cumsum(x.astype(np.int64) + b)
        inside = (r >= 0) & (r < (1 << 12))
        for row, state in CROSSINGS:
            assert bool(inside[row]) == state, (bottom, row)
        for edge in (41, 3 * R + LANE, R, CHUNK):  # in range in front of it, replaced from it on: inside a run, at a lane, a tile, a chunk
            assert inside[edge - 1] and not inside[edge]
        for edge in (70, 5 * R + LANE, 2 * R, CHUNK + R):  # and back
            assert not inside[edge - 1] and inside[edge]
        assert (r < 0).any() == bottom and (r >= 1 << 12).any() == (not bottom)
    # the masks
    assert not mask_bits("zero", N_BIG).any() and mask_bits("one", N_BIG).all() and 0.1 < mask_bits("coin", N_BIG).mean() < 0.15
    ends = mask_bits("ends", N_BIG)
    assert ends.sum() == 2 and ends[0] and ends[-1]
    x, b, k, sel = walk_under(9, 12, N_BIG, "ends")
    want, word0, outside = expect_sum(x, b, k, 12, miss_of(12), sel)
    assert outside == 1 and want[0] != want[-1] == miss_of(12)  # in range up to the last row, which alone is replaced
    # delta
    for co in range(1, 33):
        x = delta_values(CO_SWEEP_C, co, N_BIG)
        want, outside = expect_delta(x, 0, 0, co, miss_of(co))
        assert outside >= N_BIG / 8 and N_BIG - outside >= N_BIG / 8, co
    for c in range(1, 33):
        x = delta_values(c, 12, N_BIG)
        want, outside = expect_delta(x, 0, 0, 12, miss_of(12))
        assert outside >= N_BIG / 8 and N_BIG - outside >= N_BIG / 8 and int(x.max()) <= top(c), c
        assert c < 6 or int(x.max()) >> (c - 3), c  # the top bits are used


def test_carry_columns_need_64_bits():
    """(no device needed) the 64-bit cases: a chunk's total of 2^32 - 1 rows exceeds 32 bits, and word 0 is computed in Python ints"""
    n = N_CARRY
    assert n > CHUNK and CHUNK * top(32) >= 1 << 45
    for b, k, co in carry_cases():
        lo, hi = rule(32, n, b, k)
        assert INT64_MIN <= lo and hi <= INT64_MAX and want_family(32, n, b, k, co) == CHECKED_KERNEL
    b, k, co = carry_cases()[1]
    r = [k + (i + 1) * top(32) for i in range(n)]
    assert [i for i in range(n) if 0 <= r[i] < 1 << 32] == [n - 6, n - 5]  # only the last rows are in range


def carry_cases():
    n = N_CARRY
    return [(-(top(32) - 1), 0, 16),                      # every term is 1: row i holds i + 1
            (0, -(n - 5) * top(32), 32),                  # only the last rows are in range
            (-(top(32) - 1), (1 << 62) - 5, 32),          # k near 2^62
            (0, -(1 << 62) - 12345, 32),                  # k near -2^62
            (0, -(1 << 62), 1)]


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

class Sum:
    """one running_sum call through the C ABI: the column in hostile surroundings, the mask a view with ones behind it, the output,
    the two result words and the workspace each in a Guarded buffer full of SENTINEL"""

    def __init__(self, O, eng, x, c, b, k, co, sel=None, exclusive=False, ws=None):
        self.O, self.eng, self.x, self.c, self.b, self.k, self.co, self.sel, self.exclusive = O, eng, x, c, b, k, co, sel, exclusive
        self.n = n = len(x)
        self.miss = miss_of(co)
        self.col = hostile_pack(O, x, c) if n else None
        self.mask = hostile_bitmap(sel)[0] if sel is not None and n else None
        self.out = Guarded(payload(n, co))
        self.result = Guarded(16, back=64, front=64)
        self.ws = ws if ws is not None else Guarded(8 * words_of(n))
        assert self.ws.nbytes >= 8 * words_of(n)

    def call(self, L, **kw):
        a = dict(col=self.col.data_ptr() if self.n else None, n=self.n, c=self.c, mask=self.mask.data_ptr() if self.mask is not None else None, b=self.b,
                 k=self.k, flags=EXCLUSIVE if self.exclusive else INCLUSIVE, co=self.co, miss=self.miss, out=self.out.ptr, result=self.result.ptr,
                 ws=self.ws.ptr)
        a.update(kw)
        rc = L.mi355_running_sum_dev(self.eng._ctx, a["col"], a["n"], a["c"], a["mask"], a["b"], a["k"], a["flags"], a["co"], a["miss"], a["out"],
                                     a["result"], a["ws"])
        self.eng.synchronize()
        return rc

    def run(self, L, what=""):
        """-> the launch record, after every byte, both words, the guards and the input have been checked"""
        tag = (what, self.n, self.c, self.b, self.k, self.co, self.exclusive)
        want, word0, outside = expect_sum(self.x, self.b, self.k, self.co, self.miss, self.sel, self.exclusive)
        wb = self.O.pack(want, self.co)[: self.out.nbytes]
        self.out.t.fill_(SENTINEL)
        self.result.t.fill_(SENTINEL)
        before = self.col.clone()
        assert self.call(L) == 0, (tag, L.mi355_last_error())
        have = self.out.fetch()  # asserts the guard bytes on both sides
        bad = np.nonzero(have != wb)[0]
        assert bad.size == 0, (tag, "byte", int(bad[0]), "of", len(wb), "have", int(have[bad[0]]), "want", int(wb[bad[0]]), "wrong bytes", int(bad.size))
        if (self.n * self.co) % 8:
            assert int(have[-1]) >> ((self.n * self.co) % 8) == 0, (tag, "bits behind the last value are not zero")
        words = [int(v) for v in self.result.fetch().view(np.int64)]
        assert words == [word0, outside], (tag, "result words", words, "want", [word0, outside])
        self.ws.fetch()  # its guards
        assert bool((self.col == before).all()), (tag, "the column was written")
        rec = record(L, self.eng)
        fam = want_family(self.c, self.n, self.b, self.k, self.co)
        assert [base_name(r[0]) for r in rec] == [TOTALS_KERNEL, SCAN_KERNEL, fam], (tag, rec)
        assert rec[2][0].startswith(f"{fam}<{self.co}>") and all(r[3] == 0 for r in rec), (tag, rec)
        assert rec[1][1] == -(-(-(-self.n // CHUNK)) // GROUP) and rec[0][2] == rec[2][2] >= 4 * 2 * 256 * self.c, (tag, rec)
        assert fam == CHECKED_KERNEL or outside == 0
        return rec


class Delta:
    def __init__(self, O, eng, x, c, first, k, co):
        self.O, self.eng, self.x, self.c, self.first, self.k, self.co = O, eng, x, c, first, k, co
        self.n = len(x)
        self.miss = miss_of(co)
        self.col = hostile_pack(O, x, c) if self.n else None
        self.out = Guarded(payload(self.n, co))
        self.counter = Guarded(8, back=64, front=64)

    def call(self, L, **kw):
        a = dict(col=self.col.data_ptr() if self.n else None, n=self.n, c=self.c, first=self.first, k=self.k, co=self.co, miss=self.miss,
                 out=self.out.ptr, counter=self.counter.ptr)
        a.update(kw)
        rc = L.mi355_delta_dev(self.eng._ctx, a["col"], a["n"], a["c"], a["first"], a["k"], a["co"], a["miss"], a["out"], a["counter"])
        self.eng.synchronize()
        return rc

    def run(self, L, what=""):
        tag = (what, self.n, self.c, self.first, self.k, self.co)
        want, outside = expect_delta(self.x, self.first, self.k, self.co, self.miss)
        wb = self.O.pack(want, self.co)[: self.out.nbytes]
        self.out.t.fill_(SENTINEL)
        self.counter.t.fill_(SENTINEL)
        before = self.col.clone()
        assert self.call(L) == 0, (tag, L.mi355_last_error())
        have = self.out.fetch()
        bad = np.nonzero(have != wb)[0]
        assert bad.size == 0, (tag, "byte", int(bad[0]), "of", len(wb), "have", int(have[bad[0]]), "want", int(wb[bad[0]]), "wrong bytes", int(bad.size))
        if (self.n * self.co) % 8:
            assert int(have[-1]) >> ((self.n * self.co) % 8) == 0, (tag, "bits behind the last value are not zero")
        got = int(self.counter.fetch().view(np.int64)[0])
        assert got == outside, (tag, "counter", got, "want", outside)
        assert bool((self.col == before).all()), (tag, "the column was written")
        (label, grid, lds, flags), = rec = record(L, self.eng)
        fam = want_delta_family(self.c, self.k, self.co)
        assert label.startswith(f"{fam}<{self.co}>") and flags == 0 and lds >= 4 * 2 * 256 * self.c, (tag, rec)
        assert fam == DELTA_CHECKED_KERNEL or outside == 0
        return rec


def one_block(eng):
    """a context manager: one block of four waves, so that a wave walks several chunks (running_sum) or strides over tiles (delta)"""
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


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_tails(L, O, eng, n):
    """both flags through the checked kernel on a walk around 2^12, the exact kernel into 32 bits; word 0 is the inclusive value of
    row n - 1 under either flag"""
    x, b, k = walk(9, 12, n)
    words = []
    for exclusive in (False, True):
        s = Sum(O, eng, x, 9, b, k, 12, exclusive=exclusive)
        rec = s.run(L)
        assert base_name(rec[2][0]) == CHECKED_KERNEL and base_name(rec[0][0]) == TOTALS_KERNEL
        words.append(int(s.result.fetch().view(np.int64)[0]))
    assert words[0] == words[1] == k + int((x.astype(np.int64) + b).sum())
    for exclusive in (False, True):
        rec = Sum(O, eng, uniform(9, n), 9, 0, 3, 32, exclusive=exclusive).run(L)
        assert base_name(rec[2][0]) == EXACT_KERNEL


@gpu
def test_empty_column(L, O, eng):
    """n == 0: nothing is launched, word 0 gets k and word 1 gets 0, with or without buffers"""
    x = np.zeros(0, dtype=np.uint32)
    for k in (0, 5, -7, INT64_MAX, INT64_MIN, (1 << 40) + 3):
        s = Sum(O, eng, x, 9, -5, k, 12)
        s.result.t.fill_(SENTINEL)
        for kw in ({}, dict(out=None, ws=None)):
            assert s.call(L, **kw) == 0 and record(L, eng) == []
            assert [int(v) for v in s.result.fetch().view(np.int64)] == [k, 0], k
    assert s.call(L, result=None) == 0 and (s.out.fetch() == SENTINEL).all()
    d = Delta(O, eng, x, 9, 0, 0, 9)
    assert d.call(L) == 0 and record(L, eng) == [] and int(d.counter.fetch().view(np.int64)[0]) == 0
    assert d.call(L, out=None, counter=None) == 0


@gpu
@pytest.mark.parametrize("c", range(1, 33))
def test_every_input_width(L, O, eng, c):
    x, b, k = walk(c, C_SWEEP_CO, N_BIG)
    rec = Sum(O, eng, x, c, b, k, C_SWEEP_CO).run(L)
    assert base_name(rec[2][0]) == CHECKED_KERNEL
    if c <= 12:  # ... and through the exact kernel where the sums fit 32 bits
        rec = Sum(O, eng, uniform(c, N_BIG), c, 0, 0, 32).run(L)
        assert base_name(rec[2][0]) == EXACT_KERNEL


@gpu
@pytest.mark.parametrize("co", range(1, 33))
def test_every_output_width_through_both_kernels(L, O, eng, co):
    x, b, k = walk(CO_SWEEP_C, co, N_BIG)
    rec = Sum(O, eng, x, CO_SWEEP_C, b, k, co).run(L)
    assert base_name(rec[2][0]) == CHECKED_KERNEL and rec[2][0].startswith(f"{CHECKED_KERNEL}<{co}>")
    c, n = exact_case(co)
    rec = Sum(O, eng, uniform(c, n), c, 0, 0, co, exclusive=bool(co & 1)).run(L)
    assert base_name(rec[2][0]) == EXACT_KERNEL and rec[2][0].startswith(f"{EXACT_KERNEL}<{co}>")


@gpu
def test_exact_kernel_wraps_in_32_bits(L, O, eng):
    """b < 0 and k = -n b: the sums stay in [0, 2^32) while b, k and the carry are reduced mod 2^32"""
    n = N_BIG
    for b, k, co in ((-100, 100 * n, 32), (-511, 511 * n, 26), (40000, (1 << 32) - 1 - n * (40000 + 511), 32)):
        rec = Sum(O, eng, uniform(9, n, 1), 9, b, k, co).run(L)
        assert base_name(rec[2][0]) == EXACT_KERNEL


@gpu
@pytest.mark.parametrize("case", range(5))
def test_carry_needs_64_bits(L, O, eng, case):
    """a c = 32 column of 2^32 - 1 over more than one chunk: a chunk's total is 2^46; with b = -(2^32 - 2) every term is 1"""
    b, k, co = carry_cases()[case]
    x = np.full(N_CARRY, top(32), dtype=np.uint32)
    s = Sum(O, eng, x, 32, b, k, co)
    rec = s.run(L)
    assert base_name(rec[2][0]) == CHECKED_KERNEL
    term = top(32) + b
    assert int(s.result.fetch().view(np.int64)[0]) == k + N_CARRY * term  # Python ints


@gpu
@pytest.mark.parametrize("bottom", [False, True], ids=["above", "below"])
def test_sums_leave_the_range_and_return(L, O, eng, bottom):
    """b < 0; crossings inside a lane's run, at a lane, a tile and a chunk boundary, in both directions, around 2^co and around 0"""
    x, b, k = walk(9, 12, N_WALK, 3, bottom, CROSSINGS)
    for exclusive in (False, True):
        Sum(O, eng, x, 9, b, k, 12, exclusive=exclusive).run(L)


@gpu
@pytest.mark.parametrize("kind", ["zero", "one", "coin", "half", "ends"])
def test_masks(L, O, eng, kind):
    x, b, k, sel = walk_under(9, 12, N_BIG, kind)
    for exclusive in (False, True):
        rec = Sum(O, eng, x, 9, b, k, 12, sel=sel, exclusive=exclusive).run(L, what=kind)
        assert base_name(rec[2][0]) == CHECKED_KERNEL
    Sum(O, eng, uniform(9, N_BIG), 9, 0, 0, 32, sel=sel).run(L, what=kind)  # the exact kernel under the mask


@gpu
def test_second_scan_group(L, O, eng):
    """1025 chunks: the last chunk's carry comes from group_totals"""
    x, b, k = walk(9, 12, N_GROUPS)
    rec = Sum(O, eng, x, 9, b, k, 12).run(L)
    assert rec[1][1] == 2 and base_name(rec[2][0]) == CHECKED_KERNEL


@gpu
def test_one_block_walks_many_chunks(L, O, eng):
    x, b, k = walk(9, 12, N_ONE_BLOCK)
    sel = mask_bits("half", N_ONE_BLOCK)
    with one_block(eng):
        for s in (Sum(O, eng, x, 9, b, k, 12), Sum(O, eng, x, 9, b, k, 12, sel=sel, exclusive=True), Sum(O, eng, uniform(9, N_ONE_BLOCK), 9, 0, 0, 32)):
            rec = s.run(L, what="one block")
            assert rec[0][1] == rec[2][1] == 1
    assert Sum(O, eng, x, 9, b, k, 12).run(L)[2][1] > 1


@gpu
@pytest.mark.parametrize("density", [0.0, 1 / 8, 1 / 2, 1.0])
def test_bitmap_as_the_column(L, O, eng, density):
    """row_positions: the exclusive sum of a result bitmap (exactly ceil(n / 8) bytes, ones behind them) against np.cumsum(bits) -
    bits; the slot compact gives every selected row is its position"""
    from shared_simd_scan_amd.engine import PackedColumn

    n = N_BIG
    bits = np.random.default_rng(int(density * 64)).random(n) < density
    bitmap, whole = hostile_bitmap(bits)
    pos, result = eng.row_positions(bitmap, n)
    eng.synchronize()
    rec = record(L, eng)
    assert [base_name(r[0]) for r in rec] == [TOTALS_KERNEL, SCAN_KERNEL, EXACT_KERNEL] and pos.c == n.bit_length() == 17
    want = (np.cumsum(bits) - bits).astype(np.uint32)
    assert (pos.data.cpu().numpy()[: payload(n, 17)] == O.pack(want, 17)[: payload(n, 17)]).all()
    assert [int(v) for v in result.cpu()] == [int(bits.sum()), 0]
    values = uniform(13, n, 4)
    out, count = eng.compact(PackedColumn(plain_pack(O, values, 13), n, 13), bitmap)
    eng.synchronize()
    slots = O.decompress(out.cpu().numpy(), n, 13).view(np.uint32)
    assert int(count.item()) == int(bits.sum()) and (slots[want[bits]] == values[bits]).all()


@gpu
def test_row_range_views(L, O, eng):
    """rows [lead, lead + n) of a longer column summed into rows [lead_out, lead_out + n) of a longer SENTINEL buffer, both 16 bytes
    aligned and no more: exactly the slice's bytes change and the foreign rows reach neither them nor a result word"""
    import torch

    n, lead = 2 * R + 504, 2 * R + 128
    for c, co, make in ((9, 12, lambda: walk(9, 12, n)), (9, 32, lambda: (uniform(9, n), 0, 3))):
        x, b, k = make()
        lead_out = lead_rows(co)
        assert (lead * c // 8) % 32 == 16 and (lead_out * co // 8) % 32 == 16
        whole = np.concatenate([uniform(c, lead, 8), x, np.full(4096, top(c), dtype=np.uint32)])
        col = hostile_pack(O, whole, c)[lead * c // 8:]
        s = Sum(O, eng, x, c, b, k, co)
        long_out = Guarded(payload(lead_out + n + 1000, co))
        for sel in (None, mask_bits("half", n)):
            mask_ptr = None
            if sel is not None:
                front = np.full(16, 0xFF, dtype=np.uint8)
                view, buf = hostile_bitmap(sel, offset=16, front=front)
                mask_ptr = view.data_ptr()
                assert mask_ptr % 32 == 16
            long_out.t.fill_(SENTINEL)
            s.result.t.fill_(SENTINEL)
            at = lead_out * co // 8
            assert s.call(L, col=col.data_ptr(), mask=mask_ptr, out=long_out.ptr.value + at) == 0
            want, word0, outside = expect_sum(x, b, k, co, s.miss, sel)
            have = long_out.fetch()
            assert (have[:at] == SENTINEL).all() and (have[at + payload(n, co):] == SENTINEL).all()
            assert (have[at: at + payload(n, co)] == O.pack(want, co)[: payload(n, co)]).all()
            assert [int(v) for v in s.result.fetch().view(np.int64)] == [word0, outside]
            s.ws.fetch()


@gpu
def test_workspace_holds_leftovers(L, O, eng):
    """the workspace of a larger call, as that call left it, under a smaller one: nothing stale is read"""
    big_x, b, k = walk(9, 12, N_ONE_BLOCK)
    big = Sum(O, eng, big_x, 9, b, k, 12)
    big.run(L, what="the larger call")
    for n in (3 * CHUNK + 5, CHUNK, 77):
        x, b, k = walk(9, 12, n, 7)
        Sum(O, eng, x, 9, b, k, 12, ws=big.ws).run(L, what="leftovers")
        Sum(O, eng, x, 9, b, k, 12, exclusive=True, sel=mask_bits("half", n), ws=big.ws).run(L, what="leftovers")
    assert not (big.ws.fetch() == SENTINEL).all()


@gpu
def test_round_trip(L, O, eng):
    """delta with k = 2^c - 1 into c + 1 bits loses nothing; the running sum with b = -(2^c - 1) gives the column back, byte for byte"""
    from shared_simd_scan_amd.engine import PackedColumn

    n = N_BIG
    for c in (1, 9, 17, 31):
        x = uniform(c, n, 2)
        col = PackedColumn(hostile_pack(O, x, c), n, c)
        cnt = eng._int64()
        d = eng.delta(col, k=top(c), co=c + 1, out_of_range=cnt)
        (label, _, _, _), = record(L, eng)
        assert base_name(label) == DELTA_EXACT_KERNEL
        want_d = (np.diff(x.astype(np.int64), prepend=0) + top(c)).astype(np.uint32)
        assert (d.data.cpu().numpy()[: payload(n, c + 1)] == O.pack(want_d, c + 1)[: payload(n, c + 1)]).all()
        back, result = eng.running_sum(d, b=-top(c), k=0, co=c)
        eng.synchronize()
        assert base_name(record(L, eng)[2][0]) == CHECKED_KERNEL
        assert (back.data.cpu().numpy()[: payload(n, c)] == O.pack(x, c)[: payload(n, c)]).all()
        assert [int(v) for v in result.cpu()] == [int(x[-1]), 0] and int(cnt.item()) == 0
        back, result = eng.delta_decode(d, 0, min_delta=-top(c), co=c)  # the same through the convenience
        eng.synchronize()
        assert (back.data.cpu().numpy()[: payload(n, c)] == O.pack(x, c)[: payload(n, c)]).all()


# ---- delta ----

@gpu
@pytest.mark.parametrize("n", SIZES)
def test_delta_sizes_and_tails(L, O, eng, n):
    x = delta_values(9, 9, n)
    for first in (0, 511):
        rec = Delta(O, eng, x, 9, first, 0, 9).run(L)
        assert base_name(rec[0][0]) == DELTA_CHECKED_KERNEL
        rec = Delta(O, eng, uniform(9, n), 9, first, 511, 10).run(L)
        assert base_name(rec[0][0]) == DELTA_EXACT_KERNEL


@gpu
@pytest.mark.parametrize("c", range(1, 33))
def test_delta_every_input_width(L, O, eng, c):
    for first in (0, top(c)):
        rec = Delta(O, eng, delta_values(c, 12, N_BIG), c, first, 0, 12).run(L)
        assert base_name(rec[0][0]) == DELTA_CHECKED_KERNEL
    if c < 32:
        rec = Delta(O, eng, uniform(c, N_BIG), c, top(c), top(c), c + 1).run(L)
        assert base_name(rec[0][0]) == DELTA_EXACT_KERNEL
    Delta(O, eng, uniform(c, N_BIG), c, 0, -5, 32).run(L)


@gpu
@pytest.mark.parametrize("co", range(1, 33))
def test_delta_every_output_width_through_both_kernels(L, O, eng, co):
    rec = Delta(O, eng, delta_values(CO_SWEEP_C, co, N_BIG), CO_SWEEP_C, 0, 0, co).run(L)
    assert base_name(rec[0][0]) == DELTA_CHECKED_KERNEL
    if co > 1:  # (co = 1 admits no exact delta)
        c = min(co - 1, 9)
        rec = Delta(O, eng, uniform(c, N_BIG), c, 0, (1 << co) - 1 - top(c), co).run(L)
        assert base_name(rec[0][0]) == DELTA_EXACT_KERNEL and rec[0][0].startswith(f"{DELTA_EXACT_KERNEL}<{co}>")


@gpu
def test_descents_are_counted(L, O, eng):
    """k = 0, co = c: the counter is numpy's number of descents -- placed at a lane, a tile and, for the tile-striding waves of a
    one-block grid, a grid-stride boundary -- and 0 on a sorted column; is_sorted is that counter"""
    from shared_simd_scan_amd.engine import PackedColumn

    n, c = 9 * R + 700, 17
    base = np.sort(uniform(c - 1, n, 3).astype(np.int64))  # (room for the steps below)
    assert (np.diff(base) >= 0).all()
    d = Delta(O, eng, base.astype(np.uint32), c, 0, 0, c)
    d.run(L, what="sorted")
    assert int(d.counter.fetch().view(np.int64)[0]) == 0
    at = [LANE, 5 * LANE, R, 3 * R, 4 * R, 8 * R, 9 * R, 40, n - 1]  # 4 R, 8 R: where a wave of a 4-wave grid takes its next tile
    x = base.copy()
    for row in at:
        x[row:] += 3
        x[row] = x[row - 1] - 1  # one descent, AT row
    x = x.astype(np.uint32)
    assert int(x.max()) <= top(c) and (np.nonzero(np.diff(x.astype(np.int64)) < 0)[0] + 1).tolist() == sorted(at)
    with one_block(eng):
        d = Delta(O, eng, x, c, 0, 0, c)
        (label, grid, _, _), = d.run(L, what="descents, one block")
        assert grid == 1 and int(d.counter.fetch().view(np.int64)[0]) == len(at)
        (label, grid, _, _), = Delta(O, eng, delta_values(9, 9, N_ONE_BLOCK), 9, 0, 0, 9).run(L, what="one block")
        assert grid == 1
    d.run(L, what="descents, whole chip")
    col = PackedColumn(hostile_pack(O, x, c), n, c)
    assert int(eng.is_sorted(col).item()) == len(at)
    assert int(eng.is_sorted(PackedColumn(hostile_pack(O, base.astype(np.uint32), c), n, c)).item()) == 0
    assert int(eng.is_sorted(PackedColumn(hostile_pack(O, base.astype(np.uint32), c), n, c), first=top(c)).item()) == 1


@gpu
def test_delta_row_range_views(L, O, eng):
    n, lead, lead_out = 2 * R + 504, 2 * R + 128, lead_rows(12)
    for c, k, co in ((9, 0, 12), (9, 511, 12)):
        x = delta_values(c, co, n, 1) if k == 0 else uniform(c, n, 5)
        assert (lead * c // 8) % 32 == 16 and (lead_out * co // 8) % 32 == 16
        whole = np.concatenate([uniform(c, lead, 8), x, np.full(4096, top(c), dtype=np.uint32)])
        col = hostile_pack(O, whole, c)[lead * c // 8:]
        d = Delta(O, eng, x, c, 77, k, co)
        long_out = Guarded(payload(lead_out + n + 1000, co))
        d.counter.t.fill_(SENTINEL)
        at = lead_out * co // 8
        assert d.call(L, col=col.data_ptr(), out=long_out.ptr.value + at) == 0
        want, outside = expect_delta(x, 77, k, co, d.miss)
        have = long_out.fetch()
        assert (have[:at] == SENTINEL).all() and (have[at + payload(n, co):] == SENTINEL).all()
        assert (have[at: at + payload(n, co)] == O.pack(want, co)[: payload(n, co)]).all()
        assert int(d.counter.fetch().view(np.int64)[0]) == outside


# ---- refusals ----

@gpu
def test_errors_launch_nothing(L, O, eng):
    n = R + 77
    x, b, k = walk(9, 12, n)
    sel = mask_bits("half", n)
    s = Sum(O, eng, x, 9, b, k, 12, sel=sel)
    s.run(L)
    valid = record(L, eng)
    big = Guarded(16384)  # stands for an input and the output at once
    col, mask, out, ws = s.col.data_ptr(), s.mask.data_ptr(), s.out.ptr.value, s.ws.ptr.value
    nb_col, nb_out = payload(n, 9), payload(n, 12)
    errors = (("c = 0", dict(c=0), b"width"), ("c = 33", dict(c=33), b"width"), ("co = 0", dict(co=0), b"width"), ("co = 33", dict(co=33), b"width"),
              ("miss = 2^co", dict(miss=1 << 12), b"miss"), ("miss = 2^32 - 1", dict(miss=top(32)), b"miss"),
              ("flags = 2", dict(flags=2), b"flags"), ("flags = 2^31", dict(flags=1 << 31), b"flags"),
              ("null column", dict(col=None), b"packed_dev"), ("null output", dict(out=None), b"out_dev"), ("null workspace", dict(ws=None), b"ws_dev"),
              ("column at +4", dict(col=col + 4), b"aligned"), ("output at +8", dict(out=out + 8), b"aligned"), ("workspace at +4", dict(ws=ws + 4), b"aligned"),
              ("mask at +2", dict(mask=mask + 2), b"mask_dev"), ("result at +4", dict(result=s.result.ptr.value + 4), b"result_dev"),
              ("output is the column", dict(col=big.ptr.value, out=big.ptr.value), b"overlaps packed_dev"),
              ("output starts in the column's last byte", dict(col=big.ptr.value, out=big.ptr.value + (nb_col - 1) // 16 * 16), b"overlaps packed_dev"),
              ("column starts inside the output", dict(col=big.ptr.value + 256, out=big.ptr.value), b"overlaps packed_dev"),
              ("output is the mask", dict(mask=big.ptr.value, out=big.ptr.value), b"overlaps mask_dev"),
              ("mask starts inside the output", dict(mask=big.ptr.value + nb_out - 4, out=big.ptr.value), b"overlaps mask_dev"),
              ("output is the workspace", dict(ws=big.ptr.value, out=big.ptr.value), b"overlaps ws_dev"),
              ("output starts in the workspace's last word", dict(ws=big.ptr.value, out=big.ptr.value + 16), b"overlaps ws_dev"),
              ("hi beyond int64", dict(b=0, k=INT64_MAX - n * 511 + 1), b"int64"), ("lo beyond int64", dict(b=-7, k=INT64_MIN + 7 * n - 1), b"int64"))
    buffers = (s.out, s.result, s.ws, big)
    for what, kw, word in errors:
        for g in buffers:
            g.t.fill_(SENTINEL)
        assert s.call(L, **kw) == E_INVALID, what
        assert word in L.mi355_last_error(), (what, L.mi355_last_error())
        assert record(L, eng) == [], what
        for g in buffers:
            assert (g.fetch() == SENTINEL).all(), what
    # neighbours that do not overlap are fine
    s.run(L)
    assert record(L, eng) == valid
    # delta
    d = Delta(O, eng, delta_values(9, 12, n), 9, 0, 0, 12)
    d.run(L)
    col, out = d.col.data_ptr(), d.out.ptr.value
    errors = (("c = 0", dict(c=0), b"width"), ("c = 33", dict(c=33), b"width"), ("co = 0", dict(co=0), b"width"), ("co = 33", dict(co=33), b"width"),
              ("miss = 2^co", dict(miss=1 << 12), b"miss"), ("first = 2^c", dict(first=512), b"first"),
              ("null column", dict(col=None), b"packed_dev"), ("null output", dict(out=None), b"out_dev"),
              ("column at +8", dict(col=col + 8), b"aligned"), ("output at +4", dict(out=out + 4), b"aligned"), ("counter at +4", dict(counter=d.counter.ptr.value + 4), b"out_of_range_dev"),
              ("output is the column", dict(col=big.ptr.value, out=big.ptr.value), b"overlaps packed_dev"),
              ("column starts inside the output", dict(col=big.ptr.value + (nb_out - 1) // 16 * 16, out=big.ptr.value), b"overlaps packed_dev"))
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
    """two versions of (x, b, k, selected): the same b and k (they are recorded), other rows and another mask"""
    out = []
    for salt in (11, 12):
        sel = mask_bits("half", N_CAP, salt)
        xs, b, k = walk(9, 12, int(sel.sum()), salt)
        x = uniform(9, N_CAP, salt).copy()
        x[sel] = xs
        out.append((frozen(x), b, k, sel))
    assert out[0][1:3] == out[1][1:3]
    return out


def test_capture_data_is_not_vacuous():
    (x0, b, k, s0), (x1, _, _, s1) = capture_versions()
    w0, w1 = expect_sum(x0, b, k, 12, miss_of(12), s0), expect_sum(x1, b, k, 12, miss_of(12), s1)
    assert (w0[0] != w1[0]).any() and w0[1] != w1[1] and w0[2] != w1[2] and min(w0[2], w1[2]) > 0, "a stale result could pass"
    d0, d1 = expect_delta(x0, 0, 0, 9, 1), expect_delta(x1, 0, 0, 9, 1)
    assert (d0[0] != d1[0]).any() and d0[1] != d1[1]


def sum_steps(O, chain):
    """capture.Steps for running_sum under a mask (checked kernel) -- chain: behind delta with k = 2^c - 1, on its output"""
    import torch

    versions = capture_versions()
    n, c, co = N_CAP, 9, 12
    miss = miss_of(co)
    if chain:
        cs, bs, ks = c + 1, versions[0][1] - top(c), versions[0][2]  # delta's terms are x_i - x_{i-1} + 511: b takes the 511 back
        wants = [expect_sum(np.diff(x.astype(np.int64), prepend=0) + top(c), bs, ks, co, miss, sel) for x, b, k, sel in versions]
    else:
        cs, bs, ks = c, versions[0][1], versions[0][2]
        wants = [expect_sum(x, b, k, co, miss, sel) for x, b, k, sel in versions]

    def steps(eng):
        from shared_simd_scan_amd.engine import PackedColumn

        stage = [(plain_pack(O, x, c), torch.from_numpy(packbits(sel)).cuda()) for x, b, k, sel in versions]
        col = PackedColumn(torch.empty_like(stage[0][0]), n, c)
        mask = torch.empty(len(stage[0][1]) + 32, dtype=torch.uint8, device="cuda")
        out, result, ws = Guarded(payload(n, co)), Guarded(16, back=64, front=64), Guarded(8 * words_of(n))
        mid = Guarded(L_size(cs, n))
        views = [g.t[g.front: g.front + g.nbytes] for g in (out, result, ws, mid)]

        def load(v):
            col.data.copy_(stage[v][0])
            mask[: len(stage[v][1])].copy_(stage[v][1])
            for g in (out, result, ws, mid):
                g.t.fill_(SENTINEL)

        def run():
            src = col
            if chain:
                src = eng.delta(col, k=top(c), co=cs, out=views[3])
            eng.running_sum(src, mask=mask, b=bs, k=ks, co=co, miss=miss, out=views[0], result=views[1].view(torch.int64), workspace=views[2].view(torch.int64))

        def check(v, what):
            assert (out.fetch() == O.pack(wants[v][0], co)[: out.nbytes]).all(), what
            assert [int(w) for w in result.fetch().view(np.int64)] == list(wants[v][1:]), what
            ws.fetch()

        def untouched():
            for g in (out, result, ws, mid):
                assert (g.fetch() == SENTINEL).all()

        def warmed(launched):
            assert [base_name(x[0]) for x in launched] == [TOTALS_KERNEL, SCAN_KERNEL, CHECKED_KERNEL]

        return capture.Steps(load, run, check, untouched, warmed)

    return steps


def L_size(c, n):
    from shared_simd_scan_amd import compressed_buffer_size

    return compressed_buffer_size(c, n)


@gpu
@pytest.mark.parametrize("chain", [False, True], ids=["running_sum", "delta-then-running_sum"])
def test_graph_capture_and_replay(O, chain):
    """the checked kernel under a mask, with its caller's workspace full of SENTINEL and no larger call before it; replays follow the
    column and the mask overwritten in place.  chain: delta in front of it in the same graph"""
    capture.capture_replay(sum_steps(O, chain), (0, 1, 0))


@gpu
def test_delta_graph_capture_and_replay(O):
    import torch

    versions = capture_versions()
    n, c = N_CAP, 9
    wants = [expect_delta(x, 0, 0, c, 1) for x, b, k, sel in versions]

    def steps(eng):
        from shared_simd_scan_amd.engine import PackedColumn

        stage = [plain_pack(O, x, c) for x, b, k, sel in versions]
        col = PackedColumn(torch.empty_like(stage[0]), n, c)
        out, counter = Guarded(payload(n, c)), Guarded(8, back=64, front=64)
        views = [g.t[g.front: g.front + g.nbytes] for g in (out, counter)]

        def load(v):
            col.data.copy_(stage[v])
            for g in (out, counter):
                g.t.fill_(SENTINEL)

        def run():
            eng.delta(col, miss=1, out=views[0], out_of_range=views[1].view(torch.int64))

        def check(v, what):
            assert (out.fetch() == O.pack(wants[v][0], c)[: out.nbytes]).all(), what
            assert int(counter.fetch().view(np.int64)[0]) == wants[v][1], what

        def untouched():
            assert (out.fetch() == SENTINEL).all() and (counter.fetch() == SENTINEL).all()

        def warmed(launched):
            assert [base_name(x[0]) for x in launched] == [DELTA_CHECKED_KERNEL]

        return capture.Steps(load, run, check, untouched, warmed)

    capture.capture_replay(steps, (0, 1, 0))
