"""A packed column computed row by row from two others (include/mi355_arith.h, ScanEngine.arith):
out[i] = r_i if 0 <= r_i < 2^co else miss, with r_i = a x_i + b y_i + k ("linear") or a x_i y_i + k ("mul"), packed in and out.

CPU: the header is plain C99 and declares exactly what _capi.HEADERS binds for it and the library exports; it carries its
graph-capture verdict; mi355_arith_kernel (pure arithmetic) names the kernel at every boundary of the range rule and refuses what
the call refuses; arith_range equals a brute force over all inputs at widths <= 4; the co=None rule; arith hands the C ABI what it
should (through a recording stand-in for the library); without a device the entry point fails with a message; every __global__
under csrc/arith/ is named by the launch record of a GPU case of this file; no source there reads a switch bit; every data recipe
of the checked kernel holds rows inside and outside the range.

GPU (-m gpu): every expectation is numpy int64 on the values the test generated (exact under the range rule; "mul" as
(x * y) * a + k), packed with the oracle's packer; nothing is derived from engine output.  Every one of the ceil(n co / 8) payload
bytes (trailing bits of the last one included) and the 0xEE guard bytes on both sides of the output (support.Guarded)
are compared exactly; both inputs must be unchanged after the call; the counter equals numpy's count.  Every case runs in hostile
surroundings: ones in each column's bits behind row n - 1 and in its pad.  A tile is R = 2048 rows, so the sizes below are the
smallest that reach one lane, one partial tile, one full tile, a full tile plus one row and many tiles with a ragged tail.
"""
import collections
import ctypes as C
import functools
import itertools
import os
import re

import numpy as np
import pytest

import capture
import support
from support import E_INVALID, SENTINEL, Guarded, L, base_name, corner_rows, eng, fake, grouped, hostile_pack, plain_pack, record  # noqa: F401  (L, eng, fake: fixtures)

HEADER = "mi355_arith.h"
LINEAR, MUL = 0, 1
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)

# the kernels of csrc/arith/, as the launch record names them: the GPU cases below assert these labels
EXACT_KERNEL = "arith_exact_kernel"
CHECKED_KERNEL = "arith_checked_kernel"

R = 2048  # rows per tile: 64 lanes x 32 rows
N_BIG = 9 * R + 1237  # nine tiles and a ragged one; not a multiple of 8
N_LONG = 64 * R + 1237  # one block's four waves walk sixteen tiles each
N_VIEW = 2 * R + 504  # a multiple of 8 (the slice ends on a byte at any width), not of 32: the last lane is ragged
SIZES = [1, 13, R - 1, R, R + 1, N_BIG]

gpu = pytest.mark.gpu

# corners: up to four (x, y) pairs placed at support.corner_rows (first tile, last full tile, ragged tail); None: the four
# extremes (0, 0), (X, Y), (X, 0), (0, Y), which reach lo and hi of a linear form
Recipe = collections.namedtuple("Recipe", "op c1 c2 a b k co corners", defaults=(None,))


def top(c):
    return (1 << c) - 1


def rid(r):
    return f"{r.op}-{r.c1}x{r.c2}-a{r.a}-b{r.b}-k{r.k}-co{r.co}"


def rule_range(op, c1, c2, a, b, k):
    """the issue's range rule, in Python ints"""
    X, Y = top(c1), top(c2)
    terms = [a * X * Y] if op == "mul" else [a * X, b * Y]
    return sum(min(0, t) for t in terms) + k, sum(max(0, t) for t in terms) + k


def want_family(r):
    lo, hi = rule_range(r.op, r.c1, r.c2, r.a, r.b, r.k)
    assert INT64_MIN <= lo and hi <= INT64_MAX, r
    return EXACT_KERNEL if lo >= 0 and hi <= top(r.co) else CHECKED_KERNEL


def miss_of(co):
    return 1 if co == 1 else 0x5A5A5A5A & top(co)


# sizes: the issue's four width triples
SIZE_CASES = [Recipe("linear", 9, 9, 1, 1, 0, 10), Recipe("linear", 17, 5, 32, 1, 0, 22),
              Recipe("linear", 32, 32, 1, -1, (1 << 32) - 1, 32), Recipe("linear", 1, 1, 1, 1, 0, 1)]
# every output width through both kernels: x + y + 1 <= 2^co - 1 at widths co - 1 (co = 1: x y <= 1) is exact with hi on the
# boundary; x + y - 1 at widths co leaves the range on both sides
CO_EXACT = [Recipe("mul", 1, 1, 1, 0, 0, 1)] + [Recipe("linear", co - 1, co - 1, 1, 1, 1, co) for co in range(2, 33)]
CO_CHECKED = [Recipe("linear", co, co, 1, 1, -1, co) for co in range(1, 33)]
# every c1 at c2 = 7 (x - y, negative when x < y), every c2 at c1 = 11 (x y, a bit narrower than the widest product)
C1_CASES = [Recipe("linear", c1, 7, 1, -1, 0, c1) for c1 in range(1, 33)]
C2_CASES = [Recipe("mul", 11, c2, 1, 0, 0, min(c2 + 10, 31)) for c2 in range(1, 33)]
LONG_CASES = [SIZE_CASES[0], SIZE_CASES[2], Recipe("mul", 20, 4, 1, 0, 0, 24), Recipe("linear", 9, 9, 1, 1, 0, 9)]
CORNER_CASES = [
    # r = 0, -1, 2^co - 1, 2^co
    Recipe("linear", 9, 9, 1, 1, -1, 9, ((0, 1), (0, 0), (511, 1), (511, 2))),
    # r = 2^32 + 5 at co = 8: the low bits are in range and it must still be miss; then 5 (in), 2^8 + 5 (out), 255 (in)
    Recipe("mul", 20, 20, 1, 0, 5, 8, ((1 << 16, 1 << 16), (0, 77), (16, 16), (125, 2))),
    # r = -2^32 + 7: negative, low 32 bits in range; then 7 (in), -2^32 - 2^16 + 7, 7 - 1 = 6 (in)
    Recipe("mul", 20, 20, -1, 0, 7, 8, ((1 << 16, 1 << 16), (0, 0), ((1 << 16) + 1, 1 << 16), (1, 1))),
]
# the exact kernel with negative terms: 3 x - 5 y + 5 Y lies in [0, 3 X + 5 Y]; the intermediate sums wrap in 32 bits
NEGATIVE_TERM_CASES = [Recipe("linear", 9, 9, 3, -5, 5 * 511, 12), Recipe("linear", 29, 28, 3, -5, 5 * top(28), 32),
                       Recipe("mul", 16, 15, -2, 0, 2 * top(16) * top(15), 32)]
OPERAND_CASES = [
    Recipe("linear", 9, 7, 0, 3, 2, 9),                 # a = 0, exact: 3 y + 2
    Recipe("linear", 9, 7, 0, -3, 200, 8),              # a = 0, checked: 200 - 3 y goes negative
    Recipe("linear", 12, 7, 5, 0, 0, 15),               # b = 0, exact
    Recipe("linear", 12, 7, 5, 0, -100, 14),            # b = 0, checked
    Recipe("mul", 9, 7, 0, 0, 9, 4),                    # a = 0 with mul: the constant 9
    Recipe("linear", 9, 5, -(1 << 31), 1, 511 << 31, 32),  # a = -2^31: in range only at x = 511, 510
    Recipe("linear", 32, 32, 1, 1, -(1 << 32) - 5, 32),     # k beyond 2^32, negative
    Recipe("linear", 32, 32, -1, -1, (1 << 33) + 3, 32),    # k beyond 2^32, positive
    Recipe("mul", 13, 13, 7, 0, -(1 << 28), 31),            # a general multiplier in 64 bits
    Recipe("linear", 20, 20, 1000, -999, 0, 28),            # general a and b in 64 bits
    Recipe("linear", 10, 10, 1000, 999, 3, 21),             # general a and b, exact
]
SAME_BUFFER_CASES = [Recipe("mul", 9, 9, 1, 0, 0, 18), Recipe("mul", 9, 9, 1, 0, 0, 16), Recipe("linear", 17, 17, 2, -1, 0, 16)]
VIEW_CASES = [SIZE_CASES[0], Recipe("linear", 12, 7, 1, -1, 0, 12), Recipe("mul", 20, 4, 1, 0, 0, 24)]
ERROR_RECIPE = Recipe("linear", 9, 12, 1, 1, -1, 12)
ERROR_N = R + 77
CAPTURE_CASES = [Recipe("linear", 3, 3, 7, 1, 0, 6), Recipe("linear", 9, 9, 1, -1, 0, 9)]  # one per kernel


@functools.lru_cache(maxsize=None)
def data(r, n, salt=0, same=False):
    """-> (x, y) uint32[n], read-only: half of the rows uniform over the column's width, half below 2^min(c, 8) (so sums,
    differences and products land on both sides of most bounds), then the recipe's corner pairs at corner_rows().
    same: y is x (one buffer as both inputs)"""
    rng = np.random.default_rng([r.c1, r.c2, n, salt, r.co])

    def column(c):
        v = rng.integers(0, 1 << c, n, dtype=np.uint64)
        small = rng.random(n) < 0.5
        v[small] = rng.integers(0, 1 << min(c, 8), int(small.sum()), dtype=np.uint64)
        return v

    x, y = column(r.c1), column(r.c2)
    X, Y = top(r.c1), top(r.c2)
    corners = r.corners or ((0, 0), (X, Y), (X, 0), (0, Y))
    for rows in corner_rows(n):
        for row, (cx, cy) in zip(rows, corners):
            x[row], y[row] = cx, cy
    if same:
        assert r.c1 == r.c2
        y = x
    x, y = x.astype(np.uint32), y.astype(np.uint32)
    for v in (x, y):
        v.setflags(write=False)
    return x, y


def expect(r, x, y, miss):
    """-> (the co-bit values the call writes, the number of rows it replaces by miss): numpy int64, exact under the range rule"""
    xi, yi = x.astype(np.int64), y.astype(np.int64)
    res = (xi * yi) * np.int64(r.a) + np.int64(r.k) if r.op == "mul" else xi * np.int64(r.a) + yi * np.int64(r.b) + np.int64(r.k)
    inside = (res >= 0) & (res < (1 << r.co))
    return np.where(inside, res, miss).astype(np.uint32), int((~inside).sum())


def payload(n, c):
    return (n * c + 7) // 8


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------

def test_arith_header_is_plain_c99():
    support.check_header_is_plain_c99(HEADER)


def test_arith_header_declares_what_python_binds(L):
    names, sigs = support.check_header_binds(L, HEADER)
    assert names == ["mi355_arith_dev", "mi355_arith_kernel"]
    sig = sigs["mi355_arith_dev"]
    assert sig[1] is C.c_int and sig[3] is C.c_uint and sig[5] is C.c_uint and sig[6] is C.c_uint64 and sig[7] is C.c_int32 and sig[8] is C.c_int32
    assert sig[9] is C.c_int64 and sig[10] is C.c_uint and sig[11] is C.c_uint32 and len(sig) == 14
    assert sigs["mi355_arith_kernel"] == [C.c_int, C.c_uint, C.c_uint, C.c_int32, C.c_int32, C.c_int64, C.c_uint]
    assert L.mi355_arith_kernel.restype is C.c_char_p
    text = support.header_text(HEADER)
    assert '#include "mi355_scan.h"' in text and text.count("#include") == 1
    assert support.header_macro(HEADER, "MI355_ARITH_LINEAR") == LINEAR and support.header_macro(HEADER, "MI355_ARITH_MUL") == MUL


def test_arith_names_are_exported():
    import shared_simd_scan_amd as pkg

    for name in ("arith_kernel", "arith_range", "arith_width"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    assert callable(pkg.ScanEngine.arith)


def test_arith_header_carries_its_capture_verdict():
    support.check_capture_verdict(HEADER, r"read at every replay", r"zeroing of out_of_range_dev")


def test_kernel_choice_at_the_boundaries(L):
    """mi355_arith_kernel needs neither a device nor a context; the kernel follows [lo, hi] against [0, 2^co - 1]"""
    from shared_simd_scan_amd import arith_kernel

    k = L.mi355_arith_kernel
    exact, checked = EXACT_KERNEL.encode(), CHECKED_KERNEL.encode()
    # hi == 2^co - 1 against 2^co: x + y + k over 9 x 9 bits has hi = 1022 + k
    assert k(LINEAR, 9, 9, 1, 1, 1, 10) == exact and k(LINEAR, 9, 9, 1, 1, 2, 10) == checked
    assert k(LINEAR, 9, 9, 1, 1, 1, 11) == exact and k(LINEAR, 9, 9, 1, 1, 1, 9) == checked
    # lo == 0 against -1
    assert k(LINEAR, 9, 9, 1, 1, 0, 11) == exact and k(LINEAR, 9, 9, 1, 1, -1, 11) == checked
    assert k(LINEAR, 9, 9, 1, -1, 511, 10) == exact and k(LINEAR, 9, 9, 1, -1, 510, 10) == checked
    assert k(LINEAR, 9, 9, 3, -5, 5 * 511, 12) == exact and k(LINEAR, 9, 9, 3, -5, 5 * 511 - 1, 12) == checked
    for co in range(1, 33):  # the widest exact result at every width, and one beyond it
        assert k(LINEAR, co, 1, 1, 0, 0, co) == exact and k(LINEAR, co, 1, 1, 0, 1, co) == checked, co
    # mul: a X Y + k
    assert k(MUL, 20, 4, 1, 0, 0, 24) == exact and k(MUL, 20, 4, 1, 0, 0, 23) == checked
    assert k(MUL, 16, 16, 1, 0, 0, 32) == exact and k(MUL, 16, 16, 1, 0, 2 * 65535 + 1, 32) == checked
    assert k(MUL, 16, 16, -1, 0, 65535 * 65535, 32) == exact and k(MUL, 16, 16, -1, 0, 65535 * 65535 - 1, 32) == checked
    # NULL for each refusal
    for op in (-1, 2, 7):
        assert k(op, 9, 9, 1, 1, 0, 10) is None, op
    for bad in (0, 33):
        assert k(LINEAR, bad, 9, 1, 1, 0, 10) is None and k(LINEAR, 9, bad, 1, 1, 0, 10) is None and k(LINEAR, 9, 9, 1, 1, 0, bad) is None, bad
    assert k(MUL, 9, 9, 1, 1, 0, 18) is None and k(MUL, 9, 9, 1, -1, 0, 18) is None  # b != 0 with mul
    # the range rule at INT64_MAX, INT64_MAX + 1 and the INT64_MIN side: x + y + k over 1 x 1 bits spans [k, k + 2]
    assert k(LINEAR, 1, 1, 1, 1, INT64_MAX - 2, 32) == checked and k(LINEAR, 1, 1, 1, 1, INT64_MAX - 1, 32) is None
    assert k(LINEAR, 1, 1, -1, -1, INT64_MIN + 2, 32) == checked and k(LINEAR, 1, 1, -1, -1, INT64_MIN + 1, 32) is None
    assert k(LINEAR, 1, 1, 1, -1, INT64_MAX - 1, 32) == checked and k(LINEAR, 1, 1, 1, -1, INT64_MAX, 32) is None
    assert k(LINEAR, 1, 1, 1, -1, INT64_MIN + 1, 32) == checked and k(LINEAR, 1, 1, 1, -1, INT64_MIN, 32) is None
    assert k(LINEAR, 32, 32, -(1 << 31), -(1 << 31), 0, 32) is None  # lo = -2^64 + 2^33
    # a X = -2^31 (2^32 - 1) = -2^63 + 2^31: k = -2^31 puts lo on INT64_MIN
    assert k(LINEAR, 32, 1, -(1 << 31), 0, -(1 << 31), 32) == checked and k(LINEAR, 32, 1, -(1 << 31), 0, -(1 << 31) - 1, 32) is None
    assert k(LINEAR, 32, 32, -(1 << 31), (1 << 31) - 1, 0, 32) == checked and k(LINEAR, 32, 32, -(1 << 31), -1, -(1 << 31), 32) is None
    # mul: c1 + c2 = 63 accepted, 32 x 32 refused (unless a == 0: then r = k whatever the product)
    assert k(MUL, 32, 31, 1, 0, 0, 32) == checked and k(MUL, 31, 32, -1, 0, 0, 32) == checked
    assert k(MUL, 32, 32, 1, 0, 0, 32) is None and k(MUL, 32, 32, -1, 0, 0, 32) is None
    assert k(MUL, 32, 32, 0, 0, 77, 7) == exact and k(MUL, 32, 32, 0, 0, 77, 6) == checked
    assert k(MUL, 32, 31, 2, 0, 0, 32) is None and k(MUL, 32, 30, 2, 0, 0, 32) == checked
    # the Python face: the same answers, and ValueError for what the call would refuse or ctypes would wrap
    assert arith_kernel("linear", 9, 9, 1, 1, 1, 10) == EXACT_KERNEL and arith_kernel("linear", 9, 9, 1, 1, 2, 10) == CHECKED_KERNEL
    assert arith_kernel("linear", 9, 9) == EXACT_KERNEL and arith_kernel("mul", 20, 4) == EXACT_KERNEL  # co=None: the width that holds hi
    assert arith_kernel("mul", 20, 4, co=23) == CHECKED_KERNEL
    for bad in (("plus", 9, 9, 1, 1, 0, 10), ("linear", 0, 9, 1, 1, 0, 10), ("linear", 9, 33, 1, 1, 0, 10), ("linear", 9, 9, 1, 1, 0, 0),
                ("linear", 9, 9, 1, 1, 0, 33), ("linear", 9, 9, 1, 1, 0, -1), ("linear", 9, 9, 1, 1, 0, (1 << 32) + 10),
                ("mul", 9, 9, 1, 1, 0, 18), ("mul", 32, 32, 1, 0, 0, 32), ("linear", 9, 9, 1 << 31, 1, 0, 10), ("linear", 9, 9, 1, -(1 << 31) - 1, 0, 10),
                ("linear", 9, 9, 1, 1, 1 << 63, 10), ("linear", 1, 1, 1, 1, INT64_MAX - 1, 32)):
        with pytest.raises(ValueError):
            arith_kernel(*bad)


OPERAND_GRID = [(1, 1, 0), (1, -1, 0), (3, -5, 75), (-2, 0, 7), (0, 4, -3), (0, 0, 5), (-(1 << 31), (1 << 31) - 1, 1 << 40), (-7, -1, -9)]


def test_arith_range_is_the_brute_force():
    """arith_range equals min / max of the expression over ALL (x, y) at widths <= 4, and this file's copy of the rule agrees"""
    from shared_simd_scan_amd import arith_range

    for c1, c2 in itertools.product(range(1, 5), repeat=2):
        xs, ys = np.meshgrid(np.arange(1 << c1, dtype=object), np.arange(1 << c2, dtype=object))
        for a, b, k in OPERAND_GRID:
            res = a * xs + b * ys + k
            lo, hi = arith_range("linear", c1, c2, a, b, k)
            # the rule bounds the expression; it is tight because the two terms are independent
            assert (lo, hi) == (int(res.min()), int(res.max())) == rule_range("linear", c1, c2, a, b, k), (c1, c2, a, b, k)
            res = a * xs * ys + k
            assert arith_range("mul", c1, c2, a, 0, k) == (int(res.min()), int(res.max())) == rule_range("mul", c1, c2, a, 0, k), (c1, c2, a, k)
    assert arith_range("linear", 9, 9) == (0, 1022) and arith_range("mul", 9, 9) == (0, 511 * 511)  # b defaults to 1 / 0
    assert arith_range("mul", 32, 32, -(1 << 31), 0, -5) == (-(1 << 31) * top(32) * top(32) - 5, -5)  # Python ints: beyond 64 bits
    for bad in (("mul", 9, 9, 1, 1, 0), ("div", 9, 9, 1, 1, 0), ("linear", 0, 9, 1, 1, 0), ("linear", 9, 9, 1 << 31, 1, 0)):
        with pytest.raises(ValueError):
            arith_range(*bad)


def test_default_width_is_the_smallest_that_holds_hi():
    from shared_simd_scan_amd import arith_width

    assert arith_width("linear", 9, 9) == 10 and arith_width("mul", 20, 4) == 24 and arith_width("linear", 3, 3, 7, 1) == 6
    assert arith_width("linear", 9, 9, 1, 1, 1) == 10 and arith_width("linear", 9, 9, 1, 1, 2) == 11  # hi = 1023 | 1024
    assert arith_width("linear", 9, 9, 0, 0, 0) == 1 and arith_width("linear", 9, 9, 0, 0, 1) == 1 and arith_width("linear", 9, 9, 0, 0, 2) == 2
    assert arith_width("linear", 31, 31, 1, 1, 1) == 32 and arith_width("mul", 16, 16) == 32
    assert arith_width("linear", 9, 9, 1, -1, 511) == 10  # lo == 0
    for bad in (("linear", 9, 9, 1, -1, 510), ("linear", 31, 31, 1, 1, 2), ("mul", 17, 16), ("linear", 9, 9, 1, 1, -1)):
        with pytest.raises(ValueError):  # lo < 0, or hi >= 2^32
            arith_width(*bad)


def test_arith_wrapper_passes_what_the_abi_takes(fake, L):
    import torch

    eng, rec, col = fake
    c1, c2 = col(9, 777), col(12, 777)
    res = eng.arith("linear", c1, c2)  # defaults: a = b = 1, k = 0, the width that holds hi, miss 0, a fresh buffer, no counter
    (name, a), = rec.calls
    assert name == "mi355_arith_dev" and a[1:12] == [LINEAR, c1.data.data_ptr(), 9, c2.data.data_ptr(), 12, 777, 1, 1, 0, 13, 0] and a[13] is None
    assert res.data.dtype == torch.uint8 and res.data.numel() == L.mi355_compressed_buffer_size(13, 777) and a[12] == res.data.data_ptr()
    assert (res.n, res.c) == (777, 13)
    rec.calls.clear()
    out = torch.zeros(1263, dtype=torch.uint8)  # ceil(777 * 13 / 8): a slice of a longer column needs no more
    cnt = torch.zeros(1, dtype=torch.int64)
    res = eng.arith("mul", c1, c2, a=-3, k=(1 << 40) + 5, co=13, miss=8191, out=out, out_of_range=cnt)  # b defaults to 0 for "mul"
    (name, a), = rec.calls
    assert a[1:] == [MUL, c1.data.data_ptr(), 9, c2.data.data_ptr(), 12, 777, -3, 0, (1 << 40) + 5, 13, 8191, out.data_ptr(), cnt.data_ptr()]
    assert res.data is out and (res.n, res.c) == (777, 13)
    rec.calls.clear()
    eng.arith("linear", c1, c1, a=-(1 << 31), b=(1 << 31) - 1, k=INT64_MIN + (1 << 41), co=32, miss=(1 << 32) - 1)  # nothing wraps on the way
    a = rec.calls[0][1]
    assert a[2] == a[4] == c1.data.data_ptr() and a[7:12] == [-(1 << 31), (1 << 31) - 1, INT64_MIN + (1 << 41), 32, (1 << 32) - 1]
    rec.calls.clear()
    for bad in (dict(miss=-1), dict(miss=1 << 13), dict(co=0), dict(co=33), dict(a=1 << 31), dict(b=-(1 << 31) - 1), dict(k=1 << 63)):
        with pytest.raises(ValueError):  # what ctypes would wrap silently
            eng.arith("linear", c1, c2, **{"co": 13, **bad})
    for bad in (dict(k=-1), dict(a=1 << 24)):  # co=None: lo < 0, hi >= 2^32
        with pytest.raises(ValueError):
            eng.arith("linear", c1, c2, **bad)
    for bad_op, kw in (("plus", {}), ("mul", dict(b=1))):
        with pytest.raises(ValueError):
            eng.arith(bad_op, c1, c2, co=13, **kw)
    with pytest.raises(AssertionError):
        eng.arith("linear", c1, c2, out=torch.zeros(1262, dtype=torch.uint8))  # shorter than the payload
    with pytest.raises(AssertionError):
        eng.arith("linear", c1, col(12, 776))  # columns of different lengths
    with pytest.raises(AssertionError):
        eng.arith("linear", c1, c2, out_of_range=torch.zeros(1, dtype=torch.int32))
    assert rec.calls == []


def test_arith_entry_point_fails_loudly_without_a_gpu(L):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    b1, b2, out = (C.c_uint8 * 1024)(), (C.c_uint8 * 1024)(), (C.c_uint8 * 1024)()
    rc = L.mi355_arith_dev(None, LINEAR, b1, 9, b2, 9, 100, 1, 1, 0, 10, 0, out, None)
    assert rc != 0 and L.mi355_last_error()


def test_every_arith_kernel_has_a_case():
    """every __global__ under csrc/arith/ is asserted from the launch record by a GPU case of this file, and the file names no
    kernel that does not exist"""
    kernels = support.global_kernels_of("arith")
    assert kernels == {EXACT_KERNEL, CHECKED_KERNEL}, kernels
    support.check_gpu_part_asserts(__file__, r"want_family\(")  # (not the constants: the GPU cases assert the predicted kernel)
    assert {want_family(r) for r in CO_EXACT} == {EXACT_KERNEL} and {want_family(r) for r in CO_CHECKED} == {CHECKED_KERNEL}
    assert [r.co for r in CO_EXACT] == [r.co for r in CO_CHECKED] == list(range(1, 33))  # all 64 instantiations run
    assert [r.c1 for r in C1_CASES] == [r.c2 for r in C2_CASES] == list(range(1, 33))


def test_arith_sources_read_no_flag_bits():
    assert [os.path.basename(p) for p in support.feature_sources("arith")] == ["arith.hip", "arith.hpp", "arith_kernels.hip", "arith_launch.hpp"]
    support.check_sources_read_no_flag_bits("arith")


def test_arith_reuses_the_lookup_pipeline():
    """the tile stream and the packed-out helpers are kernels/rt_column.hpp's, which lookup.hpp includes as well: included, not
    copied, under either name"""
    text = open(os.path.join(support.CSRC, "arith", "arith.hpp")).read()
    assert '#include "../kernels/rt_column.hpp"' in text and "lookup/lookup.hpp" not in text.split("#pragma once")[1]
    assert '#include "../kernels/rt_column.hpp"' in open(os.path.join(support.CSRC, "lookup", "lookup.hpp")).read()
    home = open(os.path.join(support.CSRC, "kernels", "rt_column.hpp")).read()
    for helper in ("rt_insert", "rt_insert_all", "rt_store", "rt_store_tail", "rt_issue_tile", "store_words_by", "columns_lds_value"):
        assert re.search(rf"\bvoid\s+{helper}\s*\(|\buint32_t\s+{helper}\s*\(", home), helper
    for helper in ("insert", "insert_all", "lookup_decode", "lookup_store", "lookup_store_tail", "columns_lds_value",
                   "rt_insert", "rt_insert_all", "rt_store", "rt_store_tail", "store_words_by"):
        assert not re.search(rf"\bvoid\s+{helper}\s*\(|\buint32_t\s+{helper}\s*\(", text), helper


def gpu_shapes():
    """every (recipe, n, same) the GPU tests below run on recipe data"""
    shapes = {(r, n, False) for r in SIZE_CASES for n in SIZES}
    shapes |= {(r, N_BIG, False) for r in CO_EXACT + CO_CHECKED + C1_CASES + C2_CASES + CORNER_CASES + NEGATIVE_TERM_CASES + OPERAND_CASES}
    shapes |= {(r, N_LONG, False) for r in LONG_CASES}
    shapes |= {(r, N_BIG, True) for r in SAME_BUFFER_CASES}
    shapes |= {(r, N_VIEW, False) for r in VIEW_CASES}
    shapes |= {(ERROR_RECIPE, ERROR_N, False)}
    return sorted(shapes, key=lambda s: (rid(s[0]), s[1], s[2]))


def test_gpu_recipes_are_what_the_library_would_launch(L):
    """(no device needed) this file's copy of the range rule is the library's, for every recipe a GPU case runs"""
    for r, n, same in gpu_shapes():
        assert L.mi355_arith_kernel({"linear": LINEAR, "mul": MUL}[r.op], r.c1, r.c2, r.a, r.b, r.k, r.co).decode() == want_family(r), r
    for r in CAPTURE_CASES:
        assert L.mi355_arith_kernel(LINEAR, r.c1, r.c2, r.a, r.b, r.k, r.co).decode() == want_family(r), r
    assert {want_family(r) for r in CAPTURE_CASES} == {EXACT_KERNEL, CHECKED_KERNEL}
    assert {want_family(r) for r in NEGATIVE_TERM_CASES} == {EXACT_KERNEL}
    assert {want_family(r) for r in CORNER_CASES} == {CHECKED_KERNEL}


@pytest.mark.parametrize("shape", [s for s in gpu_shapes() if s[1] >= 13], ids=lambda s: f"{rid(s[0])}-{s[1]}-{int(s[2])}")
def test_recipe_is_not_vacuous(shape):
    """(no device needed) a recipe of the checked kernel holds rows inside AND outside [0, 2^co), so neither the counter nor the
    miss value goes untested; a recipe of the exact kernel holds none outside; the results are not all alike; the corner pairs
    sit where corner_rows() puts them.  n = 1 holds one row and is left out."""
    r, n, same = shape
    x, y = data(r, n, 0, same)
    assert len(x) == len(y) == n and int(x.max()) <= top(r.c1) and int(y.max()) <= top(r.c2)
    want, outside = expect(r, x, y, miss_of(r.co))
    assert int(want.max()) <= top(r.co)
    if want_family(r) == CHECKED_KERNEL:
        assert 0 < outside < n, (r, outside)
    else:
        assert outside == 0
    assert len(np.unique(want)) >= 2 or (r.a == 0 and r.op == "mul"), "the expected column is constant"
    X, Y = top(r.c1), top(r.c2)
    corners = r.corners or ((0, 0), (X, Y), (X, 0), (0, Y))
    groups = corner_rows(n)
    if n >= R:
        assert any(rows[-1] == n // R * R - 1 for rows in groups), "no corner rows in the last full tile"
    if n % R >= 4 and n > 4:
        assert groups[-1][-1] == n - 1 and groups[-1][0] >= n // R * R, "no corner rows in the ragged tail"
    if not same:
        for rows in groups:
            assert [(int(x[i]), int(y[i])) for i in rows] == list(corners[:len(rows)]), rows


def test_corner_recipes_hit_their_corners():
    """(no device needed) the corner pairs produce the results their comments promise"""
    def results(r):
        return [(x * y * r.a if r.op == "mul" else r.a * x + r.b * y) + r.k for x, y in r.corners]

    assert results(CORNER_CASES[0]) == [0, -1, (1 << 9) - 1, 1 << 9]
    assert results(CORNER_CASES[1]) == [(1 << 32) + 5, 5, (1 << 8) + 5, 255]
    assert results(CORNER_CASES[2]) == [-(1 << 32) + 7, 7, -(1 << 32) - (1 << 16) + 7, 6]
    assert (results(CORNER_CASES[2])[0] & 0xFFFFFFFF) < 1 << 8 and (results(CORNER_CASES[1])[0] & 0xFFFFFFFF) < 1 << 8
    for r in NEGATIVE_TERM_CASES:  # before k is added the sum is negative in some row: it wraps in 32 bits
        x, y = data(r, N_BIG)
        part = (x.astype(np.int64) * y * r.a) if r.op == "mul" else x.astype(np.int64) * r.a + y.astype(np.int64) * r.b
        assert (part < 0).any() and rule_range(r.op, r.c1, r.c2, r.a, r.b, r.k)[0] == 0, r


@functools.lru_cache(maxsize=None)
def chain_data():
    """-> (g1, g2 in 0..6 at 3 bits, price at 17 bits, discount at 4 bits), uint32[N_BIG], read-only"""
    rng = np.random.default_rng(2026)
    g1 = rng.integers(0, 7, N_BIG, dtype=np.uint64).astype(np.uint32)
    g2 = rng.integers(0, 7, N_BIG, dtype=np.uint64).astype(np.uint32)
    price = rng.integers(0, 1 << 17, N_BIG, dtype=np.uint64).astype(np.uint32)
    discount = rng.integers(0, 11, N_BIG, dtype=np.uint64).astype(np.uint32)
    for v in (g1, g2, price, discount):
        v.setflags(write=False)
    return g1, g2, price, discount


def test_chain_data_is_not_vacuous():
    g1, g2, price, discount = chain_data()
    assert len(np.unique(g1.astype(np.int64) * 7 + g2)) == 49
    assert int((price.astype(np.int64) * discount).max()) >= 1 << 17


@functools.lru_cache(maxsize=None)
def capture_data(r):
    """two versions of (x, y) for the capture test"""
    return [data(r, N_BIG, salt) for salt in (11, 12)]


@pytest.mark.parametrize("r", CAPTURE_CASES, ids=rid)
def test_capture_data_is_not_vacuous(r):
    versions = capture_data(r)
    wants = [expect(r, x, y, miss_of(r.co)) for x, y in versions]
    assert (wants[0][0] != wants[1][0]).any(), "a stale result could pass"
    if want_family(r) == CHECKED_KERNEL:
        assert wants[0][1] != wants[1][1] and min(wants[0][1], wants[1][1]) > 0, "a stale counter could pass"


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

class Arith:
    """one engine, two uploaded columns (both in hostile surroundings), a guarded output refilled with 0xEE and a counter
    refilled with junk before every call"""

    def __init__(self, O, eng, r, n, same=False, salt=0):
        import torch

        from shared_simd_scan_amd.engine import PackedColumn

        self.O, self.eng, self.r, self.n, self.same = O, eng, r, n, same
        self.x, self.y = data(r, n, salt, same)
        self.miss = miss_of(r.co)
        self.col1 = PackedColumn(hostile_pack(O, self.x, r.c1), n, r.c1)
        self.col2 = self.col1 if same else PackedColumn(hostile_pack(O, self.y, r.c2), n, r.c2)
        self.nbytes = payload(n, r.co)
        self.out = Guarded(self.nbytes)
        self.counter = torch.empty(1, dtype=torch.int64, device="cuda")

    def out_view(self):
        return self.out.t[self.out.front: self.out.front + self.nbytes]

    def run(self, L, what="", counted=True):
        """-> checks every payload byte, the trailing bits, the guards, the inputs, the counter and the launch record; returns
        the record"""
        import torch

        r = self.r
        tag = (what, rid(r), self.n)
        want, outside = expect(r, self.x, self.y, self.miss)
        wb = self.O.pack(want, r.co)[: self.nbytes]
        self.out.t.fill_(SENTINEL)
        self.counter.fill_(-77)
        before1, before2 = self.col1.data.clone(), self.col2.data.clone()
        res = self.eng.arith(r.op, self.col1, self.col2, a=r.a, b=r.b, k=r.k, co=r.co, miss=self.miss, out=self.out_view(),
                             out_of_range=self.counter if counted else None)
        self.eng.synchronize()
        have = self.out.fetch()  # asserts the guard bytes on both sides
        assert res.data.data_ptr() == self.out_view().data_ptr() and (res.n, res.c) == (self.n, r.co)
        bad = np.nonzero(have != wb)[0]
        assert bad.size == 0, (tag, "byte", int(bad[0]), "of", self.nbytes, "have", int(have[bad[0]]), "want", int(wb[bad[0]]))
        if (self.n * r.co) % 8:
            assert int(have[-1]) >> ((self.n * r.co) % 8) == 0, (tag, "bits behind the last value are not zero")
        assert torch.equal(self.col1.data, before1) and torch.equal(self.col2.data, before2), (tag, "an input was written")
        fam = want_family(r)
        assert int(self.counter.item()) == (outside if counted else -77), (tag, "counter", int(self.counter.item()), "want", outside)
        assert fam == CHECKED_KERNEL or outside == 0
        rec = record(L, self.eng)
        (label, grid, lds, flags), = rec
        assert base_name(label) == fam and label.startswith(f"{fam}<{r.co}>"), (tag, label)
        assert flags == 0 and lds >= 4 * 2 * 256 * (r.c1 + r.c2), (tag, lds)
        return rec


@gpu
@pytest.mark.parametrize("r", SIZE_CASES, ids=rid)
def test_sizes_and_tails(L, O, eng, r):
    for n in SIZES:
        Arith(O, eng, r, n).run(L)


@gpu
@pytest.mark.parametrize("r", CO_EXACT + CO_CHECKED, ids=rid)
def test_every_output_width_through_both_kernels(L, O, eng, r):
    (label, _, _, _), = Arith(O, eng, r, N_BIG).run(L)
    assert base_name(label) == want_family(r)


@gpu
@pytest.mark.parametrize("r", C1_CASES + C2_CASES, ids=rid)
def test_every_input_width(L, O, eng, r):
    Arith(O, eng, r, N_BIG).run(L)


@gpu
@pytest.mark.parametrize("r", CORNER_CASES + NEGATIVE_TERM_CASES + OPERAND_CASES, ids=rid)
def test_corner_rows_and_operands(L, O, eng, r):
    """results at the edges of the range, results whose low 32 bits lie in range while they do not, the exact kernel's 32-bit
    wrap-around with negative terms, a = 0, b = 0, a = -2^31, k beyond 2^32"""
    Arith(O, eng, r, N_BIG).run(L)


@gpu
@pytest.mark.parametrize("r", SAME_BUFFER_CASES, ids=rid)
def test_same_buffer_as_both_inputs(L, O, eng, r):
    look = Arith(O, eng, r, N_BIG, same=True)
    assert look.col1.data.data_ptr() == look.col2.data.data_ptr()
    look.run(L, what="same buffer")


@gpu
def test_null_counter_and_empty_column(L, O, eng):
    """a null counter is accepted by both kernels; n == 0 writes the counter and no output byte, launches nothing and needs no
    buffers"""
    import torch

    for r in (SIZE_CASES[0], SIZE_CASES[2]):
        Arith(O, eng, r, N_BIG).run(L, what="null counter", counted=False)
    look = Arith(O, eng, SIZE_CASES[2], 13)
    for n_ptrs in (True, False):
        look.out.t.fill_(SENTINEL)
        look.counter.fill_(-77)
        p1, p2, po = (look.col1.data.data_ptr(), look.col2.data.data_ptr(), look.out.ptr) if n_ptrs else (None, None, None)
        rc = L.mi355_arith_dev(eng._ctx, LINEAR, p1, 32, p2, 32, 0, 1, -1, (1 << 32) - 1, 32, 0, po, look.counter.data_ptr())
        eng.synchronize()
        assert rc == 0 and record(L, eng) == [] and int(look.counter.item()) == 0
        assert (look.out.fetch() == SENTINEL).all()
    assert L.mi355_arith_dev(eng._ctx, LINEAR, None, 32, None, 32, 0, 1, -1, 0, 32, 0, None, None) == 0  # nothing at all to do
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("r", VIEW_CASES, ids=rid)
def test_row_range_views(L, O, eng, r):
    """rows [lead, lead + n) of two longer columns computed into rows [lead_out, lead_out + n) of a longer output column: exactly
    the slice's bytes change, and nothing of the foreign rows reaches them or the counter"""
    import torch

    from shared_simd_scan_amd.engine import PackedColumn

    n, lead, trail, lead_out = N_VIEW, 2 * R + 128, 4096, 384
    assert n % 8 == 0 and n % 32 and lead % 128 == 0 and lead_out % 128 == 0
    x, y = data(r, n)
    rng = np.random.default_rng([r.c1, r.c2, 13])
    cols = []
    for vals, c in ((x, r.c1), (y, r.c2)):
        junk = rng.integers(0, 1 << c, lead, dtype=np.uint64).astype(np.uint32)
        whole = PackedColumn(plain_pack(O, np.concatenate([junk, vals, np.full(trail, top(c), dtype=np.uint32)]), c), lead + n + trail, c)
        cols.append(eng.slice_rows(whole, lead, lead + n))
        assert cols[-1].n == n and cols[-1].data.data_ptr() % 16 == 0
    n_out = lead_out + n + 1000
    before = rng.integers(0, 1 << r.co, n_out, dtype=np.uint64).astype(np.uint32)
    out_whole = PackedColumn(plain_pack(O, before, r.co), n_out, r.co)
    out_bytes_before = out_whole.data.cpu().numpy().copy()
    out_slice = eng.slice_rows(out_whole, lead_out, lead_out + n)
    miss = miss_of(r.co)
    counter = torch.full((1,), -77, dtype=torch.int64, device="cuda")
    res = eng.arith(r.op, cols[0], cols[1], a=r.a, b=r.b, k=r.k, co=r.co, miss=miss, out=out_slice.data, out_of_range=counter)
    eng.synchronize()
    (label, _, _, _), = record(L, eng)
    assert base_name(label) == want_family(r) and res.data.data_ptr() == out_slice.data.data_ptr()
    want, outside = expect(r, x, y, miss)
    assert int(counter.item()) == outside
    after = before.copy()
    after[lead_out: lead_out + n] = want
    want_bytes = O.pack(after, r.co)
    have = out_whole.data.cpu().numpy()
    first, last = lead_out * r.co // 8, (lead_out + n) * r.co // 8
    assert (have[:first] == out_bytes_before[:first]).all(), "rows in front of the slice changed"
    assert (have[last:] == out_bytes_before[last:]).all(), "rows behind the slice changed"
    assert (have == want_bytes).all()
    assert (O.decompress(have, n_out, r.co).view(np.uint32) == after).all()


@gpu
def test_errors_launch_nothing(L, O, eng):
    import torch

    r, n = ERROR_RECIPE, ERROR_N
    look = Arith(O, eng, r, n)
    big = Guarded(8192)  # a buffer that can stand for an input and the output at once
    p1, p2, po = look.col1.data.data_ptr(), look.col2.data.data_ptr(), look.out.ptr.value
    cp = look.counter.data_ptr()
    miss = look.miss

    def call(op=LINEAR, p1=p1, c1=r.c1, p2=p2, c2=r.c2, n=n, a=r.a, b=r.b, k=r.k, co=r.co, miss=miss, po=po, cp=cp):
        for g in (look.out, big):
            g.t.fill_(SENTINEL)
        look.counter.fill_(-77)
        rc = L.mi355_arith_dev(eng._ctx, op, p1, c1, p2, c2, n, a, b, k, co, miss, po, cp)
        eng.synchronize()
        return rc

    want, outside = expect(r, look.x, look.y, miss)
    assert call() == 0 and base_name(record(L, eng)[0][0]) == want_family(r) == CHECKED_KERNEL and int(look.counter.item()) == outside
    valid = record(L, eng)
    nb_out, nb1, nb2 = payload(n, r.co), payload(n, r.c1), payload(n, r.c2)
    assert max(nb_out, nb1, nb2) + 512 <= 8192
    errors = (("op = 2", dict(op=2), b"op"), ("op = -1", dict(op=-1), b"op"),
              ("c1 = 0", dict(c1=0), b"c1"), ("c1 = 33", dict(c1=33), b"c1"), ("c2 = 0", dict(c2=0), b"c2"), ("c2 = 33", dict(c2=33), b"c2"),
              ("co = 0", dict(co=0), b"co"), ("co = 33", dict(co=33), b"co"),
              ("b != 0 with mul", dict(op=MUL), b"b must be 0"),
              ("miss = 2^co", dict(miss=1 << r.co), b"miss"), ("miss = 2^32 - 1", dict(miss=(1 << 32) - 1), b"miss"),
              ("hi beyond int64", dict(k=INT64_MAX - 100), b"int64"), ("lo beyond int64", dict(a=-1, b=-1, k=INT64_MIN + 100), b"int64"),
              ("mul 32 x 32", dict(op=MUL, b=0, c1=32, c2=32, k=0), b"int64"),
              ("null column 1", dict(p1=None), b"packed1_dev"), ("null column 2", dict(p2=None), b"packed2_dev"), ("null output", dict(po=None), b"out_dev"),
              ("column 1 at +4", dict(p1=p1 + 4), b"aligned"), ("column 2 at +8", dict(p2=p2 + 8), b"aligned"), ("output at +4", dict(po=po + 4), b"aligned"),
              ("counter at +4", dict(cp=cp + 4), b"out_of_range_dev"),
              ("output is column 1", dict(p1=big.ptr.value, po=big.ptr.value), b"overlaps packed1_dev"),
              ("output starts in column 1's last byte", dict(p1=big.ptr.value, po=big.ptr.value + (nb1 - 1) // 16 * 16), b"overlaps packed1_dev"),
              ("column 1 starts inside the output", dict(p1=big.ptr.value + 256, po=big.ptr.value), b"overlaps packed1_dev"),
              ("output is column 2", dict(p2=big.ptr.value, po=big.ptr.value), b"overlaps packed2_dev"),
              ("output starts in column 2's last byte", dict(p2=big.ptr.value, po=big.ptr.value + (nb2 - 1) // 16 * 16), b"overlaps packed2_dev"),
              ("column 2 starts inside the output", dict(p2=big.ptr.value + 64, po=big.ptr.value), b"overlaps packed2_dev"))
    for what, kw, word in errors:
        assert call(**kw) == E_INVALID, what
        assert word in L.mi355_last_error(), (what, L.mi355_last_error())
        assert record(L, eng) == [], what  # a refused call leaves an empty record and launches nothing
        for g in (look.out, big):
            assert (g.fetch() == SENTINEL).all(), what
        assert int(look.counter.item()) == -77, what
    # neighbours that do not overlap are fine: the output begins where column 2's bytes end
    at = (nb2 + 15) // 16 * 16
    big.t.fill_(SENTINEL)
    big.t[big.front: big.front + nb2] = torch.from_numpy(O.pack(look.y, r.c2)[:nb2].copy()).cuda()
    rc = L.mi355_arith_dev(eng._ctx, LINEAR, p1, r.c1, big.ptr.value, r.c2, n, r.a, r.b, r.k, r.co, miss, big.ptr.value + at, cp)
    eng.synchronize()
    assert rc == 0 and record(L, eng) == valid
    got = big.fetch()
    assert (got[at: at + nb_out] == O.pack(want, r.co)[:nb_out]).all()
    assert (got[nb2: at] == SENTINEL).all() and (got[at + nb_out:] == SENTINEL).all()


@gpu
@pytest.mark.parametrize("r", LONG_CASES, ids=rid)
def test_one_block_walks_many_tiles(L, O, eng, r):
    """grid_cus = 1, max_blocks_per_cu = 1: one block, its four waves walk sixteen tiles each -- the alternating images of both
    columns, the deferred stores, the per-wave counter, the ragged tail"""
    look = Arith(O, eng, r, N_LONG)
    eng.set_option("grid_cus", 1)
    eng.set_option("max_blocks_per_cu", 1)
    try:
        (label, grid, lds, flags), = look.run(L, what="one block")
        assert grid == 1 and base_name(label) == want_family(r)
    finally:
        eng.set_option("grid_cus", 0)
        eng.set_option("max_blocks_per_cu", 0)
    (label, grid, lds, flags), = look.run(L, what="whole chip")
    assert grid > 1


@gpu
def test_composite_key_then_group_aggregate(L, O, eng):
    """SELECT g1, g2, sum(price), count(*), min, max ... GROUP BY g1, g2: the key g1 * 7 + g2, then group_aggregate"""
    from shared_simd_scan_amd.engine import PackedColumn

    g1, g2, price, discount = chain_data()
    key = eng.arith("linear", PackedColumn(plain_pack(O, g1, 3), N_BIG, 3), PackedColumn(plain_pack(O, g2, 3), N_BIG, 3), a=7, b=1)
    (label, _, _, _), = record(L, eng)
    r = Recipe("linear", 3, 3, 7, 1, 0, 6)
    assert base_name(label) == want_family(r) == EXACT_KERNEL and (key.n, key.c) == (N_BIG, 6)
    agg = eng.group_aggregate(key, PackedColumn(plain_pack(O, price, 17), N_BIG, 17))
    eng.synchronize()
    # numpy's two-key group-by: np.unique over the (g1, g2) pairs, laid out at g1 * 7 + g2
    want = np.zeros((64, 4), dtype=np.uint64)
    want[:, 2] = (1 << 64) - 1
    pairs, inverse = np.unique(np.stack([g1, g2], axis=1), axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    for j, (k1, k2) in enumerate(pairs):
        v = price[inverse == j].astype(np.uint64)
        want[int(k1) * 7 + int(k2)] = (v.sum(), len(v), v.min(), v.max())
    assert (want == grouped(g1.astype(np.int64) * 7 + g2, price, 64)).all()
    assert (agg.cpu().numpy().view(np.uint64) == want).all()


@gpu
def test_product_then_aggregate(L, O, eng):
    """SELECT sum(price * discount): the product column, then aggregate"""
    from shared_simd_scan_amd.engine import PackedColumn

    g1, g2, price, discount = chain_data()
    prod = eng.arith("mul", PackedColumn(plain_pack(O, price, 17), N_BIG, 17), PackedColumn(plain_pack(O, discount, 4), N_BIG, 4))
    (label, _, _, _), = record(L, eng)
    assert base_name(label) == want_family(Recipe("mul", 17, 4, 1, 0, 0, 21)) == EXACT_KERNEL and (prod.n, prod.c) == (N_BIG, 21)
    agg = eng.aggregate(prod)
    eng.synchronize()
    p = price.astype(np.int64) * discount.astype(np.int64)
    assert [int(v) for v in agg.cpu().numpy()] == [int(p.sum()), N_BIG, int(p.min()), int(p.max())]


@gpu
def test_arith_on_compacted_columns(L, O, eng):
    """WHERE g1 = 3: both columns compacted by the one bitmap stay row-aligned; their difference as a column, then its histogram"""
    import torch

    from shared_simd_scan_amd.engine import PackedColumn

    g1, g2, price, discount = chain_data()
    bitmap, hits = eng.scan_where("==", 3, PackedColumn(plain_pack(O, g1, 3), N_BIG, 3))
    a = eng.compact_column(PackedColumn(plain_pack(O, g2, 3), N_BIG, 3), bitmap)
    b = eng.compact_column(PackedColumn(plain_pack(O, discount, 4), N_BIG, 4), bitmap)
    sel = g1 == 3
    assert a.n == b.n == int(sel.sum()) > R
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    diff = eng.arith("linear", a, b, a=1, b=-1, k=3, co=4, miss=15, out_of_range=counter)
    (label, _, _, _), = record(L, eng)
    r = Recipe("linear", 3, 4, 1, -1, 3, 4)
    assert base_name(label) == want_family(r) == CHECKED_KERNEL
    hist = eng.histogram(diff)
    eng.synchronize()
    want, outside = expect(r, g2[sel], discount[sel], 15)
    assert 0 < outside < a.n and int(counter.item()) == outside
    assert (diff.data.cpu().numpy()[: payload(a.n, 4)] == O.pack(want, 4)[: payload(a.n, 4)]).all()
    assert (hist.cpu().numpy() == np.bincount(want, minlength=16)).all()


@gpu
@pytest.mark.parametrize("r", CAPTURE_CASES, ids=rid)
def test_graph_capture_and_replay(O, r):
    """one call with its counter in a graph on a side stream: after the inputs' contents change the replay follows them"""
    import torch

    from shared_simd_scan_amd.engine import PackedColumn

    n = N_BIG
    fam = want_family(r)
    miss = miss_of(r.co)
    versions = capture_data(r)
    wants = [expect(r, x, y, miss) for x, y in versions]

    def steps(eng):
        stage = [(plain_pack(O, x, r.c1), plain_pack(O, y, r.c2)) for x, y in versions]
        col1, col2 = PackedColumn(torch.empty_like(stage[0][0]), n, r.c1), PackedColumn(torch.empty_like(stage[0][1]), n, r.c2)
        out = Guarded(payload(n, r.co))
        out_view = out.t[out.front: out.front + out.nbytes]
        counter = torch.empty(1, dtype=torch.int64, device="cuda")

        def load(v):
            col1.data.copy_(stage[v][0])
            col2.data.copy_(stage[v][1])
            out.t.fill_(SENTINEL)
            counter.fill_(-77)

        def run():
            eng.arith(r.op, col1, col2, a=r.a, b=r.b, k=r.k, co=r.co, miss=miss, out=out_view, out_of_range=counter)

        def check(v, what):
            assert (out.fetch() == O.pack(wants[v][0], r.co)[: out.nbytes]).all(), what
            assert int(counter.item()) == wants[v][1], what

        def untouched():
            assert (out.fetch() == SENTINEL).all() and int(counter.item()) == -77

        def warmed(launched):
            assert [base_name(x[0]) for x in launched] == [fam]

        return capture.Steps(load, run, check, untouched, warmed)

    capture.capture_replay(steps, (0, 1, 0))
