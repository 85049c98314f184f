"""CPU: how ScanEngine turns a caller's predicate constants into C ABI arguments (engine.clamp_const / range_bounds / key32 /
keys32), checked against exact Python-int comparisons over the constants where it can go wrong: the int64 limits, the
int32 / uint32 limits, the column's own domain edges and ints beyond 64 bits.

ctypes masks an int that does not fit an argument's C type, without an error; the tests below pin that, and run every
wrapper against a stand-in library that converts the arguments through the real argtypes, so a wrapper that hands a
constant to ctypes unconverted fails here.  The GPU side of the same constants is tests/test_predicate_edges.py.
"""
import ctypes as C
import operator
import types

import numpy as np
import pytest

from shared_simd_scan_amd import _capi, engine

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
OPS = {"==": operator.eq, "!=": operator.ne, "<": operator.lt, "<=": operator.le, ">": operator.gt, ">=": operator.ge}
WIDTHS = list(range(1, 33))


def constants(c):
    """the constant set of the predicate-edge tests, with the two that only a Python caller can pass"""
    vmax = (1 << c) - 1
    cs = [INT64_MIN, -(1 << 32) - 1, -(1 << 31) - 1, -(1 << 31), -1, 0, 1, 1 << (c - 1), vmax - 1, vmax, vmax + 1,
          (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, INT64_MAX, (1 << 64) + 5, INT64_MIN - 1]
    return sorted(set(cs))


def domain_edges(c):
    vmax = (1 << c) - 1
    return sorted({0, 1, (1 << (c - 1)) - 1, 1 << (c - 1), vmax - 1, vmax, vmax // 3})


# ---- what ctypes does with ints that do not fit ----------------------------------------------------------------------

def test_ctypes_masks_out_of_range_ints_without_error():
    """the reason every constant goes through a helper: c_uint32 / c_int32 / c_int64 keep the low bits and say nothing"""
    assert C.c_uint32(-1).value == 0xFFFFFFFF
    assert C.c_uint32((1 << 32) + 3).value == 3
    assert C.c_int32((1 << 32) + 5).value == 5
    assert C.c_int32(1 << 31).value == -(1 << 31)
    assert C.c_int64((1 << 64) + 5).value == 5
    assert C.c_int64(1 << 63).value == INT64_MIN
    assert C.c_int64(INT64_MIN - 1).value == INT64_MAX
    # the same on a call through argtypes: the callee sees the masked values
    seen = []
    proto = C.CFUNCTYPE(C.c_int, C.c_uint32, C.c_int32, C.c_int64)
    fn = proto(lambda a, b, c: seen.append((a, b, c)) or 0)
    fn(-1, (1 << 32) + 5, (1 << 64) + 5)
    assert seen == [(0xFFFFFFFF, 5, 5)]


def test_constant_arguments_have_the_c_types_the_helpers_target():
    """the helpers' ranges are chosen for these argument types (include/mi355_scan.h)"""
    sig = {name: args for name, _, args in _capi.HEADERS["mi355_scan.h"]}
    assert sig["mi355_scan_eq_dev"][4] is C.c_int32
    assert sig["mi355_scan_range_dev"][4:6] == [C.c_uint32, C.c_uint32]
    for name, idx in (("mi355_scan_where_dev", (5, 6)), ("mi355_scan_combine_dev", (5, 6)), ("mi355_scan_select_dev", (5, 6)),
                      ("mi355_scan2_dev", (4, 5, 9, 10))):
        assert all(sig[name][i] is C.c_int64 for i in idx), name


# ---- the helpers against exact comparisons ---------------------------------------------------------------------------

@pytest.mark.parametrize("c", WIDTHS)
def test_clamp_const_keeps_every_comparison(c):
    for x in constants(c):
        y = engine.clamp_const(x)
        assert -1 <= y <= 1 << 32 and C.c_int64(y).value == y
        if 0 <= x < 1 << 32:
            assert y == x
        for v in domain_edges(c):
            for op, f in OPS.items():
                assert f(v, y) == f(v, x), (c, v, op, x, y)


@pytest.mark.parametrize("c", WIDTHS)
def test_range_bounds_select_exactly_the_rows_between(c):
    for lo in constants(c):
        for hi in constants(c):
            got = engine.range_bounds(lo, hi)
            if got is not None:
                assert 0 <= got[0] <= got[1] <= 0xFFFFFFFF
                assert C.c_uint32(got[0]).value == got[0] and C.c_uint32(got[1]).value == got[1]
            for v in domain_edges(c):
                want = lo <= v <= hi
                assert (got is not None and got[0] <= v <= got[1]) == want, (c, lo, hi, v, got)


def test_range_bounds_follow_the_dropin_header():
    """include/simd_scan.hpp scan(int lo, int hi): hi < 0 or lo > hi is empty, a negative lo is 0; beyond 32 bits: hi caps at
    0xffffffff, lo >= 2^32 is empty"""
    assert engine.range_bounds(-1, 5) == (0, 5)
    assert engine.range_bounds(INT64_MIN, INT64_MAX) == (0, 0xFFFFFFFF)
    assert engine.range_bounds(0, (1 << 32) + 3) == (0, 0xFFFFFFFF)
    assert engine.range_bounds(7, 7) == (7, 7)
    for lo, hi in ((3, -1), (5, 2), (-5, -1), (1 << 32, 1 << 33), (INT64_MAX, INT64_MAX), ((1 << 64) + 5, (1 << 64) + 5)):
        assert engine.range_bounds(lo, hi) is None, (lo, hi)


@pytest.mark.parametrize("c", WIDTHS)
def test_key32_keeps_the_meaning_or_refuses(c):
    """keys in [-2^31, 2^32) keep their unsigned 32-bit pattern (at c = 32 key -1 is the value 0xffffffff); any other key
    matches nothing below c = 32 and is refused at c = 32"""
    for k in constants(c) + [-(1 << 31) + 1, (1 << 31) + 1]:
        if not -(1 << 31) <= k < 1 << 32:
            if c == 32:
                with pytest.raises(ValueError):
                    engine.key32(k, c)
                continue
            r = engine.key32(k, c)
            assert C.c_int32(r).value == r and (r & 0xFFFFFFFF) >> c, (c, k, r)  # a pattern >= 2^c: no value equals it
            continue
        r = engine.key32(k, c)
        assert C.c_int32(r).value == r and (r & 0xFFFFFFFF) == (k & 0xFFFFFFFF), (c, k, r)
        if c < 32:
            for v in domain_edges(c):
                assert ((r & 0xFFFFFFFF) == v) == (k == v), (c, k, v)


@pytest.mark.parametrize("c", [1, 9, 31, 32])
def test_keys32_is_key32_over_the_list(c):
    keys = [k for k in constants(c) if c < 32 or -(1 << 31) <= k < 1 << 32]
    got = engine.keys32(keys, c)
    assert got.dtype == np.int32 and got.flags["C_CONTIGUOUS"]
    assert got.tolist() == [engine.key32(k, c) for k in keys]
    assert engine.keys32(np.array([3, -1, 5], dtype=np.int64), c).tolist() == [3, -1, 5]
    if c == 32:
        with pytest.raises(ValueError):
            engine.keys32([3, 1 << 32], c)


# ---- every wrapper converts its constants before ctypes sees them ----------------------------------------------------

# differs from support.RecordingLib: the key lists are read through their pointers, and args() finds a call by name
class _RecordingLib:
    """stand-in for libmi355scan.so: each call converts its arguments through the real argtypes (as ctypes would) and
    records them; the key lists are read through their pointers"""

    def __init__(self):
        self.calls = []
        self._sig = {name: args for name, _, args in _capi.HEADERS["mi355_scan.h"]}

    def __getattr__(self, name):
        argtypes = self._sig[name]

        def call(*args):
            conv = []
            for t, a in zip(argtypes, args):
                if t in (C.c_int32, C.c_uint32, C.c_int64, C.c_uint64, C.c_int, C.c_uint) and isinstance(a, int):
                    a = t(a).value
                conv.append(a)
            if name in ("mi355_scan_in_dev", "mi355_shared_scan_eq_dev"):
                P = conv[5]
                conv[4] = np.ctypeslib.as_array(C.cast(conv[4], C.POINTER(C.c_int32)), shape=(P,)).tolist()
            self.calls.append((name, conv))
            return 0

        return call

    def args(self, name):
        """the converted arguments of the last call of `name`"""
        return [a for n, a in self.calls if n == name][-1]


@pytest.fixture
def fake(monkeypatch):
    import torch

    rec = _RecordingLib()
    monkeypatch.setattr(engine, "lib", lambda: rec)
    monkeypatch.setattr(engine, "check", lambda rc: None)
    eng = object.__new__(engine.ScanEngine)
    eng._ctx, eng._dev = None, torch.device("cpu")

    def col(c, n=1000):
        return types.SimpleNamespace(data=torch.zeros(64, dtype=torch.uint8), n=n, c=c)

    return eng, rec, col


def test_scan_range_wrapper_applies_the_dropin_rules(fake):
    eng, rec, col = fake
    for (lo, hi), want in (((-1, 5), (0, 5)), ((0, (1 << 32) + 3), (0, 0xFFFFFFFF)), ((INT64_MIN, INT64_MAX), (0, 0xFFFFFFFF)),
                           ((7, 9), (7, 9))):
        rec.calls.clear()
        eng.scan_range(lo, hi, col(9))
        (name, args), = rec.calls
        assert name == "mi355_scan_range_dev" and tuple(args[4:6]) == want, (lo, hi, args)
    for lo, hi in ((-5, -1), (5, 2), (1 << 32, 1 << 33)):
        rec.calls.clear()
        eng.scan_range(lo, hi, col(9))
        (name, args), = rec.calls
        assert args[4] > args[5], (lo, hi, args)  # the C side's empty range


def test_comparison_wrappers_pass_clamped_constants(fake):
    eng, rec, col = fake
    for x in constants(9):
        want = min(max(x, -1), 1 << 32)
        eng.scan_where("<", x, col(9), b=x)
        eng.scan_combine(">=", x, col(9), b=x, count_only=True)
        eng.scan_select("between", x, col(9), capacity=4, b=x)
        eng.scan2(col(9), "==", x, col(5), "!=", x, b1=x, b2=x)
        got = [tuple(rec.args(name)[5:7]) for name in ("mi355_scan_where_dev", "mi355_scan_combine_dev", "mi355_scan_select_dev")]
        got.append(tuple(rec.args("mi355_scan2_dev")[i] for i in (4, 5, 9, 10)))
        assert got == [(want, want)] * 3 + [(want,) * 4], (x, got)


@pytest.mark.parametrize("c", [9, 31, 32])
def test_key_wrappers_never_wrap_a_key_onto_a_value(fake, c):
    eng, rec, col = fake
    inside = [k for k in constants(c) if -(1 << 31) <= k < 1 << 32]
    outside = [k for k in constants(c) if k not in inside]
    for k in inside:
        rec.calls.clear()
        eng.scan(k, col(c))
        eng.scan_in([k], col(c))
        eng.shared_scan([k, 1], col(c))
        got = [rec.args("mi355_scan_eq_dev")[4], rec.args("mi355_scan_in_dev")[4][0], rec.args("mi355_shared_scan_eq_dev")[4][0]]
        assert [g & 0xFFFFFFFF for g in got] == [k & 0xFFFFFFFF] * 3, (c, k, got)
    for k in outside:
        if c == 32:
            for call in (lambda: eng.scan(k, col(c)), lambda: eng.scan_in([1, k], col(c)), lambda: eng.shared_scan([k], col(c))):
                with pytest.raises(ValueError):
                    call()
            continue
        rec.calls.clear()
        eng.scan(k, col(c))
        eng.scan_in([k], col(c))
        eng.shared_scan([k, 1], col(c))
        got = [rec.args("mi355_scan_eq_dev")[4], rec.args("mi355_scan_in_dev")[4][0], rec.args("mi355_shared_scan_eq_dev")[4][0]]
        assert all((g & 0xFFFFFFFF) >> c for g in got), (c, k, got)  # no c-bit value equals the key passed
