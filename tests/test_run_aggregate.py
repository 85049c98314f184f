"""Sum, count, min and max of a packed column per run of a table of run ends (include/mi355_run_aggregate.h,
ScanEngine.run_aggregate / sorted_group_aggregate): entry j holds the aggregates of the rows i < n with j(i) == j, j(i) the number
of j < R with end_j <= i, among the rows a mask selects; a run without a counted row reads (0, 0, UINT64_MAX, 0).

CPU: the header is plain C99 and declares exactly what _capi.HEADERS binds for it; it carries its graph-capture verdict; the names
are exported; the kernel-name function answers on both sides of every refusal; the span-slot rule; the two __global__ under
csrc/runagg/ are asserted from the launch record by a GPU case of this file; no source there names a store policy, reads a switch
bit or reaches the context's workspace, scratch or pool; the engine wrappers hand the C ABI what they should (through a recording
stand-in for the library); the data recipes are not vacuous.

GPU (-m gpu): every expectation is numpy on data the test generated (np.searchsorted for j(i), np.add.at / np.minimum.at /
np.maximum.at in uint64); nothing is derived from engine output.  The table and the counter sit in support.Guarded buffers full
of SENTINEL: exactly 32 * runs bytes are written.  Column and ends are uploaded in hostile surroundings (ones in the bits behind
the last row and in the pad), the mask with 0xFF bytes directly behind it.

A lane owns 32 rows, a tile is 2048, a wave's chunk 16384: the sizes are the smallest on both sides of each.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import capture
import support
from support import E_INVALID, SENTINEL, Guarded, L, base_name, eng, fake, hostile_bitmap, hostile_pack, plain_pack, record  # noqa: F401  (L, eng, fake: fixtures)

HEADER = "mi355_run_aggregate.h"
INIT_KERNEL = "run_aggregate_init_kernel"
AGG_KERNEL = "run_aggregate_kernel"

LANE, R, CHUNK = 32, 2048, 16384
N_BIG = 9 * 8192 + 1237        # five chunks, the last ragged in tile, lane and byte
N_CROSS = CHUNK + R + 100      # a chunk boundary, tile and lane boundaries
N_ONE_BLOCK = 9 * CHUNK + 123  # ten chunks for the four waves of a one-block grid
SIZES = [1, 31, 32, 33, 2047, 2048, 2049, 16384, 16385, N_BIG]
WIDTH_PAIRS = [(9, 1), (9, 14), (1, 32), (17, 32), (32, 14), (32, 32)]
EMPTY = (0, 0, (1 << 64) - 1, 0)

gpu = pytest.mark.gpu


def top(c):
    return (1 << c) - 1


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---- the definition, in numpy ---------------------------------------------------------------------------------------------------

def run_of_row(ends, R_, n):
    """j(i) for i < n: the number of j < R with end_j <= i (non-decreasing ends)"""
    e = np.asarray(ends[:R_], dtype=np.int64)
    assert (np.diff(e) >= 0).all()
    return np.searchsorted(e, np.arange(n, dtype=np.int64), side="right")


def reference(x, ends, R_, runs, mask=None):
    """-> (table uint64[runs, 4], counted rows behind the last run)"""
    n = len(x)
    want = np.zeros((runs, 4), dtype=np.uint64)
    want[:, 2] = EMPTY[2]
    j = run_of_row(ends, R_, n)
    sel = np.ones(n, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    inside = sel & (j < R_)
    jj, v = j[inside], x[inside].astype(np.uint64)
    np.add.at(want[:, 0], jj, v)
    np.add.at(want[:, 1], jj, np.uint64(1))
    np.minimum.at(want[:, 2], jj, v)
    np.maximum.at(want[:, 3], jj, v)
    return want, int((sel & (j == R_)).sum())


def runs_per_tile(ends, R_, n):
    """the runs a tile of 2048 rows addresses: j(last row) - j(first row) + 1, run R (the rows behind the last run) not counted"""
    j = run_of_row(ends, R_, n)
    first = np.arange(0, n, R)
    last = np.minimum(first + R - 1, n - 1)
    return np.minimum(j[last], max(R_ - 1, 0)) - np.minimum(j[first], max(R_ - 1, 0)) + 1


# ---- recipes --------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def values_of(c, n, seed=0):
    return frozen(np.random.default_rng([c, n, seed, 51]).integers(0, 1 << c, n, dtype=np.uint64).astype(np.uint32))


@functools.lru_cache(maxsize=None)
def ends_of(n, mean, seed=0, last="at"):
    """ends of runs of geometric length around `mean`; last: the last end 'below' n, 'at' n or 'above' n"""
    t = np.random.default_rng([n, mean, seed, 53]).random(n) < 1.0 / mean
    t[-1] = last != "below"
    e = (np.nonzero(t)[0] + 1).astype(np.int64)
    if last == "below" and (len(e) == 0 or e[-1] > n - 5):
        e = e[e <= n - 5]
    if last == "above":
        e[-1] = n + 5000
    return frozen(e.astype(np.uint32))


def ends_from(lengths):
    return np.cumsum(np.asarray(lengths, dtype=np.int64)).astype(np.uint32)


CROSS_ENDS = sorted({LANE * k + d for k in (1, 3, 7, 64, 65) for d in (-1, 0, 1)} | {R * k + d for k in (1, 2, 3) for d in (-1, 0, 1)}
                    | {CHUNK - 1, CHUNK, CHUNK + 1, N_CROSS})


def span_lengths(S, extra):
    """three tiles and a bit: tile 1 addresses exactly S runs of 2048 / S rows (extra = 0), or S + 1 with every run begun one row
    earlier (extra = 1)"""
    q = R // S
    return [R - extra] + [q] * (S + extra) + [R + 50 - (q - 1) * extra]


def zero_runs_in_front(ends, k=63):
    """k equal ends (runs of length zero) in front of every run"""
    e = np.asarray(ends, dtype=np.int64)
    out = np.repeat(e, k + 1).reshape(-1, k + 1)
    out[:, :k] = np.r_[0, e[:-1]][:, None]  # a run of length zero ends where the run in front of it ends
    return frozen(out.ravel().astype(np.uint32))


@functools.lru_cache(maxsize=None)
def sparse_group_keys(n=20000, groups=300, seed=0):
    """20000 rows over 300 distinct sparse 32-bit keys, the largest of them 2^32 - 1; 17-bit values; a mask that leaves one key out"""
    rng = np.random.default_rng([n, groups, seed, 57])
    domain = np.unique(np.r_[rng.integers(0, 1 << 32, groups - 1, dtype=np.uint64), np.uint64(top(32))])
    assert len(domain) == groups
    which = rng.integers(0, groups, n)
    which[:groups] = np.arange(groups)  # every key occurs
    keys = domain[which].astype(np.uint32)
    values = rng.integers(0, 1 << 17, n, dtype=np.uint64).astype(np.uint32)
    mask = (rng.random(n) < 0.5) & (which != 123)
    return frozen(keys, values, mask)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------

def test_header_is_plain_c99():
    support.check_header_is_plain_c99(HEADER)


def test_header_declares_what_python_binds(L):
    names, sigs = support.check_header_binds(L, HEADER)
    assert names == ["mi355_run_aggregate_dev", "mi355_run_aggregate_kernel", "mi355_run_aggregate_span_slots"]
    sig = sigs["mi355_run_aggregate_dev"]
    assert sig[2] is C.c_uint and sig[3] is C.c_uint64 and sig[6] is C.c_uint and sig[7] is C.c_uint64 and len(sig) == 11
    assert sigs["mi355_run_aggregate_kernel"] == [C.c_uint, C.c_uint] and sigs["mi355_run_aggregate_span_slots"] == [C.c_uint]
    assert L.mi355_run_aggregate_kernel.restype is C.c_char_p and L.mi355_run_aggregate_span_slots.restype is C.c_uint32
    text = support.header_text(HEADER)
    assert '#include "mi355_scan.h"' in text and text.count("#include") == 1
    from shared_simd_scan_amd._capi import HEADERS

    assert list(HEADERS).index(HEADER) < list(HEADERS).index("mi355_runs.h")


def test_header_carries_its_capture_verdict():
    text = support.header_text(HEADER)
    assert len(re.findall(r"graph capture: capturable\b", text)) == 1
    support.check_capture_verdict(HEADER, r"two kernels on the context's stream and nothing else", r"no memset node", r"no buffer of the context's pool",
                                  r"never synchronises, whatever its arguments", r"needs no warm-up call", r"read at every\s+\*?\s*replay")


def test_names_are_exported():
    import shared_simd_scan_amd as pkg

    for name in ("run_aggregate_kernel", "run_aggregate_span_slots"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    for name in ("run_aggregate", "sorted_group_aggregate"):
        assert callable(getattr(pkg.ScanEngine, name))


def test_kernel_name_on_both_sides_of_every_refusal(L):
    from shared_simd_scan_amd import run_aggregate_kernel

    f = L.mi355_run_aggregate_kernel
    for a in (1, 2, 9, 31, 32):
        for b in (1, 14, 32):
            assert f(a, b) == AGG_KERNEL.encode(), (a, b)
    for bad in (0, 33, 1 << 31):
        assert f(bad, 9) is None and f(9, bad) is None and f(bad, bad) is None, bad
    assert run_aggregate_kernel(9, 17) == AGG_KERNEL and run_aggregate_kernel(32, 1) == AGG_KERNEL
    for bad in ((0, 9), (9, 0), (33, 9), (9, 33), (-1, 9), (9, 1 << 32)):
        with pytest.raises(ValueError):
            run_aggregate_kernel(*bad)


def test_span_slots(L):
    from shared_simd_scan_amd import run_aggregate_span_slots

    slots = [L.mi355_run_aggregate_span_slots(c) for c in range(1, 33)]
    for c, s in zip(range(1, 33), slots):
        assert s >= 4 and s & (s - 1) == 0, (c, s)  # a power of two
        assert run_aggregate_span_slots(c) == s
    assert slots[31] <= 256
    assert all(a >= b for a, b in zip(slots, slots[1:])), slots  # non-increasing in cv
    assert L.mi355_run_aggregate_span_slots(0) == 0 == L.mi355_run_aggregate_span_slots(33)
    for bad in (0, 33, -1, 1 << 32):
        with pytest.raises(ValueError):
            run_aggregate_span_slots(bad)
    # the rule, written down independently: the largest of 1024 .. 128 slots with which the images (whole KiB) and 20-byte slots of the
    # four waves of four blocks stay inside 160 KiB, and 128 where none does; two blocks fit at every width
    for c, s in zip(range(1, 33), slots):
        image = -(-256 * c // 1024) * 1024
        fitting = [k for k in (1024, 512, 256, 128) if 4 * 4 * (2 * image + 20 * k) <= 160 * 1024]
        assert s == (fitting[0] if fitting else 128), (c, s)
        assert 2 * 4 * (2 * image + 20 * s) <= 160 * 1024, (c, s)
    assert slots[0] == 256 and slots[8] == 128


def test_every_runagg_kernel_has_a_case():
    kernels = support.global_kernels_of("runagg")
    assert kernels == {INIT_KERNEL, AGG_KERNEL}, kernels
    support.check_gpu_part_asserts(__file__, "INIT_KERNEL", "AGG_KERNEL")


def test_sources_name_no_store_policy_and_no_context_state():
    assert [os.path.basename(p) for p in support.feature_sources("runagg")] == ["run_aggregate.hip", "run_aggregate.hpp"]
    support.check_sources_read_no_flag_bits("runagg")
    assert support.store_policy_kernels("runagg") == set()
    for path in support.feature_sources("runagg"):
        text = open(path).read()
        for word in ("scan_nt_stores", "rowid_ws_get(", "kernel_scratch", "pool_get("):
            assert word not in text, (path, word)
        assert not re.search(r"\bnts\b", text) and not re.search(r"\bAUX\b", text), path
    mine = {name for name, path, _ in support.hip_functions() if path.startswith("runagg" + os.sep)}
    assert {"mi355_run_aggregate_dev", "mi355_run_aggregate_kernel", "mi355_run_aggregate_span_slots"} <= mine
    for needle in ("rowid_ws_get(", "kernel_scratch", "scan_nt_stores"):
        assert not mine & set(support.entry_points_reaching(needle)), needle


def test_wrappers_pass_what_the_abi_takes(fake):
    import torch

    eng, rec, col = fake
    rec.mi355_run_encode_workspace_words = lambda n: -(-n // CHUNK) + 1 + 1

    def last():
        (name, a), = rec.calls
        rec.calls.clear()
        return name, a

    v1, e1 = col(9, 777), col(10, 55)
    table = eng.run_aggregate(v1, e1)  # defaults: every end counts, no mask, a fresh table, no counter
    name, a = last()
    assert name == "mi355_run_aggregate_dev" and a[1:] == [v1.data.data_ptr(), 9, 777, None, e1.data.data_ptr(), 10, 55, None, table.data_ptr(), None]
    assert tuple(table.shape) == (55, 4) and table.dtype == torch.int64
    mask = torch.zeros(98, dtype=torch.uint8)
    out = torch.zeros((13, 4), dtype=torch.int64)
    unc = torch.zeros(1, dtype=torch.int64)
    got = eng.run_aggregate(v1, e1, runs=13, mask=mask, out=out, uncovered=unc)
    name, a = last()
    assert a[4] == mask.data_ptr() and a[7:] == [13, None, out.data_ptr(), unc.data_ptr()] and got[0] is out and got[1] is unc
    cnt = torch.zeros(1, dtype=torch.int64)
    table, counter = eng.run_aggregate(v1, e1, runs=cnt, uncovered=True)  # the device count: the table has every entry of the ends
    name, a = last()
    assert a[7:9] == [55, cnt.data_ptr()] and tuple(table.shape) == (55, 4) and a[10] == counter.data_ptr() and counter.dtype == torch.int64
    table = eng.run_aggregate(v1, e1, runs=0)
    name, a = last()
    assert a[5] is None and a[7] == 0 and a[9] is None and tuple(table.shape) == (0, 4)
    table = eng.run_aggregate(col(9, 0), e1)  # the empty column travels as NULL, with its mask and its ends
    name, a = last()
    assert a[1] is None and a[3] == 0 and a[4] is None and a[5] is None and a[7] == 55
    for bad in (dict(runs=56), dict(runs=-1)):
        with pytest.raises(ValueError):
            eng.run_aggregate(v1, e1, **bad)
    for bad in (dict(mask=torch.zeros(97, dtype=torch.uint8)), dict(out=torch.zeros((54, 4), dtype=torch.int64)), dict(out=torch.zeros((55, 4), dtype=torch.int32)),
                dict(uncovered=torch.zeros(1, dtype=torch.int32)), dict(runs=torch.zeros(1, dtype=torch.int32))):
        with pytest.raises(AssertionError):
            eng.run_aggregate(v1, e1, **bad)
    assert rec.calls == []
    # sorted_group_aggregate: the whole plan, in order, each call on what the one in front left
    keys, vals = col(32, 777), col(17, 777)
    gkeys, table, groups = eng.sorted_group_aggregate(keys, vals, mask=mask)
    names = [name for name, _ in rec.calls]
    assert names == ["mi355_sort_rows_dev", "mi355_pack_u32_dev", "mi355_run_encode_dev", "mi355_gather_dev", "mi355_pack_u32_dev", "mi355_gather_dev",
                     "mi355_pack_u32_dev", "mi355_run_aggregate_dev"]
    srt, pk, enc, g1, pv, g2, pm, agg = (a for _, a in rec.calls)
    rec.calls.clear()
    assert srt[1:5] == [keys.data.data_ptr(), 777, 32, None] and srt[9] == 777          # every row is sorted: no mask there
    assert pk[1] == srt[8] and pk[2:4] == [777, 32] and enc[1] == pk[4] and enc[2:5] == [777, 32, 10]
    assert g1[1:4] == [vals.data.data_ptr(), 777, 17] and g1[5] == srt[7] and g1[6] == srt[10] and pv[1] == g1[8] and pv[2:4] == [777, 17]
    assert g2[2:4] == [777, 1] and g2[5] == srt[7] and pm[1] == g2[8] and pm[2:4] == [777, 1]
    assert agg[1:4] == [pv[4], 17, 777] and agg[4] == pm[4] and agg[5] == enc[6] and agg[6:9] == [10, 777, enc[8]] and agg[9] == table.data_ptr()
    assert (gkeys.n, gkeys.c) == (777, 32) and gkeys.data.data_ptr() == enc[5] and groups.data_ptr() == enc[8] and tuple(table.shape) == (777, 4)
    eng.sorted_group_aggregate(keys, vals)
    assert [name for name, _ in rec.calls] == names[:5] + names[-1:] and rec.calls[-1][1][4] is None


def test_recipes_are_not_vacuous(L):
    for cv in (4, 9, 32):
        S = L.mi355_run_aggregate_span_slots(cv)
        for extra in (0, 1):
            e = ends_from(span_lengths(S, extra))
            n = 3 * R + 50
            assert int(e[-1]) == n and (np.diff(e.astype(np.int64)) > 0).all()
            assert runs_per_tile(e, len(e), n)[1] == S + extra, (cv, extra)  # tile 1 addresses exactly S, or S + 1, runs
    S9 = L.mi355_run_aggregate_span_slots(9)
    per = runs_per_tile(ends_of(5000, 3), len(ends_of(5000, 3)), 5000)
    assert (per[:2] > S9).all(), per                                         # mean run 3: more than S runs in a tile
    per = runs_per_tile(ends_of(N_BIG, 50), len(ends_of(N_BIG, 50)), N_BIG)
    assert (per > 1).all() and (per <= S9).all()                             # mean run 50: the span tier
    alt = ends_from([1, 2047] * 5)
    assert (runs_per_tile(alt, len(alt), 5 * R) == 2).all()
    assert set(np.diff(np.r_[0, CROSS_ENDS]).tolist()) >= {1} and CROSS_ENDS[-1] == N_CROSS
    for x in (LANE - 1, LANE, LANE + 1, R - 1, R, R + 1, 2 * R, CHUNK - 1, CHUNK, CHUNK + 1):
        assert x in CROSS_ENDS
    z = zero_runs_in_front(ends_of(N_BIG, 50))
    assert len(z) == 64 * len(ends_of(N_BIG, 50)) and (np.diff(z.astype(np.int64)) >= 0).all()
    want, _ = reference(values_of(9, N_BIG), z, len(z), len(z))
    assert (want[np.arange(len(z)) % 64 != 63] == np.array(EMPTY, dtype=np.uint64)).all() and (want[63::64, 1] > 0).all()
    # the masks that empty exactly one run: in the middle of a tile, and one that spans tiles
    e = ends_of(N_BIG, 50)
    j = one_run_inside_a_tile(e)
    assert e[j - 1] // R == (e[j] - 1) // R and e[j - 1] % R > 0 and e[j] % R > 0
    e2, j2 = one_run_across_tiles()
    assert e2[j2 - 1] // R + 2 <= (e2[j2] - 1) // R
    for ee, jj in ((e, j), (e2, j2)):
        m = np.ones(N_BIG, dtype=bool)
        m[ee[jj - 1]: ee[jj]] = False
        want, _ = reference(values_of(9, N_BIG), ee, len(ee), len(ee), m)
        assert tuple(want[jj]) == EMPTY and (want[np.arange(len(ee)) != jj, 1] > 0).all()
    for last in ("below", "at", "above"):
        ee = ends_of(N_BIG, 50, last=last)
        assert {"below": ee[-1] < N_BIG, "at": ee[-1] == N_BIG, "above": ee[-1] > N_BIG}[last]
        assert (reference(values_of(9, N_BIG), ee, len(ee), len(ee))[1] > 0) == (last == "below")
    keys, values, mask = sparse_group_keys()
    u, inv = np.unique(keys, return_inverse=True)
    assert len(u) == 300 and int(u[-1]) == top(32) and len(keys) == 20000 and not mask[inv == 123].any() and mask[inv != 123].any()
    (a0, e0), (a1, e1) = ((x, np.nonzero(np.r_[x[1:] != x[:-1], True])[0] + 1) for x, _ in capture_versions())
    assert len(e1) * 4 < len(e0), "a stale run count could pass"


def one_run_inside_a_tile(e):
    """a run of at least 3 rows that begins and ends inside one tile, away from its edges"""
    for j in range(len(e) // 2, len(e)):
        if e[j] - e[j - 1] >= 3 and e[j - 1] // R == (e[j] - 1) // R and e[j - 1] % R > 0 and e[j] % R > 0:
            return j
    raise AssertionError("no such run")


def one_run_across_tiles():
    """mean-50 runs with one run of 2 tiles and a bit spliced in -> (ends, its index)"""
    e = ends_of(N_BIG, 50).astype(np.int64)
    lo, hi = 3 * R + 700, 5 * R + 900
    kept = np.r_[e[e <= lo], hi, e[e > hi]]
    j = int(np.nonzero(kept == hi)[0][0])
    return kept.astype(np.uint32), j


@functools.lru_cache(maxsize=None)
def capture_versions():
    """two key columns of other runs and another number of runs, each with its value column"""
    n = 3 * CHUNK + 1237
    out = []
    for mean, seed in ((12, 11), (300, 12)):
        t = np.random.default_rng([mean, seed, 59]).random(n) < 1.0 / mean
        keys = (np.cumsum(np.r_[0, t[:-1]]) % 512).astype(np.uint32)
        out.append(frozen(keys, values_of(11, n, seed)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

class Agg:
    """one run_aggregate call through the C ABI: column and ends in hostile surroundings, the mask with 0xFF behind it, the table
    (exactly 32 * runs bytes) and the counter Guarded"""

    def __init__(self, O, eng, x, cv, ends, ce, runs=None, runs_dev=None, mask=None, counter=True, col=None):
        import torch

        self.O, self.eng, self.x, self.cv, self.ends, self.ce = O, eng, x, cv, ends, ce
        self.n = len(x)
        self.runs = len(ends) if runs is None else runs
        self.runs_dev = None if runs_dev is None else torch.tensor([runs_dev], dtype=torch.int64, device="cuda")
        self.R = self.runs if runs_dev is None else min(self.runs, runs_dev)
        self.mask = mask
        self.col = col if col is not None else (hostile_pack(O, x, cv) if self.n else None)
        self.et = hostile_pack(O, ends, ce) if len(ends) else None
        self.mt = hostile_bitmap(mask)[0] if mask is not None and self.n else None
        self.out = Guarded(32 * self.runs)
        self.counter = Guarded(8, back=64, front=64) if counter else None

    def call(self, L, **kw):
        a = dict(values=self.col.data_ptr() if self.col is not None else None, cv=self.cv, n=self.n, mask=self.mt.data_ptr() if self.mt is not None else None,
                 ends=self.et.data_ptr() if self.et is not None else None, ce=self.ce, runs=self.runs,
                 runs_dev=self.runs_dev.data_ptr() if self.runs_dev is not None else None, out=self.out.ptr if self.runs else None,
                 counter=self.counter.ptr if self.counter else None)
        a.update(kw)
        rc = L.mi355_run_aggregate_dev(self.eng._ctx, a["values"], a["cv"], a["n"], a["mask"], a["ends"], a["ce"], a["runs"], a["runs_dev"], a["out"], a["counter"])
        self.eng.synchronize()
        return rc

    def refill(self):
        self.out.t.fill_(SENTINEL)
        if self.counter:
            self.counter.t.fill_(SENTINEL)

    def fetch_checked(self, L, what=""):
        """the call on refilled outputs -> the table's bytes (both guards intact) after the launch record was held to the contract"""
        self.refill()
        assert self.call(L) == 0, (what, L.mi355_last_error())
        rec = record(L, self.eng)
        assert [base_name(k[0]) for k in rec] == ([INIT_KERNEL, AGG_KERNEL] if self.n else [INIT_KERNEL]), (what, rec)
        self.grid = rec[-1][1]
        return self.out.fetch()

    def run(self, L, what=""):
        """-> the counted rows behind the last run, after the table was compared with numpy's"""
        have = self.fetch_checked(L, what).view(np.uint64).reshape(self.runs, 4)
        want, uncovered = reference(self.x, self.ends, self.R, self.runs, self.mask)
        bad = np.nonzero((have != want).any(axis=1))[0]
        assert bad.size == 0, (what, "entry", int(bad[0]), "of", self.runs, "have", have[bad[0]].tolist(), "want", want[bad[0]].tolist(), "wrong", int(bad.size))
        if self.counter:
            assert int(self.counter.fetch().view(np.int64)[0]) == uncovered, what
        return uncovered


def one_block(eng):
    """a context manager: one block of four waves, so that a wave walks several chunks and carries across them"""
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
    a = Agg(O, eng, values_of(9, n), 9, ends_of(n, 50), 17)
    assert a.run(L) == 0
    assert base_name(record(L, eng)[0][0]) == INIT_KERNEL and (n == 0 or base_name(record(L, eng)[-1][0]) == AGG_KERNEL)
    rng = np.random.default_rng(n)
    Agg(O, eng, values_of(9, n), 9, ends_of(n, 50), 17, mask=rng.random(n) < 0.5).run(L, what="masked")


@gpu
@pytest.mark.parametrize("cv", range(1, 33))
def test_every_value_width(L, O, eng, cv):
    n = R + 33
    e = ends_of(n, 20, seed=cv)
    x = values_of(cv, n, seed=cv).copy()
    lengths = np.diff(np.r_[0, e.astype(np.int64)])
    j = int(np.argmax(lengths))
    assert lengths[j] > 2
    x[e[j] - lengths[j]: e[j]] = top(cv)  # at 32 bits: a sum that needs 64
    a = Agg(O, eng, x, cv, e, 12)
    a.run(L)
    if cv == 32:
        assert int(reference(x, e, len(e), len(e))[0][j, 0]) == int(lengths[j]) * top(32) > top(32)
    Agg(O, eng, x, cv, ends_from([n]), 12).run(L, what="one run")
    Agg(O, eng, x, cv, ends_of(n, 2, seed=cv), 12).run(L, what="dense")


@gpu
@pytest.mark.parametrize("cv,ce", WIDTH_PAIRS)
def test_width_pairs(L, O, eng, cv, ce):
    n = min(N_BIG, top(ce))
    Agg(O, eng, values_of(cv, n), cv, ends_of(n, 50), ce).run(L)
    Agg(O, eng, values_of(cv, n), cv, ends_of(n, 3), ce, mask=np.random.default_rng(ce).random(n) < 0.5).run(L, what="dense, masked")


@gpu
def test_crossings(L, O, eng):
    x = values_of(9, N_CROSS)
    Agg(O, eng, x, 9, np.array(CROSS_ENDS, dtype=np.uint32), 17).run(L, what="ends at lane, tile and chunk edges")
    Agg(O, eng, x, 9, ends_from([N_CROSS]), 17).run(L, what="one run over the whole column")
    n = 5 * R + 7
    Agg(O, eng, values_of(9, n), 9, ends_from([R, 3 * R, R + 7]), 17).run(L, what="one run covers tiles 1..3 exactly")
    Agg(O, eng, values_of(9, n), 9, ends_from([R - 1, 3 * R + 2, R + 6]), 17).run(L, what="one run covers tiles 1..3 and a row on either side")


@gpu
@pytest.mark.parametrize("cv", [4, 9, 32])
def test_both_tiers_and_their_boundary(L, O, eng, cv):
    S = L.mi355_run_aggregate_span_slots(cv)
    n = 3 * R + 50
    for extra in (0, 1):
        e = ends_from(span_lengths(S, extra))
        Agg(O, eng, values_of(cv, n), cv, e, 17).run(L, what=f"a tile with S + {extra} runs")
        Agg(O, eng, values_of(cv, n), cv, e, 17, mask=np.random.default_rng(extra).random(n) < 0.3).run(L, what=f"a tile with S + {extra} runs, masked")
    Agg(O, eng, values_of(cv, 5000), cv, ends_of(5000, 3), 13).run(L, what="mean run 3")
    Agg(O, eng, values_of(cv, 5 * R), cv, ends_from([1, 2047] * 5), 14).run(L, what="runs of 1 and 2047 rows")
    Agg(O, eng, values_of(cv, 5 * R), cv, ends_from([2047, 1] * 5), 14).run(L, what="runs of 2047 rows and 1")


@gpu
def test_zero_length_runs(L, O, eng):
    x = values_of(9, N_BIG)
    for mean in (50, 3, 3000):
        z = zero_runs_in_front(ends_of(N_BIG, mean))
        a = Agg(O, eng, x, 9, z, 17)
        a.run(L, what=f"63 equal ends in front of every run of about {mean} rows")
        have = a.out.fetch().view(np.uint64).reshape(-1, 4)
        assert (have[np.arange(len(z)) % 64 != 63] == np.array(EMPTY, dtype=np.uint64)).all()
    e = ends_from([R - 5, 5, 0, 0, 0, 7, R - 7, 0, 0, R, 0, N_BIG - 4 * R])
    Agg(O, eng, x, 9, e, 17).run(L, what="equal ends at a tile edge")


@gpu
def test_masks(L, O, eng):
    x = values_of(9, N_BIG)
    rng = np.random.default_rng(3)
    for mean in (50, 3, 3000):
        Agg(O, eng, x, 9, ends_of(N_BIG, mean), 17, mask=rng.random(N_BIG) < 0.5).run(L, what=f"density 1/2, runs of about {mean}")
    a = Agg(O, eng, x, 9, ends_of(N_BIG, 50), 17, mask=np.zeros(N_BIG, dtype=bool))
    assert a.run(L, what="an all-zero mask") == 0
    assert (a.out.fetch().view(np.uint64).reshape(-1, 4) == np.array(EMPTY, dtype=np.uint64)).all()
    e = ends_of(N_BIG, 50)
    j = one_run_inside_a_tile(e)
    e2, j2 = one_run_across_tiles()
    for ee, jj, what in ((e, j, "empties one run inside a tile"), (e2, j2, "empties one run that spans tiles")):
        m = np.ones(N_BIG, dtype=bool)
        m[ee[jj - 1]: ee[jj]] = False
        a = Agg(O, eng, x, 9, ee, 17, mask=m)
        a.run(L, what=what)
        assert tuple(int(v) for v in a.out.fetch().view(np.uint64).reshape(-1, 4)[jj]) == EMPTY


@gpu
def test_run_counts(L, O, eng):
    x = values_of(9, N_BIG)
    e = ends_of(N_BIG, 50)
    nt = len(e)
    assert Agg(O, eng, x, 9, e, 17, runs=nt, runs_dev=nt // 2).run(L, what="runs_dev below runs") == N_BIG - int(e[nt // 2 - 1])
    assert Agg(O, eng, x, 9, e, 17, runs=nt // 2, runs_dev=nt + 1000).run(L, what="runs_dev above runs") == N_BIG - int(e[nt // 2 - 1])
    assert Agg(O, eng, x, 9, e, 17, runs=nt).run(L, what="runs_dev NULL") == 0
    assert Agg(O, eng, x, 9, e, 17, runs=nt, runs_dev=0).run(L, what="R = 0") == N_BIG
    assert Agg(O, eng, x, 9, e[:0], 17, runs=0).run(L, what="runs = 0, no table") == N_BIG
    assert Agg(O, eng, x, 9, e, 17, runs=1).run(L, what="R = 1") == N_BIG - int(e[0])
    m = np.random.default_rng(4).random(N_BIG) < 0.5
    assert Agg(O, eng, x, 9, e, 17, runs=nt, runs_dev=nt // 2, mask=m).run(L, what="masked rows behind R are not counted") == int(m[int(e[nt // 2 - 1]):].sum())
    for last in ("below", "at", "above"):
        ee = ends_of(N_BIG, 50, last=last)
        assert (Agg(O, eng, x, 9, ee, 32 if last == "above" else 17).run(L, what=last) > 0) == (last == "below")
    Agg(O, eng, x, 9, e, 17, counter=False).run(L, what="no counter")
    # n = 0 with NULL inputs: every entry is empty, the launch record shows the init kernel alone
    a = Agg(O, eng, x[:0], 9, e, 17)
    assert a.run(L, what="n = 0") == 0
    a.refill()
    assert a.call(L, values=None, mask=None, ends=None) == 0
    assert [base_name(k[0]) for k in record(L, eng)] == [INIT_KERNEL]
    assert (a.out.fetch().view(np.uint64).reshape(-1, 4) == np.array(EMPTY, dtype=np.uint64)).all() and int(a.counter.fetch().view(np.int64)[0]) == 0


@gpu
def test_one_block_grid_carries_across_chunks(L, O, eng):
    x = values_of(9, N_ONE_BLOCK)
    with one_block(eng):
        for mean in (64, 3000, 40000, 3):
            a = Agg(O, eng, x, 9, ends_of(N_ONE_BLOCK, mean), 18)
            a.run(L, what=f"one block, runs of about {mean}")
            assert a.grid == 1
        Agg(O, eng, x, 9, ends_from([N_ONE_BLOCK]), 18).run(L, what="one block, one run")
    a = Agg(O, eng, x, 9, ends_of(N_ONE_BLOCK, 64), 18)
    a.run(L)
    assert a.grid > 1


@gpu
def test_row_range_view(L, O, eng):
    """rows [lead, lead + n) of a longer column: the rows in front are all ones, the rows behind all zero -- either would change a
    run's minimum or maximum"""
    for n in (2 * R + 504, R, 3 * LANE, CHUNK + 77):
        lead = 2 * R + 128
        x = (values_of(9, n, seed=5) % 510 + 1).astype(np.uint32)
        whole = np.concatenate([np.full(lead, 511, dtype=np.uint32), x, np.zeros(4096, dtype=np.uint32)])
        assert (lead * 9) % 128 == 0 and x.min() > 0 and x.max() < 511
        col = hostile_pack(O, whole, 9)[lead * 9 // 8:]
        assert col.data_ptr() % 16 == 0
        Agg(O, eng, x, 9, ends_of(n, 50, last="above"), 32, col=col).run(L, what="view")


@gpu
def test_unsorted_ends(L, O, eng):
    """ends in no order: the call returns OK and both guards are intact -- no stronger claim"""
    rng = np.random.default_rng(77)
    x = values_of(17, N_BIG)
    for nt, R_ in ((500, 400), (40000, 40000), (3, 2)):
        ends = rng.integers(0, N_BIG + 1000, nt, dtype=np.uint64).astype(np.uint32)
        a = Agg(O, eng, x, 17, ends, 32, runs=nt, runs_dev=R_)
        a.fetch_checked(L, what="unsorted")
        a.counter.fetch()


@gpu
def test_two_calls_give_the_same_bytes(L, O, eng):
    n = 40000
    for mean in (64, 3):
        a = Agg(O, eng, values_of(17, n), 17, ends_of(n, mean), 16, mask=np.random.default_rng(9).random(n) < 0.7)
        first = a.fetch_checked(L).copy()
        assert (a.fetch_checked(L) == first).all()
        a.run(L)


@gpu
def test_errors_launch_nothing(L, O, eng):
    n = R + 77
    x, e = values_of(9, n), ends_of(n, 50)
    m = np.random.default_rng(1).random(n) < 0.5
    a = Agg(O, eng, x, 9, e, 12, runs_dev=len(e), mask=m)
    a.run(L)
    valid = record(L, eng)
    big = Guarded(65536)  # stands for an input and the output at once
    col, et, mt, out = a.col.data_ptr(), a.et.data_ptr(), a.mt.data_ptr(), a.out.ptr.value
    errors = (("cv = 0", dict(cv=0), b"width"), ("cv = 33", dict(cv=33), b"width"), ("ce = 0", dict(ce=0), b"width"), ("ce = 33", dict(ce=33), b"width"),
              ("runs = 2^32", dict(runs=1 << 32), b"runs"), ("null output", dict(out=None), b"out_dev"), ("output at +4", dict(out=out + 4), b"out_dev"),
              ("counter at +4", dict(counter=a.counter.ptr.value + 4), b"uncovered_dev"), ("runs_dev at +4", dict(runs_dev=a.runs_dev.data_ptr() + 4), b"runs_dev"),
              ("column at +8", dict(values=col + 8), b"values_dev"), ("mask at +2", dict(mask=mt + 2), b"mask_dev"), ("ends at +1", dict(ends=et + 1), b"ends_dev"),
              ("null column", dict(values=None), b"values_dev"), ("null ends", dict(ends=None), b"ends_dev"),
              ("output is the column", dict(values=big.ptr.value, out=big.ptr.value), b"out_dev overlaps values_dev"),
              ("output starts in the column's last byte", dict(values=big.ptr.value, out=big.ptr.value + (n * 9 - 1) // 64 * 8), b"out_dev overlaps values_dev"),
              ("mask starts inside the output", dict(mask=big.ptr.value + 32 * len(e) - 4, out=big.ptr.value), b"out_dev overlaps mask_dev"),
              ("ends start inside the output", dict(ends=big.ptr.value + 32, out=big.ptr.value), b"out_dev overlaps ends_dev"),
              ("runs_dev is the output's last word", dict(runs_dev=big.ptr.value + 32 * len(e) - 8, out=big.ptr.value), b"out_dev overlaps runs_dev"),
              ("counter is the output's first word", dict(counter=big.ptr.value, out=big.ptr.value), b"out_dev overlaps uncovered_dev"))
    buffers = (a.out, a.counter, big)
    for what, kw, word in errors:
        for g in buffers:
            g.t.fill_(SENTINEL)
        assert a.call(L, **kw) == E_INVALID, what
        assert word in L.mi355_last_error(), (what, L.mi355_last_error())
        assert record(L, eng) == [], what
        for g in buffers:
            assert (g.fetch() == SENTINEL).all(), what
    # the rules' other side: a null output with runs = 0, null ends with runs = 0, null inputs with n = 0
    a.refill()
    assert a.call(L, runs=0, out=None, ends=None) == 0 and int(a.counter.fetch().view(np.int64)[0]) == int(m.sum())
    assert a.call(L, n=0, values=None, mask=None, ends=None) == 0
    a.run(L)
    assert record(L, eng) == valid


# ---- chains through existing calls ----

def column(O, x, c):
    from shared_simd_scan_amd.engine import PackedColumn

    return PackedColumn(hostile_pack(O, x, c), len(x), c)


@gpu
def test_run_encode_then_run_aggregate_and_the_five_call_chain(L, O, eng):
    """the runs of a key column, on the device: run_encode's ends and its device count feed run_aggregate; where the running sum
    fits 32 bits, lookup(arith(ends - 1), running_sum(y)) -> delta gives the same sums"""
    from shared_simd_scan_amd.engine import PackedColumn

    n = N_BIG
    t = np.random.default_rng(8).random(n) < 1 / 25
    keys = (np.cumsum(np.r_[0, t[:-1]]) % 512).astype(np.uint32)
    y = values_of(9, n, seed=9)
    ends_np = (np.nonzero(np.r_[keys[1:] != keys[:-1], True])[0] + 1).astype(np.uint32)
    r = len(ends_np)
    values, ends, count = eng.run_encode(column(O, keys, 9))
    table, unc = eng.run_aggregate(column(O, y, 9), PackedColumn(ends, n, 17), runs=count, uncovered=True)
    assert [base_name(k[0]) for k in record(L, eng)] == [INIT_KERNEL, AGG_KERNEL]
    eng.synchronize()
    want, _ = reference(y, ends_np, r, n)
    assert int(count.item()) == r and int(unc.item()) == 0 and tuple(table.shape) == (n, 4)
    assert (table.cpu().numpy().view(np.uint64) == want).all()  # the entries behind the count are empty
    assert int(y.sum()) < 1 << 32
    ecol = PackedColumn(ends, r, 17)
    sums, _ = eng.running_sum(column(O, y, 9), co=32)
    per_run = eng.delta(eng.lookup(eng.arith("linear", ecol, ecol, a=1, b=0, k=-1, co=17), sums), first=0, co=32)
    eng.synchronize()
    chain = O.decompress(np.concatenate([per_run.data.cpu().numpy(), np.zeros(4096, dtype=np.uint8)]), r, 32).view(np.uint32)[:r]
    assert (chain.astype(np.uint64) == want[:r, 0]).all()


@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["every row", "masked"])
def test_sorted_group_aggregate(L, O, eng, masked):
    """GROUP BY a sparse 32-bit key by sorting: equals np.unique + add.at / minimum.at / maximum.at, and dense_codes -> group_aggregate"""
    import torch

    keys, values, mask = sparse_group_keys()
    n = len(keys)
    sel = mask if masked else None
    mt = torch.from_numpy(support.packbits(mask)).cuda() if masked else None
    kcol, vcol = column(O, keys, 32), column(O, values, 17)
    gkeys, table, groups = eng.sorted_group_aggregate(kcol, vcol, mask=mt)
    assert [base_name(k[0]) for k in record(L, eng)] == [INIT_KERNEL, AGG_KERNEL]
    eng.synchronize()
    u, inverse = np.unique(keys, return_inverse=True)
    d = len(u)
    want = support.grouped(inverse, values, d, sel)
    assert int(groups.item()) == d == 300 and (gkeys.n, gkeys.c) == (n, 32) and tuple(table.shape) == (n, 4)
    got_keys = O.decompress(np.concatenate([gkeys.data.cpu().numpy(), np.zeros(4096, dtype=np.uint8)]), d, 32).view(np.uint32)[:d]
    assert (got_keys == u).all()
    have = table.cpu().numpy().view(np.uint64)
    assert (have[:d] == want).all() and (have[d:] == np.array(EMPTY, dtype=np.uint64)).all()
    if masked:
        assert tuple(int(v) for v in have[123]) == EMPTY  # the group the mask empties is there, with count 0
    codes, distinct, count = eng.dense_codes(kcol)
    dense = eng.group_aggregate(codes, vcol, mask=mt)
    eng.synchronize()
    assert codes.c == 9 and (dense.cpu().numpy().view(np.uint64)[:d] == have[:d]).all()


@gpu
def test_graph_capture_and_replay(O):
    """run_encode -> run_aggregate in one graph, with no warm-up of either; replays follow the key column overwritten in place --
    another number of runs, which run_aggregate reads from the device word run_encode left"""
    import torch

    versions = capture_versions()
    n, c, cv, ce = len(versions[0][0]), 9, 11, 16
    words = -(-n // CHUNK) + 1 + 1

    def steps(eng):
        from shared_simd_scan_amd.engine import PackedColumn

        stage = [(plain_pack(O, k, c), plain_pack(O, y, cv)) for k, y in versions]
        kcol, ycol = PackedColumn(torch.empty_like(stage[0][0]), n, c), PackedColumn(torch.empty_like(stage[0][1]), n, cv)
        ends, count, ws, table, unc = Guarded((n * ce + 31) // 32 * 4), Guarded(8, back=64, front=64), Guarded(8 * words), Guarded(32 * n), Guarded(8, back=64, front=64)
        guarded = (ends, count, ws, table, unc)
        views = [g.t[g.front: g.front + g.nbytes] for g in guarded]

        def load(v):
            kcol.data.copy_(stage[v][0])
            ycol.data.copy_(stage[v][1])
            for g in guarded:
                g.t.fill_(SENTINEL)

        def run():
            eng.run_encode(kcol, ends_width=ce, values=False, ends=views[0], count=views[1].view(torch.int64), workspace=views[2].view(torch.int64))
            eng.run_aggregate(ycol, PackedColumn(views[0], n, ce), runs=views[1].view(torch.int64), out=views[3].view(torch.int64).view(n, 4),
                              uncovered=views[4].view(torch.int64))

        def check(v, what):
            keys, y = versions[v]
            e = (np.nonzero(np.r_[keys[1:] != keys[:-1], True])[0] + 1).astype(np.uint32)
            want, _ = reference(y, e, len(e), n)
            assert int(count.fetch().view(np.int64)[0]) == len(e), what
            assert (table.fetch().view(np.uint64).reshape(n, 4) == want).all(), what
            assert int(unc.fetch().view(np.int64)[0]) == 0, what
            ends.fetch(), ws.fetch()

        def untouched():
            for g in guarded:
                assert (g.fetch() == SENTINEL).all()

        def warmed(launched):
            assert [base_name(x[0]) for x in launched] == [INIT_KERNEL, AGG_KERNEL]

        return capture.Steps(load, run, check, untouched, warmed)

    capture.capture_replay(steps, (0, 1, 0))
