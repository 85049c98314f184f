"""Grouped aggregates for keys beyond 12 bits (include/mi355_groupby_wide.h, ScanEngine.group_aggregate_wide): per key g of a
dense domain [0, groups), groups <= 2^26, the sum, count, min and max of the value column, optionally under a bitmap; counted
rows whose key is >= groups reach no group and are counted in `dropped`.

CPU: the header is plain C99 and declares exactly what _capi.HEADERS binds for it and the library exports, no earlier header
or list knows the names; it carries its graph-capture verdict; group_aggregate_wide hands the C ABI what it should (through a
recording stand-in for the library) and refuses a wrong `out` and differing row counts; without a device the entry point fails
with a message; every __global__ under csrc/groupby_wide/ is named by the launch record of a GPU case of this file; no source
there reads a switch bit; mi355_group_wide_front_slots is the rule of the header, restated here, at all 32 x 32 pairs of widths;
the data recipes are not vacuous.

GPU (-m gpu): every expectation is numpy arithmetic on the keys and values the test generated -- np.bincount, np.add.at on
uint64, np.minimum.at / np.maximum.at over the rows with key < groups -- packed with the oracle's packer on the way in; nothing
is derived from engine output.  The output and the counter sit inside 0xEE guard bytes (support.Guarded) that must
stay untouched; inputs and mask must be unchanged after the call.  A tile is 2048 rows (32 rows per lane), so the sizes below
are the smallest that reach one lane, one partial tile, a tile less one row, one full tile, a full tile plus one row, and many
tiles with a ragged tail.

A block's LDS front has S = 4096, 2048 or 1024 slots, slot = key & (S - 1): a recipe with more than 4096 distinct in-domain keys
in ONE block must send some keys down the miss path (global atomics) whatever S is.  The one-block cases hold that many wherever
`groups` admits it; at groups = 4097 with 32-bit columns (S = 1024) they hold more than S.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import capture
import support
from support import E_INVALID, SENTINEL, Guarded, L, eng, fake, packbits, record, upload  # noqa: F401  (L, eng, fake: fixtures)

HEADER = "mi355_groupby_wide.h"
U64_MAX = (1 << 64) - 1
MAX_GROUPS = support.header_macro(HEADER, "MI355_GROUP_WIDE_MAX_GROUPS")  # the header's limit bounds every recipe below
CU_LDS = 160 * 1024

# the kernels of csrc/groupby_wide/, as the launch record names them: the GPU cases below assert these labels
INIT_KERNEL = "group_aggregate_wide_init_kernel"
AGG_KERNEL = "group_aggregate_wide_kernel"

R = 2048  # rows per tile: 64 lanes x 32 rows
N_BIG = 9 * 8192 + 1237  # 74965: 36 tiles of 2048 rows and a ragged one
N_RAGGED = 2048 + 509
N_HOSTILE = 2048 * 3 + 509  # not a multiple of 8
SIZES = [1, 13, 2047, 2048, 2049, N_BIG]
SIZE_SHAPES = [(13, 9, 5000), (18, 17, (1 << 18) - 3), (32, 32, 4097), (5, 12, 20), (1, 1, 1)]  # (ck, cv, groups)
KEY_WIDTHS = list(range(1, 33))
VALUE_WIDTHS = [1, 9, 17, 32]
TIER_WIDTHS = [1, 9, 12]
MASK_SHAPES = [(13, 9, 5000), (32, 32, 4097)]
HOSTILE_SHAPES = [(13, 9, 5000), (32, 32, 4097)]
SAME_SHAPES = [(9, 9, 500), (17, 17, (1 << 17) - 3)]
ERROR_SHAPE = (13, 9, 5000)
ERROR_N = 4096 + 77
CAPTURE_SHAPE = (14, 12, 9000)
FRONT_GROUPS = 12286  # test_front_and_miss_path: 14-bit keys, three of them 4096 apart
DROP_GROUPS = 5000    # test_dropped_rows: 32-bit keys

gpu = pytest.mark.gpu


def pid(p):
    return "-".join(str(x) for x in p)


def width_groups(ck):
    """test_every_key_width: every group of the narrowest columns, else a domain that ends 3 short of a power of two"""
    return 1 << ck if ck <= 2 else min((1 << ck) - 3, 12286)


def image(c):
    """an image of a tile in LDS: 64 lanes x 32 rows x c bits, in whole KiB"""
    return (64 * 32 * c // 8 + 1023) // 1024 * 1024


def tiles_lds(ck, cv):
    return 4 * (2 * image(ck) + 2 * image(cv))


def front_slots(ck, cv):
    """the rule of the header, restated: the largest of 4096 / 2048 / 1024 slots of 24 bytes that fit a CU's LDS with the tiles"""
    for s in (4096, 2048):
        if 24 * s + tiles_lds(ck, cv) + 16 <= CU_LDS:
            return s
    return 1024


def populated(groups):
    return np.asarray([g for g in range(groups) if g % 7 != 5], dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def data(ck, cv, groups, n, salt=0):
    """the data recipe -> (keys, values) as read-only uint32 arrays.  Keys are uniform over the groups g < groups with
    g % 7 != 5, so empty groups exist whenever groups > 5; where the key width has room (2^ck > groups) one row in sixteen holds
    a key >= groups instead, uniform over [groups, 2^ck) -- a dropped row; values are uniform over [0, 2^cv); rows 0..7 are
    corner rows: value 0 (and 1) in the first populated group, 2^cv - 1 (and 2^cv - 2) in the last.  At cv = 32 every row of
    the last populated group has bit 31 set: that group's min and max are >= 2^31 and its sum is beyond 32 bits, so a signed
    min / max or a 32-bit partial sum cannot pass."""
    rng = np.random.default_rng([ck, cv, groups, salt])
    pop = populated(groups)
    vmax = (1 << cv) - 1
    keys = pop[rng.integers(0, len(pop), n)]
    if (1 << ck) > groups:
        out = rng.random(n) < 1 / 16
        keys[out] = rng.integers(groups, 1 << ck, int(out.sum()), dtype=np.uint64).astype(np.uint32)
    vals = rng.integers(0, vmax + 1, n, dtype=np.uint64).astype(np.uint32)
    first, last = int(pop[0]), int(pop[-1])
    corners = [(first, 0), (last, vmax), (first, 0), (last, vmax), (first, min(1, vmax)), (last, max(vmax - 1, 0)), (first, 0), (last, vmax)]
    for i, (g, v) in enumerate(corners[:n]):
        keys[i], vals[i] = g, v
    if cv == 32:
        vals[keys == last] |= np.uint32(1 << 31)
    for a in (keys, vals):
        a.setflags(write=False)
    return keys, vals


def empty_result(groups):
    want = np.zeros((groups, 4), dtype=np.uint64)
    want[:, 2] = U64_MAX
    return want


def expect(keys, vals, groups, mask_bits=None):
    """-> (uint64[groups, 4] = (sum, count, min, max) per group, the number of counted rows with key >= groups): numpy on the
    generated rows"""
    if mask_bits is not None:
        keys, vals = keys[mask_bits], vals[mask_bits]
    inside = keys.astype(np.int64) < groups
    k = keys[inside].astype(np.int64)
    v = vals[inside].astype(np.uint64)
    want = empty_result(groups)
    np.add.at(want[:, 0], k, v)  # uint64: exact modulo 2^64
    want[:, 1] = np.bincount(k, minlength=groups).astype(np.uint64)
    np.minimum.at(want[:, 2], k, v)
    np.maximum.at(want[:, 3], k, v)
    return want, int((~inside).sum())


@functools.lru_cache(maxsize=None)
def front_data(which):
    """test_front_and_miss_path -> (ck, cv, keys, values)
    "collide": three keys h, h + 4096, h + 8192 share a slot at every S; each holds a quarter of the rows, all of value
               0xffffffff at cv = 32.  At most one of them can own the slot, so at least two sums >= 2^44 travel through global
               atomics row by row.  The last quarter is uniform over the populated groups.
    "hot":     one key holds half of the rows, the other half is uniform over the (about 10 500) populated groups"""
    n, groups, ck = N_BIG, FRONT_GROUPS, 14
    rng = np.random.default_rng([77, len(which)])
    pop = populated(groups)
    keys = pop[rng.integers(0, len(pop), n)]
    if which == "collide":
        cv, h = 32, 75
        vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        part = rng.integers(0, 4, n)
        for j in range(3):
            keys[part == j] = h + 4096 * j
            vals[part == j] = 0xFFFFFFFF
    else:
        cv = 17
        vals = rng.integers(0, 1 << cv, n, dtype=np.uint64).astype(np.uint32)
        keys[rng.random(n) < 0.5] = 3001
    for a in (keys, vals):
        a.setflags(write=False)
    return ck, cv, keys, vals


@functools.lru_cache(maxsize=None)
def dropped_data():
    """test_dropped_rows -> (keys, values, corner rows): 32-bit keys over DROP_GROUPS groups; the corner keys groups - 1, groups,
    2^26, 2^28 and 0xffffffff stand in the first tile, a middle tile and the ragged tail"""
    n, groups = N_BIG, DROP_GROUPS
    rng = np.random.default_rng(505)
    pop = populated(groups)
    keys = pop[rng.integers(0, len(pop), n)]
    vals = rng.integers(0, 1 << 17, n, dtype=np.uint64).astype(np.uint32)
    corner_keys = [groups - 1, groups, 1 << 26, 1 << 28, 0xFFFFFFFF]
    rows = []
    for first in (3, 17 * R + 1000, n - len(corner_keys)):
        for j, g in enumerate(corner_keys):
            keys[first + j] = g
            rows.append(first + j)
    for a in (keys, vals):
        a.setflags(write=False)
    return keys, vals, rows


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------

def test_wide_header_is_plain_c99():
    support.check_header_is_plain_c99(HEADER)


def test_wide_header_declares_what_python_binds(L):
    names, sigs = support.check_header_binds(L, HEADER)
    assert names == ["mi355_group_aggregate_wide_dev", "mi355_group_wide_front_slots"]
    sig = sigs["mi355_group_aggregate_wide_dev"]
    assert sig[2] is C.c_uint and sig[4] is C.c_uint and sig[5] is C.c_uint64 and sig[7] is C.c_uint64 and len(sig) == 10
    assert sigs["mi355_group_wide_front_slots"] == [C.c_uint, C.c_uint] and L.mi355_group_wide_front_slots.restype is C.c_uint32
    text = support.header_text(HEADER)
    assert '#include "mi355_scan.h"' in text and text.count("#include") == 1
    assert MAX_GROUPS == 1 << 26
    # the narrow tier's header still has its one entry point
    assert support.declared("mi355_groupby.h") == ["mi355_group_aggregate_dev"]


def test_wide_names_are_exported():
    import shared_simd_scan_amd as pkg

    assert "group_wide_front_slots" in pkg.__all__ and callable(pkg.group_wide_front_slots)
    assert callable(pkg.ScanEngine.group_aggregate_wide)
    assert "group_aggregate_wide" in pkg.ScanEngine.group_aggregate.__doc__


def test_wide_header_carries_its_capture_verdict():
    support.check_capture_verdict(HEADER, r"no memset node", r"read at every replay")


def test_group_aggregate_wide_wrapper_passes_what_the_abi_takes(fake):
    import torch

    eng, rec, col = fake
    keys, vals = col(18, 777), col(17, 777)
    mask = torch.zeros(128, dtype=torch.uint8)
    out = torch.zeros((5000, 4), dtype=torch.int64)
    cnt = torch.zeros(1, dtype=torch.int64)
    got = eng.group_aggregate_wide(keys, vals, 5000, mask=mask, out=out, dropped=cnt)
    (name, a), = rec.calls
    assert name == "mi355_group_aggregate_wide_dev" and got is out
    assert a[1:] == [keys.data.data_ptr(), 18, vals.data.data_ptr(), 17, 777, mask.data_ptr(), 5000, out.data_ptr(), cnt.data_ptr()]
    rec.calls.clear()
    got = eng.group_aggregate_wide(keys, vals, (1 << 18) - 3)  # defaults: no mask, a fresh result, no counter
    (name, a), = rec.calls
    assert a[1:6] == [keys.data.data_ptr(), 18, vals.data.data_ptr(), 17, 777] and a[6] is None and a[7] == (1 << 18) - 3 and a[9] is None
    assert tuple(got.shape) == ((1 << 18) - 3, 4) and got.dtype == torch.int64 and a[8] == got.data_ptr()
    rec.calls.clear()
    eng.group_aggregate_wide(col(32, 5), col(32, 5), 1)
    eng.group_aggregate_wide(col(1, 0), col(1, 0), 2)  # an empty column: no column pointer is handed on
    assert [c[1][2] for c in rec.calls] == [32, 1] and rec.calls[1][1][1] is None and rec.calls[1][1][3] is None and rec.calls[1][1][5] == 0
    rec.calls.clear()


def test_group_aggregate_wide_wrapper_refuses_what_does_not_fit(fake):
    import torch

    eng, rec, col = fake
    keys, vals = col(18, 777), col(17, 777)
    with pytest.raises(AssertionError):
        eng.group_aggregate_wide(keys, col(17, 778), 5000)  # row counts differ
    with pytest.raises(AssertionError):
        eng.group_aggregate_wide(keys, vals, 5000, out=torch.zeros((4999, 4), dtype=torch.int64))
    with pytest.raises(AssertionError):
        eng.group_aggregate_wide(keys, vals, 5000, out=torch.zeros((5000, 3), dtype=torch.int64))
    with pytest.raises(AssertionError):
        eng.group_aggregate_wide(keys, vals, 5000, out=torch.zeros((5000, 4), dtype=torch.int32))
    with pytest.raises(AssertionError):
        eng.group_aggregate_wide(keys, vals, 5000, dropped=torch.zeros(1, dtype=torch.int32))
    for groups in (0, -1, (1 << 18) + 1):
        with pytest.raises(ValueError):
            eng.group_aggregate_wide(keys, vals, groups)
    with pytest.raises(ValueError):
        eng.group_aggregate_wide(col(32, 777), vals, MAX_GROUPS + 1)
    assert rec.calls == []


def test_wide_entry_point_fails_loudly_without_a_gpu(L):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    buf = (C.c_uint8 * 1024)()
    out = (C.c_uint64 * 80)()
    rc = L.mi355_group_aggregate_wide_dev(None, buf, 13, buf, 9, 100, None, 20, out, None)
    assert rc != 0 and L.mi355_last_error()


def test_every_groupby_wide_kernel_has_a_case():
    """every __global__ under csrc/groupby_wide/ is asserted from the launch record by a GPU case of this file (INIT_KERNEL and
    AGG_KERNEL: test_sizes_and_tails, test_errors_launch_nothing), and the file names no kernel that does not exist; the narrow
    tier's directory still holds its two"""
    kernels = support.global_kernels_of("groupby_wide")
    assert kernels == {INIT_KERNEL, AGG_KERNEL}, kernels
    support.check_gpu_part_asserts(__file__, "INIT_KERNEL", "AGG_KERNEL")
    assert support.global_kernels_of("groupby") == {"group_aggregate_init_kernel", "group_aggregate_kernel"}


def test_groupby_wide_sources_read_no_flag_bits():
    assert [os.path.basename(p) for p in support.feature_sources("groupby_wide")] == ["group_aggregate_wide.hip", "group_aggregate_wide.hpp"]
    support.check_sources_read_no_flag_bits("groupby_wide")


def test_groupby_wide_reuses_the_pipeline():
    """the decode and the tile geometry are included, not copied; one kernel, not a template of a width"""
    text = open(os.path.join(support.CSRC, "groupby_wide", "group_aggregate_wide.hpp")).read()
    assert '#include "../kernels/rt_column.hpp"' in text
    code = text.split("#pragma once")[1]
    assert "lookup/lookup.hpp" not in code and "predicates/columns.hpp" not in code
    home = open(os.path.join(support.CSRC, "kernels", "rt_column.hpp")).read()
    for helper in ("columns_lds_value", "rt_image"):
        assert helper in text and not re.search(rf"\buint32_t\s+{helper}\s*\(", text), helper
        assert re.search(rf"\buint32_t\s+{helper}\s*\(", home), helper
    assert "rt_issue_tile" in text and "global_load_lds" not in text  # the tiles' DMA is included too
    assert re.search(r"static __global__ __launch_bounds__\(kBlockThreads\) void group_aggregate_wide_kernel\(", text)
    assert not re.search(r"template\s*<[^>]*>\s*(static\s+)?__global__", text)


def test_front_slots_follow_the_rule(L):
    from shared_simd_scan_amd import group_wide_front_slots

    f = L.mi355_group_wide_front_slots
    seen = set()
    for ck in range(1, 33):
        for cv in range(1, 33):
            s = f(ck, cv)
            assert s == front_slots(ck, cv) == group_wide_front_slots(ck, cv), (ck, cv, s)
            assert 24 * s + tiles_lds(ck, cv) + 16 <= CU_LDS, (ck, cv)
            seen.add(s)
    assert seen == {4096, 2048, 1024} and f(32, 32) == 1024 and f(1, 1) == 4096
    for bad in (0, 33):
        assert f(bad, 9) == 0 and f(9, bad) == 0
        with pytest.raises(ValueError):
            group_wide_front_slots(bad, 9)
        with pytest.raises(ValueError):
            group_wide_front_slots(9, bad)


def gpu_shapes():
    """every (ck, cv, groups, n) the GPU tests below run on recipe data"""
    shapes = {(ck, cv, g, n) for ck, cv, g in SIZE_SHAPES for n in SIZES}
    shapes |= {(ck, cv, width_groups(ck), N_BIG) for ck in KEY_WIDTHS for cv in VALUE_WIDTHS}
    shapes |= {(ck, 17, 1 << ck, N_BIG) for ck in TIER_WIDTHS}
    shapes |= {(ck, cv, g, n) for ck, cv, g in MASK_SHAPES for n in (N_RAGGED, N_BIG)}
    shapes |= {(ck, cv, g, N_HOSTILE) for ck, cv, g in HOSTILE_SHAPES}
    shapes |= {(ck, cv, g, N_BIG) for ck, cv, g in SAME_SHAPES}
    shapes |= {ERROR_SHAPE + (ERROR_N,), CAPTURE_SHAPE + (N_BIG,)}
    return sorted(shapes)


@pytest.mark.parametrize("shape", [s for s in gpu_shapes() if s[3] >= 2047], ids=pid)
def test_recipe_is_not_vacuous(shape):
    """(no device needed) empty groups, dropped rows wherever the key width has room for them, at least two populated groups,
    and at 32-bit values a group that needs unsigned 64-bit care"""
    ck, cv, groups, n = shape
    keys, vals = data(ck, cv, groups, n)
    assert int(keys.max()) < 1 << ck and int(vals.max()) < 1 << cv
    want, dropped = expect(keys, vals, groups)
    assert int(want[:, 1].sum()) + dropped == n
    if (1 << ck) > groups:
        assert 0 < dropped < n // 4, "no dropped rows"
    else:
        assert dropped == 0
    if groups > 5:
        assert (want[:, 1] == 0).any(), "no empty group"
        assert (want[want[:, 1] == 0] == empty_result(1)[0]).all()
        assert int((want[:, 1] > 0).sum()) >= 2, "fewer than two populated groups"
    assert int(want[:, 3].max()) == (1 << cv) - 1 and int(want[:, 2].min()) == 0  # the corner rows
    if cv == 32:
        hard = (want[:, 0] >= 1 << 32) & (want[:, 2] >= 1 << 31) & (want[:, 3] >= 1 << 31) & (want[:, 1] > 0)
        assert hard.any(), "no group with sum >= 2^32 and min, max >= 2^31"


def test_one_block_recipes_must_miss():
    """(no device needed) more distinct in-domain keys than the front has slots: by pigeonhole some keys take the miss path"""
    for ck, cv, groups in SIZE_SHAPES:
        keys = data(ck, cv, groups, N_BIG)[0]
        distinct = len(np.unique(keys[keys < groups]))
        if groups >= 5000:
            assert distinct > 4096, (ck, cv, groups, distinct)
        elif groups > 1024:
            assert distinct > front_slots(ck, cv) == 1024, (ck, cv, groups, distinct)
    for which in ("collide", "hot"):
        ck, cv, keys, vals = front_data(which)
        assert len(np.unique(keys[keys < FRONT_GROUPS])) > 4096 and int(keys.max()) < FRONT_GROUPS <= 1 << ck
        want, dropped = expect(keys, vals, FRONT_GROUPS)
        assert dropped == 0 and (want[:, 1] == 0).any()
        if which == "collide":
            h = 75
            for s in (1024, 2048, 4096):
                assert len({(h + 4096 * j) & (s - 1) for j in range(3)}) == 1
            for j in range(3):
                g = h + 4096 * j
                assert int(want[g, 0]) >= 1 << 44 and int(want[g, 1]) >= N_BIG // 5 and int(want[g, 3]) == 0xFFFFFFFF
        else:
            assert int(want[3001, 1]) > N_BIG * 0.49


def test_dropped_recipe_is_not_vacuous():
    keys, vals, rows = dropped_data()
    groups = DROP_GROUPS
    assert sorted({int(keys[r]) for r in rows}) == [groups - 1, groups, 1 << 26, 1 << 28, 0xFFFFFFFF]
    assert rows[0] < R and R < rows[5] < N_BIG // R * R - R and rows[10] >= N_BIG // R * R and rows[-1] == N_BIG - 1
    want, dropped = expect(keys, vals, groups)
    assert dropped == 12 and int(want[groups - 1, 1]) >= 3 and (want[:, 1] == 0).any()


def test_same_buffer_recipe_is_not_vacuous():
    for c, _, groups in SAME_SHAPES:
        keys = data(c, c, groups, N_BIG)[0]
        want, dropped = expect(keys, keys, groups)
        assert int((want[:, 1] > 0).sum()) >= 2 and dropped > 0
        for g in np.nonzero(want[:, 1])[0][:200]:
            assert want[g, 0] == g * want[g, 1] and want[g, 2] == g and want[g, 3] == g


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

class Bench:
    """one engine, the uploaded columns of a shape, a guarded output and a guarded counter, both refilled with 0xEE before
    every call"""

    def __init__(self, O, eng, ck, cv, groups, n, keys=None, vals=None, same=False):
        from shared_simd_scan_amd.engine import PackedColumn

        self.eng, self.ck, self.cv, self.groups, self.n = eng, ck, cv, groups, n
        if keys is None:
            keys, vals = data(ck, cv, groups, n)
        self.keys, self.vals = keys, vals
        self.kcol = PackedColumn(upload(O, keys, ck), n, ck)
        self.vcol = self.kcol if same else PackedColumn(upload(O, vals, cv), n, cv)
        self.out = Guarded(groups * 32)
        self.cnt = Guarded(8)

    def view(self, g, shape):
        import torch

        return g.t[g.front: g.front + g.nbytes].view(torch.int64).view(*shape)

    def fetch(self):
        return self.out.fetch().view(np.uint64).reshape(self.groups, 4)  # asserts the guard bytes on both sides

    def run(self, mask_bits=None, mask=None, what="", count=True, want=None):
        """-> checks every group's four words, the counter and all guard bytes against numpy; returns (expectation, dropped)"""
        import torch

        self.out.t.fill_(SENTINEL)
        self.cnt.t.fill_(SENTINEL)
        if want is None:
            want = expect(self.keys, self.vals, self.groups, mask_bits)
        want, dropped = want
        if mask_bits is not None and mask is None:
            mask = torch.from_numpy(packbits(mask_bits)).cuda()
        before = [t.clone() for t in (self.kcol.data, self.vcol.data)] + ([mask.clone()] if mask is not None else [])
        got = self.eng.group_aggregate_wide(self.kcol, self.vcol, self.groups, mask=mask, out=self.view(self.out, (self.groups, 4)),
                                            dropped=self.view(self.cnt, (1,)) if count else None)
        self.eng.synchronize()
        have = self.fetch()
        tag = (what, self.ck, self.cv, self.groups, self.n)
        bad = np.nonzero((have != want).any(axis=1))[0]
        assert bad.size == 0, (tag, "group", int(bad[0]), "have", [int(x) for x in have[bad[0]]], "want", [int(x) for x in want[bad[0]]], len(bad))
        cnt = self.cnt.fetch()
        if count:
            assert int(cnt.view(np.uint64)[0]) == dropped, (tag, "dropped")
        else:
            assert (cnt == SENTINEL).all(), (tag, "counter written")
        assert got.data_ptr() == self.view(self.out, (self.groups, 4)).data_ptr()
        after = [self.kcol.data, self.vcol.data] + ([mask] if mask is not None else [])
        for b, a in zip(before, after):
            assert torch.equal(a, b), ("an input was written", tag)
        return want, dropped


class one_block:
    """the whole launch in one block: its four waves walk every tile, and every key meets the one front"""

    def __init__(self, eng):
        self.eng = eng

    def __enter__(self):
        self.eng.set_option("grid_cus", 1)
        self.eng.set_option("max_blocks_per_cu", 1)

    def __exit__(self, *exc):
        self.eng.set_option("grid_cus", 0)
        self.eng.set_option("max_blocks_per_cu", 0)


@gpu
@pytest.mark.parametrize("shape", SIZE_SHAPES, ids=pid)
def test_sizes_and_tails(L, O, eng, shape):
    ck, cv, groups = shape
    for n in SIZES:
        bench = Bench(O, eng, ck, cv, groups, n)
        bench.run()
        recs = record(L, eng)
        assert [r[0] for r in recs] == [INIT_KERNEL, AGG_KERNEL] and all(r[3] == 0 for r in recs), recs
        if n != N_BIG:
            continue
        with one_block(eng):
            bench.run(what="one block")
            (init_label, _, init_lds, _), (label, grid, lds, flags) = record(L, eng)
            assert init_label == INIT_KERNEL and init_lds == 0 and label == AGG_KERNEL and grid == 1 and flags == 0
            s = L.mi355_group_wide_front_slots(ck, cv)
            assert s == front_slots(ck, cv) and lds == 24 * s + tiles_lds(ck, cv) + 16, (lds, s)


@gpu
@pytest.mark.parametrize("ck", KEY_WIDTHS)
def test_every_key_width(L, O, eng, ck):
    groups = width_groups(ck)
    for cv in VALUE_WIDTHS:
        want, dropped = Bench(O, eng, ck, cv, groups, N_BIG).run()
        assert (dropped > 0) == ((1 << ck) > groups)
        assert [r[0] for r in record(L, eng)] == [INIT_KERNEL, AGG_KERNEL]


@gpu
@pytest.mark.parametrize("ck", TIER_WIDTHS)
def test_both_tiers_agree(O, eng, ck):
    import torch

    groups = 1 << ck
    bench = Bench(O, eng, ck, 17, groups, N_BIG)
    bench.run(what="wide tier")
    wide = bench.fetch()
    narrow = eng.group_aggregate(bench.kcol, bench.vcol)
    eng.synchronize()
    assert np.array_equal(narrow.cpu().numpy().view(np.uint64), wide)
    assert torch.equal(narrow, torch.from_numpy(wide.view(np.int64)).cuda())


@gpu
@pytest.mark.parametrize("which", ["collide", "hot"])
def test_front_and_miss_path(L, O, eng, which):
    ck, cv, keys, vals = front_data(which)
    bench = Bench(O, eng, ck, cv, FRONT_GROUPS, N_BIG, keys=keys, vals=vals)
    with one_block(eng):
        want, dropped = bench.run(what=which)
        assert record(L, eng)[1][:2] == (AGG_KERNEL, 1)
    assert dropped == 0
    bench.run(what=which + ", full grid")


@gpu
def test_dropped_rows(O, eng):
    from shared_simd_scan_amd.engine import PackedColumn

    keys, vals, rows = dropped_data()
    n, groups, ck, cv = N_BIG, DROP_GROUPS, 32, 17
    bench = Bench(O, eng, ck, cv, groups, n, keys=keys, vals=vals)
    want, dropped = bench.run(what="corner keys")
    assert dropped == 12
    # under a mask only the rows it lets in are counted: all corner rows out, then every second one
    bits = np.ones(n, dtype=bool)
    bits[rows] = False
    assert bench.run(mask_bits=bits, what="corners masked out")[1] == 0
    bits = np.random.default_rng(9).random(n) < 0.5
    bits[rows[::2]], bits[rows[1::2]] = True, False
    assert bench.run(mask_bits=bits, what="half of the corners")[1] == sum(1 for r in rows[::2] if keys[r] >= groups)
    # no counter: the same groups
    bench.run(what="no counter", count=False)
    # a row-range view: the rows behind it hold all-ones keys and are not counted as dropped
    short = n - 3000
    tail_keys = np.concatenate([keys[:short], np.full(3000, 0xFFFFFFFF, dtype=np.uint32)])
    bench.kcol = PackedColumn(upload(O, tail_keys, ck), short, ck)
    bench.vcol = PackedColumn(bench.vcol.data, short, cv)
    bench.keys, bench.vals, bench.n = keys[:short], vals[:short], short
    want, dropped = bench.run(what="view in front of all-ones keys")
    assert dropped == 8  # the corner rows of the first and the middle tile; none of the 3000 rows behind the view


@gpu
@pytest.mark.parametrize("shape", MASK_SHAPES, ids=pid)
def test_masks(O, eng, shape):
    ck, cv, groups = shape
    for n in (N_RAGGED, N_BIG):  # N_RAGGED: the last tile reads the mask byte by byte
        bench = Bench(O, eng, ck, cv, groups, n)
        rng = np.random.default_rng([ck, cv, n, 7])
        for density in (0.0, 1 / 64, 0.5, 1.0):
            bits = rng.random(n) < density
            want, dropped = bench.run(mask_bits=bits, what=f"density {density}")
            if density == 0.0:
                assert (want == empty_result(groups)).all() and dropped == 0
        # a mask that empties a populated group gives that group's empty result
        g = int(populated(groups)[0])
        assert (bench.keys == g).any()
        want, dropped = bench.run(mask_bits=bench.keys != g, what="group emptied")
        assert [int(x) for x in want[g]] == [0, 0, U64_MAX, 0] and int(want[:, 1].sum()) + dropped == n - int((bench.keys == g).sum())


@gpu
@pytest.mark.parametrize("shape", HOSTILE_SHAPES, ids=pid)
def test_hostile_surroundings(O, eng, shape):
    """row-range views that start at row 8192 of longer columns and are followed by rows of all-ones bits (they would be counted
    as dropped, or land in a group, if they leaked); the mask at an address that is 4 and not 16 bytes aligned, followed by 0xff
    bytes"""
    import torch

    from shared_simd_scan_amd.engine import PackedColumn

    ck, cv, groups = shape
    n, lead, trail = N_HOSTILE, 8192, 4096
    assert n % 8
    keys, vals = data(ck, cv, groups, n)
    rng = np.random.default_rng([ck, cv, 11])

    def long_column(rows, c):
        top = (1 << c) - 1
        junk = rng.integers(0, top + 1, lead, dtype=np.uint64).astype(np.uint32)
        return upload(O, np.concatenate([junk, rows, np.full(trail, top, dtype=np.uint32)]), c)

    bench = Bench(O, eng, ck, cv, groups, n)
    klong, vlong = long_column(keys, ck), long_column(vals, cv)
    bench.kcol = PackedColumn(klong[lead * ck // 8:], n, ck)
    bench.vcol = PackedColumn(vlong[lead * cv // 8:], n, cv)
    assert bench.kcol.data.data_ptr() % 16 == 0 and bench.vcol.data.data_ptr() % 16 == 0
    bench.run(what="views")
    bits = rng.random(n) < 0.5
    mb = packbits(bits)
    buf = torch.full((4 + len(mb) + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    buf[4: 4 + len(mb)] = torch.from_numpy(mb).cuda()
    mask = buf[4: 4 + len(mb)]
    assert mask.data_ptr() % 16 == 4
    want, dropped = bench.run(mask_bits=bits, mask=mask, what="views, offset mask")
    assert int(want[:, 1].sum()) + dropped == int(bits.sum())
    assert (buf[4 + len(mb):] == 0xFF).all() and (buf[:4] == 0xFF).all()


@gpu
@pytest.mark.parametrize("shape", SAME_SHAPES, ids=pid)
def test_same_buffer(O, eng, shape):
    c, _, groups = shape
    keys = data(c, c, groups, N_BIG)[0]
    bench = Bench(O, eng, c, c, groups, N_BIG, keys=keys, vals=keys, same=True)
    assert bench.vcol is bench.kcol
    bench.run(what="keys is values")


@gpu
def test_top_of_the_domain(L, O, eng):
    """groups = 2^26: 2 GiB of result, checked on the device -- the three groups that hold rows, the total count, and sampled
    slices of the rest against the empty result; 32 g needs 64-bit addressing from g = 2^26 - 1 down to 2^26 / 2"""
    import torch

    from shared_simd_scan_amd.engine import PackedColumn

    ck, cv, groups, n = 26, 17, MAX_GROUPS, 3 * R + 77
    rng = np.random.default_rng(26)
    where = np.asarray([0, 1 << 25, groups - 1], dtype=np.uint32)
    keys = where[rng.integers(0, 3, n)]
    vals = rng.integers(0, 1 << cv, n, dtype=np.uint64).astype(np.uint32)
    kcol, vcol = PackedColumn(upload(O, keys, ck), n, ck), PackedColumn(upload(O, vals, cv), n, cv)
    res = Guarded(groups * 32)
    cnt = Guarded(8)
    out = res.t[res.front: res.front + res.nbytes].view(torch.int64).view(groups, 4)
    eng.group_aggregate_wide(kcol, vcol, groups, out=out, dropped=cnt.t[cnt.front: cnt.front + 8].view(torch.int64))
    eng.synchronize()
    assert [r[0] for r in record(L, eng)] == [INIT_KERNEL, AGG_KERNEL]
    for g in where:
        v = vals[keys == g].astype(np.uint64)
        assert [int(x) for x in out[int(g)].cpu()] == [int(v.sum()), len(v), int(v.min()), int(v.max())], int(g)
    assert int(out[:, 1].sum()) == n
    empty = torch.tensor([0, 0, -1, 0], dtype=torch.int64, device="cuda")
    for lo, hi in ((1, 1 << 16), ((1 << 25) - 4096, 1 << 25), ((1 << 25) + 1, (1 << 25) + 4096), (groups - 4096, groups - 1)):
        assert bool((out[lo:hi] == empty).all()), (lo, hi)
    assert bool((res.t[:res.front] == SENTINEL).all()) and bool((res.t[res.front + res.nbytes:] == SENTINEL).all())
    assert int(cnt.fetch().view(np.uint64)[0]) == 0


@gpu
def test_errors_launch_nothing(L, O, eng):
    ck, cv, groups = ERROR_SHAPE
    n = ERROR_N
    bench = Bench(O, eng, ck, cv, groups, n)
    mask = Guarded((n + 7) // 8)
    kp, vp = bench.kcol.data.data_ptr(), bench.vcol.data.data_ptr()
    op, cp = bench.out.ptr.value, bench.cnt.ptr.value

    def call(kp=kp, ck=ck, vp=vp, cv=cv, n=n, mask_ptr=mask.ptr.value, groups=groups, out=op, cnt=cp):
        bench.out.t.fill_(SENTINEL)
        bench.cnt.t.fill_(SENTINEL)
        rc = L.mi355_group_aggregate_wide_dev(eng._ctx, kp, ck, vp, cv, n, mask_ptr, groups, out, cnt)
        eng.synchronize()
        return rc

    for what, kw, word in (("ck = 0", dict(ck=0), b"ck"), ("ck = 33", dict(ck=33), b"ck"), ("cv = 0", dict(cv=0), b"cv"), ("cv = 33", dict(cv=33), b"cv"),
                           ("groups = 0", dict(groups=0), b"groups"), ("groups > 2^ck", dict(groups=(1 << ck) + 1), b"2^ck"),
                           ("groups > 2^26", dict(ck=32, groups=MAX_GROUPS + 1), b"MI355_GROUP_WIDE_MAX_GROUPS"),
                           ("null keys", dict(kp=None), b"keys_dev"), ("null values", dict(vp=None), b"values_dev"), ("null out", dict(out=None), b"out_dev"),
                           ("keys at +4", dict(kp=kp + 4), b"keys_dev"), ("values at +8", dict(vp=vp + 8), b"values_dev"),
                           ("mask at +2", dict(mask_ptr=mask.ptr.value + 2), b"mask_dev"), ("out at +4", dict(out=op + 4), b"out_dev"),
                           ("counter at +4", dict(cnt=cp + 4), b"dropped_dev")):
        assert call(**kw) == E_INVALID, what
        assert word in L.mi355_last_error(), (what, L.mi355_last_error())
        assert record(L, eng) == [], what
        assert (bench.out.fetch() == SENTINEL).all() and (bench.cnt.fetch() == SENTINEL).all() and (mask.fetch() == SENTINEL).all(), what
    # n == 0: the empty result for every group, 0 in the counter, and no aggregation kernel
    assert call(n=0, kp=None, vp=None, mask_ptr=None) == 0
    recs = record(L, eng)
    assert len(recs) == 1 and recs[0][0] == INIT_KERNEL, recs
    assert (bench.fetch() == empty_result(groups)).all() and int(bench.cnt.fetch().view(np.uint64)[0]) == 0
    # the same arguments, valid: they do launch
    assert call(mask_ptr=None) == 0
    assert [r[0] for r in record(L, eng)] == [INIT_KERNEL, AGG_KERNEL]
    want, dropped = expect(bench.keys, bench.vals, groups)
    assert (bench.fetch() == want).all() and int(bench.cnt.fetch().view(np.uint64)[0]) == dropped > 0


@gpu
def test_graph_capture_and_replay(O):
    """a linear chain on a side stream, as tests/test_group_aggregate.py::test_graph_capture_and_replay: warm up, capture, three
    replays over keys, values and a mask overwritten in place, the counter of dropped rows included"""
    import torch

    from shared_simd_scan_amd.engine import PackedColumn

    ck, cv, groups = CAPTURE_SHAPE
    n = N_BIG
    versions = []
    for r in range(3):
        keys, vals = data(ck, cv, groups, n, salt=r + 1)
        bits = np.random.default_rng(50 + r).random(n) < (0.4, 0.5, 0.6)[r]
        versions.append((O.pack(keys, ck), O.pack(vals, cv), packbits(bits)) + expect(keys, vals, groups, bits))
    for i in range(3):
        for j in range(i):
            assert (versions[i][3][:, :2] != versions[j][3][:, :2]).any() and versions[i][4] != versions[j][4], "a stale result could pass"

    def steps(eng):
        stage = [[torch.from_numpy(x).cuda() for x in v[:3]] for v in versions]
        kcol = PackedColumn(torch.empty_like(stage[0][0]), n, ck)
        vcol = PackedColumn(torch.empty_like(stage[0][1]), n, cv)
        mask = torch.empty_like(stage[0][2])
        res, cnt = Guarded(groups * 32), Guarded(8)
        out = res.t[res.front: res.front + res.nbytes].view(torch.int64).view(groups, 4)
        dropped = cnt.t[cnt.front: cnt.front + 8].view(torch.int64)

        def load(r):
            kcol.data.copy_(stage[r][0])
            vcol.data.copy_(stage[r][1])
            mask.copy_(stage[r][2])
            res.t.fill_(SENTINEL)
            cnt.t.fill_(SENTINEL)

        def run():
            eng.group_aggregate_wide(kcol, vcol, groups, mask=mask, out=out, dropped=dropped)

        def check(r, what):
            assert np.array_equal(res.fetch().view(np.uint64).reshape(groups, 4), versions[r][3]), what
            assert int(cnt.fetch().view(np.uint64)[0]) == versions[r][4], what

        def untouched():
            assert (res.fetch() == SENTINEL).all() and (cnt.fetch() == SENTINEL).all()

        return capture.Steps(load, run, check, untouched)

    capture.capture_replay(steps, range(3))


@gpu
def test_the_chain_it_exists_for(L, O, eng):
    """GROUP BY g1, g2 over two 9-bit dictionary columns: arith builds the 18-bit key g1 * 512 + g2, group_aggregate_wide groups
    by it; the expectation is numpy on the three original columns"""
    from shared_simd_scan_amd.engine import PackedColumn

    n, cv = N_BIG, 17
    rng = np.random.default_rng(1812)
    g1 = rng.integers(0, 300, n, dtype=np.uint64).astype(np.uint32)
    g2 = rng.integers(0, 512, n, dtype=np.uint64).astype(np.uint32)
    g2[rng.random(n) < 0.3] = 7
    vals = rng.integers(0, 1 << cv, n, dtype=np.uint64).astype(np.uint32)
    c1, c2, vcol = (PackedColumn(upload(O, a, c), n, c) for a, c in ((g1, 9), (g2, 9), (vals, cv)))
    key = eng.arith("linear", c1, c2, a=512, b=1)
    assert (key.c, key.n) == (18, n)
    groups = 512 * 512
    res = Guarded(groups * 32)
    import torch

    out = res.t[res.front: res.front + res.nbytes].view(torch.int64).view(groups, 4)
    eng.group_aggregate_wide(key, vcol, groups, out=out)
    eng.synchronize()
    assert [r[0] for r in record(L, eng)] == [INIT_KERNEL, AGG_KERNEL]
    want, dropped = expect(g1 * np.uint32(512) + g2, vals, groups)
    assert dropped == 0 and int((want[:, 1] > 0).sum()) > 4096 and (want[300 * 512:, 1] == 0).all()
    have = res.fetch().view(np.uint64).reshape(groups, 4)
    bad = np.nonzero((have != want).any(axis=1))[0]
    assert bad.size == 0, (int(bad[0]), [int(x) for x in have[bad[0]]], [int(x) for x in want[bad[0]]])
