"""Grouped aggregates over two packed columns (include/mi355_groupby.h, ScanEngine.group_aggregate): per value g of the key
column the sum, count, min and max of the value column, optionally under a bitmap.

CPU: the header is plain C99 and declares exactly what _capi.HEADERS binds for it and the library exports; it carries its
graph-capture verdict; group_aggregate hands the C ABI what it should (through a recording stand-in for the library, the idea
of tests/test_scan_columns.py); without a device the entry point fails with a message; every __global__ under csrc/groupby/
is named by the launch record of a GPU case of this file; no source there reads a switch bit; the data recipe is not vacuous.

GPU (-m gpu): every expectation is numpy arithmetic on the keys and values the test generated -- np.bincount, np.add.at on
uint64, np.minimum.at / np.maximum.at -- packed with the oracle's packer on the way in; nothing is derived from engine output.
The output sits inside 0xEE guard bytes (support.Guarded) that must stay untouched.  Tiles are 2048 rows (32 rows per
lane), so the sizes below are the smallest that reach one lane, one partial tile, one full tile, a full tile plus one row,
one tile per wave of a block, and many tiles with a ragged tail.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import capture
import support
from support import E_INVALID, SENTINEL, Guarded, L, eng, fake, packbits, record, upload  # noqa: F401  (L, eng, fake: fixtures)

HEADER = "mi355_groupby.h"
U64_MAX = (1 << 64) - 1

# the kernels of csrc/groupby/, as the launch record names them: the GPU cases below assert these labels
INIT_KERNEL = "group_aggregate_init_kernel"
AGG_KERNEL = "group_aggregate_kernel"

N_BIG = 8192 * 9 + 1237  # 74965: 36 tiles of 2048 rows and a ragged one
SIZES = [1, 13, 509, 2048, 2049, 8192, N_BIG]
SIZE_PAIRS = [(3, 9), (9, 9), (12, 32), (1, 17)]
KEY_WIDTHS = list(range(1, 13))
VALUE_WIDTHS = [1, 9, 16, 17, 31, 32]
SAME_WIDTHS = [1, 9, 12]
MASK_PAIRS = [(3, 9), (5, 17), (12, 32)]
N_RAGGED = 2048 + 509
HOSTILE_PAIRS = [(3, 9), (12, 32)]
N_HOSTILE = 2048 * 3 + 509  # not a multiple of 8

gpu = pytest.mark.gpu


def pid(p):
    return "-".join(str(x) for x in p)


def populated(ck):
    return [g for g in range(1 << ck) if g % 7 != 5]


@functools.lru_cache(maxsize=None)
def data(ck, cv, n, salt=0):
    """the data recipe -> (keys, values) as read-only uint32 arrays.  Keys are uniform over the groups g with g % 7 != 5, so
    empty groups exist whenever 2^ck > 5; values are uniform over [0, 2^cv); rows 0..7 are corner rows: value 0 (and 1) in
    the first populated group, 2^cv - 1 (and 2^cv - 2) in the last.  At cv = 32 every row of the last populated group has bit
    31 set: that group's min and max are >= 2^31 and its sum is beyond 32 bits, so a signed min / max or a 32-bit partial sum
    cannot pass."""
    rng = np.random.default_rng([ck, cv, salt])
    pop = np.asarray(populated(ck), dtype=np.uint32)
    vmax = (1 << cv) - 1
    keys = pop[rng.integers(0, len(pop), n)]
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


def expect(keys, vals, ck, mask_bits=None):
    """uint64[2^ck, 4] = (sum, count, min, max) per group, numpy on the generated rows"""
    groups = 1 << ck
    if mask_bits is not None:
        keys, vals = keys[mask_bits], vals[mask_bits]
    k = keys.astype(np.int64)
    v = vals.astype(np.uint64)
    want = empty_result(groups)
    np.add.at(want[:, 0], k, v)  # uint64: exact modulo 2^64
    want[:, 1] = np.bincount(k, minlength=groups).astype(np.uint64)
    np.minimum.at(want[:, 2], k, v)
    np.maximum.at(want[:, 3], k, v)
    return want


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------

def test_groupby_header_is_plain_c99():
    support.check_header_is_plain_c99(HEADER)


def test_groupby_header_declares_what_python_binds(L):
    names, sigs = support.check_header_binds(L, HEADER)
    assert names == ["mi355_group_aggregate_dev"]
    sig = sigs["mi355_group_aggregate_dev"]
    assert sig[2] is C.c_uint and sig[4] is C.c_uint and sig[5] is C.c_uint64 and len(sig) == 8


def test_groupby_header_carries_its_capture_verdict():
    support.check_capture_verdict(HEADER)


def test_group_aggregate_wrapper_passes_what_the_abi_takes(fake):
    import torch

    eng, rec, col = fake
    keys, vals = col(5, 777), col(17, 777)
    mask = torch.zeros(128, dtype=torch.uint8)
    out = torch.zeros((32, 4), dtype=torch.int64)
    got = eng.group_aggregate(keys, vals, mask=mask, out=out)
    (name, a), = rec.calls
    assert name == "mi355_group_aggregate_dev" and got is out
    assert a[1:] == [keys.data.data_ptr(), 5, vals.data.data_ptr(), 17, 777, mask.data_ptr(), out.data_ptr()]
    rec.calls.clear()
    got = eng.group_aggregate(keys, vals)
    (name, a), = rec.calls
    assert a[1:6] == [keys.data.data_ptr(), 5, vals.data.data_ptr(), 17, 777] and a[6] is None
    assert tuple(got.shape) == (32, 4) and got.dtype == torch.int64 and a[7] == got.data_ptr()
    rec.calls.clear()
    for ck in (1, 12):
        got = eng.group_aggregate(col(ck, 5), col(32, 5))
        assert tuple(got.shape) == (1 << ck, 4)
    assert [c[1][2] for c in rec.calls] == [1, 12]
    rec.calls.clear()
    with pytest.raises(AssertionError):
        eng.group_aggregate(keys, col(17, 778))  # row counts differ
    with pytest.raises(AssertionError):
        eng.group_aggregate(keys, vals, out=torch.zeros((16, 4), dtype=torch.int64))  # 2^5 groups need 32 rows
    with pytest.raises(AssertionError):
        eng.group_aggregate(keys, vals, out=torch.zeros((32, 4), dtype=torch.int32))
    assert rec.calls == []


def test_group_entry_point_fails_loudly_without_a_gpu(L):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    buf = (C.c_uint8 * 1024)()
    out = (C.c_uint64 * 32)()
    rc = L.mi355_group_aggregate_dev(None, buf, 3, buf, 9, 100, None, out)
    assert rc != 0 and L.mi355_last_error()


def test_every_groupby_kernel_has_a_case():
    """the rule test_shared_where_cpu.py applies to csrc/predicates/: every __global__ under csrc/groupby/ is asserted from the
    launch record by a GPU case of this file (INIT_KERNEL: test_errors_launch_nothing, AGG_KERNEL: test_sizes_and_tails and
    others), and the file names no kernel that does not exist"""
    kernels = support.global_kernels_of("groupby")
    assert kernels == {INIT_KERNEL, AGG_KERNEL}, kernels
    support.check_gpu_part_asserts(__file__, "INIT_KERNEL", "AGG_KERNEL")


def test_groupby_sources_read_no_flag_bits():
    support.check_sources_read_no_flag_bits("groupby")


def gpu_shapes():
    """every (ck, cv, n) the GPU tests below run on recipe data"""
    shapes = {(ck, cv, n) for ck, cv in SIZE_PAIRS for n in SIZES}
    shapes |= {(ck, cv, N_BIG) for ck in KEY_WIDTHS for cv in VALUE_WIDTHS}
    shapes |= {(ck, cv, n) for ck, cv in MASK_PAIRS for n in (N_RAGGED, N_BIG)}
    shapes |= {(ck, cv, N_HOSTILE) for ck, cv in HOSTILE_PAIRS}
    shapes |= {(3, 9, 4096 + 77), (5, 12, N_BIG)}  # errors, graph capture
    return sorted(shapes)


@pytest.mark.parametrize("shape", [s for s in gpu_shapes() if s[2] >= 2048], ids=pid)
def test_recipe_is_not_vacuous(shape):
    """(no device needed) empty groups, at least two populated ones, and at 32-bit values a group that needs unsigned 64-bit care"""
    ck, cv, n = shape
    keys, vals = data(ck, cv, n)
    want = expect(keys, vals, ck)
    groups = 1 << ck
    assert int(want[:, 1].sum()) == n
    if groups > 5:
        assert (want[:, 1] == 0).any(), "no empty group"
        assert (want[want[:, 1] == 0] == empty_result(1)[0]).all()
    assert int((want[:, 1] > 0).sum()) >= 2, "fewer than two populated groups"
    assert int(want[:, 3].max()) == (1 << cv) - 1 and int(want[:, 2].min()) == 0  # the corner rows
    if cv == 32:
        hard = (want[:, 0] >= 1 << 32) & (want[:, 2] >= 1 << 31) & (want[:, 3] >= 1 << 31) & (want[:, 1] > 0)
        assert hard.any(), "no group with sum >= 2^32 and min, max >= 2^31"


def test_same_buffer_recipe_is_not_vacuous():
    for c in SAME_WIDTHS:
        keys = data(c, c, N_BIG)[0]
        want = expect(keys, keys, c)
        assert int((want[:, 1] > 0).sum()) >= 2
        for g in np.nonzero(want[:, 1])[0]:
            assert want[g, 0] == g * want[g, 1] and want[g, 2] == g and want[g, 3] == g


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

class Bench:
    """one engine, the uploaded columns of a width pair, a guarded output that is refilled with 0xEE before every call"""

    def __init__(self, O, eng, ck, cv, n, keys=None, vals=None, same=False):
        from shared_simd_scan_amd.engine import PackedColumn

        self.eng, self.ck, self.cv, self.n, self.groups = eng, ck, cv, n, 1 << ck
        if keys is None:
            keys, vals = data(ck, cv, n)
        self.keys, self.vals = keys, vals
        self.kcol = PackedColumn(upload(O, keys, ck), n, ck)
        self.vcol = self.kcol if same else PackedColumn(upload(O, vals, cv), n, cv)
        self.out = Guarded(self.groups * 32)

    def out_view(self):
        import torch

        return self.out.t[self.out.front: self.out.front + self.out.nbytes].view(torch.int64).view(self.groups, 4)

    def fetch(self):
        return self.out.fetch().view(np.uint64).reshape(self.groups, 4)  # asserts the guard bytes on both sides

    def run(self, mask_bits=None, mask=None, what=""):
        """-> checks every group's four words and the guard bytes against numpy; returns the expectation"""
        import torch

        self.out.t.fill_(SENTINEL)
        want = expect(self.keys, self.vals, self.ck, mask_bits)
        if mask_bits is not None and mask is None:
            mask = torch.from_numpy(packbits(mask_bits)).cuda()
        before = mask.clone() if mask is not None else None
        got = self.eng.group_aggregate(self.kcol, self.vcol, mask=mask, out=self.out_view())
        self.eng.synchronize()
        have = self.fetch()
        tag = (what, self.ck, self.cv, self.n)
        bad = np.nonzero((have != want).any(axis=1))[0]
        assert bad.size == 0, (tag, "group", int(bad[0]), "have", [int(x) for x in have[bad[0]]], "want", [int(x) for x in want[bad[0]]])
        assert got.data_ptr() == self.out_view().data_ptr()
        if mask is not None:
            assert torch.equal(mask, before), ("mask written", tag)
        return want


@gpu
@pytest.mark.parametrize("pair", SIZE_PAIRS, ids=pid)
def test_sizes_and_tails(L, O, eng, pair):
    ck, cv = pair
    for n in SIZES:
        bench = Bench(O, eng, ck, cv, n)
        bench.run()
        recs = record(L, eng)
        assert [r[0] for r in recs] == [INIT_KERNEL, f"{AGG_KERNEL}<{ck}>"] and all(r[3] == 0 for r in recs), recs
        if n != N_BIG:
            continue
        # one block: its four waves walk several tiles each -- prefetch, the second LDS image, the ragged tail
        eng.set_option("grid_cus", 1)
        eng.set_option("max_blocks_per_cu", 1)
        try:
            bench.run(what="capped")
            (init_label, _, _, _), (label, grid, lds, flags) = record(L, eng)
            assert init_label == INIT_KERNEL and grid == 1 and label == f"{AGG_KERNEL}<{ck}>" and flags == 0 and lds > 0
        finally:
            eng.set_option("grid_cus", 0)
            eng.set_option("max_blocks_per_cu", 0)


@gpu
@pytest.mark.parametrize("ck", KEY_WIDTHS)
def test_every_key_width(L, O, eng, ck):
    for cv in VALUE_WIDTHS:
        Bench(O, eng, ck, cv, N_BIG).run()
        assert record(L, eng)[-1][0] == f"{AGG_KERNEL}<{ck}>"


@gpu
@pytest.mark.parametrize("c", SAME_WIDTHS)
def test_same_buffer(O, eng, c):
    keys = data(c, c, N_BIG)[0]
    bench = Bench(O, eng, c, c, N_BIG, keys=keys, vals=keys, same=True)
    assert bench.vcol is bench.kcol
    bench.run(what="keys is values")


@gpu
def test_what_a_wrong_accumulator_shows(O, eng):
    n, top = N_BIG, 0xFFFFFFFF
    vals = np.full(n, top, dtype=np.uint32)
    # every row in one group: a 32-bit partial sum anywhere wraps, a signed min / max sees -1
    want = Bench(O, eng, 3, 32, n, keys=np.full(n, 6, dtype=np.uint32), vals=vals).run(what="one group")
    assert [int(x) for x in want[6]] == [n * top, n, top, top] and n * top >= 1 << 48
    # two groups, alternating rows: every replicated copy of both groups holds a share that must reach the result
    keys = (np.arange(n) & 1).astype(np.uint32)
    want = Bench(O, eng, 1, 32, n, keys=keys, vals=vals).run(what="alternating")
    assert [int(x) for x in want[0]] == [(n + 1) // 2 * top, (n + 1) // 2, top, top]
    assert [int(x) for x in want[1]] == [n // 2 * top, n // 2, top, top]


@gpu
@pytest.mark.parametrize("pair", MASK_PAIRS, ids=pid)
def test_masks(O, eng, pair):
    ck, cv = pair
    for n in (N_RAGGED, N_BIG):  # N_RAGGED: the last tile reads the mask byte by byte
        bench = Bench(O, eng, ck, cv, n)
        rng = np.random.default_rng([ck, cv, n, 7])
        for density in (0.0, 1 / 64, 0.5, 1.0):
            bits = rng.random(n) < density
            want = bench.run(mask_bits=bits, what=f"density {density}")
            if density == 0.0:
                assert (want == empty_result(bench.groups)).all()
        # a mask that empties a populated group gives that group's empty result
        g = populated(ck)[1]
        assert (bench.keys == g).any()
        want = bench.run(mask_bits=bench.keys != g, what="group emptied")
        assert [int(x) for x in want[g]] == [0, 0, U64_MAX, 0] and int(want[:, 1].sum()) == n - int((bench.keys == g).sum())


@gpu
@pytest.mark.parametrize("pair", HOSTILE_PAIRS, ids=pid)
def test_hostile_surroundings(O, eng, pair):
    """row-range views that start at row 8192 of longer columns and are followed by rows of all-ones bits (they would land in
    the last group if they leaked); the mask at an address that is 4 and not 16 bytes aligned, followed by 0xff bytes"""
    import torch

    from shared_simd_scan_amd.engine import PackedColumn

    ck, cv = pair
    n, lead, trail = N_HOSTILE, 8192, 4096
    assert n % 8
    keys, vals = data(ck, cv, n)
    rng = np.random.default_rng([ck, cv, 11])

    def long_column(rows, c):
        top = (1 << c) - 1
        junk = rng.integers(0, top + 1, lead, dtype=np.uint64).astype(np.uint32)
        return upload(O, np.concatenate([junk, rows, np.full(trail, top, dtype=np.uint32)]), c)

    bench = Bench(O, eng, ck, cv, n)
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
    want = bench.run(mask_bits=bits, mask=mask, what="views, offset mask")
    assert int(want[:, 1].sum()) == int(bits.sum())
    assert (buf[4 + len(mb):] == 0xFF).all() and (buf[:4] == 0xFF).all()


@gpu
def test_errors_launch_nothing(L, O, eng):
    n, ck, cv = 4096 + 77, 3, 9
    bench = Bench(O, eng, ck, cv, n)
    mask = Guarded((n + 7) // 8)
    kp, vp = bench.kcol.data.data_ptr(), bench.vcol.data.data_ptr()

    def call(kp=kp, ck=ck, vp=vp, cv=cv, n=n, mask_ptr=mask.ptr.value, out=bench.out.ptr.value):
        bench.out.t.fill_(SENTINEL)
        rc = L.mi355_group_aggregate_dev(eng._ctx, kp, ck, vp, cv, n, mask_ptr, out)
        eng.synchronize()
        return rc

    for what, kw, word in (("ck = 0", dict(ck=0), b"12"), ("ck = 13", dict(ck=13), b"12"), ("cv = 0", dict(cv=0), b"32"), ("cv = 33", dict(cv=33), b"32"),
                           ("keys at +4", dict(kp=kp + 4), b"aligned"), ("out at +4", dict(out=bench.out.ptr.value + 4), b"aligned"),
                           ("mask at +2", dict(mask_ptr=mask.ptr.value + 2), b"aligned"), ("null out", dict(out=None), b"out_dev"),
                           ("null values", dict(vp=None), b"mi355_histogram_dev"), ("null keys", dict(kp=None), b"keys_dev")):
        assert call(**kw) == E_INVALID, what
        assert word in L.mi355_last_error(), (what, L.mi355_last_error())
        assert record(L, eng) == [], what
        assert (bench.out.fetch() == SENTINEL).all() and (mask.fetch() == SENTINEL).all(), what
    # n == 0: the empty result for every group, and no aggregation kernel
    assert call(n=0, kp=None, vp=None, mask_ptr=None) == 0
    recs = record(L, eng)
    assert len(recs) == 1 and recs[0][0] == INIT_KERNEL, recs
    assert (bench.fetch() == empty_result(bench.groups)).all()
    # the same arguments, valid: they do launch
    assert call(mask_ptr=None) == 0
    assert [r[0] for r in record(L, eng)] == [INIT_KERNEL, f"{AGG_KERNEL}<{ck}>"]
    assert (bench.fetch() == expect(bench.keys, bench.vals, ck)).all()


@gpu
def test_graph_capture_and_replay(O):
    """a linear chain on a side stream, as tests/test_scan_columns.py::test_graph_capture_and_replay: warm up, capture, three
    replays over keys, values and a mask overwritten in place"""
    import torch

    from shared_simd_scan_amd.engine import PackedColumn

    n, ck, cv = N_BIG, 5, 12
    groups = 1 << ck
    versions = []
    for r in range(3):
        keys, vals = data(ck, cv, n, salt=r + 1)
        bits = np.random.default_rng(50 + r).random(n) < (0.4, 0.5, 0.6)[r]
        versions.append((O.pack(keys, ck), O.pack(vals, cv), packbits(bits), expect(keys, vals, ck, bits)))
    for i in range(3):
        for j in range(i):
            assert (versions[i][3][:, :2] != versions[j][3][:, :2]).any(), "a stale result could pass"

    def steps(eng):
        stage = [[torch.from_numpy(x).cuda() for x in v[:3]] for v in versions]
        kcol = PackedColumn(torch.empty_like(stage[0][0]), n, ck)
        vcol = PackedColumn(torch.empty_like(stage[0][1]), n, cv)
        mask = torch.empty_like(stage[0][2])
        res = Guarded(groups * 32)
        out = res.t[res.front: res.front + res.nbytes].view(torch.int64).view(groups, 4)

        def load(r):
            kcol.data.copy_(stage[r][0])
            vcol.data.copy_(stage[r][1])
            mask.copy_(stage[r][2])
            res.t.fill_(SENTINEL)

        def run():
            eng.group_aggregate(kcol, vcol, mask=mask, out=out)

        def check(r, what):
            assert np.array_equal(res.fetch().view(np.uint64).reshape(groups, 4), versions[r][3]), what

        def untouched():
            assert (res.fetch() == SENTINEL).all()

        return capture.Steps(load, run, check, untouched)

    capture.capture_replay(steps, range(3))
