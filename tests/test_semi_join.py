"""Semi-join of a packed column against a device-resident bitmap set (include/mi355_semijoin.h, ScanEngine.semi_join):
bitmap[i] = (v_i < set_bits and bit v_i of the set) XOR negate, AND and_mask[i].

CPU: the header is plain C99 and declares exactly what _capi.HEADERS binds for it and the library exports; it carries its
graph-capture verdict; mi355_semijoin_kernel (pure arithmetic) names the tier at every boundary; semi_join hands the C ABI what
it should (through a recording stand-in for the library); without a device the entry point fails with a message; every
__global__ under csrc/semijoin/ is named by the launch record of a GPU case of this file; no source there reads a switch bit;
the data recipe is not vacuous.

GPU (-m gpu): every expectation is numpy on the values and the set the test generated -- res = (v < m) & set[min(v, m - 1)]
(all zero when m == 0), XOR negate, AND mask -- packed with the oracle's packer on the way in; nothing is derived from engine
output.  Every byte of the bitmap (tail bits included), the hit count and the 0xEE guard bytes on both sides of the bitmap
(support.Guarded) are compared exactly; set, mask and column must be unchanged after the call.  Tiles are 8192 rows
at c <= 16 and 4096 above, so the sizes below are the smallest that reach one lane, one partial tile, one full tile, a full
tile plus one row and many tiles with a ragged tail.
"""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import capture
import support
from support import E_INVALID, SENTINEL, Guarded, L, base_name, eng, fake, header_macro, packbits, record, upload  # noqa: F401  (L, eng, fake: fixtures)

HEADER = "mi355_semijoin.h"

# the kernels of csrc/semijoin/, as the launch record names them: the GPU cases below assert these labels
LDS_KERNEL = "semijoin_lds_kernel"
GLOBAL_KERNEL = "semijoin_global_kernel"


LDS_MAX = header_macro(HEADER, "MI355_SEMIJOIN_LDS_MAX_BITS")

N_BIG = 8192 * 9 + 1237  # 74965: nine tiles of 8192 rows (eighteen of 4096) and a ragged one; not a multiple of 8
SIZES = [1, 13, 509, 4096, 4097, 8192, 8193, N_BIG]
SIZE_CASES = [(9, 512), (9, 300), (17, 100003), (32, 5000)]
# every width: m = min(2^c, 3001); c = 20 and c = 32 also 2^19; and, so that every instantiation of the second tier runs as well,
# every width that can reach beyond the LDS ceiling also LDS_MAX + 1
WIDTH_CASES = ([(c, min(1 << c, 3001)) for c in range(1, 33)] + [(20, 1 << 19), (32, 1 << 19)]
               + [(c, LDS_MAX + 1) for c in range(20, 33)])
SET_SIZES = [1, 7, 8, 9, 31, 32, 33, 509, LDS_MAX - 1, LDS_MAX, LDS_MAX + 1, (1 << 22) + 5]
SET_SIZE_CASES = [(24, m) for m in SET_SIZES] + [(5, 1000)]
HOSTILE_CASES = [(24, 3000 + r) for r in (0, 1, 7)] + [(24, LDS_MAX + 8 + r) for r in (0, 1, 7)]
MASK_CASES = [(9, 300), (24, 3001), (24, LDS_MAX + 1)]
VIEW_CASES = [(9, 300), (24, LDS_MAX + 1)]
N_VIEW = 8192 * 2 + 509
ERROR_CASE = (9, 300, 4096 + 77)
CAPTURE_CASES = [(12, 3001), (24, LDS_MAX + 1)]  # (fact width, rows of the dimension table): one per tier

gpu = pytest.mark.gpu


def pid(p):
    return "-".join(str(x) for x in p)


def reach_of(c, m):
    """what a c-bit value can address of an m-bit set"""
    return min(m, 1 << c)


def tile_rows(c):
    return 8192 if c <= 16 else 4096


def corner_rows(c, n):
    """rows that carry the corner values: the first four of the first tile, the last four of the last full tile, the last four
    of the ragged tail (as far as they exist)"""
    t = tile_rows(c)
    rows = [list(range(min(4, n)))]
    nfull = n // t
    if nfull >= 1:
        rows.append(list(range(nfull * t - 4, nfull * t)))
    if n % t >= 4 and n > 4:
        rows.append(list(range(n - 4, n)))
    return rows


@functools.lru_cache(maxsize=None)
def data(c, m, n, salt=0):
    """the data recipe -> (values uint32[n], set bool[m]), read-only.  Set: every bit a coin flip, then bit reach - 1 one,
    bit reach - 2 zero (a one and a zero among the last eight reachable bits) and bit 0 one (reach >= 3), reach = min(m, 2^c).
    Values: half of them uniform below reach, half uniform over [0, 2^c), then the corner values 0, reach - 1, m (clamped to
    2^c - 1) and 2^c - 1 at corner_rows()."""
    rng = np.random.default_rng([c, m % (1 << 31), m >> 31, n, salt])
    top = (1 << c) - 1
    reach = reach_of(c, m)
    bits = rng.random(m) < 0.5
    if reach >= 1:
        bits[reach - 1] = True
    if reach >= 2:
        bits[reach - 2] = False
    if reach >= 3:
        bits[0] = True
    vals = rng.integers(0, top + 1, n, dtype=np.uint64)
    if reach:
        low = rng.random(n) < 0.5
        vals[low] = rng.integers(0, reach, int(low.sum()), dtype=np.uint64)
    corners = [0, max(reach - 1, 0), min(m, top), top]
    for rows in corner_rows(c, n):
        for r, v in zip(rows, corners):
            vals[r] = v
    vals = vals.astype(np.uint32)
    for a in (vals, bits):
        a.setflags(write=False)
    return vals, bits


def in_set(vals, bits, m):
    """the expectation's core, as the issue words it: (v < m) & set[min(v, m - 1)], all zero when m == 0"""
    v = vals.astype(np.int64)
    if m == 0:
        return np.zeros(len(v), dtype=bool)
    return (v < m) & bits[np.minimum(v, m - 1)]


def expect(vals, bits, m, negate=False, mask_bits=None):
    res = in_set(vals, bits, m) ^ bool(negate)
    if mask_bits is not None:
        res = res & mask_bits
    return res


def mask_recipe(vals, bits, m, negate=False, salt=0):
    """a coin flip per row; the first row the (possibly negated) predicate selects is masked off, the second kept"""
    rng = np.random.default_rng([len(vals), m % (1 << 31), salt, 77])
    mb = rng.random(len(vals)) < 0.5
    sel = np.nonzero(in_set(vals, bits, m) ^ bool(negate))[0]
    if len(sel) >= 1:
        mb[sel[0]] = False
    if len(sel) >= 2:
        mb[sel[1]] = True
    return mb


STAR_M, STAR_N = 3001, N_BIG


@functools.lru_cache(maxsize=None)
def star_data():
    """the star-join chain's tables -> (dim attribute uint32[m] at 5 bits, fact fk at 12 bits, group at 6, value at 17), read-only"""
    rng = np.random.default_rng(2024)
    attr = rng.integers(0, 32, STAR_M, dtype=np.uint64).astype(np.uint32)
    fk = rng.integers(0, 1 << 12, STAR_N, dtype=np.uint64).astype(np.uint32)
    group = rng.integers(0, 1 << 6, STAR_N, dtype=np.uint64).astype(np.uint32)
    value = rng.integers(0, 1 << 17, STAR_N, dtype=np.uint64).astype(np.uint32)
    for a in (attr, fk, group, value):
        a.setflags(write=False)
    return attr, fk, group, value


def star_selection(attr, fk, m):
    f = fk.astype(np.int64)
    return (f < m) & (attr[np.minimum(f, m - 1)] == 3)


@functools.lru_cache(maxsize=None)
def capture_data(c, m):
    """the capture test's tables -> (fact fk uint32[N_BIG] at c bits, two versions of the m-row 5-bit dimension attribute)"""
    rng = np.random.default_rng([c, 99])
    fk = rng.integers(0, min(1 << c, m + m // 8 + 8), N_BIG, dtype=np.uint64).astype(np.uint32)
    fk[:4] = [0, m - 1, m, min(m + 1, (1 << c) - 1)]
    attrs = []
    for r in range(2):
        attr = np.random.default_rng([c, 100 + r]).integers(0, 32, m, dtype=np.uint64).astype(np.uint32)
        attr[m - 1] = 3
        attr[0] = 3 if r == 0 else 4
        attr.setflags(write=False)
        attrs.append(attr)
    fk.setflags(write=False)
    return fk, attrs


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------

def test_semijoin_header_is_plain_c99():
    support.check_header_is_plain_c99(HEADER)


def test_semijoin_header_declares_what_python_binds(L):
    names, sigs = support.check_header_binds(L, HEADER)
    assert names == ["mi355_semijoin_dev", "mi355_semijoin_kernel"]
    sig = sigs["mi355_semijoin_dev"]
    assert sig[2] is C.c_uint64 and sig[3] is C.c_uint and sig[5] is C.c_uint64 and sig[6] is C.c_int and len(sig) == 10
    assert sigs["mi355_semijoin_kernel"] == [C.c_uint, C.c_uint64] and L.mi355_semijoin_kernel.restype is C.c_char_p


def test_semijoin_header_carries_its_capture_verdict():
    support.check_capture_verdict(HEADER, r"read at every replay")


def test_kernel_choice_at_the_boundaries(L):
    """mi355_semijoin_kernel needs neither a device nor a context; the tier follows min(set_bits, 2^c)"""
    from shared_simd_scan_amd import semi_join_kernel

    k = L.mi355_semijoin_kernel
    assert LDS_MAX >= 1 << 19, "the LDS tier must hold at least 64 KiB of set"
    for c in (24, 32):
        assert [k(c, m) for m in (0, 1, LDS_MAX)] == [LDS_KERNEL.encode()] * 3, c
        assert k(c, LDS_MAX + 1) == GLOBAL_KERNEL.encode() and k(c, 1 << 32) == GLOBAL_KERNEL.encode(), c
        assert k(c, (1 << 32) + 1) is None, c
    for m in (0, 1, 3001, 1 << 32):
        assert k(0, m) is None and k(33, m) is None, m
    # a narrow column reaches only the first 2^c bits, however large the set is
    for c in (1, 5, 9, 16, 19):
        assert 1 << c <= LDS_MAX and k(c, 1 << 32) == LDS_KERNEL.encode() and k(c, LDS_MAX + 1) == LDS_KERNEL.encode(), c
    assert 1 << 20 > LDS_MAX and k(20, 1 << 32) == GLOBAL_KERNEL.encode() and k(20, LDS_MAX) == LDS_KERNEL.encode()
    assert semi_join_kernel(9, 512) == LDS_KERNEL and semi_join_kernel(24, LDS_MAX + 1) == GLOBAL_KERNEL
    for bad in ((0, 5), (33, 5), (9, (1 << 32) + 1), (9, -1), (9, (1 << 64) + 3)):
        with pytest.raises(ValueError):
            semi_join_kernel(*bad)


def test_width_cases_reach_both_tiers(L):
    """(no device needed) what test_every_width runs launches both families, the second one at every width that has it"""
    fam = {(c, m): L.mi355_semijoin_kernel(c, m).decode() for c, m in WIDTH_CASES}
    assert {c for (c, m), f in fam.items() if f == LDS_KERNEL} == set(range(1, 33))
    assert {c for (c, m), f in fam.items() if f == GLOBAL_KERNEL} == set(range(20, 33))
    assert fam[(20, 1 << 19)] == LDS_KERNEL and fam[(32, 1 << 19)] == LDS_KERNEL


def test_semi_join_wrapper_passes_what_the_abi_takes(fake):
    import torch

    eng, rec, col = fake
    fact = col(17, 777)
    sset = torch.zeros(512, dtype=torch.uint8)
    mask = torch.zeros(128, dtype=torch.uint8)
    out = torch.zeros(98, dtype=torch.uint8)
    bitmap, hits = eng.semi_join(fact, sset, 4001, negate=True, and_mask=mask, bitmap=out)
    (name, a), = rec.calls
    assert name == "mi355_semijoin_dev" and bitmap is out and hits.dtype == torch.int64 and hits.numel() == 1
    assert a[1:] == [fact.data.data_ptr(), 777, 17, sset.data_ptr(), 4001, 1, mask.data_ptr(), out.data_ptr(), hits.data_ptr()]
    rec.calls.clear()
    bitmap, hits = eng.semi_join(fact, sset, 4096)  # defaults: IN, no mask, a fresh bitmap of ceil(n/8) bytes, a count
    (name, a), = rec.calls
    assert a[1:7] == [fact.data.data_ptr(), 777, 17, sset.data_ptr(), 4096, 0] and a[7] is None
    assert bitmap.dtype == torch.uint8 and bitmap.numel() == 98 and a[8] == bitmap.data_ptr() and a[9] == hits.data_ptr()
    rec.calls.clear()
    bitmap, hits = eng.semi_join(fact, sset, 4096, bitmap=False)  # count only: no bitmap pointer reaches the ABI
    (name, a), = rec.calls
    assert bitmap is None and a[8] is None and a[9] == hits.data_ptr()
    rec.calls.clear()
    bitmap, hits = eng.semi_join(fact, sset, 4096, want_hits=False)
    (name, a), = rec.calls
    assert hits is None and a[9] is None and a[8] == bitmap.data_ptr()
    rec.calls.clear()
    bitmap, hits = eng.semi_join(fact, None, 0, negate=True)  # the empty set needs no buffer
    (name, a), = rec.calls
    assert a[4] is None and a[5] == 0 and a[6] == 1
    rec.calls.clear()
    huge = types.SimpleNamespace(dtype=torch.uint8, numel=lambda: 1 << 29, data_ptr=lambda: 1 << 20)  # 512 MiB, never touched
    eng.semi_join(col(32, 5), huge, 1 << 32)  # 2^32 does not wrap to 0 on the way
    assert rec.calls[0][1][4:6] == [1 << 20, 1 << 32]
    rec.calls.clear()
    for bad in (-1, (1 << 32) + 1, 1 << 64):
        with pytest.raises(ValueError):
            eng.semi_join(fact, sset, bad)
    with pytest.raises(AssertionError):
        eng.semi_join(fact, sset, 512 * 8 + 1)  # the set's tensor is shorter than ceil(set_bits / 8)
    with pytest.raises(AssertionError):
        eng.semi_join(fact, None, 5)
    with pytest.raises(AssertionError):
        eng.semi_join(fact, sset, 100, bitmap=False, want_hits=False)
    assert rec.calls == []


def test_semijoin_entry_point_fails_loudly_without_a_gpu(L):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    buf = (C.c_uint8 * 1024)()
    out = (C.c_uint8 * 1024)()
    hits = (C.c_uint64 * 1)()
    rc = L.mi355_semijoin_dev(None, buf, 100, 9, buf, 512, 0, None, out, hits)
    assert rc != 0 and L.mi355_last_error()


def test_every_semijoin_kernel_has_a_case():
    """every __global__ under csrc/semijoin/ is asserted from the launch record by a GPU case of this file, and the file names
    no kernel that does not exist"""
    kernels = support.global_kernels_of("semijoin")
    assert kernels == {LDS_KERNEL, GLOBAL_KERNEL}, kernels
    support.check_gpu_part_asserts(__file__, "LDS_KERNEL", "GLOBAL_KERNEL")


def test_semijoin_sources_read_no_flag_bits():
    support.check_sources_read_no_flag_bits("semijoin")


def test_header_limit_is_the_kernels(L):
    """the macro, the introspection call and the budget the header describes agree: 160 KiB minus four 16 KiB tiles, four 1 KiB
    mask images and 64 bytes, in whole 16 bytes"""
    assert LDS_MAX == 8 * ((160 * 1024 - 4 * (16384 + 1024) - 64) // 16 * 16)
    assert L.mi355_semijoin_kernel(32, LDS_MAX) == LDS_KERNEL.encode() and L.mi355_semijoin_kernel(32, LDS_MAX + 1) == GLOBAL_KERNEL.encode()


def gpu_shapes():
    """every (c, m, n) the GPU tests below run on recipe data"""
    shapes = {(c, m, n) for c, m in SIZE_CASES for n in SIZES}
    shapes |= {(c, m, N_BIG) for c, m in WIDTH_CASES + SET_SIZE_CASES + HOSTILE_CASES + MASK_CASES}
    shapes |= {(c, m, N_VIEW) for c, m in VIEW_CASES}
    shapes |= {ERROR_CASE}
    return sorted(shapes)


@pytest.mark.parametrize("shape", [s for s in gpu_shapes() if s[2] >= 13], ids=pid)
def test_recipe_is_not_vacuous(shape):
    """(no device needed) what every case must exercise.  `reach` = min(m, 2^c) stands for m where the issue says m - 1: no
    c-bit value addresses a bit beyond it (c = 5, m = 1000).  n = 1 holds one row and is left out."""
    c, m, n = shape
    vals, bits = data(c, m, n)
    v = vals.astype(np.int64)
    reach, top = reach_of(c, m), (1 << c) - 1
    assert len(bits) == m and reach >= 1
    res = expect(vals, bits, m)
    assert res.any() and not res.all(), "the expected bitmap is constant"
    if m < 1 << c:
        assert (v >= m).any(), "no row beyond the set"
        assert (v == m).any() and not res[v == m].any(), "a value equal to m must exist and miss"
    assert (v == 0).any() and (v == reach - 1).any(), "no row addresses bit 0 / bit reach - 1"
    last_byte = (reach - 1) // 8
    assert ((v < reach) & (v // 8 == last_byte)).any(), "no row addresses the set's last byte"
    assert res[v == reach - 1].all(), "bit reach - 1 is set: its rows hit"
    if reach >= 2:
        tail = bits[max(reach - 8, 0):reach]
        assert tail.any() and not tail.all(), "the last eight reachable bits are constant"
    # the corner values sit at fixed rows of the first tile, the last full tile and the ragged tail
    corners = [0, reach - 1, min(m, top), top]
    groups = corner_rows(c, n)
    t = tile_rows(c)
    assert groups[0][0] == 0
    if n >= t:
        assert any(rows[-1] == n // t * t - 1 for rows in groups), "no corner rows in the last full tile"
    if n % t >= 4 and n > 4:
        assert groups[-1][-1] == n - 1 and groups[-1][0] >= n // t * t, "no corner rows in the ragged tail"
    for rows in groups:
        assert [int(v[r]) for r in rows] == corners[:len(rows)], rows
    # under a mask some row is in the set but masked off, and some row survives
    for negate in (False, True):
        mb = mask_recipe(vals, bits, m, negate)
        sel = expect(vals, bits, m, negate)
        assert (sel & ~mb).any() and (sel & mb).any(), negate


@pytest.mark.parametrize("shape", [s for s in gpu_shapes() if s[2] < 13], ids=pid)
def test_one_row_shapes_see_both_results(shape):
    """(no device needed) n = 1 holds one row, value 0: it cannot carry the properties above, but the two runs every such shape
    gets (IN and NOT IN) expect a one and a zero between them, and the row addresses bit 0 of the set"""
    c, m, n = shape
    assert n == 1
    vals, bits = data(c, m, n)
    assert int(vals[0]) == 0 and m >= 1
    assert bool(expect(vals, bits, m)[0]) == bool(bits[0]) and bool(expect(vals, bits, m, negate=True)[0]) != bool(bits[0])


def test_star_join_data_is_not_vacuous():
    attr, fk, group, value = star_data()
    m = STAR_M
    f = fk.astype(np.int64)
    sel = star_selection(attr, fk, m)
    assert (f >= m).any(), "no foreign key beyond the dimension table"
    assert (attr == 3).any() and (attr != 3).any()
    assert sel.any() and not sel.all()
    assert (sel[f < m]).any() and (~sel[f < m]).any(), "inside the table both outcomes occur"
    assert not sel[f >= m].any()
    assert len(np.unique(group[sel])) >= 2 and len(np.unique(group[sel])) <= 64
    assert (np.bincount(group[sel], minlength=64) == 0).sum() < 64


@pytest.mark.parametrize("case", CAPTURE_CASES, ids=pid)
def test_capture_data_is_not_vacuous(case):
    c, m = case
    fk, attrs = capture_data(c, m)
    f = fk.astype(np.int64)
    assert (f >= m).any() and (f == m).any() and (f == m - 1).any() and (f == 0).any()
    sels = [star_selection(a, fk, m) for a in attrs]
    for sel in sels:
        assert sel.any() and not sel.all() and not sel[f >= m].any()
    assert (sels[0] != sels[1]).any(), "a stale result could pass"
    assert sels[0][0] and not sels[1][0], "row 0 (key 0) flips between the versions"
    assert (L_family(c, m) == LDS_KERNEL) == (reach_of(c, m) <= LDS_MAX)


def L_family(c, m):
    from shared_simd_scan_amd import semi_join_kernel

    return semi_join_kernel(c, m)


def test_empty_set_expectation():
    vals, bits = data(24, 0, N_BIG)
    assert len(bits) == 0 and not expect(vals, bits, 0).any() and expect(vals, bits, 0, negate=True).all()


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

def family(L, c, m):
    return L.mi355_semijoin_kernel(c, m).decode()


class Join:
    """one engine, an uploaded column and set, a guarded bitmap that is refilled with 0xEE before every call"""

    def __init__(self, O, eng, c, m, n, vals=None, bits=None):
        import torch

        from shared_simd_scan_amd.engine import PackedColumn

        self.eng, self.c, self.m, self.n = eng, c, m, n
        if vals is None:
            vals, bits = data(c, m, n)
        self.vals, self.bits = vals, bits
        self.col = PackedColumn(upload(O, vals, c), n, c)
        self.set = torch.from_numpy(packbits(bits)).cuda() if m else None
        self.nbytes = (n + 7) // 8
        self.out = Guarded(self.nbytes)

    def out_view(self):
        return self.out.t[self.out.front: self.out.front + self.nbytes]

    def run(self, negate=False, mask_bits=None, mask=None, in_place=False, count_only=False, what=""):
        """-> checks every byte of the bitmap, the guards, the count and the inputs against numpy; returns the expectation"""
        import torch

        tag = (what, self.c, self.m, self.n, negate)
        want = expect(self.vals, self.bits, self.m, negate, mask_bits)
        self.out.t.fill_(SENTINEL)
        if mask_bits is not None and mask is None and not in_place:
            mask = torch.from_numpy(packbits(mask_bits)).cuda()
        if in_place:
            mask = self.out_view()
            mask.copy_(torch.from_numpy(packbits(mask_bits)).cuda())
        col_before = self.col.data.clone()
        set_before = self.set.clone() if self.set is not None else None
        mask_before = mask.clone() if mask is not None and not in_place else None
        bitmap, hits = self.eng.semi_join(self.col, self.set, self.m, negate=negate, and_mask=mask,
                                          bitmap=False if count_only else self.out_view())
        self.eng.synchronize()
        have = self.out.fetch()  # asserts the guard bytes on both sides
        assert int(hits.item()) == int(want.sum()), (tag, "hits", int(hits.item()), "want", int(want.sum()))
        if count_only:
            assert bitmap is None and (in_place or (have == SENTINEL).all()), (tag, "a count-only call stored something")
        else:
            assert bitmap.data_ptr() == self.out_view().data_ptr()
            wb = packbits(want)
            bad = np.nonzero(have != wb)[0]
            assert bad.size == 0, (tag, "byte", int(bad[0]), "of", self.nbytes, "have", int(have[bad[0]]), "want", int(wb[bad[0]]))
        assert torch.equal(self.col.data, col_before), (tag, "column written")
        if set_before is not None:
            assert torch.equal(self.set, set_before), (tag, "set written")
        if mask_before is not None:
            assert torch.equal(mask, mask_before), (tag, "mask written")
        return want


@gpu
@pytest.mark.parametrize("case", SIZE_CASES, ids=pid)
def test_sizes_and_tails(L, O, eng, case):
    c, m = case
    for n in SIZES:
        join = Join(O, eng, c, m, n)
        join.run()
        (label, grid, lds, flags), = record(L, eng)
        assert base_name(label) == LDS_KERNEL and label.startswith(f"{LDS_KERNEL}<{c},") and flags == 0 and lds >= (reach_of(c, m) + 7) // 8, label
        join.run(negate=True)
        if n != N_BIG:
            continue
        # one block: its four waves walk several tiles each -- prefetch, deferred stores, the ragged tail
        eng.set_option("grid_cus", 1)
        eng.set_option("max_blocks_per_cu", 1)
        try:
            join.run(what="capped")
            join.run(negate=True, mask_bits=mask_recipe(join.vals, join.bits, m, True), what="capped, masked")
            (label, grid, lds, flags), = record(L, eng)
            assert grid == 1 and base_name(label) == LDS_KERNEL and flags == 0
        finally:
            eng.set_option("grid_cus", 0)
            eng.set_option("max_blocks_per_cu", 0)


@gpu
@pytest.mark.parametrize("case", WIDTH_CASES, ids=pid)
def test_every_width(L, O, eng, case):
    c, m = case
    join = Join(O, eng, c, m, N_BIG)
    join.run()
    (label, grid, lds, flags), = record(L, eng)
    want_family = LDS_KERNEL if reach_of(c, m) <= LDS_MAX else GLOBAL_KERNEL
    assert base_name(label) == want_family == family(L, c, m) and label.startswith(f"{want_family}<{c},") and flags == 0, label
    join.run(negate=True, mask_bits=mask_recipe(join.vals, join.bits, m, True), what="masked NOT IN")
    if want_family == GLOBAL_KERNEL:
        eng.set_option("grid_cus", 1)
        eng.set_option("max_blocks_per_cu", 1)
        try:
            join.run(what="capped")
            (label, grid, lds, flags), = record(L, eng)
            assert grid == 1 and base_name(label) == GLOBAL_KERNEL and lds == 0
        finally:
            eng.set_option("grid_cus", 0)
            eng.set_option("max_blocks_per_cu", 0)


@gpu
@pytest.mark.parametrize("case", SET_SIZE_CASES, ids=pid)
def test_set_sizes(L, O, eng, case):
    c, m = case
    join = Join(O, eng, c, m, N_BIG)
    want = join.run()
    (label, grid, lds, flags), = record(L, eng)
    # the tier switches between LDS_MAX and LDS_MAX + 1 reachable bits, and nowhere else
    assert base_name(label) == (LDS_KERNEL if reach_of(c, m) <= LDS_MAX else GLOBAL_KERNEL), (label, m)
    if m in (LDS_MAX - 1, LDS_MAX):
        assert base_name(label) == LDS_KERNEL and lds >= m // 8
    if m == LDS_MAX + 1:
        assert base_name(label) == GLOBAL_KERNEL and lds == 0
    if m > 1 << c:
        assert not want[join.vals.astype(np.int64) >= 1 << c].any()
    join.run(negate=True)


@gpu
@pytest.mark.parametrize("with_buffer", [False, True], ids=["null", "buffer"])
def test_empty_set(L, O, eng, with_buffer):
    import torch

    c, n = 24, N_BIG
    vals, bits = data(c, 0, n)
    join = Join(O, eng, c, 0, n)
    if with_buffer:
        join.set = torch.full((64,), 0xFF, dtype=torch.uint8, device="cuda")  # set_bits == 0: not one bit of it counts
    assert not join.run(what="empty").any()
    (label, _, _, _), = record(L, eng)
    assert base_name(label) == LDS_KERNEL
    assert join.run(negate=True, what="empty, NOT IN").all()
    mb = np.random.default_rng(3).random(n) < 0.5
    assert (join.run(negate=True, mask_bits=mb, what="empty, NOT IN, masked") == mb).all()
    assert not join.run(mask_bits=mb, what="empty, masked").any()


@gpu
@pytest.mark.parametrize("case", HOSTILE_CASES, ids=pid)
def test_hostile_set_surroundings(L, O, eng, case):
    """the set is a view at a 4-byte-aligned, not 16-byte-aligned offset inside a buffer of 0xff; the bits >= m of its last byte
    are ones: neither they nor anything around the set may reach a result (a value equal to m misses)"""
    import torch

    c, m = case
    n = N_BIG
    join = Join(O, eng, c, m, n)
    sb = packbits(join.bits).copy()
    if m % 8:
        sb[-1] |= (0xFF << (m % 8)) & 0xFF
    for offset in (4, 12, 8):
        buf = torch.full((offset + len(sb) + 256,), 0xFF, dtype=torch.uint8, device="cuda")
        base = (-buf.data_ptr()) % 16  # make the view's address = offset mod 16 whatever the allocation's is
        buf = buf[base:]
        buf[offset: offset + len(sb)] = torch.from_numpy(sb).cuda()
        join.set = buf[offset: offset + len(sb)]
        assert join.set.data_ptr() % 16 == offset
        want = join.run(what=f"set at +{offset}")
        (label, _, _, _), = record(L, eng)
        assert base_name(label) == (LDS_KERNEL if m <= LDS_MAX else GLOBAL_KERNEL)
        at_m = join.vals.astype(np.int64) == m
        assert at_m.any() and not want[at_m].any()
        join.run(negate=True, what=f"set at +{offset}, NOT IN")
        assert (buf[:offset] == 0xFF).all() and (buf[offset + len(sb):] == 0xFF).all()


@gpu
@pytest.mark.parametrize("case", MASK_CASES, ids=pid)
def test_masks_negate_in_place_count_only(L, O, eng, case):
    c, m = case
    n = N_BIG
    assert n % tile_rows(c) and n % 8
    join = Join(O, eng, c, m, n)
    fam = LDS_KERNEL if reach_of(c, m) <= LDS_MAX else GLOBAL_KERNEL
    for negate in (False, True):
        mb = mask_recipe(join.vals, join.bits, m, negate)
        want = join.run(negate=negate, mask_bits=mb, what="and_mask")
        (label, _, _, _), = record(L, eng)
        assert base_name(label) == fam
        assert int(want.sum()) < int(expect(join.vals, join.bits, m, negate).sum())
        join.run(negate=negate, mask_bits=mb, in_place=True, what="and_mask is bitmap")
        # count only: the stored form's popcount, and not one byte written
        join.run(negate=negate, count_only=True, what="count only")
        join.run(negate=negate, mask_bits=mb, count_only=True, what="count only, masked")
    for density in (0.0, 1.0):
        join.run(mask_bits=np.full(n, bool(density)), what=f"mask density {density}")


@gpu
@pytest.mark.parametrize("case", VIEW_CASES, ids=pid)
def test_row_range_views(L, O, eng, case):
    """rows [8192, 8192 + n) of a longer column, followed by rows of all-ones values: the bitmap is written to exactly ceil(n/8)
    bytes inside its guards and nothing of the foreign rows reaches it or the count"""
    c, m = case
    n, lead, trail = N_VIEW, 8192, 4096
    assert n % 8 and lead % 128 == 0
    vals, bits = data(c, m, n)
    rng = np.random.default_rng([c, 13])
    top = (1 << c) - 1
    junk = rng.integers(0, top + 1, lead, dtype=np.uint64).astype(np.uint32)
    join = Join(O, eng, c, m, n)
    from shared_simd_scan_amd.engine import PackedColumn

    whole = PackedColumn(upload(O, np.concatenate([junk, vals, np.full(trail, top, dtype=np.uint32)]), c), lead + n + trail, c)
    join.col = eng.slice_rows(whole, lead, lead + n)
    assert join.col.n == n and join.col.data.data_ptr() % 16 == 0
    join.run(what="view")
    (label, _, _, _), = record(L, eng)
    assert base_name(label) == (LDS_KERNEL if reach_of(c, m) <= LDS_MAX else GLOBAL_KERNEL)
    join.run(negate=True, mask_bits=mask_recipe(vals, bits, m, True), what="view, masked NOT IN")  # NOT IN: rows behind would count
    join.run(negate=True, count_only=True, what="view, count only")


@gpu
def test_errors_launch_nothing(L, O, eng):
    import torch

    c, m, n = ERROR_CASE
    join = Join(O, eng, c, m, n)
    hits = Guarded(8)
    mask = Guarded((n + 7) // 8)
    big = Guarded(4096)  # a buffer that can stand for set and bitmap at once
    cp, sp = join.col.data.data_ptr(), join.set.data_ptr()

    def call(cp=cp, n=n, c=c, sp=sp, m=m, negate=0, mask_ptr=None, out=join.out.ptr.value, hp=hits.ptr.value):
        for g in (join.out, hits, mask, big):
            g.t.fill_(SENTINEL)
        rc = L.mi355_semijoin_dev(eng._ctx, cp, n, c, sp, m, negate, mask_ptr, out, hp)
        eng.synchronize()
        return rc

    assert call() == 0 and record(L, eng) and base_name(record(L, eng)[0][0]) == LDS_KERNEL
    valid = record(L, eng)
    errors = (("c = 0", dict(c=0), b"32"), ("c = 33", dict(c=33), b"32"), ("set_bits = 2^32 + 1", dict(m=(1 << 32) + 1), b"2^32"),
              ("null column", dict(cp=None), b"packed_dev"), ("null set", dict(sp=None), b"set_dev"),
              ("no output", dict(out=None, hp=None), b"both null"),
              ("column at +4", dict(cp=cp + 4), b"aligned"), ("set at +2", dict(sp=sp + 2), b"aligned"),
              ("bitmap at +4", dict(out=join.out.ptr.value + 4), b"aligned"), ("mask at +4", dict(mask_ptr=mask.ptr.value + 4), b"aligned"),
              ("hits at +4", dict(hp=hits.ptr.value + 4), b"aligned"),
              ("set is bitmap", dict(sp=big.ptr.value, out=big.ptr.value), b"overlaps"),
              ("set ends inside bitmap", dict(sp=big.ptr.value, m=8 * 64, out=big.ptr.value + 48), b"overlaps"),
              ("bitmap ends inside set", dict(sp=big.ptr.value + 512, m=8 * 1024, out=big.ptr.value), b"overlaps"))
    for what, kw, word in errors:
        assert call(**kw) == E_INVALID, what
        assert word in L.mi355_last_error(), (what, L.mi355_last_error())
        assert record(L, eng) == [], what  # a refused call leaves an empty record and launches nothing
        for g in (join.out, hits, mask, big):
            assert (g.fetch() == SENTINEL).all(), what
    # neighbours that do not overlap are fine: the set ends where the bitmap begins
    nb = (n + 7) // 8
    assert nb + 512 <= 4096
    big.t.fill_(SENTINEL)
    big.t[big.front: big.front + 512] = torch.from_numpy(np.resize(packbits(join.bits), 512)).cuda()
    rc = L.mi355_semijoin_dev(eng._ctx, cp, n, c, big.ptr.value, m, 0, None, big.ptr.value + 512, hits.ptr.value)
    eng.synchronize()
    assert rc == 0 and record(L, eng) == valid
    want = expect(join.vals, join.bits, m)
    assert (big.fetch()[512: 512 + nb] == packbits(want)).all() and (big.fetch()[512 + nb:] == SENTINEL).all()
    assert int(hits.fetch().view(np.uint64)[0]) == int(want.sum())
    # n == 0: a count of zero, nothing launched, nothing else written
    assert call(n=0, cp=None) == 0 and record(L, eng) == []
    assert int(hits.fetch().view(np.uint64)[0]) == 0 and (join.out.fetch() == SENTINEL).all()


@gpu
def test_star_join_chain(L, O, eng):
    """scan_where(dim) -> semi_join(fact.fk) -> group_aggregate, no host round trip: the dimension scan's bitmap is the set"""
    import torch

    from shared_simd_scan_amd.engine import PackedColumn

    m, n = STAR_M, STAR_N
    attr, fk, group, value = star_data()
    dim = PackedColumn(upload(O, attr, 5), m, 5)
    fact_fk = PackedColumn(upload(O, fk, 12), n, 12)
    gcol, vcol = PackedColumn(upload(O, group, 6), n, 6), PackedColumn(upload(O, value, 17), n, 17)
    dim_bitmap, dim_hits = eng.scan_where("==", 3, dim)
    bitmap, hits = eng.semi_join(fact_fk, dim_bitmap, m)
    (label, _, _, _), = record(L, eng)
    assert base_name(label) == LDS_KERNEL
    agg = eng.group_aggregate(gcol, vcol, mask=bitmap)
    eng.synchronize()
    sel = star_selection(attr, fk, m)
    assert int(dim_hits.item()) == int((attr == 3).sum())
    assert (bitmap.cpu().numpy() == packbits(sel)).all() and int(hits.item()) == int(sel.sum())
    want = np.zeros((64, 4), dtype=np.uint64)
    want[:, 2] = (1 << 64) - 1
    k, v = group[sel].astype(np.int64), value[sel].astype(np.uint64)
    np.add.at(want[:, 0], k, v)
    want[:, 1] = np.bincount(k, minlength=64).astype(np.uint64)
    np.minimum.at(want[:, 2], k, v)
    np.maximum.at(want[:, 3], k, v)
    assert (agg.cpu().numpy().view(np.uint64) == want).all()


@gpu
@pytest.mark.parametrize("case", CAPTURE_CASES, ids=pid)
def test_graph_capture_and_replay(O, case):
    """scan_where(dim) + semi_join in one graph, a linear chain on a side stream: after the dimension column's contents change
    the replay follows the new set"""
    import torch

    from shared_simd_scan_amd.engine import PackedColumn

    c, m = case
    n = N_BIG
    fam = LDS_KERNEL if reach_of(c, m) <= LDS_MAX else GLOBAL_KERNEL
    fk, attrs = capture_data(c, m)
    versions = [(O.pack(attr, 5), star_selection(attr, fk, m)) for attr in attrs]

    def steps(eng):
        stage = [torch.from_numpy(v[0]).cuda() for v in versions]
        dim = PackedColumn(torch.empty_like(stage[0]), m, 5)
        fact = PackedColumn(upload(O, fk, c), n, c)
        dim_bitmap = torch.empty((m + 7) // 8, dtype=torch.uint8, device="cuda")
        dim_hits = torch.empty(1, dtype=torch.int64, device="cuda")
        res = Guarded((n + 7) // 8)
        out = res.t[res.front: res.front + res.nbytes]
        hits_box = []

        def load(r):
            dim.data.copy_(stage[r])
            dim_bitmap.fill_(0xFF)
            res.t.fill_(SENTINEL)

        def run():
            eng.scan_where("==", 3, dim, bitmap=dim_bitmap, hits=dim_hits)
            hits_box[:] = [eng.semi_join(fact, dim_bitmap, m, bitmap=out)[1]]

        def check(r, what):
            want = versions[r][1]
            assert (res.fetch() == packbits(want)).all() and int(hits_box[0].item()) == int(want.sum()), what

        def untouched():  # (the hit count is allocated by the call: it has no state from before the capture)
            assert (res.fetch() == SENTINEL).all()

        def warmed(launched):
            assert base_name(launched[-1][0]) == fam

        return capture.Steps(load, run, check, untouched, warmed)

    capture.capture_replay(steps, (0, 1, 0))
