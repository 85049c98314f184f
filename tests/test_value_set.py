"""The set of values that occur in a packed column, as a bitmap over the value domain, and the members' ranks as a packed table
(include/mi355_distinct.h; ScanEngine.value_set, count_distinct, distinct_values, set_ranks, dense_codes).

CPU: the header is plain C99 and declares exactly what _capi.HEADERS binds for it and the library exports; it carries both of its
graph-capture verdicts; mi355_value_set_kernel (pure arithmetic) names the tier at every boundary; the engine's wrappers hand the
C ABI what they should (through a recording stand-in for the library); without a device the entry points fail with a message;
every __global__ under csrc/distinct/ is named by the launch record of a GPU case of this file; no source there reads a switch
bit; the data recipe is not vacuous.

GPU (-m gpu): every expectation is numpy on the values and masks the test generated -- np.unique of the selected rows, packed with
np.packbits(bitorder="little") -- and the oracle's packer on the way in; nothing is derived from engine output.  Every byte of the
set (the tail bits of its last byte included), both counts and the 0xFF guard bytes around the set are compared exactly.  Tiles
are 8192 rows at c <= 16 and 4096 above.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import capture
import support
from support import E_INVALID, SENTINEL, Guarded, L, base_name, eng, fake, header_macro, hostile_pack, packbits, record, upload  # noqa: F401  (L, eng, fake: fixtures)

HEADER = "mi355_distinct.h"

# the kernels of csrc/distinct/, as the launch record names them: the GPU cases below assert these labels
LDS_KERNEL = "value_set_lds_kernel"
GLOBAL_KERNEL = "value_set_global_kernel"
RANKS_KERNEL = "set_ranks_kernel"
PREFIX_KERNELS = ["rowid_count_kernel", "rowid_scan_kernel"]  # kernels/bitmap.hpp: the chunk prefix set_ranks borrows

LDS_MAX = header_macro(HEADER, "MI355_VALUE_SET_LDS_MAX_BITS")

K = 8192
N_BIG = K * 9 + 1237  # 74965: nine tiles of 8192 rows (eighteen of 4096) and a ragged one; not a multiple of 8
SIZES = [0, 1, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049, K, N_BIG]
SIZE_CASES = [(9, 512), (9, 300), (17, 100003), (24, LDS_MAX + 1), (32, 5000)]
STRADDLE = (1 << 24) + 5
# every width with its full domain where that fits the test's memory (c <= 24: a set of 2 MiB), beyond that a set the values
# straddle; and, so that the LDS tier's instantiation runs at every width too, the widths that reach the global tier also at 3001
WIDTH_CASES = [(c, 1 << c) for c in range(1, 25)] + [(c, STRADDLE) for c in range(25, 33)] + [(c, 3001) for c in range(20, 33)]
SET_SIZE_CASES = ([(24, m) for m in (0, 1, 7, 8, 9, 31, 32, 33, LDS_MAX, LDS_MAX + 1, (1 << 24) - 1, 1 << 24, (1 << 24) + 1)]
                  + [(12, m) for m in ((1 << 12) - 1, 1 << 12, (1 << 12) + 1)] + [(5, 1000)])
HUGE_CASE = (32, 1 << 32)
ACCUMULATE_CASES = [(12, 3001), (24, LDS_MAX + 9)]  # one per tier; neither a multiple of 8
CONTENTION_CASES = [(12, 1 << 12), (24, 1 << 24)]
MASK_CASES = [(9, 300), (24, LDS_MAX + 1)]
VIEW_CASES = [(9, 300), (24, LDS_MAX + 1)]
N_VIEW = K * 2 + 509
ERROR_CASE = (9, 300, 4096 + 77)
RANK_WIDTHS = [1, 7, 8, 9, 16, 17, 31, 32]
M_RANKS = 16384 * 5 + 77                # six chunks of the set, the last ragged, not a multiple of 8
M_RANKS_GROUPS = (1 << 24) + 16384 * 3 + 77  # two scan groups of 1024 chunks
CAPTURE_CASE = (17, 12)  # (column width, table width)

gpu = pytest.mark.gpu


def pid(p):
    return "-".join(str(x) for x in p)


def reach_of(c, m):
    """what a c-bit value can address of an m-bit set"""
    return min(m, 1 << c)


def tier_of(c, m):
    return LDS_KERNEL if reach_of(c, m) <= LDS_MAX else GLOBAL_KERNEL


def tile_rows(c):
    return K if c <= 16 else 4096


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


def lonely_value(c, m):
    """the value that only masked-out rows carry under mask "lonely" (reach >= 8: apart from every corner value)"""
    reach = reach_of(c, m)
    return reach // 2 if reach >= 8 else None


@functools.lru_cache(maxsize=None)
def data(c, m, n, salt=0):
    """the data recipe -> values uint32[n], read-only.  Half of the rows uniform below reach = min(m, 2^c), half uniform over
    [0, min(2^c, m + m / 8 + 8)) -- values that straddle the set's end --, then the corner values 0, reach - 1, m (clamped to
    2^c - 1) and 2^c - 1 at corner_rows(), and lonely_value() at rows 5 and n - 6 (n >= 16)."""
    rng = np.random.default_rng([c, m % (1 << 31), m >> 31, n, salt])
    top = (1 << c) - 1
    reach = reach_of(c, m)
    vals = rng.integers(0, min(top + 1, m + m // 8 + 8), n, dtype=np.uint64)
    if reach:
        low = rng.random(n) < 0.5
        vals[low] = rng.integers(0, reach, int(low.sum()), dtype=np.uint64)
    lone = lonely_value(c, m)
    if lone is not None:
        vals[vals == lone] = lone - 1
        if n >= 16:
            vals[5] = vals[n - 6] = lone
    corners = [0, max(reach - 1, 0), min(m, top), top]
    for rows in corner_rows(c, n):
        for r, v in zip(rows, corners):
            vals[r] = v
    vals = vals.astype(np.uint32)
    vals.setflags(write=False)
    return vals


def mask_recipe(kind, vals, c, m):
    """-> bool[n] (None for kind "none"): "zero", "one", "eighth" (a coin of 1/8 per row), "lonely" (a coin of 1/2, then every row
    that carries lonely_value() off: a value that alone masked-out rows carry must not reach the set)"""
    n = len(vals)
    rng = np.random.default_rng([n, c, m % (1 << 31), 77])
    if kind == "none":
        return None
    if kind == "zero":
        return np.zeros(n, dtype=bool)
    if kind == "one":
        return np.ones(n, dtype=bool)
    if kind == "eighth":
        return rng.random(n) < 0.125
    assert kind == "lonely"
    mb = rng.random(n) < 0.5
    mb[vals == lonely_value(c, m)] = False
    return mb


def set_bytes_of(members, m):
    """the members (unique values below m) as the bytes of an m-bit set: np.packbits(bitorder="little") of the bit vector,
    built byte-wise so that a 2^32-bit set costs its 512 MiB and no more"""
    out = np.zeros((m + 7) // 8, dtype=np.uint8)
    u = members.astype(np.uint64)
    np.bitwise_or.at(out, (u >> np.uint64(3)).astype(np.int64), (np.uint64(1) << (u & np.uint64(7))).astype(np.uint8))
    return out


def expect(vals, m, mask_bits=None):
    """-> (the set's ceil(m/8) bytes, distinct qualifying values, selected rows beyond the set)"""
    v = vals.astype(np.int64) if mask_bits is None else vals[mask_bits].astype(np.int64)
    members = np.unique(v[v < m])
    return set_bytes_of(members, m), len(members), int((v >= m).sum())


def rank_table(bits, ct, miss):
    """-> uint32[m]: the rank of every member among the members where it fits ct bits, else miss; miss for a clear bit"""
    ranks = np.cumsum(bits, dtype=np.int64) - bits
    fits = bits & (ranks < (1 << ct))
    return np.where(fits, ranks, miss).astype(np.uint32), int(bits.sum()), int((bits & ~fits).sum())


@functools.lru_cache(maxsize=None)
def rank_set(kind, m):
    rng = np.random.default_rng([m % (1 << 31), 5])
    bits = {"empty": np.zeros(m, dtype=bool), "full": np.ones(m, dtype=bool), "random": rng.random(m) < 0.5}.get(kind)
    if kind == "first":
        bits = np.zeros(m, dtype=bool)
        bits[0] = True
    if kind == "last":
        bits = np.zeros(m, dtype=bool)
        bits[m - 1] = True
    bits.setflags(write=False)
    return bits


@functools.lru_cache(maxsize=None)
def sparse_keys(n=N_BIG, distinct=300):
    """a sparse 32-bit key column: `distinct` keys spread over the whole domain, 0 and 2^32 - 1 among them -> (keys, values at 17 bits)"""
    rng = np.random.default_rng(4242)
    domain = np.unique(np.concatenate([rng.integers(0, 1 << 32, distinct - 2, dtype=np.uint64), np.array([0, (1 << 32) - 1], dtype=np.uint64)]))
    keys = domain[rng.integers(0, len(domain), n)].astype(np.uint32)
    keys[:len(domain)] = domain.astype(np.uint32)
    values = rng.integers(0, 1 << 17, n, dtype=np.uint64).astype(np.uint32)
    for a in (keys, values):
        a.setflags(write=False)
    return keys, values


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------

def test_distinct_header_is_plain_c99():
    support.check_header_is_plain_c99(HEADER)


def test_distinct_header_declares_what_python_binds(L):
    names, sigs = support.check_header_binds(L, HEADER)
    assert names == ["mi355_set_ranks_dev", "mi355_value_set_dev", "mi355_value_set_kernel"]
    sig = sigs["mi355_value_set_dev"]
    assert sig[2] is C.c_uint64 and sig[3] is C.c_uint and sig[6] is C.c_uint64 and sig[7] is C.c_int and len(sig) == 9
    assert sigs["mi355_value_set_kernel"] == [C.c_uint, C.c_uint64] and L.mi355_value_set_kernel.restype is C.c_char_p
    sig = sigs["mi355_set_ranks_dev"]
    assert sig[2] is C.c_uint64 and sig[3] is C.c_uint and sig[4] is C.c_uint32 and len(sig) == 7
    assert "mi355_scan.h" in support.header_text(HEADER) and support.header_text(HEADER).count("#include") == 1


def test_distinct_header_carries_its_capture_verdicts():
    support.check_capture_verdict(HEADER, r"graph capture: capturable -- whatever its arguments", r"graph capture: capturable after a warm-up call")
    text = support.header_text(HEADER)
    value_set_doc, set_ranks_doc = text[:text.index("mi355_value_set_dev(")], text[text.index("mi355_value_set_kernel(unsigned"):]
    assert "read at every replay" in value_set_doc and "read at every replay" in set_ranks_doc
    for section in ("set ", "rows ", "outputs ", "kernels ", "errors ", "stream ", "record ", "graph capture:"):
        assert f" *   {section}" in text, section


def test_kernel_choice_at_the_boundaries(L):
    """mi355_value_set_kernel needs neither a device nor a context; the tier follows min(set_bits, 2^c)"""
    from shared_simd_scan_amd import value_set_kernel

    k = L.mi355_value_set_kernel
    lds, glob = LDS_KERNEL.encode(), GLOBAL_KERNEL.encode()
    assert 1 << 16 <= LDS_MAX <= 753152
    for c in (24, 32):
        assert [k(c, m) for m in (0, 1, LDS_MAX)] == [lds] * 3, c
        assert k(c, LDS_MAX + 1) == glob and k(c, 1 << 32) == glob, c
        assert k(c, (1 << 32) + 1) is None, c
    for m in (0, 1, 3001, 1 << 32):
        assert k(0, m) is None and k(33, m) is None, m
    # a narrow column reaches only the first 2^c bits, however large the set is: set_bits larger and smaller than 2^c
    for c in range(1, 33):
        full = lds if 1 << c <= LDS_MAX else glob
        assert k(c, 1 << c) == full and k(c, min((1 << c) + 1, 1 << 32)) == full and k(c, 1 << 32) == full, c
        assert k(c, max((1 << c) - 1, 0)) == (lds if (1 << c) - 1 <= LDS_MAX else glob), c
        assert k(c, min(1 << c, LDS_MAX)) == lds, c
    assert k(16, 1 << 32) == lds, "a 16-bit column stays in LDS with its full domain"
    assert k(17, 1 << 32) == (lds if 1 << 17 <= LDS_MAX else glob)
    first_global = LDS_MAX.bit_length()  # the narrowest width whose domain 2^c exceeds the limit
    assert 1 << first_global > LDS_MAX >= 1 << (first_global - 1)
    assert k(first_global, LDS_MAX + 1) == glob and k(first_global, LDS_MAX) == lds
    assert value_set_kernel(9, 512) == LDS_KERNEL and value_set_kernel(32, LDS_MAX + 1) == GLOBAL_KERNEL
    for bad in ((0, 5), (33, 5), (9, (1 << 32) + 1), (9, -1), (9, (1 << 64) + 3)):
        with pytest.raises(ValueError):
            value_set_kernel(*bad)


def test_width_cases_reach_both_tiers(L):
    """(no device needed) what test_every_width runs launches the LDS tier at every width and the global tier at every width that has it"""
    fam = {(c, m): L.mi355_value_set_kernel(c, m).decode() for c, m in WIDTH_CASES}
    assert {c for (c, m), f in fam.items() if f == LDS_KERNEL} == set(range(1, 33))
    has_global = {c for c in range(1, 33) if 1 << c > LDS_MAX}
    assert {c for (c, m), f in fam.items() if f == GLOBAL_KERNEL} == has_global and has_global
    assert {tier_of(c, m) for c, m in SIZE_CASES} == {LDS_KERNEL, GLOBAL_KERNEL}


def test_value_set_wrapper_passes_what_the_abi_takes(fake):
    import torch

    eng, rec, col = fake
    fact = col(17, 777)
    mask = torch.zeros(128, dtype=torch.uint8)
    vset, counts = eng.value_set(fact)  # defaults: the whole domain, no mask, a fresh set, overwrite
    (name, a), = rec.calls
    assert name == "mi355_value_set_dev" and counts.dtype == torch.int64 and counts.numel() == 2
    assert a[1:] == [fact.data.data_ptr(), 777, 17, None, vset.data_ptr(), 1 << 17, 0, counts.data_ptr()]
    assert vset.dtype == torch.uint8 and vset.numel() == (1 << 17) // 8 + 32  # scan_output_buffer_size
    rec.calls.clear()
    out = torch.zeros(512, dtype=torch.uint8)
    mine = torch.zeros(2, dtype=torch.int64)
    vset, counts = eng.value_set(fact, 4001, mask=mask, out=out, accumulate=True, counts=mine)
    (name, a), = rec.calls
    assert vset is out and counts is mine
    assert a[1:] == [fact.data.data_ptr(), 777, 17, mask.data_ptr(), out.data_ptr(), 4001, 1, mine.data_ptr()]
    rec.calls.clear()
    eng.value_set(fact, 0)  # the empty set needs no buffer
    assert rec.calls[0][1][5:8] == [None, 0, 0]
    rec.calls.clear()
    eng.value_set(col(32, 5))  # 2^32 does not wrap to 0 on the way
    assert rec.calls[0][1][6] == 1 << 32
    rec.calls.clear()
    for bad in (-1, (1 << 32) + 1, 1 << 64):
        with pytest.raises(ValueError):
            eng.value_set(fact, bad)
    with pytest.raises(AssertionError):
        eng.value_set(fact, 512 * 8 + 1, out=out)  # the set's tensor is shorter than the dwords of set_bits
    with pytest.raises(AssertionError):
        eng.value_set(fact, 100, accumulate=True)  # nothing to accumulate into
    assert rec.calls == []


def test_set_ranks_and_dense_codes_wrappers(fake):
    import torch

    eng, rec, col = fake
    sset = torch.zeros(512, dtype=torch.uint8)
    table, counts = eng.set_ranks(sset, 4001, 12, miss=7)
    (name, a), = rec.calls
    assert name == "mi355_set_ranks_dev" and (table.n, table.c) == (4001, 12) and counts.numel() == 2
    assert a[1:] == [sset.data_ptr(), 4001, 12, 7, table.data.data_ptr(), counts.data_ptr()]
    assert table.data.numel() == (4001 * 12 + 7) // 8 + 256  # compressed_buffer_size: what lookup takes
    rec.calls.clear()
    eng.set_ranks(None, 0, 5)
    assert rec.calls[0][1][1:3] == [None, 0] and rec.calls[0][1][5] is None
    rec.calls.clear()
    for bad in (dict(ct=0), dict(ct=33), dict(ct=5, miss=32), dict(ct=5, miss=-1)):
        with pytest.raises(ValueError):
            eng.set_ranks(sset, 100, **bad)
    with pytest.raises(ValueError):
        eng.set_ranks(sset, (1 << 32) + 1, 5)
    with pytest.raises(AssertionError):
        eng.set_ranks(sset, 512 * 8 + 1, 5)
    assert rec.calls == []
    # dense_codes: value_set over the whole domain -> set_ranks -> lookup, then the values; with ct given nothing is read back
    fact = col(13, 777)
    mask = torch.zeros(128, dtype=torch.uint8)
    codes, values, count = eng.dense_codes(fact, ct=6, mask=mask, miss=63)
    assert [name for name, _ in rec.calls] == ["mi355_value_set_dev", "mi355_set_ranks_dev", "mi355_lookup_dev", "mi355_bitmap_to_rowids_dev"]
    vs, sr, lk, ids = (a for _, a in rec.calls)
    assert vs[1:5] == [fact.data.data_ptr(), 777, 13, mask.data_ptr()] and vs[6:8] == [1 << 13, 0]
    assert sr[1] == vs[5] and sr[2:5] == [1 << 13, 6, 63]  # the set value_set wrote, ranked at ct bits
    assert lk[1:4] == [fact.data.data_ptr(), 777, 13] and lk[4] == sr[5] and lk[5:8] == [1 << 13, 6, 63] and lk[8] == codes.data.data_ptr()
    assert (codes.n, codes.c) == (777, 6)
    assert ids[1] == vs[5] and ids[2] == 1 << 13 and ids[4] == values.data_ptr() and ids[5] == 777 and values.numel() == 777
    rec.calls.clear()
    values, count = eng.distinct_values(fact, capacity=50)
    assert [name for name, _ in rec.calls] == ["mi355_value_set_dev", "mi355_bitmap_to_rowids_dev"]
    assert rec.calls[1][1][1] == rec.calls[0][1][5] and rec.calls[1][1][2] == 1 << 13 and rec.calls[1][1][5] == 50


def test_distinct_entry_points_fail_loudly_without_a_gpu(L):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    buf = (C.c_uint8 * 1024)()
    out = (C.c_uint8 * 4096)()
    cnt = (C.c_uint64 * 2)()
    assert L.mi355_value_set_dev(None, buf, 100, 9, None, out, 512, 0, cnt) != 0 and L.mi355_last_error()
    assert L.mi355_set_ranks_dev(None, buf, 512, 9, 0, out, cnt) != 0 and L.mi355_last_error()


def test_every_distinct_kernel_has_a_case():
    """every __global__ under csrc/distinct/ is asserted from the launch record by a GPU case of this file, and the file names
    no kernel that does not exist"""
    kernels = support.global_kernels_of("distinct")
    assert kernels == {LDS_KERNEL, GLOBAL_KERNEL, RANKS_KERNEL}, kernels
    support.check_gpu_part_asserts(__file__, "LDS_KERNEL", "GLOBAL_KERNEL", "RANKS_KERNEL")


def test_distinct_sources_read_no_flag_bits():
    support.check_sources_read_no_flag_bits("distinct")


def test_header_limit_is_what_the_function_switches_at(L):
    assert L.mi355_value_set_kernel(32, LDS_MAX) == LDS_KERNEL.encode() and L.mi355_value_set_kernel(32, LDS_MAX + 1) == GLOBAL_KERNEL.encode()
    assert 1 << 16 <= LDS_MAX <= header_macro("mi355_semijoin.h", "MI355_SEMIJOIN_LDS_MAX_BITS") == 753152


def gpu_shapes():
    """every (c, m, n) the GPU tests below run on recipe data"""
    shapes = {(c, m, n) for c, m in SIZE_CASES for n in SIZES}
    shapes |= {(c, m, N_BIG) for c, m in WIDTH_CASES + SET_SIZE_CASES + ACCUMULATE_CASES + MASK_CASES + [HUGE_CASE]}
    shapes |= {(c, m, N_VIEW) for c, m in VIEW_CASES}
    shapes |= {ERROR_CASE}
    return sorted(shapes)


@pytest.mark.parametrize("shape", [s for s in gpu_shapes() if s[2] >= 2 * K and s[1] >= 1], ids=pid)
def test_recipe_is_not_vacuous(shape):
    """(no device needed) what the cases of at least two tiles must exercise"""
    c, m, n = shape
    vals = data(c, m, n)
    v = vals.astype(np.int64)
    reach, top, t = reach_of(c, m), (1 << c) - 1, tile_rows(c)
    assert (v == reach - 1).any(), "no row carries the set's last reachable bit"
    if m < 1 << c:
        assert (v == m).any() and (v == m - 1).any(), "no value at set_bits - 1 and set_bits"
        assert (v >= m).any(), "no row beyond the set"
    sbytes, distinct, outside = expect(vals, m)
    assert distinct >= 1 and outside == int((v >= m).sum())
    if reach >= 64:
        assert 1 < distinct, "a constant column"
    # rows in the last full tile and in the ragged tail carry corner values, and the corners differ from the rest where they can
    groups = corner_rows(c, n)
    assert n % t >= 4 and any(rows[-1] == n // t * t - 1 for rows in groups) and groups[-1][-1] == n - 1
    corners = [0, max(reach - 1, 0), min(m, top), top]
    for rows in groups:
        assert [int(v[r]) for r in rows] == corners
    # masked-out rows that alone carry some value: the value is there, every row that carries it is off, and it is in no expectation
    lone = lonely_value(c, m)
    if (c, m) in MASK_CASES:
        assert lone is not None
        mb = mask_recipe("lonely", vals, c, m)
        assert (v == lone).sum() >= 2 and not mb[v == lone].any() and mb.any() and not mb.all()
        masked_bytes, masked_distinct, _ = expect(vals, m, mb)
        assert (sbytes[lone // 8] >> (lone % 8)) & 1 and not (masked_bytes[lone // 8] >> (lone % 8)) & 1
        eighth = mask_recipe("eighth", vals, c, m)
        assert 0 < eighth.sum() < n // 4
        assert mask_recipe("none", vals, c, m) is None and not mask_recipe("zero", vals, c, m).any() and mask_recipe("one", vals, c, m).all()


def test_rank_recipe_is_not_vacuous():
    assert M_RANKS % 8 and M_RANKS > 5 * 16384 and M_RANKS_GROUPS > 1024 * 16384 and M_RANKS_GROUPS % 8
    bits = rank_set("random", M_RANKS)
    for ct in RANK_WIDTHS:
        table, members, unfit = rank_table(bits, ct, (1 << ct) - 1)
        assert members == int(bits.sum()) > 16384
        assert (unfit > 0) == (ct < 16), ct  # rank overflow at the small widths, none at the wide ones
        assert unfit == max(members - (1 << ct), 0)
    assert rank_set("first", M_RANKS)[0] and rank_set("first", M_RANKS).sum() == 1
    assert rank_set("last", M_RANKS)[-1] and rank_set("last", M_RANKS).sum() == 1


def test_sparse_keys_are_sparse():
    keys, values = sparse_keys()
    u = np.unique(keys)
    assert 250 <= len(u) <= 300 and u[0] == 0 and u[-1] == (1 << 32) - 1 and np.diff(u.astype(np.int64)).min() > 1


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

GUARD = 256


class SetBuffer:
    """a set of m bits inside 0xFF guard bytes, itself pre-filled with 0xFF (or with `prefill` bytes)"""

    def __init__(self, m):
        import torch

        self.m, self.nbytes = m, (m + 7) // 8
        self.t = torch.empty(GUARD + self.nbytes + GUARD, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.view = self.t[GUARD:]  # whole dwords behind the set's last byte are writable: the guard

    def fill(self, prefill=None):
        import torch

        self.t.fill_(0xFF)
        if prefill is not None:
            self.t[GUARD: GUARD + self.nbytes] = torch.from_numpy(prefill).cuda()

    def fetch(self):
        h = self.t.cpu().numpy()
        assert (h[:GUARD] == 0xFF).all(), "guard in front of the set overwritten"
        tail = h[GUARD + self.nbytes:]
        assert (tail == 0xFF).all(), f"guard behind the set overwritten at +{int(np.argmax(tail != 0xFF))}"
        return h[GUARD: GUARD + self.nbytes]


def hostile_mask(mask_bits):
    """the mask's bytes with ones behind bit n, in a buffer of 0xFF -> device tensor (4-byte aligned)"""
    import torch

    n = len(mask_bits)
    mb = packbits(mask_bits).copy()
    if n % 8:
        mb[-1] |= (0xFF << (n % 8)) & 0xFF
    buf = torch.full((len(mb) + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    buf[:len(mb)] = torch.from_numpy(mb).cuda()
    return buf


class Column:
    """one engine and a column uploaded in hostile surroundings (support.hostile_pack)"""

    def __init__(self, O, eng, L, c, vals):
        from shared_simd_scan_amd.engine import PackedColumn

        self.eng, self.L, self.c, self.vals, self.n = eng, L, c, vals, len(vals)
        self.col = PackedColumn(hostile_pack(O, vals, c) if self.n else upload(O, np.zeros(1, dtype=np.uint32), c), self.n, c)
        self.buffers = {}

    def run(self, m, mask_bits=None, accumulate=None, what=""):
        """value_set into a guarded set pre-filled with 0xFF (accumulate: the bytes it holds before) -> checks every byte, the
        guards, both counts, the kernel and the inputs against numpy; returns (distinct, outside)"""
        import torch

        tag = (what, self.c, m, self.n)
        sbuf = self.buffers.setdefault(m, SetBuffer(m))
        sbuf.fill(accumulate)
        want, distinct, outside = expect(self.vals, m, mask_bits)
        if accumulate is not None:
            keep = accumulate.copy()
            fresh = int(np.unpackbits(want & ~keep).sum())
            want = want | keep  # bits >= m of the last byte are in `keep`: they stay as they were
        else:
            fresh = distinct
        mask = hostile_mask(mask_bits) if mask_bits is not None and self.n else None
        col_before = self.col.data.clone()
        counts = torch.full((2,), -7, dtype=torch.int64, device="cuda")
        vset, got = self.eng.value_set(self.col, m, mask=mask, out=sbuf.view, accumulate=accumulate is not None, counts=counts)
        self.eng.synchronize()
        have = sbuf.fetch()  # asserts the guard bytes on both sides
        bad = np.nonzero(have != want)[0]
        assert bad.size == 0, (tag, "byte", int(bad[0]), "of", len(want), "have", int(have[bad[0]]), "want", int(want[bad[0]]))
        assert got.tolist() == [fresh, outside], (tag, got.tolist(), [fresh, outside])
        assert torch.equal(self.col.data, col_before), (tag, "column written")
        rec = record(self.L, self.eng)
        if self.n:
            (label, grid, lds, flags), = rec
            assert base_name(label) == tier_of(self.c, m) and label == f"{tier_of(self.c, m)}<{self.c}>" and flags == 0, (tag, label)
            assert (lds >= (reach_of(self.c, m) + 31) // 32 * 4) if base_name(label) == LDS_KERNEL else lds == 0, (tag, lds)
        else:
            assert rec == [], tag
        return distinct, outside


class capped:
    """grid_cus = 1 and one block per CU: one block whose four waves walk every tile and which merges over itself"""

    def __init__(self, eng):
        self.eng = eng

    def __enter__(self):
        self.eng.set_option("grid_cus", 1)
        self.eng.set_option("max_blocks_per_cu", 1)

    def __exit__(self, *exc):
        self.eng.set_option("grid_cus", 0)
        self.eng.set_option("max_blocks_per_cu", 0)


@gpu
@pytest.mark.parametrize("case", SIZE_CASES, ids=pid)
def test_sizes_and_tails(L, O, eng, case):
    c, m = case
    for n in SIZES:
        col = Column(O, eng, L, c, data(c, m, n))
        default = col.run(m)
        if n:
            assert base_name(record(L, eng)[0][0]) in (LDS_KERNEL, GLOBAL_KERNEL)
        with capped(eng):
            assert col.run(m, what="capped") == default
            if n:
                (label, grid, lds, flags), = record(L, eng)
                assert grid == 1 and base_name(label) == tier_of(c, m)
            if n >= 8:
                mb = mask_recipe("eighth", col.vals, c, m)
                masked = col.run(m, mask_bits=mb, what="capped, masked")
        if n >= 8:
            assert col.run(m, mask_bits=mb, what="masked") == masked


@gpu
@pytest.mark.parametrize("case", WIDTH_CASES, ids=pid)
def test_every_width(L, O, eng, case):
    c, m = case
    col = Column(O, eng, L, c, data(c, m, N_BIG))
    distinct, outside = col.run(m)
    (label, grid, lds, flags), = record(L, eng)
    want_family = LDS_KERNEL if reach_of(c, m) <= LDS_MAX else GLOBAL_KERNEL
    assert base_name(label) == want_family == L.mi355_value_set_kernel(c, m).decode() and label == f"{want_family}<{c}>", label
    assert (outside > 0) == (m < 1 << c)
    col.run(m, mask_bits=mask_recipe("eighth", col.vals, c, m), what="masked")
    if want_family == GLOBAL_KERNEL:
        with capped(eng):
            col.run(m, what="capped")
            (label, grid, lds, flags), = record(L, eng)
            assert grid == 1 and base_name(label) == GLOBAL_KERNEL and lds == 0


@gpu
@pytest.mark.parametrize("case", SET_SIZE_CASES, ids=pid)
def test_set_sizes(L, O, eng, case):
    c, m = case
    col = Column(O, eng, L, c, data(c, m, N_BIG))
    distinct, outside = col.run(m)
    (label, grid, lds, flags), = record(L, eng)
    # the tier switches between LDS_MAX and LDS_MAX + 1 reachable bits, and nowhere else
    assert base_name(label) == (LDS_KERNEL if reach_of(c, m) <= LDS_MAX else GLOBAL_KERNEL), (label, m)
    if m == 0:
        assert (distinct, outside) == (0, N_BIG)
    if m >= 1 << c:
        assert outside == 0
    col.run(m, mask_bits=mask_recipe("eighth", col.vals, c, m), what="masked")


@gpu
def test_the_whole_32_bit_domain(L, O, eng):
    """set_bits = 2^32: a set of 512 MiB, every value inside, the global tier"""
    c, m = HUGE_CASE
    col = Column(O, eng, L, c, data(c, m, N_BIG))
    distinct, outside = col.run(m)
    assert outside == 0 and distinct > N_BIG // 2
    assert base_name(record(L, eng)[0][0]) == GLOBAL_KERNEL


@gpu
@pytest.mark.parametrize("case", ACCUMULATE_CASES, ids=pid)
def test_accumulate_keeps_what_is_there(L, O, eng, case):
    """accumulate: bits that were set survive (those behind set_bits in the last byte too), out[0] counts only the new ones, and
    a second identical call turns on nothing"""
    c, m = case
    assert m % 8
    vals = data(c, m, N_BIG)
    col = Column(O, eng, L, c, vals)
    rng = np.random.default_rng([c, 31])
    pre = rng.integers(0, 256, (m + 7) // 8, dtype=np.uint64).astype(np.uint8)
    pre[-1] |= (0xFF << (m % 8)) & 0xFF
    want, distinct, outside = expect(vals, m)
    assert 0 < int(np.unpackbits(want & ~pre).sum()) < distinct, "the pre-existing bits must cover some members and not all"
    col.run(m, accumulate=pre, what="accumulate")
    assert base_name(record(L, eng)[0][0]) == tier_of(c, m)
    after = col.buffers[m].fetch().copy()
    assert (after == (want | pre)).all()
    col.run(m, accumulate=after, what="second identical call")  # asserts out[0] == 0: nothing is new
    with capped(eng):
        col.run(m, accumulate=pre, what="accumulate, capped")
    # the union over two columns: the second call ORs into the first's set
    other = data(c, m, N_BIG, salt=1)
    first, _, _ = expect(vals, m)
    Column(O, eng, L, c, other).run(m, accumulate=np.ascontiguousarray(first), what="union of two columns")


@gpu
@pytest.mark.parametrize("case", CONTENTION_CASES, ids=pid)
def test_contention_shapes(L, O, eng, case):
    """every lane of a wave hits one word: an all-equal column, two values in one word, a sorted column"""
    c, m = case
    n = N_BIG
    top = (1 << c) - 1
    shapes = {"all equal": np.full(n, top - 3, dtype=np.uint32),
              "two values in one word": np.where(np.arange(n) % 3 == 0, 64 + 5, 64 + 29).astype(np.uint32),
              "sorted": np.sort(np.random.default_rng(c).integers(0, top + 1, n, dtype=np.uint64)).astype(np.uint32)}
    for what, vals in shapes.items():
        col = Column(O, eng, L, c, vals)
        distinct, outside = col.run(m, what=what)
        assert base_name(record(L, eng)[0][0]) == tier_of(c, m)
        assert outside == 0 and distinct == {"all equal": 1, "two values in one word": 2}.get(what, distinct)
        with capped(eng):
            col.run(m, what=what + ", capped")


@gpu
@pytest.mark.parametrize("case", MASK_CASES, ids=pid)
def test_masks(L, O, eng, case):
    c, m = case
    vals = data(c, m, N_BIG)
    col = Column(O, eng, L, c, vals)
    unmasked = col.run(m)
    for kind in ("none", "zero", "one", "eighth", "lonely"):
        got = col.run(m, mask_bits=mask_recipe(kind, vals, c, m), what=f"mask {kind}")
        assert base_name(record(L, eng)[0][0]) == tier_of(c, m)
        if kind in ("none", "one"):
            assert got == unmasked
        if kind == "zero":
            assert got == (0, 0)
        if kind == "lonely":
            assert got[0] < unmasked[0]


@gpu
@pytest.mark.parametrize("case", VIEW_CASES, ids=pid)
def test_row_range_views(L, O, eng, case):
    """rows [8192, 8192 + n) of a longer column, between rows that carry values no row of the view has: nothing of the foreign
    rows reaches the set or the counts"""
    from shared_simd_scan_amd.engine import PackedColumn

    c, m = case
    n, lead, trail = N_VIEW, K, 4096
    assert n % 8 and lead % 128 == 0
    vals = data(c, m, n)
    foreign = lonely_value(c, m) + 1
    vals = np.where(vals == foreign, foreign + 1, vals).astype(np.uint32)
    whole = np.concatenate([np.full(lead, foreign, dtype=np.uint32), vals, np.full(trail, foreign, dtype=np.uint32)])
    assert foreign < reach_of(c, m) and not (vals == foreign).any()
    col = Column(O, eng, L, c, vals)
    col.col = eng.slice_rows(PackedColumn(upload(O, whole, c), len(whole), c), lead, lead + n)
    assert col.col.n == n and col.col.data.data_ptr() % 16 == 0
    col.run(m, what="view")
    assert base_name(record(L, eng)[0][0]) == tier_of(c, m)
    mb = mask_recipe("eighth", vals, c, m)
    col.run(m, mask_bits=mb, what="view, masked")
    with capped(eng):
        col.run(m, mask_bits=mb, what="view, masked, capped")


@gpu
def test_errors_launch_nothing(L, O, eng):
    c, m, n = ERROR_CASE
    vals = data(c, m, n)
    col = Column(O, eng, L, c, vals)
    sset, out, mask, big, table = Guarded((m + 7) // 8 + 3), Guarded(16), Guarded((n + 7) // 8), Guarded(8192), Guarded(8192)
    cp, sp, op = col.col.data.data_ptr(), sset.ptr.value, out.ptr.value
    everything = (sset, out, mask, big, table)

    def call(cp=cp, n=n, c=c, mp=None, sp=sp, m=m, acc=0, op=op):
        for g in everything:
            g.t.fill_(SENTINEL)
        rc = L.mi355_value_set_dev(eng._ctx, cp, n, c, mp, sp, m, acc, op)
        eng.synchronize()
        return rc

    assert call() == 0 and base_name(record(L, eng)[0][0]) == LDS_KERNEL
    valid = record(L, eng)
    want, distinct, outside = expect(vals, m)
    assert (sset.fetch()[:len(want)] == want).all() and out.fetch().view(np.uint64).tolist() == [distinct, outside]
    nb_col = (n * c + 7) // 8
    b = big.ptr.value
    errors = (("c = 0", dict(c=0), b"32"), ("c = 33", dict(c=33), b"32"), ("set_bits = 2^32 + 1", dict(m=(1 << 32) + 1), b"2^32"),
              ("null column", dict(cp=None), b"packed_dev"), ("null set", dict(sp=None), b"set_dev"), ("null out", dict(op=None), b"out_dev"),
              ("column at +4", dict(cp=cp + 4), b"aligned"), ("set at +2", dict(sp=sp + 2), b"aligned"),
              ("mask at +2", dict(mp=mask.ptr.value + 2), b"aligned"), ("out at +4", dict(op=op + 4), b"aligned"),
              ("set is the column", dict(cp=b, sp=b), b"overlaps packed_dev"),
              ("set starts in the column's last byte", dict(cp=b, sp=b + (nb_col - 1) // 4 * 4), b"overlaps packed_dev"),
              ("column starts inside the set", dict(cp=b + 16, sp=b), b"overlaps packed_dev"),
              ("set is the mask", dict(mp=b, sp=b), b"overlaps mask_dev"),
              ("mask starts in the set's last byte", dict(mp=b + (m + 7) // 8 - 1 - ((m + 7) // 8 - 1) % 4, sp=b), b"overlaps mask_dev"),
              ("set is out", dict(sp=b, op=b), b"overlaps out_dev"), ("out inside the set", dict(sp=b, op=b + 32), b"overlaps out_dev"))
    for what, kw, word in errors:
        assert call(**kw) == E_INVALID, what
        assert word in L.mi355_last_error(), (what, L.mi355_last_error())
        assert record(L, eng) == [], what  # a refused call leaves an empty record and launches nothing
        for g in everything:
            assert (g.fetch() == SENTINEL).all(), what
    # neighbours that do not overlap are fine: the set ends where the counts begin
    set_room = ((m + 31) // 32 * 4 + 7) // 8 * 8
    big.t.fill_(SENTINEL)
    assert L.mi355_value_set_dev(eng._ctx, cp, n, c, None, b, m, 0, b + set_room) == 0
    eng.synchronize()
    assert record(L, eng) == valid
    got = big.fetch()
    assert (got[:len(want)] == want).all() and got[set_room: set_room + 16].view(np.uint64).tolist() == [distinct, outside]
    # n == 0: the set is cleared, the counts are {0, 0}, nothing is launched, neither column nor mask is needed; under accumulate the set stays
    assert call(n=0, cp=None) == 0 and record(L, eng) == []
    assert (sset.fetch()[:len(want)] == 0).all() and (sset.fetch()[len(want):] == SENTINEL).all() and out.fetch().view(np.uint64).tolist() == [0, 0]
    assert call(n=0, cp=None, acc=1) == 0 and record(L, eng) == [] and (sset.fetch() == SENTINEL).all() and out.fetch().view(np.uint64).tolist() == [0, 0]
    # set_bits == 0: no set byte is written, every row is outside; no set needed
    assert call(m=0, sp=None) == 0 and base_name(record(L, eng)[0][0]) == LDS_KERNEL
    assert (sset.fetch() == SENTINEL).all() and out.fetch().view(np.uint64).tolist() == [0, n]
    # set_ranks: every refusal, nothing launched, nothing written
    tp = table.ptr.value

    def ranks(sp=sp, m=m, ct=9, miss=0, tp=tp, op=op):
        for g in everything:
            g.t.fill_(SENTINEL)
        rc = L.mi355_set_ranks_dev(eng._ctx, sp, m, ct, miss, tp, op)
        eng.synchronize()
        return rc

    assert ranks() == 0 and [base_name(r[0]) for r in record(L, eng)] == PREFIX_KERNELS + [RANKS_KERNEL]
    errors = (("ct = 0", dict(ct=0), b"32"), ("ct = 33", dict(ct=33), b"32"), ("miss = 2^ct", dict(miss=512), b"miss"),
              ("set_bits = 2^32 + 1", dict(m=(1 << 32) + 1), b"2^32"), ("null set", dict(sp=None), b"set_dev"), ("null table", dict(tp=None), b"table_dev"),
              ("null out", dict(op=None), b"out_dev"), ("set at +2", dict(sp=sp + 2), b"aligned"), ("table at +4", dict(tp=tp + 4), b"aligned"),
              ("out at +4", dict(op=op + 4), b"aligned"), ("set is the table", dict(sp=b, tp=b), b"overlaps set_dev"),
              ("set starts in the table's last byte", dict(tp=b, sp=b + ((m * 9 + 7) // 8 - 1) // 4 * 4), b"overlaps set_dev"),
              ("table starts inside the set", dict(sp=b, tp=b + 32), b"overlaps set_dev"), ("out inside the table", dict(tp=b, op=b + 64), b"overlaps"))
    for what, kw, word in errors:
        assert ranks(**kw) == E_INVALID, what
        assert word in L.mi355_last_error(), (what, L.mi355_last_error())
        assert record(L, eng) == [], what
        for g in everything:
            assert (g.fetch() == SENTINEL).all(), what
    # set_bits == 0 writes no table byte and gives {0, 0}; neither set nor table needed
    assert ranks(m=0, sp=None, tp=None) == 0 and record(L, eng) == []
    assert (table.fetch() == SENTINEL).all() and out.fetch().view(np.uint64).tolist() == [0, 0]


def run_set_ranks(L, O, eng, bits, ct, miss, what=""):
    """set_ranks over `bits` in hostile surroundings (ones behind bit m, 0xFF behind the set) into a guarded table -> checks every
    byte of the table, the guards, both counts and the launch record"""
    import torch

    m = len(bits)
    sb = packbits(bits).copy()
    if m % 8:
        sb[-1] |= (0xFF << (m % 8)) & 0xFF
    sset = torch.full((len(sb) + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    sset[:len(sb)] = torch.from_numpy(sb).cuda()
    set_before = sset.clone()
    nbytes = (m * ct + 7) // 8
    table = Guarded(nbytes)
    entries, members, unfit = rank_table(bits, ct, miss)
    tab, counts = eng.set_ranks(sset, m, ct, miss=miss, out=table.t[table.front:])
    eng.synchronize()
    have = table.fetch()  # exactly ceil(m ct / 8) bytes inside the guards
    want = O.pack(entries, ct)[:nbytes]
    bad = np.nonzero(have != want)[0]
    assert bad.size == 0, (what, m, ct, "byte", int(bad[0]), "of", nbytes, "have", int(have[bad[0]]), "want", int(want[bad[0]]))
    assert counts.tolist() == [members, unfit], (what, m, ct, counts.tolist(), [members, unfit])
    assert torch.equal(sset, set_before), "set written"
    assert (tab.n, tab.c) == (m, ct)
    labels = [r[0] for r in record(L, eng)]
    assert [base_name(x) for x in labels] == PREFIX_KERNELS + [RANKS_KERNEL] and labels[-1] == f"{RANKS_KERNEL}<{ct}>", labels
    return unfit


@gpu
@pytest.mark.parametrize("ct", RANK_WIDTHS)
def test_set_ranks(L, O, eng, ct):
    miss = (1 << ct) - 1
    m = M_RANKS
    for kind in ("empty", "full", "first", "last", "random"):
        unfit = run_set_ranks(L, O, eng, rank_set(kind, m), ct, miss, kind)
        if kind == "full":
            assert unfit == max(m - (1 << ct), 0)
        if kind == "random":
            assert (unfit > 0) == (ct < 16), "rank overflow at the small widths only"
    with capped(eng):
        run_set_ranks(L, O, eng, rank_set("random", m), ct, 0, "random, capped")
    for small in (1, 7, 8, 9, 31, 32, 33, 16384, 16385):
        run_set_ranks(L, O, eng, rank_set("random", small), ct, miss, "small")


@gpu
@pytest.mark.parametrize("ct", [9, 31])
def test_set_ranks_across_scan_groups(L, O, eng, ct):
    run_set_ranks(L, O, eng, rank_set("random", M_RANKS_GROUPS), ct, 3, "two scan groups")
    assert base_name(record(L, eng)[-1][0]) == RANKS_KERNEL and record(L, eng)[1][1] == 2  # rowid_scan_kernel: a block per group
    with capped(eng):
        run_set_ranks(L, O, eng, rank_set("random", M_RANKS_GROUPS), ct, 3, "two scan groups, capped")


@gpu
def test_value_set_feeds_semi_join_and_bitmap_combine(L, O, eng):
    """a IN (SELECT b FROM other WHERE mask): value_set(b) is the set semi_join takes; INTERSECT of two columns' values is
    bitmap_combine on two sets; SELECT DISTINCT is the set's row ids"""
    import torch

    from shared_simd_scan_amd.engine import PackedColumn

    for c in (12, 24):
        m, n = 1 << c, N_BIG
        rng = np.random.default_rng([c, 8])
        a = rng.integers(0, m, n, dtype=np.uint64).astype(np.uint32)
        b = rng.integers(0, m, 3001, dtype=np.uint64).astype(np.uint32)
        mb = rng.random(len(b)) < 0.5
        acol, bcol = PackedColumn(upload(O, a, c), n, c), PackedColumn(upload(O, b, c), len(b), c)
        bset, bcounts = eng.value_set(bcol, mask=torch.from_numpy(packbits(mb)).cuda())
        assert base_name(record(L, eng)[0][0]) == tier_of(c, m)
        bitmap, hits = eng.semi_join(acol, bset, m)
        want = np.isin(a, b[mb])
        assert (bitmap.cpu().numpy() == packbits(want)).all() and int(hits.item()) == int(want.sum()) and want.any() and not want.all()
        aset, acounts = eng.value_set(acol)
        both, count = eng.bitmap_combine("and", aset, bset, m)
        common = np.intersect1d(a, b[mb])
        assert int(count.item()) == len(common) > 0 and int(eng.bitmap_count(aset, m).item()) == len(np.unique(a)) == int(acounts[0].item())
        ids, k = eng.bitmap_to_rowids(both, m, len(common) + 5)
        assert int(k.item()) == len(common) and (ids[:len(common)].cpu().numpy() == common).all()
        values, k = eng.distinct_values(acol)
        u = np.unique(a)
        assert int(k.item()) == len(u) and (values[:len(u)].cpu().numpy() == u).all()
        assert eng.count_distinct(bcol, mask=torch.from_numpy(packbits(mb)).cuda()) == len(np.unique(b[mb])) == int(bcounts[0].item())


@gpu
def test_dense_codes_of_a_sparse_key_feed_group_aggregate_wide(L, O, eng):
    """GROUP BY a sparse 32-bit key: dense_codes -> group_aggregate_wide equals np.unique(return_inverse) + bincount / add.at"""
    from shared_simd_scan_amd.engine import PackedColumn

    keys, values = sparse_keys()
    n = len(keys)
    kcol, vcol = PackedColumn(upload(O, keys, 32), n, 32), PackedColumn(upload(O, values, 17), n, 17)
    codes, distinct, count = eng.dense_codes(kcol)
    assert [base_name(r[0]) for r in record(L, eng)][-1:] == ["rowid_write_kernel"]
    u, inverse = np.unique(keys, return_inverse=True)
    d = len(u)
    assert int(count.item()) == d and codes.c == max(1, (d - 1).bit_length()) and codes.n == n
    assert (distinct[:d].cpu().numpy().astype(np.uint64) == u.astype(np.uint64)).all()
    assert (O.decompress(codes.data.cpu().numpy(), n, codes.c).astype(np.int64) == inverse).all()
    agg = eng.group_aggregate_wide(codes, vcol, d)
    eng.synchronize()
    want = np.zeros((d, 4), dtype=np.uint64)
    want[:, 2] = (1 << 64) - 1
    v = values.astype(np.uint64)
    np.add.at(want[:, 0], inverse, v)
    want[:, 1] = np.bincount(inverse, minlength=d).astype(np.uint64)
    np.minimum.at(want[:, 2], inverse, v)
    np.maximum.at(want[:, 3], inverse, v)
    assert (agg.cpu().numpy().view(np.uint64) == want).all()


@gpu
def test_dense_codes_after_compact_round_trip(L, O, eng):
    """after compact a column keeps its width though few of its values survive: dense_codes narrows it, values[codes] decodes;
    under a mask, rows whose value only masked-out rows carry get miss"""
    import torch

    from shared_simd_scan_amd.engine import PackedColumn

    c, n = 20, N_BIG
    rng = np.random.default_rng(20)
    vals = (rng.integers(0, 40, n, dtype=np.uint64) * 26000 + 17).astype(np.uint32)
    keep = rng.random(n) < 0.25
    col = PackedColumn(upload(O, vals, c), n, c)
    small = eng.compact_column(col, torch.from_numpy(packbits(keep)).cuda())
    assert small.n == int(keep.sum()) and small.c == c
    codes, values, count = eng.dense_codes(small)
    names = [base_name(r[0]) for r in record(L, eng)]
    d = int(count.item())
    assert d == len(np.unique(vals[keep])) == 40 and codes.c == 6
    decoded = values.cpu().numpy()[O.decompress(codes.data.cpu().numpy(), small.n, codes.c).astype(np.int64)]
    assert (decoded == vals[keep]).all()
    # the kernels of the chain, from the records of its four calls
    vset, counts = eng.value_set(small)
    assert base_name(record(L, eng)[0][0]) == GLOBAL_KERNEL and int(counts[0].item()) == 40
    table, tcounts = eng.set_ranks(vset, 1 << c, 6, miss=63)
    assert base_name(record(L, eng)[-1][0]) == RANKS_KERNEL and tcounts.tolist() == [40, 0]
    # a mask that removes the only rows of the largest value: those rows get miss
    sv = vals[keep]
    mb = sv != sv.max()
    codes, values, count = eng.dense_codes(small, ct=6, mask=torch.from_numpy(packbits(mb)).cuda(), miss=63)
    got = O.decompress(codes.data.cpu().numpy(), small.n, 6).astype(np.int64)
    assert int(count.item()) == 39 and (got[~mb] == 63).all() and (values.cpu().numpy()[got[mb]] == sv[mb]).all() and (~mb).any()
    assert names[-1] == "rowid_write_kernel"


@gpu
def test_graph_capture_and_replay(O):
    """value_set -> set_ranks -> lookup in one graph, a linear chain on a side stream, after a warm-up call: once the column's
    contents change the replay follows them"""
    import torch

    from shared_simd_scan_amd import lib
    from shared_simd_scan_amd.engine import PackedColumn

    c, ct = CAPTURE_CASE
    n, m = N_BIG, 1 << c
    versions = []
    for r in range(2):
        vals = (np.random.default_rng([c, r]).integers(0, 900 + 100 * r, n, dtype=np.uint64) * (131 - 2 * r)).astype(np.uint32)
        u, inverse = np.unique(vals, return_inverse=True)
        versions.append((O.pack(vals, c), expect(vals, m), inverse, len(u)))
    assert versions[0][3] != versions[1][3] and (versions[0][2] != versions[1][2]).any(), "a stale result could pass"

    def steps(eng):
        stage = [torch.from_numpy(v[0]).cuda() for v in versions]
        col = PackedColumn(torch.empty_like(stage[0]), n, c)
        sbuf = SetBuffer(m)
        table = torch.empty(lib().mi355_compressed_buffer_size(ct, m), dtype=torch.uint8, device="cuda")
        codes = Guarded((n * ct + 7) // 8, back=4096)
        counts = torch.empty(2, dtype=torch.int64, device="cuda")
        box = []

        def load(r):
            col.data.copy_(stage[r])
            sbuf.fill()
            table.fill_(0xFF)
            codes.t.fill_(SENTINEL)
            counts.fill_(-7)

        def run():
            vset, _ = eng.value_set(col, m, out=sbuf.view, counts=counts)
            tab, tc = eng.set_ranks(vset, m, ct, miss=(1 << ct) - 1, out=table)
            eng.lookup(col, tab, miss=(1 << ct) - 1, out=codes.t[codes.front:])
            box[:] = [tc]

        def check(r, what):
            packed, (sbytes, distinct, outside), inverse, d = versions[r]
            assert (sbuf.fetch() == sbytes).all() and counts.tolist() == [distinct, outside] and distinct == d, what
            assert box[0].tolist() == [d, 0], what
            assert (O.decompress(codes.fetch(), n, ct).astype(np.int64)[:n] == inverse).all(), what

        def untouched():
            assert (codes.fetch() == SENTINEL).all() and counts.tolist() == [-7, -7]

        def warmed(launched):  # the record of the chain's last call
            names = [base_name(r[0]) for r in launched]
            assert names and names[0].startswith("lookup_")

        return capture.Steps(load, run, check, untouched, warmed)

    capture.capture_replay(steps, (0, 1, 0))


@gpu
def test_capture_refuses_to_grow_the_workspace(O):
    """a fresh context that has ranked a small set only: under capture a larger one is refused (MI355_E_INVALID, the message names
    graph capture), nothing is enqueued for it and the capture stays intact -- the small call around it replays"""
    import torch

    from shared_simd_scan_amd import lib

    ct, small_m, big_m = 9, M_RANKS, 40 * M_RANKS
    bits = rank_set("random", small_m)

    def setup(eng):
        sset = torch.from_numpy(packbits(bits)).cuda()
        big_set = torch.zeros((big_m + 7) // 8, dtype=torch.uint8, device="cuda")
        out, refused = Guarded((small_m * ct + 7) // 8), Guarded((big_m * ct + 7) // 8)
        cnt = torch.full((4,), -7, dtype=torch.int64, device="cuda")

        def small():
            assert lib().mi355_set_ranks_dev(eng._ctx, sset.data_ptr(), small_m, ct, 0, out.ptr, cnt.data_ptr()) == 0

        def big():
            return lib().mi355_set_ranks_dev(eng._ctx, big_set.data_ptr(), big_m, ct, 0, refused.ptr, cnt.data_ptr() + 16)

        def reset():
            out.t.fill_(SENTINEL)
            cnt.fill_(-7)

        def check_small():
            entries, members, unfit = rank_table(bits, ct, 0)
            assert cnt.tolist() == [members, unfit, -7, -7] and (out.fetch() == O.pack(entries, ct)[:out.nbytes]).all()

        return small, big, reset, check_small, refused

    capture.refused_under_capture(setup)
