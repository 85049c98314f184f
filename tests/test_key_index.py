"""The row of every key of a packed column, as the packed table lookup reads (include/mi355_keyindex.h; ScanEngine.key_index,
build_table).

CPU: the header is plain C99 and declares exactly what _capi.HEADERS binds for it and the library exports; it carries its
graph-capture verdict; mi355_key_index_kernel (pure arithmetic) names the tier at every boundary; the engine's wrappers hand the
C ABI what they should (through a recording stand-in for the library); without a device the entry point fails with a message;
every __global__ under csrc/keyindex/ is named by the launch record of a GPU case of this file; no source there reads a switch
bit; the data recipe is not vacuous.

GPU (-m gpu): every expectation is numpy on the keys and masks the test generated -- np.minimum.at / np.maximum.at of the row
index over the selected rows, then the oracle's packer; nothing is derived from engine output.  Every byte of the table (the tail
bits of its last byte included), all four counts and the guard bytes around the table are compared exactly.  Tiles are 8192 rows
at ck <= 16 and 4096 above.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import capture
import support
from support import E_INVALID, SENTINEL, Guarded, L, base_name, eng, fake, header_macro, hostile_pack, packbits, record, upload  # noqa: F401  (L, eng, fake: fixtures)

HEADER = "mi355_keyindex.h"

# the kernels of csrc/keyindex/, as the launch record names them: the GPU cases below assert these labels
LDS_KERNEL = "key_index_lds_kernel"
GLOBAL_KERNEL = "key_index_global_kernel"
PACK_KERNEL = "key_index_pack_kernel"

LDS_MAX = header_macro(HEADER, "MI355_KEY_INDEX_LDS_MAX_ROWS")
FIRST, LAST = header_macro(HEADER, "MI355_KEY_INDEX_FIRST"), header_macro(HEADER, "MI355_KEY_INDEX_LAST")
KEEPS = ("first", "last")

K = 8192
N_BIG = K * 9 + 1237  # 74965: nine tiles of 8192 rows (eighteen of 4096) and a ragged one; not a multiple of 8
CT_BIG = 17           # the narrowest width that holds every row id of N_BIG rows, and N_BIG itself
SIZES = [0, 1, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049, K, N_BIG]
SIZE_CASES = [(9, 512), (9, 300), (17, 100003), (15, 16385)]
STRADDLE = (1 << 24) + 5
# every key width: with its full domain where that fits the LDS tier; beyond, at 3001 entries (the LDS tier's instantiation) and at
# the full domain, or from 25 bits on a table the keys straddle (the global tier's)
WIDTH_CASES = ([(ck, 1 << ck) for ck in range(1, 15)] + [(ck, m) for ck in range(15, 25) for m in (3001, 1 << ck)]
               + [(ck, m) for ck in range(25, 33) for m in (3001, STRADDLE)])
CT_CASE = (17, 100003)
CT_WIDTHS = [1, 7, 8, 9, 16, 17, 31, 32]
TABLE_SIZE_CASES = ([(15, m) for m in (0, 1, 7, 8, 9, 31, 32, 33, 2047, 2048, 2049, 16383, 16384, 16385, (1 << 15) - 1, 1 << 15, (1 << 15) + 1,
                                       (1 << 15) + 77)] + [(5, 1000)])
KEEP_CASES = [(12, 1 << 12), (17, 1 << 17)]  # one per tier
MASK_CASES = [(9, 300), (17, 100003)]
VIEW_CASES = [(9, 300), (17, 100003)]
N_VIEW = K * 2 + 509
FIRST_ROWS = [0, 12345, (1 << 32) - 1 - N_BIG]
FIRST_ROW_CASE = (17, 100003)
HYGIENE = [(1 << 17, 0), (3001, 1), (1 << 17, 2)]  # (table_rows, salt) at ck = 17, bitmap_to_rowids in front of the last
ERROR_CASE = (9, 300, 4096 + 77)
CAPTURE_CASE = (17, 12)  # (key width, table width)

gpu = pytest.mark.gpu


def pid(p):
    return "-".join(str(x) for x in p)


def reach_of(ck, m):
    """what a ck-bit key can address of a table of m entries"""
    return min(m, 1 << ck)


def tier_of(ck, m):
    return LDS_KERNEL if reach_of(ck, m) <= LDS_MAX else GLOBAL_KERNEL


def tile_rows(ck):
    return K if ck <= 16 else 4096


def corner_rows(ck, n):
    """rows that carry the corner keys: the first four of the first tile, the last four of the last full tile, the last four
    of the ragged tail (as far as they exist)"""
    t = tile_rows(ck)
    rows = [list(range(min(4, n)))]
    nfull = n // t
    if nfull >= 1:
        rows.append(list(range(nfull * t - 4, nfull * t)))
    if n % t >= 4 and n > 4:
        rows.append(list(range(n - 4, n)))
    return rows


def lonely_key(ck, m):
    """the key that only masked-out rows carry under mask "lonely" (reach >= 8: apart from every corner key)"""
    reach = reach_of(ck, m)
    return reach // 2 if reach >= 8 else None


def vacant_key(ck, m):
    """a key below the table's end that no row carries (reach >= 8)"""
    return lonely_key(ck, m) + 1 if reach_of(ck, m) >= 8 else None


@functools.lru_cache(maxsize=None)
def data(ck, m, n, salt=0):
    """the data recipe -> keys uint32[n], read-only.  Half of the rows uniform below reach = min(m, 2^ck), half uniform over
    [0, min(2^ck, m + m / 8 + 8)) -- keys that straddle the table's end --, none at vacant_key(), then the corner keys 0,
    reach - 1, m (clamped to 2^ck - 1) and 2^ck - 1 at corner_rows(), and lonely_key() at rows 5 and n - 6 (n >= 16)."""
    rng = np.random.default_rng([ck, m % (1 << 31), m >> 31, n, salt, 11])
    top = (1 << ck) - 1
    reach = reach_of(ck, m)
    vals = rng.integers(0, min(top + 1, m + m // 8 + 8), n, dtype=np.uint64)
    if reach:
        low = rng.random(n) < 0.5
        vals[low] = rng.integers(0, reach, int(low.sum()), dtype=np.uint64)
    lone = lonely_key(ck, m)
    if lone is not None:
        vals[(vals == lone) | (vals == lone + 1)] = lone - 1
        if n >= 16:
            vals[5] = vals[n - 6] = lone
    corners = [0, max(reach - 1, 0), min(m, top), top]
    for rows in corner_rows(ck, n):
        for r, v in zip(rows, corners):
            vals[r] = v
    vals = vals.astype(np.uint32)
    vals.setflags(write=False)
    return vals


def mask_recipe(kind, vals, ck, m):
    """-> bool[n] (None for kind "none"): "zero", "one", "eighth" (a coin of 1/8 per row), "lonely" (a coin of 1/2, then every row
    that carries lonely_key() off: a key that alone masked-out rows carry must stay `miss`)"""
    n = len(vals)
    rng = np.random.default_rng([n, ck, m % (1 << 31), 77])
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
    mb[vals == lonely_key(ck, m)] = False
    return mb


def default_miss(n, ct, first_row=0):
    """what ScanEngine.key_index takes for miss=None: the id behind the last row where ct bits hold it"""
    return first_row + n if first_row + n < 1 << ct else 0


def expect(vals, m, ct, mask_bits=None, keep="first", first_row=0, miss=0):
    """-> (the table's m entries uint32, [members, outside, inside, unfit]): np.minimum.at / np.maximum.at of the row index over
    the selected rows"""
    idx = np.arange(len(vals), dtype=np.int64) if mask_bits is None else np.nonzero(mask_bits)[0].astype(np.int64)
    k = vals[idx].astype(np.int64)
    inside = k < m
    if keep == "first":
        win = np.full(m, 1 << 40, dtype=np.int64)
        np.minimum.at(win, k[inside], idx[inside])
        present = win != 1 << 40
    else:
        assert keep == "last"
        win = np.full(m, -1, dtype=np.int64)
        np.maximum.at(win, k[inside], idx[inside])
        present = win >= 0
    ids = first_row + win
    fits = present & (ids < 1 << ct)
    entries = np.where(fits, ids, miss).astype(np.uint32)
    return entries, [int(present.sum()), int((~inside).sum()), int(inside.sum()), int((present & ~fits).sum())]


@functools.lru_cache(maxsize=None)
def permutation(ck, duplicate=False):
    """a random permutation of the ck-bit domain as a key column (every key exactly once); duplicate: row 77's key also at row 5"""
    vals = np.random.default_rng([ck, 9]).permutation(1 << ck).astype(np.uint32)
    if duplicate:
        vals[5] = vals[77]
    vals.setflags(write=False)
    return vals


@functools.lru_cache(maxsize=None)
def dimension(rows=5000, ck=17, ca=12):
    """a dimension of `rows` rows whose pk is a shuffled sparse subset of the ck-bit domain, an attribute of ca bits, and a fact
    column of N_BIG foreign keys of which about a quarter are absent from the dimension -> (pk, attr, fk)"""
    rng = np.random.default_rng(1717)
    pk = rng.permutation(1 << ck)[:rows].astype(np.uint32)
    attr = rng.integers(0, 1 << ca, rows, dtype=np.uint64).astype(np.uint32)
    fk = pk[rng.integers(0, rows, N_BIG)]
    absent = rng.random(N_BIG) < 0.25
    fk = np.where(absent, rng.integers(0, 1 << ck, N_BIG, dtype=np.uint64).astype(np.uint32), fk).astype(np.uint32)
    for a in (pk, attr, fk):
        a.setflags(write=False)
    return pk, attr, fk


def join(pk, attr, fk, miss, keep=None):
    """numpy's dictionary lookup: attr of the dimension row whose pk is fk_i (rows where `keep` is False are no part of the
    dimension), `miss` where there is none"""
    d = {int(p): int(a) for j, (p, a) in enumerate(zip(pk, attr)) if keep is None or keep[j]}
    return np.array([d.get(int(f), miss) for f in fk], dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------

def test_key_index_header_is_plain_c99():
    support.check_header_is_plain_c99(HEADER)


def test_key_index_header_declares_what_python_binds(L):
    names, sigs = support.check_header_binds(L, HEADER)
    assert names == ["mi355_key_index_dev", "mi355_key_index_kernel"]
    sig = sigs["mi355_key_index_dev"]
    assert len(sig) == 12 and sig[2] is C.c_uint64 and sig[3] is C.c_uint and sig[5] is C.c_uint64 and sig[6] is C.c_int
    assert sig[8] is C.c_uint64 and sig[9] is C.c_uint and sig[10] is C.c_uint32
    assert sigs["mi355_key_index_kernel"] == [C.c_uint, C.c_uint64] and L.mi355_key_index_kernel.restype is C.c_char_p
    assert "mi355_scan.h" in support.header_text(HEADER) and support.header_text(HEADER).count("#include") == 1
    assert (FIRST, LAST, LDS_MAX) == (0, 1, 16384)


def test_key_index_header_carries_its_capture_verdict():
    support.check_capture_verdict(HEADER, r"graph capture: capturable after a warm-up call")
    text = support.header_text(HEADER)
    assert "read at every replay" in text and "refused with MI355_E_INVALID" in text
    for section in ("widths ", "rows ", "outputs ", "kernels ", "errors ", "stream ", "record ", "graph capture:"):
        assert f" *   {section}" in text, section


def test_kernel_choice_at_the_boundaries(L):
    """mi355_key_index_kernel needs neither a device nor a context; the tier follows min(table_rows, 2^ck)"""
    from shared_simd_scan_amd import key_index_kernel

    k = L.mi355_key_index_kernel
    lds, glob = LDS_KERNEL.encode(), GLOBAL_KERNEL.encode()
    assert k(14, 1 << 14) == lds and k(32, 16384) == lds and k(15, 16384) == lds
    assert k(15, 16385) == glob and k(32, 1 << 32) == glob
    for m in (0, 1, 3001, 1 << 32):
        assert k(0, m) is None and k(33, m) is None, m
    for ck in (1, 14, 15, 32):
        assert k(ck, (1 << 32) + 1) is None, ck
    # a narrow key reaches only the first 2^ck entries, however large the table is
    for ck in range(1, 33):
        full = lds if 1 << ck <= LDS_MAX else glob
        assert k(ck, 1 << ck) == full and k(ck, 1 << 32) == full, ck
        assert k(ck, 0) == lds and k(ck, min(1 << ck, LDS_MAX)) == lds, ck
    assert key_index_kernel(9, 512) == LDS_KERNEL and key_index_kernel(32, LDS_MAX + 1) == GLOBAL_KERNEL
    for bad in ((0, 5), (33, 5), (9, (1 << 32) + 1), (9, -1), (9, (1 << 64) + 3)):
        with pytest.raises(ValueError):
            key_index_kernel(*bad)


def test_width_cases_reach_both_tiers(L):
    """(no device needed) what test_every_key_width runs launches the LDS tier at every width and the global tier at every width
    that has it"""
    fam = {(ck, m): L.mi355_key_index_kernel(ck, m).decode() for ck, m in WIDTH_CASES}
    assert {ck for (ck, m), f in fam.items() if f == LDS_KERNEL} == set(range(1, 33))
    assert {ck for (ck, m), f in fam.items() if f == GLOBAL_KERNEL} == set(range(15, 33))
    assert {tier_of(ck, m) for ck, m in SIZE_CASES} == {LDS_KERNEL, GLOBAL_KERNEL}
    assert [tier_of(ck, m) for ck, m in KEEP_CASES] == [LDS_KERNEL, GLOBAL_KERNEL]


def test_key_index_wrapper_passes_what_the_abi_takes(fake):
    import torch

    eng, rec, col = fake
    keys = col(13, 777)
    table, counts = eng.key_index(keys)  # defaults: the whole domain, the width that holds n, miss = n, the first row, no mask
    (name, a), = rec.calls
    assert name == "mi355_key_index_dev" and counts.dtype == torch.int64 and counts.numel() == 4
    assert (table.n, table.c) == (1 << 13, 10) and (777).bit_length() == 10
    assert a[1:] == [keys.data.data_ptr(), 777, 13, None, 0, FIRST, table.data.data_ptr(), 1 << 13, 10, 777, counts.data_ptr()]
    assert table.data.numel() == ((1 << 13) * 10 + 7) // 8 + 256  # compressed_buffer_size: what lookup takes
    rec.calls.clear()
    mask = torch.zeros(128, dtype=torch.uint8)
    out = torch.zeros(8192, dtype=torch.uint8)
    mine = torch.zeros(4, dtype=torch.int64)
    table, counts = eng.key_index(keys, 4001, 12, mask=mask, keep="last", first_row=12345, miss=7, out=out, counts=mine)
    (name, a), = rec.calls
    assert table.data is out and counts is mine and (table.n, table.c) == (4001, 12)
    assert a[1:] == [keys.data.data_ptr(), 777, 13, mask.data_ptr(), 12345, LAST, out.data_ptr(), 4001, 12, 7, mine.data_ptr()]
    rec.calls.clear()
    # ct follows first_row + n; miss is first_row + n where ct bits hold it, else 0
    eng.key_index(keys, 100, first_row=1 << 20)
    assert rec.calls[0][1][9:11] == [21, (1 << 20) + 777]
    rec.calls.clear()
    eng.key_index(keys, 100, ct=8)
    assert rec.calls[0][1][9:11] == [8, 0]
    rec.calls.clear()
    eng.key_index(col(9, 1023), 100)  # n = 2^ct - 1: n itself is representable
    assert rec.calls[0][1][9:11] == [10, 1023]
    rec.calls.clear()
    eng.key_index(col(9, 1024), 100)
    assert rec.calls[0][1][9:11] == [11, 1024]
    rec.calls.clear()
    eng.key_index(col(9, 0), 100)  # an empty column travels as NULL, with its mask
    assert rec.calls[0][1][1:5] == [None, 0, 9, None] and rec.calls[0][1][9:11] == [1, 0]
    rec.calls.clear()
    eng.key_index(keys, 0)  # the empty table needs no buffer
    assert rec.calls[0][1][7:9] == [None, 0]
    rec.calls.clear()
    eng.key_index(col(32, 5), ct=1, miss=0)  # 2^32 does not wrap to 0 on the way
    assert rec.calls[0][1][8] == 1 << 32
    rec.calls.clear()
    eng.key_index(keys, 100, first_row=(1 << 32) - 1 - 777)
    assert rec.calls[0][1][5] == (1 << 32) - 1 - 777 and rec.calls[0][1][9:11] == [32, (1 << 32) - 1]
    rec.calls.clear()
    for bad in (dict(table_rows=-1), dict(table_rows=(1 << 32) + 1), dict(table_rows=1 << 64), dict(ct=0), dict(ct=33), dict(ct=5, miss=32),
                dict(ct=5, miss=-1), dict(keep="middle"), dict(keep=0), dict(first_row=-1), dict(first_row=1 << 32)):
        with pytest.raises(ValueError):
            eng.key_index(keys, **bad)
    with pytest.raises(ValueError):
        eng.key_index(col(9, 1 << 32), 100)  # n = 2^32 is one row too many
    with pytest.raises(AssertionError):
        eng.key_index(keys, 8192 * 8 // 12 + 1, 12, out=out)  # the table's tensor is shorter than its bytes
    with pytest.raises(AssertionError):
        eng.key_index(keys, 100, counts=torch.zeros(2, dtype=torch.int64))
    assert rec.calls == []


def test_build_table_is_key_index_then_lookup(fake):
    import torch

    eng, rec, col = fake
    keys, values = col(13, 777), col(21, 777)
    mask = torch.zeros(128, dtype=torch.uint8)
    table, counts = eng.build_table(keys, values, 4001, mask=mask, keep="last", miss=99)
    assert [name for name, _ in rec.calls] == ["mi355_key_index_dev", "mi355_lookup_dev"]
    ki, lk = (a for _, a in rec.calls)
    # the index: 4001 entries at the width that holds n = 777, miss = n, first_row = 0
    assert ki[1:7] == [keys.data.data_ptr(), 777, 13, mask.data_ptr(), 0, LAST] and ki[8:11] == [4001, 10, 777] and ki[11] == counts.data_ptr()
    # lookup of the index through the values, a table of n rows indexed by row
    assert lk[1] == ki[7] and lk[2:4] == [4001, 10] and lk[4:8] == [values.data.data_ptr(), 777, 21, 99] and lk[8] == table.data.data_ptr()
    assert (table.n, table.c) == (4001, 21) and counts.numel() == 4
    rec.calls.clear()
    table, _ = eng.build_table(keys, values)
    ki, lk = (a for _, a in rec.calls)
    assert ki[4:7] == [None, 0, FIRST] and ki[8:11] == [1 << 13, 10, 777] and lk[7] == 0 and (table.n, table.c) == (1 << 13, 21)
    rec.calls.clear()
    with pytest.raises(AssertionError):
        eng.build_table(keys, col(21, 776))  # one value per key row
    with pytest.raises(ValueError):
        eng.build_table(keys, values, miss=1 << 21)
    assert [name for name, _ in rec.calls] in ([], ["mi355_key_index_dev"])


def test_key_index_fails_loudly_without_a_gpu(L):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    buf = (C.c_uint8 * 1024)()
    out = (C.c_uint8 * 4096)()
    cnt = (C.c_uint64 * 4)()
    assert L.mi355_key_index_dev(None, buf, 100, 9, None, 0, FIRST, out, 512, 9, 0, cnt) != 0 and L.mi355_last_error()


def test_every_key_index_kernel_has_a_case():
    """every __global__ under csrc/keyindex/ is asserted from the launch record by a GPU case of this file, and the file names
    no kernel that does not exist"""
    assert [p.rsplit("/", 1)[1] for p in support.feature_sources("keyindex")] == ["key_index.hip", "key_index.hpp"]
    kernels = support.global_kernels_of("keyindex")
    assert kernels == {LDS_KERNEL, GLOBAL_KERNEL, PACK_KERNEL}, kernels
    support.check_gpu_part_asserts(__file__, "LDS_KERNEL", "GLOBAL_KERNEL", "PACK_KERNEL")


def test_key_index_sources_read_no_flag_bits():
    support.check_sources_read_no_flag_bits("keyindex")


def gpu_shapes():
    """every (ck, m, n) the GPU tests below run on recipe data"""
    shapes = {(ck, m, n) for ck, m in SIZE_CASES for n in SIZES}
    shapes |= {(ck, m, N_BIG) for ck, m in WIDTH_CASES + TABLE_SIZE_CASES + MASK_CASES + [CT_CASE, FIRST_ROW_CASE]}
    shapes |= {(ck, m, N_VIEW) for ck, m in VIEW_CASES}
    shapes |= {(17, m, N_BIG) for m, _ in HYGIENE}
    shapes |= {ERROR_CASE}
    return sorted(shapes)


@pytest.mark.parametrize("shape", [s for s in gpu_shapes() if s[2] >= 2 * K and s[1] >= 1], ids=pid)
def test_recipe_is_not_vacuous(shape):
    """(no device needed) what the cases of at least two tiles must exercise: a key with several selected rows (first and last
    differ), a key with none, a row outside the table, corner keys in the last full tile and in the ragged tail"""
    ck, m, n = shape
    vals = data(ck, m, n)
    v = vals.astype(np.int64)
    reach, top, t = reach_of(ck, m), (1 << ck) - 1, tile_rows(ck)
    first, cf = expect(vals, m, 32, keep="first", miss=(1 << 32) - 1)
    last, cl = expect(vals, m, 32, keep="last", miss=(1 << 32) - 1)
    assert cf == cl and cf[1] + cf[2] == n and cf[3] == 0 and cf[0] >= 1
    assert (first != last).any() and cf[2] > cf[0], "no key with several rows: first and last agree everywhere"
    assert (v == reach - 1).any(), "no row carries the table's last reachable key"
    if m < 1 << ck:
        assert (v == m).any() and (v == m - 1).any(), "no key at table_rows - 1 and table_rows"
        assert cf[1] > 0, "no row outside the table"
    else:
        assert cf[1] == 0
    if reach >= 8:
        vacant = vacant_key(ck, m)
        assert vacant < reach and first[vacant] == (1 << 32) - 1 and cf[0] < reach, "no key without a row"
    if m > 1 << ck:
        assert (first[1 << ck:] == (1 << 32) - 1).all()
    groups = corner_rows(ck, n)
    assert n % t >= 4 and any(rows[-1] == n // t * t - 1 for rows in groups) and groups[-1][-1] == n - 1
    corners = [0, max(reach - 1, 0), min(m, top), top]
    for rows in groups:
        assert [int(v[r]) for r in rows] == corners
    # masked-out rows that alone carry some key: the key has rows, every one of them is off, and its entry is miss under the mask
    lone = lonely_key(ck, m)
    if (ck, m) in MASK_CASES:
        mb = mask_recipe("lonely", vals, ck, m)
        assert (v == lone).sum() >= 2 and not mb[v == lone].any() and mb.any() and not mb.all()
        masked, cm = expect(vals, m, 32, mb, miss=(1 << 32) - 1)
        assert first[lone] == 5 and last[lone] == n - 6 and masked[lone] == (1 << 32) - 1 and cm[0] < cf[0]
        eighth = mask_recipe("eighth", vals, ck, m)
        assert 0 < eighth.sum() < n // 4
        e_first, ce = expect(vals, m, 32, eighth, "first", miss=(1 << 32) - 1)
        e_last, _ = expect(vals, m, 32, eighth, "last", miss=(1 << 32) - 1)
        assert (e_first != e_last).any() and (e_first != first).any()
    # row ids beyond the table's width where the case intends them
    if (ck, m, n) == CT_CASE + (N_BIG,):
        for ct in CT_WIDTHS:
            _, c = expect(vals, m, ct, miss=0)
            assert (c[3] > 0) == (ct < CT_BIG), ct
            assert c[3] < c[0] or ct == 1, "every member unfit: the table would be all miss"
    if (ck, m, n) == FIRST_ROW_CASE + (N_BIG,):
        unfit = [expect(vals, m, 16, first_row=f)[1][3] for f in FIRST_ROWS]
        assert 0 < unfit[0] < unfit[1] < unfit[2] == cf[0], unfit  # the upper rows overflow 16 bits; behind 2^32 - 1 - n all do
        assert [expect(vals, m, 32, first_row=f)[1][3] for f in FIRST_ROWS] == [0, 0, 0]


def test_contention_recipe_is_not_vacuous():
    for ck, m in KEEP_CASES:
        assert m == 1 << ck
        perm, dup = permutation(ck), permutation(ck, duplicate=True)
        first, c = expect(perm, m, 32)
        assert c == [m, 0, m, 0] and (perm[first] == np.arange(m)).all(), "the table is the inverse permutation"
        df, cd = expect(dup, m, 32, keep="first", miss=(1 << 32) - 1)
        dl, _ = expect(dup, m, 32, keep="last", miss=(1 << 32) - 1)
        assert cd[2] - cd[0] == 1 and cd[0] == m - 1 and (df != dl).sum() == 1 and df[dup[5]] == 5 and dl[dup[5]] == 77
    pk, attr, fk = dimension()
    assert len(np.unique(pk)) == len(pk) == 5000 and 0.1 < np.isin(fk, pk, invert=True).mean() < 0.4


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

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


class Keys:
    """one engine and a key column uploaded in hostile surroundings (support.hostile_pack)"""

    def __init__(self, O, eng, L, ck, vals, offset=0):
        from shared_simd_scan_amd.engine import PackedColumn

        self.O, self.eng, self.L, self.ck, self.vals, self.n = O, eng, L, ck, vals, len(vals)
        self.col = PackedColumn(hostile_pack(O, vals, ck, offset) if self.n else upload(O, np.zeros(1, dtype=np.uint32), ck), self.n, ck)
        assert self.col.data.data_ptr() % 16 == 0

    def run(self, m, ct=CT_BIG, mask_bits=None, keep="first", first_row=0, miss=None, what="", front=4096):
        """key_index into a guarded table pre-filled with the sentinel -> checks every byte, the guards, the four counts, the launch
        record and the inputs against numpy; returns the counts"""
        import torch

        tag = (what, self.ck, m, self.n, ct, keep, first_row)
        nbytes = (m * ct + 7) // 8
        table = Guarded(nbytes, front=front)
        assert table.ptr.value % 16 == 0
        want_miss = default_miss(self.n, ct, first_row) if miss is None else miss
        entries, want_counts = expect(self.vals, m, ct, mask_bits, keep, first_row, want_miss)
        want = self.O.pack(entries, ct)[:nbytes] if m else np.zeros(0, dtype=np.uint8)
        mask = hostile_mask(mask_bits) if mask_bits is not None and self.n else None
        col_before = self.col.data.clone()
        counts = torch.full((4,), -7, dtype=torch.int64, device="cuda")
        tab, got = self.eng.key_index(self.col, m, ct, mask=mask, keep=keep, first_row=first_row, miss=miss, out=table.t[table.front:], counts=counts)
        self.eng.synchronize()
        have = table.fetch()  # asserts the guard bytes on both sides: exactly ceil(m ct / 8) bytes are written
        bad = np.nonzero(have != want)[0]
        assert bad.size == 0, (tag, "byte", int(bad[0]), "of", nbytes, "have", int(have[bad[0]]), "want", int(want[bad[0]]))
        assert got.tolist() == want_counts, (tag, got.tolist(), want_counts)
        assert (tab.n, tab.c) == (m, ct) and got is counts
        assert torch.equal(self.col.data, col_before), (tag, "keys written")
        labels = [(r[0], r[2], r[3]) for r in record(self.L, self.eng)]
        tier = tier_of(self.ck, m)
        if self.n:
            label, lds, flags = labels.pop(0)
            assert label == f"{tier}<{self.ck}>" and flags == 0, (tag, label)
            assert (lds >= 4 * reach_of(self.ck, m)) if tier == LDS_KERNEL else lds == 0, (tag, lds)
        if m:
            label, lds, flags = labels.pop(0)
            assert label == f"{PACK_KERNEL}<{ct}>" and (lds, flags) == (0, 0), (tag, label)
        assert labels == [], (tag, labels)
        return want_counts


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
    ck, m = case
    for n in SIZES:
        keys = Keys(O, eng, L, ck, data(ck, m, n))
        ct = max(1, n.bit_length())
        default = keys.run(m, ct)
        if n:
            assert base_name(record(L, eng)[0][0]) in (LDS_KERNEL, GLOBAL_KERNEL)
        assert base_name(record(L, eng)[-1][0]) == PACK_KERNEL
        keys.run(m, ct, keep="last")
        with capped(eng):
            assert keys.run(m, ct, what="capped") == default
            assert [r[1] for r in record(L, eng)] == [1] * (2 if n else 1), "one block each"
            if n >= 8:
                mb = mask_recipe("eighth", keys.vals, ck, m)
                masked = keys.run(m, ct, mask_bits=mb, keep="last", what="capped, masked")
        if n >= 8:
            assert keys.run(m, ct, mask_bits=mb, keep="last", what="masked") == masked
        if n == 0:
            assert default == [0, 0, 0, 0]


@gpu
@pytest.mark.parametrize("case", WIDTH_CASES, ids=pid)
def test_every_key_width(L, O, eng, case):
    ck, m = case
    keys = Keys(O, eng, L, ck, data(ck, m, N_BIG))
    members, outside, inside, unfit = keys.run(m)
    (label, grid, lds, flags), pack = record(L, eng)
    want_family = LDS_KERNEL if reach_of(ck, m) <= LDS_MAX else GLOBAL_KERNEL
    assert base_name(label) == want_family == L.mi355_key_index_kernel(ck, m).decode() and label == f"{want_family}<{ck}>", label
    assert (outside > 0) == (m < 1 << ck) and unfit == 0 and inside > members
    keys.run(m, mask_bits=mask_recipe("eighth", keys.vals, ck, m), keep="last", what="masked")
    if want_family == GLOBAL_KERNEL:
        with capped(eng):
            keys.run(m, keep="last", what="capped")
            (label, grid, lds, flags), pack = record(L, eng)
            assert grid == 1 and base_name(label) == GLOBAL_KERNEL and lds == 0


@gpu
@pytest.mark.parametrize("ct", CT_WIDTHS)
def test_every_table_width(L, O, eng, ct):
    """the narrow widths make most members unfit: the count is exact, and `miss` takes their place"""
    ck, m = CT_CASE
    keys = Keys(O, eng, L, ck, data(ck, m, N_BIG))
    for keep in KEEPS:
        for miss in ((1 << ct) - 1, 0, None):
            members, outside, inside, unfit = keys.run(m, ct, keep=keep, miss=miss)
            assert record(L, eng)[-1][0] == f"{PACK_KERNEL}<{ct}>"
            assert (unfit > 0) == (ct < CT_BIG)
    with capped(eng):
        keys.run(m, ct, mask_bits=mask_recipe("eighth", keys.vals, ck, m), what="capped, masked")


@gpu
@pytest.mark.parametrize("case", TABLE_SIZE_CASES, ids=pid)
def test_table_sizes(L, O, eng, case):
    ck, m = case
    keys = Keys(O, eng, L, ck, data(ck, m, N_BIG))
    members, outside, inside, unfit = keys.run(m)
    rec = record(L, eng)
    # the tier switches between LDS_MAX and LDS_MAX + 1 reachable entries, and nowhere else
    assert base_name(rec[0][0]) == (LDS_KERNEL if reach_of(ck, m) <= LDS_MAX else GLOBAL_KERNEL), (rec, m)
    if m == 0:
        assert (members, outside, inside) == (0, N_BIG, 0) and len(rec) == 1
    else:
        assert base_name(rec[1][0]) == PACK_KERNEL
    if m >= 1 << ck:
        assert outside == 0 and members <= 1 << ck  # beyond 2^ck every entry is miss: expect() has no key there
    keys.run(m, mask_bits=mask_recipe("eighth", keys.vals, ck, m), keep="last", what="masked")
    with capped(eng):
        keys.run(m, keep="last", what="capped")


@gpu
@pytest.mark.parametrize("case", KEEP_CASES, ids=pid)
def test_keep_rule_under_contention(L, O, eng, case):
    """every wave of every block raises one slot (an all-equal column), runs of equal keys (a sorted one), no two rows on a slot (a
    permutation: the table is its inverse), and one duplicate"""
    ck, m = case
    top = (1 << ck) - 1
    shapes = {"all equal": np.full(N_BIG, top - 3, dtype=np.uint32),
              "sorted": np.sort(np.random.default_rng(ck).integers(0, top + 1, N_BIG, dtype=np.uint64)).astype(np.uint32),
              "permutation": permutation(ck), "one duplicate": permutation(ck, duplicate=True)}
    for what, vals in shapes.items():
        keys = Keys(O, eng, L, ck, vals)
        ct = max(1, len(vals).bit_length())
        for keep in KEEPS:
            members, outside, inside, unfit = keys.run(m, ct, keep=keep, what=what)
            assert base_name(record(L, eng)[0][0]) == tier_of(ck, m) and base_name(record(L, eng)[1][0]) == PACK_KERNEL
            assert outside == 0 and unfit == 0
            if what == "all equal":
                assert (members, inside) == (1, N_BIG)
            if what == "permutation":
                assert members == inside == m
            if what == "one duplicate":
                assert inside - members == 1
            with capped(eng):
                keys.run(m, ct, keep=keep, what=what + ", capped")


@gpu
@pytest.mark.parametrize("case", MASK_CASES, ids=pid)
def test_masks(L, O, eng, case):
    ck, m = case
    vals = data(ck, m, N_BIG)
    keys = Keys(O, eng, L, ck, vals)
    for keep in KEEPS:
        unmasked = keys.run(m, keep=keep)
        for kind in ("none", "zero", "one", "eighth", "lonely"):  # hostile_mask: garbage in the mask bits >= n, 0xFF behind them
            got = keys.run(m, mask_bits=mask_recipe(kind, vals, ck, m), keep=keep, what=f"mask {kind}")
            assert base_name(record(L, eng)[0][0]) == tier_of(ck, m)
            if kind in ("none", "one"):
                assert got == unmasked
            if kind == "zero":
                assert got == [0, 0, 0, 0]
            if kind == "lonely":
                assert got[0] < unmasked[0]


@gpu
@pytest.mark.parametrize("case", VIEW_CASES, ids=pid)
def test_row_range_views(L, O, eng, case):
    """rows [8192, 8192 + n) of a longer column, between rows that carry a key no row of the view has: nothing of the foreign
    rows reaches the table or the counts; a column uploaded at an offset; the table a 16-byte-aligned slice of a longer buffer"""
    from shared_simd_scan_amd.engine import PackedColumn

    ck, m = case
    n, lead, trail = N_VIEW, K, 4096
    assert n % 8 and lead % 128 == 0
    vals = data(ck, m, n)
    foreign = vacant_key(ck, m)
    whole = np.concatenate([np.full(lead, foreign, dtype=np.uint32), vals, np.full(trail, foreign, dtype=np.uint32)])
    assert foreign < reach_of(ck, m) and not (vals == foreign).any()
    keys = Keys(O, eng, L, ck, vals, offset=48)
    keys.run(m, what="offset 48", front=4096 + 16)
    view = Keys(O, eng, L, ck, vals)
    view.col = eng.slice_rows(PackedColumn(upload(O, whole, ck), len(whole), ck), lead, lead + n)
    assert view.col.n == n and view.col.data.data_ptr() % 16 == 0
    for keep in KEEPS:
        view.run(m, keep=keep, what="view", front=4096 + 16)
        assert base_name(record(L, eng)[0][0]) == tier_of(ck, m)
    mb = mask_recipe("eighth", vals, ck, m)
    view.run(m, mask_bits=mb, what="view, masked", front=4096 + 48)
    with capped(eng):
        view.run(m, mask_bits=mb, keep="last", what="view, masked, capped")


@gpu
@pytest.mark.parametrize("first_row", FIRST_ROWS)
def test_first_row(L, O, eng, first_row):
    ck, m = FIRST_ROW_CASE
    keys = Keys(O, eng, L, ck, data(ck, m, N_BIG))
    for keep in KEEPS:
        for ct in (16, 32):  # 16: the upper rows overflow; 32: the largest id is 2^32 - 2 and fits
            members, outside, inside, unfit = keys.run(m, ct, keep=keep, first_row=first_row)
            assert base_name(record(L, eng)[-1][0]) == PACK_KERNEL
            assert (unfit > 0) == (ct == 16) and (unfit == members) == (ct == 16 and first_row >= 1 << 16)


@gpu
def test_workspace_hygiene(L, O, eng):
    """a large call, a small one, another user of the selection workspace, the large call again, on different data each time: no
    slot of an earlier call shows"""
    import torch

    ck = 17
    for step, (m, salt) in enumerate(HYGIENE):
        if step == 2:
            bits = np.random.default_rng(5).random(1 << 20) < 0.5
            ids, count = eng.bitmap_to_rowids(torch.from_numpy(packbits(bits)).cuda(), len(bits), len(bits))
            eng.synchronize()
            assert int(count.item()) == int(bits.sum()) and base_name(record(L, eng)[0][0]) == "rowid_count_kernel"
        keys = Keys(O, eng, L, ck, data(ck, m, N_BIG, salt))
        for keep in KEEPS:
            keys.run(m, keep=keep, what=f"step {step}")
            assert base_name(record(L, eng)[0][0]) == tier_of(ck, m)
    # LAST leaves large codes for low rows' neighbours, FIRST for low rows: each after the other on one table
    a, b = Keys(O, eng, L, ck, data(ck, 1 << 17, N_BIG, 3)), Keys(O, eng, L, ck, data(ck, 1 << 17, 2049, 4))
    for keep_a, keep_b in (("first", "last"), ("last", "first")):
        a.run(1 << 17, keep=keep_a)
        b.run(1 << 17, keep=keep_b, what="after a larger column")


@gpu
def test_errors_launch_nothing(L, O, eng):
    ck, m, n = ERROR_CASE
    ct = 13
    vals = data(ck, m, n)
    keys = Keys(O, eng, L, ck, vals)
    table, out, mask, big = Guarded((m * ct + 7) // 8), Guarded(32), Guarded((n + 7) // 8), Guarded(8192)
    kp, tp, op = keys.col.data.data_ptr(), table.ptr.value, out.ptr.value
    everything = (table, out, mask, big)

    def call(kp=kp, n=n, ck=ck, mp=None, first_row=0, keep=FIRST, tp=tp, m=m, ct=ct, miss=0, op=op):
        for g in everything:
            g.t.fill_(SENTINEL)
        rc = L.mi355_key_index_dev(eng._ctx, kp, n, ck, mp, first_row, keep, tp, m, ct, miss, op)
        eng.synchronize()
        return rc

    assert call() == 0 and [base_name(r[0]) for r in record(L, eng)] == [LDS_KERNEL, PACK_KERNEL]
    valid = record(L, eng)
    entries, counts = expect(vals, m, ct)
    want = O.pack(entries, ct)[:table.nbytes]
    assert (table.fetch() == want).all() and out.fetch().view(np.uint64).tolist() == counts
    nb_keys, nb_table = (n * ck + 7) // 8, table.nbytes
    b = big.ptr.value
    errors = (("ck = 0", dict(ck=0), b"ck"), ("ck = 33", dict(ck=33), b"ck"), ("ct = 0", dict(ct=0), b"ct"), ("ct = 33", dict(ct=33), b"ct"),
              ("table_rows = 2^32 + 1", dict(m=(1 << 32) + 1), b"table_rows"), ("n = 2^32", dict(n=1 << 32), b"n="),
              ("first_row = 2^32", dict(first_row=1 << 32), b"first_row"), ("miss = 2^ct", dict(miss=1 << ct), b"miss"),
              ("keep = 2", dict(keep=2), b"keep"), ("keep = -1", dict(keep=-1), b"keep"),
              ("null keys", dict(kp=None), b"keys_dev"), ("null table", dict(tp=None), b"table_dev"), ("null out", dict(op=None), b"out_dev"),
              ("keys at +4", dict(kp=kp + 4), b"aligned"), ("mask at +2", dict(mp=mask.ptr.value + 2), b"aligned"),
              ("table at +8", dict(tp=tp + 8), b"aligned"), ("out at +4", dict(op=op + 4), b"aligned"),
              ("table is the keys", dict(kp=b, tp=b), b"overlaps keys_dev"),
              ("table starts in the keys' last byte", dict(kp=b, tp=b + (nb_keys - 1) // 16 * 16), b"overlaps keys_dev"),
              ("keys start inside the table", dict(kp=b + 16, tp=b), b"overlaps keys_dev"),
              ("table is the mask", dict(mp=b, tp=b), b"overlaps mask_dev"),
              ("mask starts in the table's last byte", dict(mp=b + (nb_table - 1) // 4 * 4, tp=b), b"overlaps mask_dev"),
              ("table is out", dict(tp=b, op=b), b"overlaps out_dev"), ("out inside the table", dict(tp=b, op=b + 32), b"overlaps out_dev"),
              ("out's last word in the table", dict(tp=b + 32, op=b + 8), b"overlaps out_dev"))
    for what, kw, word in errors:
        assert call(**kw) == E_INVALID, what
        assert word in L.mi355_last_error(), (what, L.mi355_last_error())
        assert record(L, eng) == [], what  # a refused call leaves an empty record and launches nothing
        for g in everything:
            assert (g.fetch() == SENTINEL).all(), what
    # neighbours that do not overlap are fine: the table ends where the counts begin
    room = (nb_table + 15) // 16 * 16
    big.t.fill_(SENTINEL)
    assert L.mi355_key_index_dev(eng._ctx, kp, n, ck, None, 0, FIRST, b, m, ct, 0, b + room) == 0
    eng.synchronize()
    assert record(L, eng) == valid
    got = big.fetch()
    assert (got[:nb_table] == want).all() and got[room: room + 32].view(np.uint64).tolist() == counts
    assert (got[nb_table: room] == SENTINEL).all() and (got[room + 32:] == SENTINEL).all()
    # n == 0: an all-miss table, {0, 0, 0, 0}, only the pack kernel; neither keys nor mask are needed
    assert call(n=0, kp=None, miss=5) == 0 and [base_name(r[0]) for r in record(L, eng)] == [PACK_KERNEL]
    assert (table.fetch() == O.pack(np.full(m, 5, dtype=np.uint32), ct)[:nb_table]).all() and out.fetch().view(np.uint64).tolist() == [0, 0, 0, 0]
    # table_rows == 0: no table byte is written, every row is outside; no table needed
    assert call(m=0, tp=None) == 0 and [base_name(r[0]) for r in record(L, eng)] == [LDS_KERNEL]
    assert (table.fetch() == SENTINEL).all() and out.fetch().view(np.uint64).tolist() == [0, n, 0, 0]


@gpu
def test_graph_capture_and_replay(O):
    """key_index under a mask, after a warm-up call: three versions of keys and mask are replayed, each exact"""
    import torch

    from shared_simd_scan_amd.engine import PackedColumn

    ck, ct = CAPTURE_CASE
    n, m = N_BIG, 1 << ck
    miss = (1 << ct) - 1
    versions = []
    for r in range(3):
        vals = data(ck, m, n, salt=20 + r)
        mb = np.random.default_rng([r, 3]).random(n) < 0.5
        mb[n - 3:] = True  # rows whose id does not fit ct bits are selected
        entries, counts = expect(vals, m, ct, mb, "last", 0, miss)
        versions.append((O.pack(vals, ck), packbits(mb), O.pack(entries, ct)[:(m * ct + 7) // 8], counts))
    assert all(c[3] > 0 for *_, c in versions), "no unfit member"
    assert not any(np.array_equal(versions[i][2], versions[j][2]) for i, j in ((0, 1), (1, 2), (0, 2))), "a stale result could pass"

    def steps(eng):
        stage = [(torch.from_numpy(v[0]).cuda(), torch.from_numpy(v[1]).cuda()) for v in versions]
        col = PackedColumn(torch.empty_like(stage[0][0]), n, ck)
        mask = torch.empty_like(stage[0][1])
        table = Guarded((m * ct + 7) // 8)
        counts = torch.empty(4, dtype=torch.int64, device="cuda")

        def load(r):
            col.data.copy_(stage[r][0])
            mask.copy_(stage[r][1])
            table.t.fill_(SENTINEL)
            counts.fill_(-7)

        def run():
            eng.key_index(col, m, ct, mask=mask, keep="last", miss=miss, out=table.t[table.front:], counts=counts)

        def check(r, what):
            assert (table.fetch() == versions[r][2]).all() and counts.tolist() == versions[r][3], what

        def untouched():
            assert (table.fetch() == SENTINEL).all() and counts.tolist() == [-7] * 4

        def warmed(launched):
            assert [x[0] for x in launched] == [f"{GLOBAL_KERNEL}<{ck}>", f"{PACK_KERNEL}<{ct}>"]

        return capture.Steps(load, run, check, untouched, warmed)

    capture.capture_replay(steps, (1, 2, 0))


@gpu
def test_capture_refuses_to_grow_the_workspace(O):
    """a fresh context that has indexed a small table only: under capture a larger one is refused (MI355_E_INVALID, the message
    names graph capture), nothing is enqueued for it and the capture stays intact -- the small call around it replays"""
    import torch

    from shared_simd_scan_amd import lib

    ck, ct, small_m, big_m = 17, CT_BIG, 3001, 1 << 17
    vals = data(ck, small_m, N_BIG)

    def setup(eng):
        col = upload(O, vals, ck)
        out, refused = Guarded((small_m * ct + 7) // 8), Guarded((big_m * ct + 7) // 8)
        cnt = torch.full((8,), -7, dtype=torch.int64, device="cuda")

        def small():
            assert lib().mi355_key_index_dev(eng._ctx, col.data_ptr(), N_BIG, ck, None, 0, FIRST, out.ptr, small_m, ct, 0, cnt.data_ptr()) == 0

        def big():
            return lib().mi355_key_index_dev(eng._ctx, col.data_ptr(), N_BIG, ck, None, 0, FIRST, refused.ptr, big_m, ct, 0, cnt.data_ptr() + 32)

        def reset():
            out.t.fill_(SENTINEL)
            cnt.fill_(-7)

        def check_small():
            entries, counts = expect(vals, small_m, ct)
            assert cnt.tolist() == counts + [-7] * 4 and (out.fetch() == O.pack(entries, ct)[:out.nbytes]).all()

        return small, big, reset, check_small, refused

    capture.refused_under_capture(setup)


@gpu
def test_join_end_to_end(L, O, eng):
    """SELECT d.attr FROM fact f JOIN dim d ON f.fk = d.pk [WHERE d.attr < 2048]: lookup(fk, build_table(pk, attr)), the two-step
    form through the index, and the filtered form with a scan over the dimension as the mask, against numpy's dictionary lookup"""
    from shared_simd_scan_amd.engine import PackedColumn

    ck, ca, miss = 17, 12, 4095
    pk, attr, fk = dimension()
    rows, n = len(pk), len(fk)
    pcol, acol, fcol = (PackedColumn(upload(O, v, c), len(v), c) for v, c in ((pk, ck), (attr, ca), (fk, ck)))

    def values(col):
        eng.synchronize()
        return O.decompress(col.data.cpu().numpy(), col.n, col.c).astype(np.int64)

    want = join(pk, attr, fk, miss)
    assert (want == miss).sum() > n // 8 and (want != miss).sum() > n // 2
    table, counts = eng.build_table(pcol, acol, miss=miss)
    assert [base_name(r[0]) for r in record(L, eng)][0].startswith("lookup_") and counts.tolist() == [rows, 0, rows, 0]
    assert (table.n, table.c) == (1 << ck, ca)
    assert (values(eng.lookup(fcol, table, miss=miss)) == want).all()
    # the two-step form: one index, any number of attributes
    index, counts = eng.key_index(pcol)
    assert [base_name(r[0]) for r in record(L, eng)] == [GLOBAL_KERNEL, PACK_KERNEL] and (index.n, index.c) == (1 << ck, 13)
    dim_row = eng.lookup(fcol, index, miss=rows)
    assert (values(eng.lookup(dim_row, acol, miss=miss)) == want).all()
    assert (values(eng.lookup(dim_row, pcol, miss=0))[want != miss] == fk[want != miss]).all(), "the key itself is an attribute too"
    # the filtered form: the mask is a scan over the dimension
    bitmap, hits = eng.scan_where("<", 2048, acol)
    keep = attr < 2048
    want = join(pk, attr, fk, miss, keep)
    table, counts = eng.build_table(pcol, acol, mask=bitmap, miss=miss)
    assert counts.tolist() == [int(keep.sum()), 0, int(keep.sum()), 0] and int(hits.item()) == int(keep.sum())
    assert (values(eng.lookup(fcol, table, miss=miss)) == want).all() and 0 < (want != miss).sum() < (join(pk, attr, fk, miss) != miss).sum()
    # a table narrower than the domain: keys beyond it are outside, and the facts that carry them get miss
    half = 1 << (ck - 1)
    table, counts = eng.build_table(pcol, acol, half, miss=miss)
    assert counts.tolist() == [int((pk < half).sum()), int((pk >= half).sum()), int((pk < half).sum()), 0]
    assert (values(eng.lookup(fcol, table, miss=miss)) == join(pk, attr, fk, miss, pk < half)).all()
