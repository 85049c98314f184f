"""Every feature entry point on columns whose row ids, packed bit offsets or byte offsets pass 2^31 and 2^32.

The entry points' own test files stop at about 1.7e7 rows, where no packed bit offset reaches 2^32, no byte offset 2^31 and no row
id 2^31: a kernel that narrowed `tile * TILE_BYTES`, `before * C` or a chunk index to 32 bits would pass them all.  Here each entry
point runs on the smallest column at which such arithmetic can go wrong (the shapes below), and every result is checked twice:

  1. at full size, on the device, by a route that shares nothing with the kernels: `decompress` of row slices (verified beyond
     2^32 rows by test_gpu_parity.py) -> plain torch over int64 values (large_routes.py) -> re-packed by torch arithmetic; every
     output byte, count and result word is compared;
  2. in windows on the host, by numpy over the oracle's generator: at row 0, across each crossing (two tiles either side) and over
     the ragged end.  Where a result depends on all the rows in front of it (a running sum, a rank among ties) the window check
     is made where the host knows those rows, and the docstring says so.

Inputs come from the "splitmix" generator (never "mod": a wrapped offset must read other values -- test_inputs_differ_where_an_
offset_would_wrap proves that for every width and crossing used), masks and run-structured columns from torch.  Outputs lie inside
0xEE guards that are checked on the device after every call.  Bit-exact everywhere.

The CPU part (-m "not gpu") pins the shapes, the inputs, the routes themselves (against the numpy expectations of support.py and
of the entry points' own files), the coverage of every exported *_dev that takes a row count, and the pure size functions of the C
API at these row counts."""
import os
import re

import numpy as np
import pytest

import large_routes as R
from support import (INCLUDE, SENTINEL, Guarded, L, declared, eng, grouped, header_macro, header_text, key_index_expect, packbits, payload,  # noqa: F401
                     plain_pack, pred, rng_of, top_k_expect)

gpu = pytest.mark.gpu

# ---- shapes -------------------------------------------------------------------------------------------------------------------

CHUNK, TILE = 16384, 2048
RAG = 3 * CHUNK + TILE + 77             # three chunks, one tile, 77 rows: ragged in chunk, tile, lane and byte
N_ROWS = (1 << 32) + RAG                # row ids and row counts cross 2^31 and 2^32
N_ROWS_MAX = (1 << 32) - 1              # the most run_encode and key_index take
N_SORT = 1 << 32                        # the most sort_rows takes
X_BITS = -(-(1 << 32) // 31)            # the first row of a 31-bit column whose bit offset is >= 2^32
N_BITS = -(-X_BITS // CHUNK) * CHUNK + RAG
N_BYTES = (1 << 30) + RAG               # 32-bit values: byte offsets cross 2^31 (row 2^29) and 2^32 (row 2^30)
N_POS = (1 << 31) + RAG                 # row_positions: positions cross 2^31
N_SMALL = 9 * 8192 + 1237               # where the routes meet numpy on the CPU
S = 1 << 27                             # rows per slice of a full-size route

# the rows at which something crosses, by shape, and what crosses there: (row, the crossing in bits of the packed stream)
CROSSINGS = {
    "rows": lambda c: [(1 << 31, (1 << 31) * c), (1 << 32, (1 << 32) * c)],
    "bits": lambda c: [(X_BITS, 1 << 32)],
    "bytes": lambda c: [(1 << 29, 1 << 34), (1 << 30, 1 << 35)],
}
SHAPE_ROWS = {"rows": N_ROWS, "bits": N_BITS, "bytes": N_BYTES}
SHAPE_WIDTHS = {"rows": (1, 2, 3), "bits": (31,), "bytes": (32,)}

# the generator seed of every splitmix column, by width: chosen so that test_inputs_differ_where_an_offset_would_wrap holds
SEED = {1: 1021, 2: 1002, 3: 1003, 9: 1009, 14: 1014, 31: 1031, 32: 1032}
# (shape, kind, width) of every generated column that lies across a crossing
INPUTS = [(shape, "splitmix", c) for shape in ("rows", "bits", "bytes") for c in SHAPE_WIDTHS[shape]] + [("bits", "index", 31)]
# the narrow operands beside them, and the 2^32-row column of sort_rows: their own offsets cross nothing, but a wrapped ROW index
# (the crossing row as a row count) must read other values there too
NARROW_INPUTS = [("bits", 9), ("bits", 14), ("bytes", 3), ("bytes", 1), ("sort", 2)]


def test_shapes_are_ragged_where_they_should_be():
    assert RAG == 51277 and RAG // CHUNK == 3 and RAG % CHUNK // TILE == 1 and RAG % TILE == 77
    assert 77 % 32 == 13 and 77 % 8 == 5
    assert N_ROWS - (1 << 32) == RAG and N_ROWS_MAX % TILE == TILE - 1 and N_SORT % CHUNK == 0
    assert (X_BITS - 1) * 31 < 1 << 32 <= X_BITS * 31
    assert (X_BITS - 1) * 31 % 32 + 31 > 32                      # the value in front of bit 2^32 straddles two dwords, and the crossing
    assert ((X_BITS - 1) * 31 + 31) > 1 << 32
    assert (N_BITS - RAG) % CHUNK == 0 and 0 <= N_BITS - RAG - X_BITS < CHUNK
    assert N_BITS * 31 / 8 < 540e6
    assert (1 << 29) * 4 == 1 << 31 and (1 << 30) * 4 == 1 << 32 and N_BYTES - (1 << 30) == RAG
    assert N_POS - (1 << 31) == RAG and N_POS < 1 << 32
    for n in (N_ROWS, N_BITS, N_BYTES, N_POS):
        assert n % CHUNK == RAG % CHUNK and n % TILE == 77
    assert S % 128 == 0 and N_SMALL % 8192 == 1237


def wrapped_window(O, kind, c, seed, row, crossing_bits, W=4096):
    """the W values a kernel would decode at `row` had its bit offset lost `crossing_bits`"""
    start = row * c - crossing_bits
    assert 0 <= start < 64 * c
    rows = start // c + W + 2
    stream = np.unpackbits(O.pack(O.gen_values(kind, rows, c, seed), c), bitorder="little")
    bits = stream[start: start + W * c].reshape(W, c).astype(np.uint64)
    return (bits << np.arange(c, dtype=np.uint64)).sum(axis=1)


@pytest.mark.parametrize("shape,kind,c", INPUTS)
def test_inputs_differ_where_an_offset_would_wrap(O, shape, kind, c):
    """a window of 4096 rows at each crossing differs in more than half of its rows from what the wrapped offset would read"""
    seed = SEED[c] if kind == "splitmix" else 0
    for row, crossing_bits in CROSSINGS[shape](c):
        true = O.gen_values(kind, 4096, c, seed, first=row).astype(np.uint64)
        wrapped = wrapped_window(O, kind, c, seed, row, crossing_bits)
        assert (true != wrapped).mean() > 0.5, (shape, c, row)


@pytest.mark.parametrize("shape,c", NARROW_INPUTS)
def test_narrow_inputs_differ_where_a_row_index_would_wrap(O, shape, c):
    """the narrow operand of a two-column case, in windows of 4096 rows at the wide operand's crossing rows: had the ROW index
    wrapped there (back to row 0), more than half of the rows would read another value"""
    rows = [1 << 31] if shape == "sort" else [row for row, _ in CROSSINGS[shape](c)]
    for row in rows:
        true = O.gen_values("splitmix", 4096, c, SEED[c], first=row)
        wrapped = O.gen_values("splitmix", 4096, c, SEED[c], first=0)
        assert (true != wrapped).mean() > 0.5, (shape, c, row)


# ---- the case table: every entry point and its cases; each test below takes its cases from here --------------------------------

CASES = {
    "mi355_shared_scan_where_dev": ["rows", "bits", "bits-capped", "bytes"],
    "mi355_scan_columns_dev": ["bytes_vs_1", "rows_1_vs_2", "9_vs_bits", "9_vs_bits-capped"],
    "mi355_group_aggregate_dev": ["bytes", "rows"],
    "mi355_group_aggregate_wide_dev": ["bits", "bits-capped", "rows"],
    "mi355_semijoin_dev": ["bits", "bits-capped", "bytes_table", "rows", "table"],
    "mi355_lookup_dev": ["bytes", "out", "table31", "table31-capped", "bytes_table"],
    "mi355_compact_dev": ["bytes", "rows"],
    "mi355_arith_dev": ["mul_out", "linear_rows"],
    "mi355_top_k_dev": ["rows", "bits", "bits-capped", "bytes"],
    "mi355_sort_rows_dev": ["rows", "bytes"],
    "mi355_value_set_dev": ["bits", "bits-capped", "bytes", "rows"],
    "mi355_set_ranks_dev": ["table"],
    "mi355_key_index_dev": ["rows"],
    "mi355_running_sum_dev": ["rows_all", "rows_mask", "positions"],
    "mi355_delta_dev": ["bits", "bits-capped", "bytes", "rows"],
    "mi355_run_encode_dev": ["rows", "bits", "bits-capped"],
    "mi355_run_decode_dev": ["rows", "rows_uncovered", "bits", "bits-capped"],
    "mi355_search_sorted_dev": ["bytes_edges", "rows", "table", "table-capped"],
    "mi355_run_aggregate_dev": ["bytes", "rows"],
    "mi355_gather_dev": ["rows", "bits", "first_row"],
    "mi355_aggregate_dev": ["rows", "bits", "bits-capped"],
    "mi355_histogram_dev": ["rows"],
    "mi355_bitmap_combine_dev": ["rows"],
    "mi355_bitmap_count_dev": ["rows"],
    "mi355_pack_u32_dev": ["bits", "bits-capped"],
    "mi355_pack_u16_dev": ["rows"],
}

_PARITY = "covered by test_more_than_2_pow_32_rows"
_ROUND2 = "covered by test_more_than_2_pow_32_rows_round2_kernels"
_FORWARDS = "forwards to mi355_scan_combine_dev, " + _ROUND2
_GENERATED = "checked against the oracle by every case here, across every crossing"
_MEASURES = "has no kernel of its own: it times the scan and decompress kernels " + _PARITY
REASONS = (_PARITY, _ROUND2, _FORWARDS, _GENERATED, _MEASURES, "host-pointer drop-in")  # a reason is one of these, to the letter
EXEMPT = {
    "mi355_scan_eq_dev": _PARITY,
    "mi355_scan_range_dev": _PARITY,
    "mi355_scan_combine_dev": _ROUND2,
    "mi355_scan_where_dev": _FORWARDS,
    "mi355_scan_in_dev": _ROUND2,
    "mi355_scan2_dev": _ROUND2,
    "mi355_scan_select_dev": _ROUND2,
    "mi355_shared_scan_eq_dev": _ROUND2,
    "mi355_decompress_dev": _ROUND2,
    "mi355_bitmap_to_rowids_dev": _PARITY,
    "mi355_generate_dev": _GENERATED,
    "mi355_tune_dev": _MEASURES,
}


def row_count_entry_points():
    """every exported mi355_*_dev whose declaration takes a row, entry or run count by value"""
    found = []
    for header in sorted(h for h in os.listdir(INCLUDE) if h.endswith(".h")):
        text = header_text(header)
        for name in declared(header):
            if not name.endswith("_dev"):
                continue
            args = re.search(rf"\b{name}\(([^;]*?)\);", text, flags=re.S).group(1)
            if re.search(r"\buint64_t (n|rows|runs|set_bits|table_rows)\b", args):
                found.append(name)
    return found


def test_every_entry_point_that_takes_a_row_count_has_a_large_case():
    names = row_count_entry_points()
    assert len(names) > 30 and "mi355_lookup_dev" in names and "mi355_set_ranks_dev" in names
    for name in names:
        assert (name in CASES) != (name in EXEMPT), f"{name}: give it a case in CASES (or, for a round-1/2 kernel, a reason in EXEMPT)"
        if name in CASES:
            assert CASES[name], name
            test = globals().get("test_" + name[len("mi355_"): -len("_dev")])
            assert test is not None, f"{name}: no test function runs its cases"
            marks = [m for m in test.pytestmark if m.name == "parametrize"]
            assert marks and list(marks[0].args[1]) == CASES[name], name
            assert any(m.name == "gpu" for m in test.pytestmark), name
        else:
            assert EXEMPT[name] in REASONS, name
    assert set(CASES) | set(EXEMPT) <= set(names), sorted((set(CASES) | set(EXEMPT)) - set(names))


def test_size_functions_do_not_wrap(L):
    """the pure size functions of the C API at every shape's row count, against their formulas written out; monotone in n"""
    ceil = lambda a, b: -(-a // b)
    prefix = lambda n: ceil(n, 16384) + 1 + ceil(n, 16777216)
    sizes = sorted([N_SMALL, N_BITS, N_BYTES, N_POS, N_ROWS_MAX, N_SORT, N_ROWS])
    for f in (L.mi355_running_sum_workspace_words, L.mi355_run_encode_workspace_words):
        got = [f(n) for n in sizes]
        assert got == [prefix(n) for n in sizes] and got == sorted(got)
    for c in (1, 2, 8, 9, 16, 17, 24, 25, 32):
        passes = ceil(c, 8)
        assert L.mi355_sort_rows_passes(c) == passes
        assert L.mi355_top_k_passes(c) == (1 if c <= 12 else 2 if c <= 24 else 3)
        last = 0
        for n in [s for s in sizes if s <= N_SORT]:
            for capacity in (100_000, n):
                spans = ceil(n, 16384)
                counters = spans << min(c, 8)
                want = counters + 1 + ceil(counters, 1024) + 8 + min(passes - 1, 2) * min(capacity, n)  # counters, their prefix, the state
                got = L.mi355_sort_rows_workspace_words(n, capacity, c)
                assert got == want, (n, capacity, c, got, want)
            assert got >= last
            last = got
        assert L.mi355_sort_rows_workspace_words(N_SORT + 1, 1, c) == 0  # what the call refuses
    for n in sizes:
        assert L.mi355_compressed_buffer_size(31, n) == ceil(31 * n, 8) + 256
        assert L.mi355_compressed_buffer_size(32, n) == 4 * n + 256
        assert L.mi355_bitmap_stride(n) == ceil(ceil(n, 8), 256) * 256
    lds = header_macro("mi355_search.h", "MI355_SEARCH_LDS_MAX_BYTES")
    strides = []
    for rows in (256, lds // 4, lds // 4 + 1, X_BITS, N_BITS, N_ROWS_MAX):
        want = 1
        while (rows // want) * 4 > lds:  # the smallest power of two with floor(rows / S) * 4 <= the LDS bound
            want *= 2
        strides.append(L.mi355_search_sorted_stride(rows))
        assert strides[-1] == want, rows
    assert strides == sorted(strides) and strides[1] == 1 and strides[2] == 2 and strides[-1] > 1 << 16
    # the kernel families chosen by a set's or a table's size: the LDS tier for a few entries, the global one from some size on
    # and up to 2^32 entries, nothing (NULL) beyond -- no size in between falls back
    table_sizes = [6, 256, 1 << 20, N_BITS, 1 << 31, N_POS, N_ROWS_MAX, 1 << 32]
    for stem, family in (("semijoin", lambda s: L.mi355_semijoin_kernel(32, s)), ("value_set", lambda s: L.mi355_value_set_kernel(32, s)),
                         ("lookup", lambda s: L.mi355_lookup_kernel(32, s, 31)), ("key_index", lambda s: L.mi355_key_index_kernel(32, s))):
        got = [family(s) for s in table_sizes]
        assert got[0] == f"{stem}_lds_kernel".encode() and got[-1] == f"{stem}_global_kernel".encode(), (stem, got)
        tiers = [g == f"{stem}_global_kernel".encode() for g in got]
        assert all(g in (f"{stem}_lds_kernel".encode(), f"{stem}_global_kernel".encode()) for g in got) and tiers == sorted(tiers), (stem, got)
        assert family((1 << 32) + 1) is None and family(N_ROWS) is None, stem
    # running_sum: every partial sum lies in [k + n min(0, b), k + n max(0, 2^c - 1 + b)]; inside [0, 2^co) the exact kernel,
    # inside int64 the checked one, else the call is refused
    def running_want(c, n, b, k, co):
        lo, hi = k + n * min(0, b), k + n * max(0, (1 << c) - 1 + b)
        if lo < -(1 << 63) or hi >= 1 << 63:
            return None
        return b"running_sum_exact_kernel" if 0 <= lo and hi < 1 << co else b"running_sum_checked_kernel"
    seen = set()
    for c, b, k, co in ((1, 0, 0, 32), (1, 0, 0, 31), (3, 0, 0, 9), (3, 0, 0, 12), (32, 0, 0, 32), (31, -5, 1 << 40, 32)):
        for n in (N_SMALL, N_BITS, N_BYTES, N_POS, N_ROWS_MAX, 1 << 32, N_ROWS):
            got = L.mi355_running_sum_kernel(c, n, b, k, co)
            assert got == running_want(c, n, b, k, co), (c, n, b, k, co, got)
            seen.add(got)
    assert seen == {None, b"running_sum_exact_kernel", b"running_sum_checked_kernel"}
    assert L.mi355_running_sum_kernel(1, N_POS, 0, 0, 32) == b"running_sum_exact_kernel"      # row_positions' case
    assert L.mi355_running_sum_kernel(1, 1 << 32, 0, 0, 32) == b"running_sum_checked_kernel"  # one row more: a position of 2^32
    assert L.mi355_running_sum_kernel(3, N_ROWS, 0, 0, 9) == b"running_sum_checked_kernel"
    assert L.mi355_search_sorted_kernel(32, 31, 32, N_BITS) == b"search_global_kernel"
    assert L.mi355_search_sorted_kernel(32, 32, 9, 256) == b"search_lds_kernel"
    assert L.mi355_search_sorted_kernel(32, 31, 32, 1 << 32) is None


# ---- the routes against numpy, on the CPU ---------------------------------------------------------------------------------------

def small_slices(n=N_SMALL, step=4 * 8192 + 40):
    return [(i, min(n, i + step)) for i in range(0, n, step)]


def t64(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int64))


def test_routes_pack_and_bitmaps_match_numpy(O):
    import torch

    rng = rng_of("pack")
    for c in (1, 2, 3, 9, 12, 14, 31, 32):
        v = rng.integers(0, 1 << c, N_SMALL, dtype=np.uint64).astype(np.uint32)
        assert np.array_equal(R.pack_values(t64(v), c).numpy(), payload(v, c)), c
        assert np.array_equal(R.u32(torch.from_numpy(v.view(np.int32))).numpy(), v.astype(np.int64))
    bits = rng.integers(0, 2, N_SMALL).astype(bool)
    bm = R.pack_bitmap(torch.from_numpy(bits))
    assert np.array_equal(bm.numpy(), packbits(bits))
    assert np.array_equal(R.unpack_bitmap(bm, N_SMALL).numpy(), bits)
    assert R.popcount(bm, step=1000) == int(bits.sum())
    rows = np.nonzero(rng.integers(0, 50, N_SMALL) == 0)[0]
    sparse = np.zeros(N_SMALL, dtype=bool)
    sparse[rows] = True
    for invert in (False, True):
        got = R.bitmap_of_rows(t64(rows), N_SMALL, pad=32, invert=invert).numpy()
        assert np.array_equal(got[: (N_SMALL + 7) // 8], packbits(sparse != invert)) and not got[(N_SMALL + 7) // 8:].any()


def test_routes_rowwise_match_numpy():
    import torch

    rng = rng_of("rowwise")
    v = rng.integers(0, 1 << 32, N_SMALL, dtype=np.uint64).astype(np.int64)
    for op, a, b in (("==", int(v[5]), 0), ("!=", int(v[5]), 0), ("<", 1 << 31, 0), ("<=", int(v[7]), 0), (">", 1 << 30, 0), (">=", int(v[9]), 0),
                     ("between", 1 << 30, 1 << 31), ("not_between", 1 << 30, 1 << 31)):
        assert np.array_equal(R.pred(t64(v), op, a, b).numpy(), pred(v, op, a, b)), op
    r = v - (1 << 31)
    got, replaced = R.fit(t64(r), 31, 77)
    bad = (r < 0) | (r >= 1 << 31)
    assert np.array_equal(got.numpy(), np.where(bad, 77, r)) and replaced == int(bad.sum())
    member = rng.integers(0, 2, 5000).astype(bool)
    probe = rng.integers(0, 6000, N_SMALL)
    got = R.member(torch.from_numpy(packbits(member)), t64(probe), 5000).numpy()
    assert np.array_equal(got, (probe < 5000) & member[np.minimum(probe, 4999)])
    table = rng.integers(0, 8, 5000)
    got = R.table_value(t64(table).to(torch.uint8), t64(probe), 6).numpy()
    assert np.array_equal(got, np.where(probe < 5000, table[np.minimum(probe, 4999)], 6))
    srt = np.sort(rng.integers(0, 1 << 32, 300, dtype=np.uint64).astype(np.int64))
    srt[10:14] = srt[10]
    probe = np.concatenate([v[:5000], srt])
    for side in ("left", "right"):
        pos, found = R.search_sorted(t64(srt), t64(probe), side=side)
        assert np.array_equal(pos.numpy(), np.searchsorted(srt, probe, side=side))
        assert np.array_equal(found.numpy(), np.isin(probe, srt))
        pos, _ = R.search_sorted(t64(srt), t64(probe), side=side, exact=True, miss=999)
        assert np.array_equal(pos.numpy(), np.where(np.isin(probe, srt), np.searchsorted(srt, probe, side=side), 999))


def test_routes_with_a_carry_match_numpy():
    import torch

    rng = rng_of("carry")
    v = rng.integers(0, 8, N_SMALL).astype(np.int64)
    sel = rng.integers(0, 2, N_SMALL).astype(bool)
    keys = rng.integers(0, 40, N_SMALL).astype(np.int64)
    # grouped aggregates, with and without a selection; keys >= groups are dropped
    keys = np.concatenate([keys[:-3000], rng.integers(0, 200, 3000)])  # (both sides of R.DENSE, and keys beyond every table)
    for groups, use in ((40, None), (40, sel), (33, sel), (150, sel), (200, None)):
        acc = R.Grouped(groups, "cpu")
        for i0, i1 in small_slices():
            acc.step(t64(keys[i0:i1]), t64(v[i0:i1]), None if use is None else torch.from_numpy(use[i0:i1]))
        counted = (np.ones(N_SMALL, dtype=bool) if use is None else use) & (keys < groups)
        assert np.array_equal(acc.table().numpy().astype(np.uint64), grouped(keys, v, groups, counted))
        assert acc.dropped == int(((np.ones(N_SMALL, dtype=bool) if use is None else use) & (keys >= groups)).sum())
    acc = [0, 0, -1, 0]
    for i0, i1 in small_slices():
        acc = R.aggregate(acc, t64(v[i0:i1] + 3), torch.from_numpy(sel[i0:i1]))
    assert acc == [int((v[sel] + 3).sum()), int(sel.sum()), int(v[sel].min()) + 3, int(v[sel].max()) + 3]
    # running sums and differences
    for b, k, exclusive, use in ((0, 0, False, None), (-3, 1000, True, sel), (2, 5, False, sel)):
        rs = R.RunningSum(b=b, k=k, exclusive=exclusive)
        got = np.concatenate([rs.step(t64(v[i0:i1]), None if use is None else torch.from_numpy(use[i0:i1])).numpy() for i0, i1 in small_slices()])
        term = np.where(np.ones(N_SMALL, dtype=bool) if use is None else use, v + b, 0)
        incl = np.cumsum(term) + k
        assert np.array_equal(got, incl - term if exclusive else incl) and rs.total == int(incl[-1])
    d = R.Delta(first=5, k=7)
    got = np.concatenate([d.step(t64(v[i0:i1])).numpy() for i0, i1 in small_slices()])
    assert np.array_equal(got, np.diff(np.concatenate([[5], v])) + 7)
    # runs: a run-structured column, with a boundary on a slice edge and none on the next
    lens = rng.integers(1, 400, 2000)
    vals = rng.integers(0, 8, 2000)
    vals[1:][vals[1:] == vals[:-1]] ^= 1
    col = np.repeat(vals, lens)[:N_SMALL]
    assert len(col) == N_SMALL
    runs = R.Runs()
    for i0, i1 in small_slices():
        runs.step(t64(col[i0:i1]))
    rv, re_ = runs.tables()
    cut = np.nonzero(np.diff(col))[0]
    want_ends = np.concatenate([cut + 1, [N_SMALL]])
    assert np.array_equal(re_.numpy(), want_ends) and np.array_equal(rv.numpy(), col[want_ends - 1])
    for i0, i1 in small_slices(N_SMALL + 500):
        got, behind = R.run_decode(rv, re_, i0, i1, 6)
        want = np.concatenate([col, np.full(500, 6)])[i0:i1]
        assert np.array_equal(got.numpy(), want) and behind == max(0, i1 - max(i0, N_SMALL))
        assert np.array_equal(R.run_of_rows(re_, i0, i1).numpy(), np.searchsorted(want_ends, np.arange(i0, i1), side="right"))
    # top_k, both directions, the cut among ties; sort_rows; key_index; set_ranks; value_set
    for largest, k in ((True, 30000), (False, 12345), (True, 10 ** 9), (False, 0)):
        hist = torch.bincount(t64(v[sel]), minlength=8)
        result = R.top_k_result(hist, k, largest)
        want_bits, want = top_k_expect(v, sel, k, largest)
        assert result == want
        tk = R.TopK(result, largest)
        got = np.concatenate([tk.step(t64(v[i0:i1]), torch.from_numpy(sel[i0:i1])).numpy() for i0, i1 in small_slices()])
        assert np.array_equal(got, want_bits), (largest, k)
    wide = rng.integers(0, 1 << 20, N_SMALL).astype(np.int64)
    wide[::7] = wide[3]  # ties at what becomes a threshold
    for largest, k in ((True, 9000), (False, 10500), (True, 3), (False, 10 ** 9)):
        high = torch.bincount(t64(wide[sel] >> 16), minlength=16)
        low_of = lambda h: torch.bincount(t64(wide[sel & (wide >> 16 == h)] & 0xFFFF), minlength=1 << 16)
        assert R.top_k_result_wide(high, low_of, k, largest) == top_k_expect(wide, sel, k, largest)[1], (largest, k)
    rows = np.nonzero(sel)[0]
    for descending in (False, True):
        got_rows, got_vals = R.sort_rows(t64(rows), t64(v[rows]), descending)
        order = np.lexsort((rows, -v[rows] if descending else v[rows]))
        assert np.array_equal(got_rows.numpy(), rows[order]) and np.array_equal(got_vals.numpy(), v[rows][order])
    for keep in ("first", "last"):
        for table_rows, ct, first_row in ((40, 32, 0), (33, 16, 100), (150, 17, 100), (200, 32, 0)):
            ki = R.KeyIndex(table_rows, keep, "cpu")
            for i0, i1 in small_slices():
                ki.step(t64(keys[i0:i1]), i0, torch.from_numpy(sel[i0:i1]))
            table, counts = ki.table(ct, 9, first_row)
            want_table, want_counts = key_index_expect(keys, sel, table_rows, keep, first_row, ct, 9)
            assert np.array_equal(table.numpy(), want_table) and counts == want_counts
    sr = R.SetRanks(12, 4095)
    got = np.concatenate([sr.step(torch.from_numpy(sel[i0:i1])).numpy() for i0, i1 in small_slices()])
    rank = np.cumsum(sel) - 1
    assert np.array_equal(got, np.where(sel & (rank < 4096), rank, 4095))
    assert sr.counts == [int(sel.sum()), int((sel & (rank >= 4096)).sum())]
    flags = torch.zeros(30, dtype=torch.bool)
    beyond = sum(R.value_set(flags, t64(keys[i0:i1]), 30, torch.from_numpy(sel[i0:i1])) for i0, i1 in small_slices())
    assert np.array_equal(np.nonzero(flags.numpy())[0], np.unique(keys[sel & (keys < 30)])) and beyond == int((sel & (keys >= 30)).sum())


# GPU
# ---- what the GPU cases share ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def capped():
    """one block of four waves: a wave walks across the crossing with a previous tile's values still in its LDS"""
    from shared_simd_scan_amd import ScanEngine

    e = ScanEngine(0)
    e.set_option("grid_cus", 1)
    e.set_option("max_blocks_per_cu", 1)
    yield e
    e.close()


@pytest.fixture
def budget():
    """every case starts from an empty cache, stays below 16 GiB of device memory and leaves an empty cache"""
    import torch

    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    peak = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()
    assert peak < 16 << 30, f"peak device memory {peak / 2 ** 30:.2f} GiB"


def pick(case, eng, capped):
    return (capped if case.endswith("-capped") else eng), case.split("-")[0]


def windows(n, crossing_rows):
    """(first row, rows) of the host windows: row 0, two tiles either side of each crossing, the ragged end"""
    if n <= 8 * TILE:
        return [(0, n)]
    out = [(0, 4 * TILE)]
    for x in crossing_rows:
        if x < n:
            a = (x // TILE - 2) * TILE
            out.append((a, min(5 * TILE, n - a)))
    a = (n // TILE - 2) * TILE
    out.append((a, n - a))
    return out


def crossing_rows(shape, c):
    return [row for row, _ in CROSSINGS[shape](c)]


def generated(eng, O, n, c, rows=(), kind="splitmix"):
    """a generated column, checked against the oracle's generator and packer in every window"""
    seed = SEED[c] if kind == "splitmix" else 0
    col = eng.generate(kind, n, c, seed)
    for a, ln in windows(n, rows):
        have = col.data[a * c // 8: a * c // 8 + (ln * c + 7) // 8].cpu().numpy()
        assert np.array_equal(have, payload(O.gen_values(kind, ln, c, seed, first=a), c)), (n, c, a)
    return col


def shape_column(eng, O, shape, c, n=None):
    return generated(eng, O, SHAPE_ROWS[shape] if n is None else n, c, crossing_rows(shape, c))


def host(O, c, a, ln, kind="splitmix"):
    return O.gen_values(kind, ln, c, SEED[c] if kind == "splitmix" else 0, first=a).astype(np.int64)


def slices(n, step=S):
    return [(i, min(n, i + step)) for i in range(0, n, step)]


def decoded(eng, col, i0, i1):
    return R.u32(eng.decompress(eng.slice_rows(col, i0, i1)))


def bit_slice(bitmap, i0, i1):
    """rows [i0, i1) of a bitmap (i0 a multiple of 8) as bool"""
    return R.unpack_bitmap(bitmap[i0 // 8: (i1 + 7) // 8], i1 - i0)


def same_bitmap(bm, i0, i1, bits):
    import torch

    return torch.equal(bm[i0 // 8: (i1 + 7) // 8], R.pack_bitmap(bits))


def same_packed(out, co, i0, i1, values):
    import torch

    return torch.equal(out[i0 * co // 8: (i1 * co + 7) // 8], R.pack_values(values, co))


def window_bitmap(bm, a, ln):
    return bm[a // 8: a // 8 + (ln + 7) // 8].cpu().numpy()


def window_packed(out, co, a, ln):
    return out[a * co // 8: a * co // 8 + (ln * co + 7) // 8].cpu().numpy()


def random_bitmap(n, seed, ands=1, pad=32, force=()):
    """a canonical bitmap of n rows of density 2^-ands from torch's generator, `force` rows set, `pad` zero bytes behind it"""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    nb = (n + 7) // 8
    m = torch.randint(0, 256, (nb + pad,), dtype=torch.uint8, device="cuda", generator=g)
    for _ in range(ands - 1):
        m &= torch.randint(0, 256, (nb + pad,), dtype=torch.uint8, device="cuda", generator=g)
    for r in force:
        m[r >> 3] |= 1 << (r & 7)
    m[nb:] = 0
    if n % 8:
        m[nb - 1] &= (1 << (n % 8)) - 1
    return m


def sparse_rows(n, count, seed, force=()):
    """`count` random rows of [0, n) and the `force` rows, sorted and distinct -> int64 device tensor"""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    r = torch.randint(0, n, (count,), dtype=torch.int64, device="cuda", generator=g)
    return torch.unique(torch.cat([r, torch.tensor(sorted(force), dtype=torch.int64, device="cuda")]))


def near(n, *xs):
    """rows to force: a few either side of each x, and the first and last rows of the column"""
    rows = {0, 1, n - 1, n - 2, n - 9}
    for x in xs:
        rows |= {x - 2, x - 1, x, x + 1, x + 31}
    return sorted(r for r in rows if 0 <= r < n)


def bit_column(bitmap, n):
    """a bitmap with at least 256 bytes behind its payload, as a column of 1-bit values"""
    from shared_simd_scan_amd.engine import PackedColumn

    assert bitmap.numel() >= (n + 7) // 8 + 256
    return PackedColumn(bitmap, n, 1)


def words(t):
    return [int(x) for x in t.cpu().tolist()]


def as_i64(g, *shape):
    import torch

    return g.body.view(torch.int64).view(*shape)


# ---- the cases ------------------------------------------------------------------------------------------------------------------

WHERE = {"rows": 3, "bits": 31, "bytes": 32}


@gpu
@pytest.mark.parametrize("case", CASES["mi355_shared_scan_where_dev"])
def test_shared_scan_where(O, L, eng, capped, budget, case):
    """three mixed predicates, both layouts, with hit counts; every bitmap byte against decompress -> torch"""
    e, shape = pick(case, eng, capped)
    c, n = WHERE[shape], SHAPE_ROWS[shape]
    top = 1 << c
    preds = [("between", top // 4, top // 2), (">=", top // 3), ("!=", 5)]
    P, nb, stride = len(preds), (n + 7) // 8, L.mi355_bitmap_stride(n)
    col = shape_column(eng, O, shape, c)
    gp, gl = Guarded(P * stride), Guarded(nb * P)
    per, hits_p = e.shared_scan_where(preds, col, out=gp.body.view(P, stride))
    lin, hits_l = e.shared_scan_where(preds, col, layout="linear", out=gl.body)
    assert gp.guards_intact() and gl.guards_intact()
    lin = lin.view(-1, P)
    want_hits = [0] * P
    for i0, i1 in slices(n):
        v = decoded(eng, col, i0, i1)
        for k, p in enumerate(preds):
            bits = R.pred(v, *p)
            want_hits[k] += int(bits.sum().item())
            assert same_bitmap(per[k], i0, i1, bits), (k, i0)
            assert same_bitmap(lin[:, k], i0, i1, bits), (k, i0)
    assert words(hits_p) == want_hits and words(hits_l) == want_hits
    for a, ln in windows(n, crossing_rows(shape, c)):
        v = host(O, c, a, ln)
        for k, p in enumerate(preds):
            want = packbits(pred(v, *p))
            assert np.array_equal(window_bitmap(per[k], a, ln), want), (k, a)
            assert np.array_equal(window_bitmap(lin[:, k].contiguous(), a, ln), want), (k, a)


# (shape of the crossing column, c1, c2, which of the two crosses, op, a, b)
COLUMNS = {"bytes_vs_1": ("bytes", 32, 1, 1, "between", 0, 1 << 31), "rows_1_vs_2": ("rows", 1, 2, 1, "<", 0, 0),
           "9_vs_bits": ("bits", 9, 31, 2, "<", -(1 << 30), 0)}


@gpu
@pytest.mark.parametrize("case", CASES["mi355_scan_columns_dev"])
def test_scan_columns(O, eng, capped, budget, case):
    """(col1 - col2) OP a, b over two widths: the wide column crosses, the other stays narrow (ROWS: both cross in rows)"""
    e, name = pick(case, eng, capped)
    shape, c1, c2, _, op, a, b = COLUMNS[name]
    n = SHAPE_ROWS[shape]
    rows = crossing_rows(shape, c1)
    col1, col2 = generated(eng, O, n, c1, rows), generated(eng, O, n, c2, rows)
    g = Guarded((n + 7) // 8)
    bm, hits = e.scan_columns(col1, op, col2, a=a, b=b, bitmap=g.body)
    assert g.guards_intact()
    total = 0
    for i0, i1 in slices(n):
        bits = R.pred(decoded(eng, col1, i0, i1) - decoded(eng, col2, i0, i1), op, a, b)
        total += int(bits.sum().item())
        assert same_bitmap(bm, i0, i1, bits), i0
    assert words(hits) == [total]
    for w0, ln in windows(n, rows):
        want = packbits(pred(host(O, c1, w0, ln) - host(O, c2, w0, ln), op, a, b))
        assert np.array_equal(window_bitmap(bm, w0, ln), want), w0


def skewed_pair(n):
    """keys and values of one bit each, made by torch: nearly every key 0, nearly every value 1 -- group 0's count and sum pass
    2^32 -- with ones (keys) and zeros (values) forced either side of rows 2^31 and 2^32 and in the last rows"""
    key_rows = sparse_rows(n, 20000, 71, near(n, 1 << 31, 1 << 32))
    zero_rows = sparse_rows(n, 10000, 72, near(n, (1 << 31) + 64, (1 << 32) + 64))
    return R.bitmap_of_rows(key_rows, n, pad=256), R.bitmap_of_rows(zero_rows, n, pad=256, invert=True), key_rows, zero_rows


def grouped_rows_case(e, n, groups, call):
    """group 0 of a 1-bit key holds more than 2^32 rows, and more than 2^32 ones"""
    import torch

    keys, values, key_rows, zero_rows = skewed_pair(n)
    g = Guarded(groups * 32)
    call(bit_column(keys, n), bit_column(values, n), as_i64(g, groups, 4))
    assert g.guards_intact()
    acc = R.Grouped(groups, "cuda")
    for i0, i1 in slices(n):
        acc.step(bit_slice(keys, i0, i1).to(torch.int64), bit_slice(values, i0, i1).to(torch.int64))
    assert torch.equal(as_i64(g, groups, 4), acc.table())
    # the same table from how the columns were made: numpy over the forced and random rows alone
    kr, zr = key_rows.cpu().numpy(), zero_rows.cpu().numpy()
    both = len(np.intersect1d(kr, zr))
    ones = [n - len(kr) - (len(zr) - both), len(kr) - both]
    want = [[ones[0], n - len(kr), 0 if len(zr) > both else 1, 1], [ones[1], len(kr), 0 if both else 1, 1]]
    assert as_i64(g, groups, 4).cpu().tolist() == want
    assert want[0][0] > 1 << 32 and want[0][1] > 1 << 32


def grouped_wide_column_case(e, O, shape, ck, cv, groups, call):
    import torch

    n = SHAPE_ROWS[shape]
    rows = crossing_rows(shape, cv)
    keys, values = generated(e, O, n, ck, rows), generated(e, O, n, cv, rows)
    g = Guarded(groups * 32)
    call(keys, values, as_i64(g, groups, 4))
    assert g.guards_intact()
    acc = R.Grouped(groups, "cuda")
    for i0, i1 in slices(n):
        acc.step(decoded(e, keys, i0, i1), decoded(e, values, i0, i1))
    got = as_i64(g, groups, 4)
    assert torch.equal(got, acc.table())
    assert int(got[:, 1].sum().item()) == n
    # host: the rows of the windows alone can only bound the table -- a group's min / max lie outside or on the window's
    table = got.cpu().numpy()
    for a, ln in windows(n, rows):
        w = grouped(host(O, ck, a, ln), host(O, cv, a, ln), groups)
        seen = w[:, 1] > 0
        assert (table[seen, 2].astype(np.uint64) <= w[seen, 2]).all() and (table[seen, 3].astype(np.uint64) >= w[seen, 3]).all()
        assert (table[:, 1].astype(np.uint64) >= w[:, 1]).all()


@gpu
@pytest.mark.parametrize("case", CASES["mi355_group_aggregate_dev"])
def test_group_aggregate(O, eng, budget, case):
    """bytes: 32-bit values across byte 2^31 and 2^32 under 3-bit keys; rows: 1-bit keys and values on 2^32 + RAG rows.  The
    host windows cannot give a group's aggregates over all rows (no host generates 2^30 values here), so they bound the table:
    counts at least, minima at most and maxima at least the windows' own; the `rows` table is also derived on the host from the
    rows torch placed"""
    if case == "rows":
        grouped_rows_case(eng, N_ROWS, 2, lambda k, v, out: eng.group_aggregate(k, v, out=out))
    else:
        grouped_wide_column_case(eng, O, "bytes", 3, 32, 8, lambda k, v, out: eng.group_aggregate(k, v, out=out))


@gpu
@pytest.mark.parametrize("case", CASES["mi355_group_aggregate_wide_dev"])
def test_group_aggregate_wide(O, eng, capped, budget, case):
    """bits: 31-bit values across bit 2^32 under 14-bit keys; rows: as group_aggregate's, with groups = 2"""
    e, name = pick(case, eng, capped)
    if name == "rows":
        grouped_rows_case(eng, N_ROWS, 2, lambda k, v, out: e.group_aggregate_wide(k, v, 2, out=out))
    else:
        grouped_wide_column_case(eng, O, "bits", 14, 31, 1 << 14, lambda k, v, out: e.group_aggregate_wide(k, v, 1 << 14, out=out))


def probe_values(rng, *edges, count=3000, below=1 << 32):
    """a small 32-bit probe: random values below `below` and the values either side of every edge"""
    forced = sorted({x + d for x in edges for d in (-2, -1, 0, 1, 2) if 0 <= x + d < 1 << 32} | {0, (1 << 32) - 1})
    return np.concatenate([rng.integers(0, below, count, dtype=np.uint64), np.array(forced, dtype=np.uint64)]).astype(np.uint32)


@gpu
@pytest.mark.parametrize("case", CASES["mi355_semijoin_dev"])
def test_semijoin(O, eng, capped, budget, case):
    """bits / bytes_table / rows: the column crosses; bytes_table and table: a set of 2^32 bits, whose byte index passes 2^28 and
    whose bit index passes 2^31 -- probed by the 32-bit column, and by a small one with values either side of 2^31 and at 2^32 - 1"""
    import torch

    from shared_simd_scan_amd.engine import PackedColumn

    e, case = pick(case, eng, capped)
    set_bits = {"bits": 1 << 31, "bytes_table": 1 << 32, "rows": 6, "table": 1 << 32}[case]
    if case == "table":
        values = probe_values(rng_of("semijoin"), 1 << 31, 1 << 28, 1 << 30)
        n, c, rows = len(values), 32, []
        col = PackedColumn(plain_pack(O, values, 32), n, 32)
        host_values = lambda a, ln: values[a: a + ln].astype(np.int64)
    else:
        shape = case.split("_")[0]
        c, n = WHERE[shape], SHAPE_ROWS[shape]
        rows = crossing_rows(shape, c)
        col = shape_column(eng, O, shape, c)
        host_values = lambda a, ln: host(O, c, a, ln)
    if set_bits == 6:
        the_set = torch.zeros(64, dtype=torch.uint8, device="cuda")
        the_set[0] = 0b101101
    else:
        force = [0, 1, (1 << 31) - 1, (1 << 31) + 1, set_bits - 1] if case == "table" else []
        the_set = random_bitmap(set_bits, 81, force=[f for f in force if f < set_bits])
    g = Guarded((n + 7) // 8)
    bm, hits = e.semi_join(col, the_set, set_bits, bitmap=g.body)
    assert g.guards_intact()
    total = 0
    for i0, i1 in slices(n):
        bits = R.member(the_set, decoded(eng, col, i0, i1), set_bits)
        total += int(bits.sum().item())
        assert same_bitmap(bm, i0, i1, bits), i0
    assert words(hits) == [total]
    for a, ln in windows(n, rows):
        v = host_values(a, ln)
        inside = v < set_bits
        idx = np.where(inside, v, 0)
        byte = the_set[torch.from_numpy(idx >> 3).cuda()].cpu().numpy()  # the bytes of the INPUT set the window's values name
        assert np.array_equal(window_bitmap(bm, a, ln), packbits(inside & ((byte >> (idx & 7)) & 1).astype(bool))), a


@gpu
@pytest.mark.parametrize("case", CASES["mi355_lookup_dev"])
def test_lookup(O, eng, capped, budget, case):
    """bytes: a 32-bit column across byte 2^31 and 2^32 into a 3-bit table of 2^30 entries; out: a 1-bit column into 32-bit
    entries, so that the OUTPUT crosses them; table31: a 31-bit table whose bit offsets cross 2^32, probed either side;
    bytes_table: a 1-bit table of 2^32 entries (entry index beyond 2^31) probed by the 32-bit column"""
    import torch

    from shared_simd_scan_amd.engine import PackedColumn

    e, case = pick(case, eng, capped)
    rng = rng_of("lookup", case)
    if case == "out":
        n, c, rows = N_BYTES, 1, crossing_rows("bytes", 32)
        col = generated(eng, O, n, 1, rows)
        entries = np.array([0x9E3779B9, 0x7F4A7C15], dtype=np.uint32)
        table, miss = PackedColumn(plain_pack(O, entries, 32), 2, 32), 0
        decoded_table = torch.from_numpy(entries.astype(np.int64)).cuda()
        host_values, host_table = (lambda a, ln: host(O, 1, a, ln)), (lambda v: entries.astype(np.int64)[v])
    elif case == "bytes":
        n, c, rows = N_BYTES, 32, crossing_rows("bytes", 32)
        col = generated(eng, O, n, 32, rows)
        table, miss = generated(eng, O, 1 << 30, 3, [1 << 29]), 5
        decoded_table = torch.cat([decoded(eng, table, i0, i1).to(torch.uint8) for i0, i1 in slices(table.n)])
        host_values = lambda a, ln: host(O, 32, a, ln)
        host_table = lambda v: np.array([int(O.gen_values("splitmix", 1, 3, SEED[3], first=int(x))[0]) if x < 1 << 30 else miss for x in v])
    elif case == "bytes_table":
        n, c, rows = N_BYTES, 32, crossing_rows("bytes", 32)
        col = generated(eng, O, n, 32, rows)
        bits = random_bitmap(1 << 32, 82, pad=256)
        table, miss, decoded_table = PackedColumn(bits, 1 << 32, 1), 0, None
        host_values = lambda a, ln: host(O, 32, a, ln)
        host_table = lambda v: (bits[torch.from_numpy(v >> 3).cuda()].cpu().numpy() >> (v & 7)) & 1
    else:
        values = probe_values(rng, X_BITS, N_BITS, below=N_BITS)
        n, c, rows = len(values), 32, []
        col = PackedColumn(plain_pack(O, values, 32), n, 32)
        table, miss, decoded_table = generated(eng, O, N_BITS, 31, [X_BITS], kind="index"), (1 << 31) - 1, None
        host_values = lambda a, ln: values[a: a + ln].astype(np.int64)
        host_table = lambda v: np.where(v < N_BITS, v, miss)
    ct = table.c
    g = Guarded((n * ct + 7) // 8)
    out = e.lookup(col, table, miss=miss, out=g.body).data
    assert g.guards_intact()
    for i0, i1 in slices(n):
        v = decoded(eng, col, i0, i1)
        if case == "bytes_table":
            want = R.member(table.data, v, 1 << 32).to(torch.int64)
        elif case == "table31":
            want = R.table_value(torch.cat([decoded(eng, table, j0, j1) for j0, j1 in slices(N_BITS)]), v, miss)
        else:
            want = R.table_value(decoded_table, v, miss)
        assert same_packed(out, ct, i0, i1, want), i0
    for a, ln in windows(n, rows):
        assert np.array_equal(window_packed(out, ct, a, ln), payload(host_table(host_values(a, ln)), ct)), a


@gpu
@pytest.mark.parametrize("case", CASES["mi355_compact_dev"])
def test_compact(O, eng, budget, case):
    """bytes: a dense bitmap (all ones but sparse zeros) over 32-bit values, so that input AND output cross byte 2^31 and 2^32;
    rows: a sparse bitmap with selected rows beyond 2^32 and a capacity that cuts inside the last chunk.  The first byte behind
    ceil(min(count, capacity) c / 8) stays 0xEE"""
    import torch

    if case == "bytes":
        n, c, rows = N_BYTES, 32, crossing_rows("bytes", 32)
        zero_rows = sparse_rows(n, 5000, 91, near(n, 1 << 29, 1 << 30))
        bitmap = R.bitmap_of_rows(zero_rows, n, invert=True)
        count = n - zero_rows.numel()
        capacity = count
    else:
        n, c, rows = N_ROWS, 3, crossing_rows("rows", 3)
        last = list(range(n - 2000, n, 7))  # 286 selected rows in the last chunk
        sel_rows = sparse_rows(n, 30000, 92, near(n, 1 << 31, 1 << 32) + last)
        bitmap = R.bitmap_of_rows(sel_rows, n)
        count = sel_rows.numel()
        capacity = count - 150
    col = generated(eng, O, n, c, rows)
    written = (min(count, capacity) * c + 7) // 8
    g = Guarded((capacity * c + 31) // 32 * 4)
    out, got_count = eng.compact(col, bitmap, capacity=capacity, out=g.body)
    assert g.guards_intact() and words(got_count) == [count]
    assert bool((g.body[written:] == SENTINEL).all().item()), "bytes behind the last value written"
    taken = 0
    kept = []
    for i0, i1 in slices(n):
        v = decoded(eng, col, i0, i1)[bit_slice(bitmap, i0, i1)]
        if case == "bytes":
            assert taken * c % 8 == 0
            assert torch.equal(out[taken * 4: (taken + v.numel()) * 4], R.pack_values(v, 32)), i0
        else:
            kept.append(v)
        taken += v.numel()
    assert taken == count
    if case == "rows":
        assert torch.equal(out[:written], R.pack_values(torch.cat(kept)[:capacity], c))
        sel = sel_rows.cpu().numpy()[:capacity]
        t0 = (capacity - 300) // 8 * 8  # host: the first 300 and the last 300-odd values kept, from the oracle's generator
        value_of = lambda some: np.array([int(O.gen_values("splitmix", 1, c, SEED[c], first=int(r))[0]) for r in some])
        assert sel[-1] > 1 << 32 and sel[capacity - 100] > 1 << 32
        assert np.array_equal(out[: 300 * c // 8].cpu().numpy(), payload(value_of(sel[:300]), c)[: 300 * c // 8])
        assert np.array_equal(out[t0 * c // 8: written].cpu().numpy(), payload(value_of(sel[t0:]), c))
    else:
        for a, ln in windows(n, rows):  # host: the selected rows of a window land at (rows in front) - (zeros in front)
            zr = zero_rows.cpu().numpy()
            first = a - int(np.searchsorted(zr, a))
            keep = ~np.isin(np.arange(a, a + ln), zr)
            want = host(O, c, a, ln)[keep]
            assert np.array_equal(out[first * 4: (first + len(want)) * 4].cpu().numpy(), payload(want, 32)), a


@gpu
@pytest.mark.parametrize("case", CASES["mi355_arith_dev"])
def test_arith(O, eng, budget, case):
    """mul_out: 32-bit x times 1-bit y into 32 bits -- input and output cross byte 2^31 and 2^32; linear_rows: 1 bit + 1 bit into
    2 bits on 2^32 + RAG rows (nothing can be replaced in either: the counter reads 0)"""
    if case == "mul_out":
        n, c1, c2, co, op, rows = N_BYTES, 32, 1, 32, "mul", crossing_rows("bytes", 32)
        f = lambda x, y: x * y
    else:
        n, c1, c2, co, op, rows = N_ROWS, 1, 1, 2, "linear", crossing_rows("rows", 1)
        f = lambda x, y: x + y
    col1 = generated(eng, O, n, c1, rows)
    if case == "mul_out":
        col2 = generated(eng, O, n, c2, rows)
        second = lambda i0, i1: decoded(eng, col2, i0, i1)
        host_second = lambda a, ln: host(O, c2, a, ln)
    else:  # the second 1-bit column is a torch-made bitmap: two generated columns of one width would be the same column
        import torch

        y = random_bitmap(n, 110, pad=256, force=near(n, 1 << 31, 1 << 32))
        col2 = bit_column(y, n)
        second = lambda i0, i1: bit_slice(y, i0, i1).to(torch.int64)
        host_second = lambda a, ln: np.unpackbits(window_bitmap(y, a, ln), bitorder="little")[:ln].astype(np.int64)
    g = Guarded((n * co + 7) // 8)
    import torch

    counter = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    out = eng.arith(op, col1, col2, co=co, miss=1, out=g.body, out_of_range=counter).data
    assert g.guards_intact()
    replaced = 0
    for i0, i1 in slices(n):
        want, bad = R.fit(f(decoded(eng, col1, i0, i1), second(i0, i1)), co, 1)
        replaced += bad
        assert same_packed(out, co, i0, i1, want), i0
    assert words(counter) == [replaced]
    for a, ln in windows(n, rows):
        r = f(host(O, c1, a, ln), host_second(a, ln))
        want = np.where((r < 0) | (r >= 1 << co), 1, r)
        assert np.array_equal(window_packed(out, co, a, ln), payload(want, co)), a


@gpu
@pytest.mark.parametrize("case", CASES["mi355_top_k_dev"])
def top_k_wide_case(e, eng, O, shape, c, mask):
    """values too wide for one table of counts: the threshold from two levels of counts (high 15 / 16 bits, then the low 16 of
    the rows in the threshold's bin), the bitmap from R.TopK.  Host: in every window a row that is not equal to the threshold is
    selected exactly when it qualifies and lies beyond it (ties at 31 and 32 bits are a handful; the torch route covers them)"""
    import torch

    n, rows = SHAPE_ROWS[shape], crossing_rows(shape, c)
    col = shape_column(eng, O, shape, c)
    qual = lambda i0, i1: None if mask is None else bit_slice(mask, i0, i1)

    def counts(bins, high=None):
        h = torch.zeros(bins, dtype=torch.int64, device="cuda")
        for i0, i1 in slices(n):
            v, q = decoded(eng, col, i0, i1), qual(i0, i1)
            if q is not None:
                v = v[q]
            v = (v >> 16) if high is None else (v[(v >> 16) == high] & 0xFFFF)
            h += torch.bincount(v, minlength=bins)
        return h

    hist_high = counts(1 << (c - 16))
    total = int(hist_high.sum().item())
    assert total == (n if mask is None else R.popcount(mask))
    k = total // 3 + 7
    for largest in (True, False):
        want = R.top_k_result_wide(hist_high, lambda high: counts(1 << 16, high), k, largest)
        g = Guarded((n + 7) // 8)
        bm, result = e.top_k(col, k, largest=largest, mask=mask, out=g.body)
        assert g.guards_intact()
        assert words(result) == want and want[0] == k
        route = R.TopK(want, largest)
        for i0, i1 in slices(n):
            assert same_bitmap(bm, i0, i1, route.step(decoded(eng, col, i0, i1), qual(i0, i1))), (largest, i0)
        T = want[1]
        for a, ln in windows(n, rows):
            v = host(O, c, a, ln)
            sel = np.ones(ln, dtype=bool) if mask is None else np.unpackbits(window_bitmap(mask, a, ln), bitorder="little")[:ln].astype(bool)
            got = np.unpackbits(window_bitmap(bm, a, ln), bitorder="little")[:ln].astype(bool)
            assert np.array_equal(got[v != T], (sel & ((v > T) if largest else (v < T)))[v != T]), (largest, a)
        assert R.popcount(bm) == k
        del bm, g


@gpu
@pytest.mark.parametrize("case", CASES["mi355_top_k_dev"])
def test_top_k(O, eng, capped, budget, case):
    """bits: the 31-bit column, a third of its rows, largest and smallest; bytes: the 32-bit column under a 1/2 mask; rows:
    2^32 + RAG rows of 2 bits, largest and smallest, k chosen so that the cut falls among the ties inside a chunk beyond row
    2^32.  The host window at row 0 is exact (every tie in front of the cut is taken); the windows behind the cut hold the rows
    strictly beyond the threshold only -- none, the threshold being the extreme value"""
    import torch

    e, case = pick(case, eng, capped)
    if case == "bits":
        return top_k_wide_case(e, eng, O, "bits", 31, None)
    if case == "bytes":
        return top_k_wide_case(e, eng, O, "bytes", 32, random_bitmap(N_BYTES, 111, force=near(N_BYTES, 1 << 29, 1 << 30)))
    n, c = N_ROWS, 2
    rows = crossing_rows("rows", c)
    col = generated(eng, O, n, c, rows)
    cut = (1 << 32) + CHUNK + 1000
    hist = torch.zeros(4, dtype=torch.int64, device="cuda")
    before = {0: 0, 3: 0}
    for i0, i1 in slices(n):
        v = decoded(eng, col, i0, i1)
        hist += torch.bincount(v, minlength=4)
        for T in before:
            before[T] += int((v[: max(0, min(i1, cut) - i0)] == T).sum().item())
    for largest, T in ((True, 3), (False, 0)):
        k = before[T] + 5
        g = Guarded((n + 7) // 8)
        bm, result = eng.top_k(col, k, largest=largest, out=g.body)
        assert g.guards_intact()
        want = R.top_k_result(hist, k, largest)
        assert want == [k, T, 0, int(hist[T].item())] and words(result) == want
        route = R.TopK(want, largest)
        for i0, i1 in slices(n):
            assert same_bitmap(bm, i0, i1, route.step(decoded(eng, col, i0, i1))), (largest, i0)
        for a, ln in windows(n, rows):
            v = host(O, c, a, ln)
            assert a + ln <= cut or a >= cut + CHUNK
            assert np.array_equal(window_bitmap(bm, a, ln), packbits((v == T) & (a < cut))), (largest, a)
        assert R.popcount(bm) == k and R.popcount(bm[(1 << 32) // 8:]) > 5
        del bm, g


@gpu
@pytest.mark.parametrize("case", CASES["mi355_sort_rows_dev"])
def test_sort_rows(O, L, eng, budget, case):
    """rows: n = 2^32 rows of 2 bits under a mask of about 1e5 rows that holds rows either side of 2^31 and the last rows; bytes:
    the 32-bit column under a random 1/1024 mask (four passes, about 1e6 rows).  Both with values: capacity just enough, then
    one too few (all or nothing: not a byte written, the count still given).  Host, rows: complete -- numpy sorts the oracle's
    values of the rows torch selected.  Host, bytes: the output is fetched and must be strictly increasing in (value, row id),
    hold only rows of the mask, as many as the mask has, and for the selected rows of every window the oracle's value"""
    import torch

    if case == "rows":
        n, c, crossings = N_SORT, 2, [1 << 31]
        sel_rows = sparse_rows(n, 100_000, 93, near(n, 1 << 31) + list(range(n - 40, n)))
        mask = R.bitmap_of_rows(sel_rows, n)
    else:
        n, c, crossings = N_BYTES, 32, crossing_rows("bytes", 32)
        mask = random_bitmap(n, 112, ands=10, force=near(n, 1 << 29, 1 << 30))
        sel_rows = torch.cat([torch.nonzero(bit_slice(mask, i0, i1)).view(-1) + i0 for i0, i1 in slices(n)])
        assert 900_000 < sel_rows.numel() < 1_200_000 and sel_rows.numel() == R.popcount(mask)
    col = generated(eng, O, n, c, crossings)
    count = sel_rows.numel()
    got_rows, got_vals = [], []
    for i0, i1 in slices(n):
        idx = torch.nonzero(bit_slice(mask, i0, i1)).view(-1)
        got_rows.append(idx + i0)
        got_vals.append(decoded(eng, col, i0, i1)[idx])
    assert torch.equal(torch.cat(got_rows), sel_rows)
    want_rows, want_vals = R.sort_rows(sel_rows, torch.cat(got_vals))
    sel = sel_rows.cpu().numpy()
    if case == "rows":
        v = np.array([int(O.gen_values("splitmix", 1, c, SEED[c], first=int(r))[0]) for r in sel])
        order = np.lexsort((sel, v))
        assert np.array_equal(want_rows.cpu().numpy(), sel[order]) and np.array_equal(want_vals.cpu().numpy(), v[order])
    for capacity in (count, count - 1):
        gr, gv = Guarded(capacity * 8), Guarded(capacity * 4)
        got = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        rc = L.mi355_sort_rows_dev(eng._ctx, col.data.data_ptr(), n, c, mask.data_ptr(), 0, 0, gr.ptr, gv.ptr, capacity, got.data_ptr())
        assert rc == 0, L.mi355_last_error()
        assert gr.guards_intact() and gv.guards_intact() and words(got) == [count]
        if capacity == count:
            assert torch.equal(gr.body.view(torch.int64), want_rows)
            assert torch.equal(R.u32(gv.body.view(torch.int32)), want_vals)
            assert int(want_rows.max().item()) == n - 1
            if case == "bytes":
                out_rows = gr.body.view(torch.int64).cpu().numpy()
                out_vals = gv.body.view(torch.int32).cpu().numpy().view(np.uint32).astype(np.uint64)
                key = (out_vals << np.uint64(31)) | out_rows.astype(np.uint64)  # rows < 2^31 here
                assert n < 1 << 31 and (key[1:] > key[:-1]).all() and len(key) == count
                in_mask = (mask[gr.body.view(torch.int64) >> 3].to(torch.int64) >> (gr.body.view(torch.int64) & 7)) & 1
                assert bool(in_mask.all().item())
                for a, ln in windows(n, crossings):
                    here = np.unpackbits(window_bitmap(mask, a, ln), bitorder="little")[:ln].astype(bool)
                    w_rows, w_vals = np.arange(a, a + ln)[here], host(O, c, a, ln)[here]
                    pos = np.nonzero(np.isin(out_rows, w_rows))[0]
                    by_row = pos[np.argsort(out_rows[pos])]
                    assert np.array_equal(out_rows[by_row], w_rows) and np.array_equal(out_vals[by_row].astype(np.int64), w_vals), a
        else:
            assert bool((gr.body == SENTINEL).all().item()) and bool((gv.body == SENTINEL).all().item())


@gpu
@pytest.mark.parametrize("case", CASES["mi355_value_set_dev"])
def test_value_set(O, eng, capped, budget, case):
    """bits: the 31-bit column into a set of 2^31 bits; bytes: 2^30 + RAG 32-bit values into a set of 2^32 bits; rows: 2^32 + RAG rows of 3 bits under a random mask into a set of
    5 bits -- the rows beyond the set are counted past 2^32 rows.  The host windows can only say which members MUST be there"""
    import torch

    e, case = pick(case, eng, capped)
    if case == "bytes":
        n, c, set_bits, mask = N_BYTES, 32, 1 << 32, None
        rows = crossing_rows("bytes", 32)
    elif case == "bits":
        n, c, set_bits, mask = N_BITS, 31, 1 << 31, None
        rows = crossing_rows("bits", 31)
    else:
        n, c, set_bits = N_ROWS, 3, 5
        rows = crossing_rows("rows", 3)
        mask = random_bitmap(n, 94, force=near(n, 1 << 31, 1 << 32))
    col = generated(eng, O, n, c, rows)
    g = Guarded((set_bits + 31) // 32 * 4)
    out, counts = e.value_set(col, set_bits, mask=mask, out=g.body)
    assert g.guards_intact()
    flags = torch.zeros(set_bits, dtype=torch.bool, device="cuda")
    beyond = 0
    for i0, i1 in slices(n):
        beyond += R.value_set(flags, decoded(eng, col, i0, i1), set_bits, None if mask is None else bit_slice(mask, i0, i1))
    step = 1 << 28
    members = 0
    for j0 in range(0, set_bits, step):
        part = flags[j0: j0 + step]
        members += int(part.sum().item())
        assert torch.equal(out[j0 // 8: (min(set_bits, j0 + step) + 7) // 8], R.pack_bitmap(part)), j0
    assert words(counts) == [members, beyond]
    for a, ln in windows(n, rows):
        v = host(O, c, a, ln)
        if mask is not None:
            v = v[np.unpackbits(window_bitmap(mask, a, ln), bitorder="little")[:ln].astype(bool)]
        v = np.unique(v[v < set_bits])
        byte = out[torch.from_numpy(v >> 3).cuda()].cpu().numpy()
        assert ((byte >> (v & 7)) & 1).all(), a


@gpu
@pytest.mark.parametrize("case", CASES["mi355_set_ranks_dev"])
def test_set_ranks(O, eng, budget, case):
    """a set of 2^32 bits with seven members either side of 2^31, ct = 3, miss = 7: a table of 1.5 GiB whose entry index passes
    2^31 and whose bit offset passes 2^32 three times; every byte against torch, the members' entries on the host"""
    import torch

    set_bits, ct, miss = 1 << 32, 3, 7
    # (entry 2^32 // 3 straddles bit 2^32 of the table, entry 2^33 // 3 bit 2^33)
    members = sorted([5, (1 << 32) // 3, (1 << 31) - 1, 1 << 31, (1 << 31) + 77, (1 << 33) // 3, (1 << 32) - 1])
    assert (1 << 32) // 3 * 3 < 1 << 32 < (1 << 32) // 3 * 3 + 3 and (1 << 33) // 3 * 3 < 1 << 33 < (1 << 33) // 3 * 3 + 3
    the_set = R.bitmap_of_rows(torch.tensor(members, dtype=torch.int64, device="cuda"), set_bits)
    g = Guarded((set_bits * ct + 7) // 8)
    table, counts = eng.set_ranks(the_set, set_bits, ct, miss=miss, out=g.body)
    assert g.guards_intact() and words(counts) == [7, 0]
    route = R.SetRanks(ct, miss)
    for i0, i1 in slices(set_bits):
        assert same_packed(table.data, ct, i0, i1, route.step(bit_slice(the_set, i0, i1))), i0
    assert route.counts == [7, 0]
    for rank, j in enumerate(members):  # host: entry j holds its rank, its neighbours hold miss
        a = j // 8 * 8 - (8 if j >= 8 else 0)
        want = np.full(24, miss)
        for other_rank, other in enumerate(members):
            if a <= other < a + 24:
                want[other - a] = other_rank
        assert want[j - a] == rank
        have = window_packed(table.data, ct, a, 24)
        want_bytes = payload(want, ct)
        if a + 24 <= set_bits:
            assert np.array_equal(have, want_bytes), j
        else:
            assert np.array_equal(have[: (set_bits - a) * ct // 8], want_bytes[: (set_bits - a) * ct // 8]), j


@gpu
@pytest.mark.parametrize("case", CASES["mi355_key_index_dev"])
def test_key_index(O, eng, budget, case):
    """n = 2^32 - 1 rows of 3-bit keys into a table of 32-bit row ids, keep first and last, with and without a mask: with `last`
    the table holds ids next to 2^32 - 1.  Host: the first / last row of a key lies in the first / last window for every key the
    window holds (the masked `last` table from the rows torch forced)"""
    import torch

    n, ck, ct = N_ROWS_MAX, 3, 32
    keys = generated(eng, O, n, ck, [1 << 31])
    mask = random_bitmap(n, 95, ands=2, force=near(n, 1 << 31))
    routes = {(keep, m): R.KeyIndex(8, keep, "cuda") for keep in ("first", "last") for m in (False, True)}
    for i0, i1 in slices(n):
        k, sel = decoded(eng, keys, i0, i1), bit_slice(mask, i0, i1)
        for (keep, m), route in routes.items():
            route.step(k, i0, sel if m else None)
    head, tail = host(O, ck, 0, 4 * TILE), host(O, ck, n - 4 * TILE, 4 * TILE)
    for (keep, m), route in routes.items():
        g, gc = Guarded(8 * 4), Guarded(32, back=64, front=64)
        table, counts = eng.key_index(keys, ct=ct, mask=mask if m else None, keep=keep, out=g.body, counts=as_i64(gc, 4))
        assert g.guards_intact() and gc.guards_intact()
        want, want_counts = route.table(ct, n)
        assert torch.equal(R.u32(table.data[:32].view(torch.int32)), want), (keep, m)
        assert words(counts) == want_counts and want_counts[0] == 8 and want_counts[3] == 0
        assert want_counts[2] == (R.popcount(mask) if m else n)
        if not m:
            got = want.cpu().numpy()
            if keep == "first":
                assert np.array_equal(got, [int(np.argmax(head == j)) for j in range(8)])
            else:
                assert np.array_equal(got, [n - 1 - int(np.argmax(tail[::-1] == j)) for j in range(8)])
                assert got.max() == n - 1 and (got > (1 << 32) - 200).all()


@gpu
@pytest.mark.parametrize("case", CASES["mi355_running_sum_dev"])
def test_running_sum(O, eng, budget, case):
    """rows_all: every row of a 3-bit column into 9 bits -- nearly every row is replaced, that count and the int64 total pass
    2^32; rows_mask: about 200 selected rows either side of row 2^32 into 12 bits; positions: row_positions of an all-ones-but-
    sparse-zeros bitmap of 2^31 + RAG rows (the 32-bit kernel; positions pass 2^31, the output byte 2^33).  Host: rows_mask and
    positions in every window (the host knows every selected / cleared row); rows_all at row 0, and as `miss` behind"""
    import torch

    if case == "positions":
        n, c, co, miss = N_POS, 1, 32, 0
        zero_rows = sparse_rows(n, 3000, 96, near(n, 1 << 31, 1 << 30))
        bitmap = R.bitmap_of_rows(zero_rows, n, pad=256, invert=True)
        col, mask, rows = bit_column(bitmap, n), None, [1 << 29, 1 << 30, 1 << 31]
        route = R.RunningSum(exclusive=True)
        values = lambda i0, i1: bit_slice(bitmap, i0, i1).to(torch.int64)
    else:
        n, c, miss = N_ROWS, 3, 1
        rows = crossing_rows("rows", 3)
        col = generated(eng, O, n, c, rows)
        co = 9 if case == "rows_all" else 12
        route = R.RunningSum()
        values = lambda i0, i1: decoded(eng, col, i0, i1)
        mask = None
        if case == "rows_mask":
            sel_rows = sparse_rows(n, 180, 97, near(n, 1 << 31, 1 << 32))
            mask = R.bitmap_of_rows(sel_rows, n)
    g = Guarded((n * co + 7) // 8)
    gr = Guarded(16, back=64, front=64)
    out, result = eng.running_sum(col, mask=mask, exclusive=(case == "positions"), co=co, miss=miss, out=g.body, result=as_i64(gr, 2))
    assert g.guards_intact() and gr.guards_intact()
    replaced = 0
    for i0, i1 in slices(n, S // 4 if case == "positions" else S):  # (an 8 GiB output: smaller temporaries)
        want, bad = R.fit(route.step(values(i0, i1), None if mask is None else bit_slice(mask, i0, i1)), co, miss)
        replaced += bad
        assert same_packed(out.data, co, i0, i1, want), i0
    assert words(result) == [route.total, replaced]
    if case == "rows_all":
        assert replaced > 1 << 32 and route.total > 1 << 32
        v = host(O, c, 0, 4 * TILE)
        r = np.cumsum(v)
        assert np.array_equal(window_packed(out.data, co, 0, 4 * TILE), payload(np.where(r >= 1 << co, miss, r), co))
        for a, ln in windows(n, rows)[1:]:
            assert np.array_equal(window_packed(out.data, co, a, ln), payload(np.full(ln, miss), co)), a
    else:
        known = (sel_rows if case == "rows_mask" else zero_rows).cpu().numpy()
        if case == "rows_mask":
            term = np.array([int(O.gen_values("splitmix", 1, c, SEED[c], first=int(r))[0]) for r in known])
            assert route.total == int(term.sum()) and replaced == 0 and known[-1] > 1 << 32
        else:
            assert route.total == n - len(known) and route.total > 1 << 31
        for a, ln in windows(n, rows):
            at = np.arange(a, a + ln)
            if case == "rows_mask":  # inclusive: the terms of the selected rows <= the row
                want = np.concatenate([[0], np.cumsum(term)])[np.searchsorted(known, at, side="right")]
            else:                    # exclusive: the rows in front, less the cleared ones among them
                want = at - np.searchsorted(known, at, side="left")
            assert np.array_equal(window_packed(out.data, co, a, ln), payload(want, co)), a


DELTA = {"bits": (31, (1 << 31) - 1, 32), "bytes": (32, 0, 32), "rows": (2, 3, 3)}  # shape: c, k, co


@gpu
@pytest.mark.parametrize("case", CASES["mi355_delta_dev"])
def test_delta(O, eng, capped, budget, case):
    """bits: 31-bit values into 32 bits (k = 2^31 - 1: nothing is replaced); bytes: 32-bit values with k = 0, co = 32 -- the
    counter is the column's number of descents; rows: 2 bits into 3 on 2^32 + RAG rows"""
    import torch

    e, shape = pick(case, eng, capped)
    c, k, co = DELTA[shape]
    n, rows, first, miss = SHAPE_ROWS[shape], crossing_rows(shape, c), 1, 2
    col = shape_column(eng, O, shape, c)
    g = Guarded((n * co + 7) // 8)
    counter = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    out = e.delta(col, first=first, k=k, co=co, miss=miss, out=g.body, out_of_range=counter).data
    assert g.guards_intact()
    route, replaced = R.Delta(first=first, k=k), 0
    for i0, i1 in slices(n):
        want, bad = R.fit(route.step(decoded(eng, col, i0, i1)), co, miss)
        replaced += bad
        assert same_packed(out, co, i0, i1, want), i0
    assert words(counter) == [replaced] and (replaced > 1 << 28 if shape == "bytes" else replaced == 0)
    for a, ln in windows(n, rows):
        v = np.concatenate([[first], host(O, c, 0, ln)]) if a == 0 else host(O, c, a - 1, ln + 1)
        r = np.diff(v) + k
        assert np.array_equal(window_packed(out, co, a, ln), payload(np.where((r < 0) | (r >= 1 << co), miss, r), co)), a


def run_column(n):
    """a 1-bit column of n <= 2^32 rows in runs, made by torch: bytes of 0x00 / 0xFF repeated (runs of a multiple of 8 rows, mean
    about 2^16), then single rows flipped by hand either side of row 2^31 and in the last rows, which makes runs of 1 to 3 rows"""
    import torch

    g = torch.Generator(device="cuda").manual_seed(98)
    nb = (n + 7) // 8
    lens = torch.randint(1, 1 << 14, (nb // (1 << 13) + 2048,), dtype=torch.int64, device="cuda", generator=g)
    kinds = (torch.arange(lens.numel(), device="cuda") % 2 * 255).to(torch.uint8)
    data = torch.repeat_interleave(kinds, lens)
    assert data.numel() >= nb
    data = torch.cat([data[:nb], torch.zeros(256, dtype=torch.uint8, device="cuda")])
    for r in ((1 << 31) - 1, (1 << 31) + 2, (1 << 31) + 3, n - 2, n - 5, n - 6, 9):
        data[r >> 3] ^= 1 << (r & 7)
    if n % 8:
        data[nb - 1] &= (1 << (n % 8)) - 1
    return data


def run_tables(data, n):
    import torch

    route = R.Runs()
    for i0, i1 in slices(n):
        route.step(bit_slice(data, i0, i1).to(torch.int64))
    return route.tables()


def bits_run_column(O):
    """the BITS shape in runs of mean 64, made and packed by torch: 31-bit values repeated 1..127 times, with runs of one row
    placed by hand either side of the row whose bit offset is 2^32, at row 0 and in the last rows -> (the rows' values int64, the
    packed column).  The packed bytes are checked against the oracle's packer in every window"""
    import torch

    from shared_simd_scan_amd.engine import PackedColumn

    n, c = N_BITS, 31
    g = torch.Generator(device="cuda").manual_seed(113)
    lens = torch.randint(1, 128, (n // 64 + 40_000,), dtype=torch.int64, device="cuda", generator=g)
    vals = torch.randint(0, 1 << 31, (lens.numel(),), dtype=torch.int64, device="cuda", generator=g)
    rowvals = torch.repeat_interleave(vals, lens)
    assert rowvals.numel() >= n
    rowvals = rowvals[:n].clone()
    for r, v in ((0, 7), (X_BITS - 1, 1), (X_BITS, 2), (X_BITS + 1, 3), (n - 2, 6), (n - 1, 5)):
        rowvals[r] = v
    data = torch.cat([R.pack_values(rowvals[i0:i1], c) for i0, i1 in slices(n, 1 << 24)] + [torch.zeros(256, dtype=torch.uint8, device="cuda")])
    for a, ln in windows(n, [X_BITS]):
        assert np.array_equal(window_packed(data, c, a, ln), payload(rowvals[a: a + ln].cpu().numpy(), c)), a
    return rowvals, PackedColumn(data, n, c)


def run_case(O, name):
    """-> (column, n, c, ends' width, the runs' values and ends from the torch route, rows(a, ln): a window's values on the host,
    crossing rows)"""
    import torch

    if name == "bits":
        rowvals, col = bits_run_column(O)
        route = R.Runs()
        for i0, i1 in slices(N_BITS):
            route.step(rowvals[i0:i1])
        values, ends = route.tables()
        return col, N_BITS, 31, 28, values, ends, (lambda a, ln: rowvals[a: a + ln].cpu().numpy()), [X_BITS]
    n = N_ROWS_MAX
    data = run_column(n)
    values, ends = run_tables(data, n)
    rows = lambda a, ln: np.unpackbits(window_bitmap(data, a, ln), bitorder="little")[:ln].astype(np.int64)
    return bit_column(data, n), n, 1, 32, values, ends, rows, [1 << 31]


@gpu
@pytest.mark.parametrize("case", CASES["mi355_run_encode_dev"])
def test_run_encode(O, eng, capped, budget, case):
    """rows: n = 2^32 - 1 rows of one bit, mean run about 2^16 with runs of one to three rows at row 2^31 and in front of the last
    row, ends at 32 bits: the last end is 2^32 - 1; bits: the 31-bit shape in runs of mean 64, ends at 28 bits, with runs of one
    row either side of bit 2^32.  Exactly ceil(runs c / 8) and ceil(runs ce / 8) bytes are written: the bytes behind stay 0xEE.
    Host: the runs that end inside a window, from the rows torch made; both tables decoded by the oracle"""
    import torch

    e, name = pick(case, eng, capped)
    col, n, c, ce, values, ends, rows_of, crossings = run_case(O, name)
    runs = values.numel()
    assert (40_000 < runs < 100_000) if name == "rows" else (n // 80 < runs < n // 50)
    assert int(ends[-1].item()) == n and n.bit_length() == ce
    nv, ne = (runs * c + 7) // 8, (runs * ce + 7) // 8
    gv, ge = Guarded((runs * c + 31) // 32 * 4), Guarded((runs * ce + 31) // 32 * 4)
    got_values, got_ends, count = e.run_encode(col, capacity=runs, ends_width=ce, values=gv.body, ends=ge.body)
    assert gv.guards_intact() and ge.guards_intact() and words(count) == [runs]
    assert torch.equal(got_values[:nv], R.pack_values(values, c)) and torch.equal(got_ends[:ne], R.pack_values(ends, ce))
    assert bool((got_values[nv:] == SENTINEL).all().item()) and bool((got_ends[ne:] == SENTINEL).all().item()), "bytes behind the tables written"
    host_ends = O.decompress(got_ends[:ne].cpu().numpy(), runs, ce).view(np.uint32).astype(np.int64)
    host_values = O.decompress(got_values[:nv].cpu().numpy(), runs, c).view(np.uint32).astype(np.int64)
    if name == "rows":
        assert list(host_ends[-5:]) == [n - 6, n - 4, n - 2, n - 1, n]  # the rows flipped by hand in the column's last byte
    else:
        assert list(host_ends[-2:]) == [n - 1, n] and {X_BITS, X_BITS + 1, X_BITS + 2} <= set(host_ends.tolist())
    for a, ln in windows(n, crossings):
        w = rows_of(a, ln)
        want = np.nonzero(np.diff(w))[0] + 1 + a
        here = (host_ends > a) & (host_ends < a + ln)
        assert np.array_equal(host_ends[here], want) and np.array_equal(host_values[here], w[want - 1 - a]), a
        assert len(want) >= 2
    assert words(e.count_runs(col)) == [runs]


@gpu
@pytest.mark.parametrize("case", CASES["mi355_run_decode_dev"])
def test_run_decode(O, eng, capped, budget, case):
    """the tables of run_encode's columns (from the torch route, packed by torch) back to the column: rows to n = 2^32 - 1 rows,
    rows_uncovered to 2^32 + RAG rows -- the rows behind the last end get `miss` and are counted -- bits to the 31-bit shape.
    The column's bytes ARE the host expectation: torch built them"""
    import torch

    from shared_simd_scan_amd.engine import PackedColumn

    e, name = pick(case, eng, capped)
    col, n_col, c, ce, values, ends, _, _ = run_case(O, "bits" if name == "bits" else "rows")
    runs = values.numel()
    pad = torch.zeros(256, dtype=torch.uint8, device="cuda")
    vcol = PackedColumn(torch.cat([R.pack_values(values, c), pad]), runs, c)
    ecol = PackedColumn(torch.cat([R.pack_values(ends, ce), pad]), runs, ce)
    n = N_ROWS if name == "rows_uncovered" else n_col
    g = Guarded((n * c + 7) // 8)
    counter = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    out = e.run_decode(vcol, ecol, n, miss=1, out=g.body, uncovered=counter).data
    assert g.guards_intact() and words(counter) == [n - n_col]
    data = col.data
    nb = (n_col * c + 7) // 8
    assert torch.equal(out[: nb - 1], data[: nb - 1])
    last = int(data[nb - 1].item())
    if name == "rows_uncovered":  # the column's last byte holds 7 rows; row 2^32 - 1 and the rows behind it are miss = 1
        assert int(out[nb - 1].item()) == last | 0x80
        rest = out[nb:]
        assert bool((rest[:-1] == 0xFF).all().item()) and int(rest[-1].item()) == (1 << (n % 8)) - 1
    else:
        assert int(out[nb - 1].item()) == last and out.numel() == nb
    for i0, i1 in slices(n):  # and the route of run_decode itself
        want, _ = R.run_decode(values, ends, i0, i1, 1)
        assert same_packed(out, c, i0, i1, want), i0


@gpu
@pytest.mark.parametrize("case", CASES["mi355_search_sorted_dev"])
def test_search_sorted(O, eng, capped, budget, case):
    """bytes_edges: the 32-bit column into 256 sorted 32-bit edges (made by numpy: edges from "index" would all lie below nearly
    every value), 9-bit positions; rows: 2^32 + RAG 3-bit rows into the six entries 0..5 from "index"; table: a sorted 31-bit
    table from "index" whose bit offsets cross 2^32 (the sampled tier), probed either side, `exact` with the found bitmap and
    the count"""
    import torch

    from shared_simd_scan_amd.engine import PackedColumn, search_sorted_kernel

    e, case = pick(case, eng, capped)
    if case == "table":
        values = probe_values(rng_of("search"), X_BITS, N_BITS, 1 << 31, below=N_BITS + 1000)
        n = len(values)
        col = PackedColumn(plain_pack(O, values, 32), n, 32)
        table = generated(eng, O, N_BITS, 31, [X_BITS], kind="index")
        assert search_sorted_kernel(32, 31, 32, N_BITS) == "search_global_kernel"
        miss = (1 << 32) - 1
        v = values.astype(np.int64)
        for side in ("left", "right"):
            g, gf = Guarded(n * 4), Guarded((n + 7) // 8)
            out, found, hits = e.search_sorted(col, table, side=side, exact=True, miss=miss, co=32, out=g.body, found=gf.body, hits=True)
            assert g.guards_intact() and gf.guards_intact()
            inside = v < N_BITS  # the table holds 0 .. N_BITS - 1, each once
            want = np.where(inside, v + (side == "right"), miss)
            assert np.array_equal(out.data[: n * 4].cpu().numpy(), payload(want, 32))
            assert np.array_equal(found.cpu().numpy(), packbits(inside)) and words(hits) == [int(inside.sum())]
            assert inside[-14:].any() and not inside[-14:].all()
        return
    if case == "bytes_edges":
        n, c, co, side, rows = N_BYTES, 32, 9, "right", crossing_rows("bytes", 32)
        edges = np.sort(rng_of("edges").integers(0, 1 << 32, 256, dtype=np.uint64)).astype(np.uint32)
        table = PackedColumn(plain_pack(O, edges, 32), 256, 32)
    else:
        n, c, co, side, rows = N_ROWS, 3, 3, "left", crossing_rows("rows", 3)
        edges = np.arange(6, dtype=np.uint32)
        table = generated(eng, O, 6, 3, kind="index")
    col = generated(eng, O, n, c, rows)
    g = Guarded((n * co + 7) // 8)
    out, _, _ = eng.search_sorted(col, table, side=side, co=co, out=g.body)
    assert g.guards_intact()
    t = torch.from_numpy(edges.astype(np.int64)).cuda()
    for i0, i1 in slices(n):
        want, _ = R.search_sorted(t, decoded(eng, col, i0, i1), side=side)
        assert same_packed(out.data, co, i0, i1, want), i0
    for a, ln in windows(n, rows):
        want = np.searchsorted(edges.astype(np.int64), host(O, c, a, ln), side=side)
        assert np.array_equal(window_packed(out.data, co, a, ln), payload(want, co)), a


@gpu
@pytest.mark.parametrize("case", CASES["mi355_run_aggregate_dev"])
def test_run_aggregate(O, eng, budget, case):
    """bytes: 32-bit values across byte 2^31 and 2^32 in runs of mean 4096; rows: 2^32 + RAG 1-bit values (all ones but sparse
    zeros) under a random mask, ends up to 2^32 - 1 at 32 bits -- the selected rows behind the last end are `uncovered`.  Host:
    the runs that lie inside a window, from the oracle's values (bytes) or from the rows torch cleared (rows)"""
    import torch

    from shared_simd_scan_amd.engine import PackedColumn

    rng = rng_of("run_aggregate", case)
    if case == "bytes":
        n, cv, ce, rows = N_BYTES, 32, 31, crossing_rows("bytes", 32)
        values = generated(eng, O, n, cv, rows)
        ends = np.unique(np.concatenate([rng.integers(1, n, n // 4096), [1 << 29, (1 << 29) + 1, 1 << 30, n - 77, n]]))
        mask = None
        column = lambda i0, i1: decoded(eng, values, i0, i1)
    else:
        n, cv, ce, rows = N_ROWS, 1, 32, crossing_rows("rows", 1)
        zero_rows = sparse_rows(n, 10000, 99, near(n, 1 << 31, 1 << 32))
        bits = R.bitmap_of_rows(zero_rows, n, pad=256, invert=True)
        values = bit_column(bits, n)
        ends = np.unique(np.concatenate([rng.integers(1, 1 << 32, 1 << 16), [1 << 31, (1 << 31) + 1, (1 << 32) - 3, (1 << 32) - 1]]))
        mask = random_bitmap(n, 100, force=near(n, 1 << 31, 1 << 32))
        column = lambda i0, i1: bit_slice(bits, i0, i1).to(torch.int64)
    runs = len(ends)
    t = torch.from_numpy(ends.astype(np.int64)).cuda()
    ecol = PackedColumn(torch.cat([R.pack_values(t, ce), torch.zeros(256, dtype=torch.uint8, device="cuda")]), runs, ce)
    g = Guarded(runs * 32)
    counter = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    eng.run_aggregate(values, ecol, mask=mask, out=as_i64(g, runs, 4), uncovered=counter)
    assert g.guards_intact()
    acc = R.Grouped(runs, "cuda")
    for i0, i1 in slices(n):
        acc.step(R.run_of_rows(t, i0, i1), column(i0, i1), None if mask is None else bit_slice(mask, i0, i1))
    got = as_i64(g, runs, 4)
    assert torch.equal(got, acc.table())
    assert words(counter) == [acc.dropped] and int(got[:, 1].sum().item()) + acc.dropped == (n if mask is None else R.popcount(mask))
    assert acc.dropped > RAG // 4 if case == "rows" else acc.dropped == 0
    table = got.cpu().numpy()
    checked = 0
    for a, ln in windows(n, rows):
        inside = np.nonzero((ends > a) & (ends <= a + ln))[0][1:]  # runs that start and end inside the window
        checked += len(inside[:40])
        if case == "bytes":
            v = host(O, cv, a, ln)
        else:
            v = (~np.isin(np.arange(a, a + ln), zero_rows.cpu().numpy())).astype(np.int64)
        sel = np.ones(ln, dtype=bool) if mask is None else np.unpackbits(window_bitmap(mask, a, ln), bitorder="little")[:ln].astype(bool)
        for j in inside[:40]:
            lo, hi = int(ends[j - 1]) - a, int(ends[j]) - a
            w = v[lo:hi][sel[lo:hi]]
            want = [int(w.sum()), len(w), int(w.min()) if len(w) else -1, int(w.max()) if len(w) else 0]
            assert table[j].tolist() == want, (a, j)
    assert checked >= 2  # at the least the two runs placed by hand: [2^29, 2^29 + 1) and [n - 77, n), or [2^31, 2^31 + 1) and [2^32 - 3, 2^32 - 1)


@gpu
@pytest.mark.parametrize("case", CASES["mi355_gather_dev"])
def test_gather(O, eng, budget, case):
    """rows: row ids beyond 2^31 and 2^32 into a 3-bit column of 2^32 + RAG rows; bits: ids either side of the row whose bit
    offset is 2^32, into the 31-bit column; first_row: a 9-bit row range that starts at row
    2^32 + 640, ids either side of it (outside: -1).  Host: the oracle's value of every id"""
    import torch

    if case in ("rows", "bits"):
        n, c, first_row = (N_ROWS, 3, 0) if case == "rows" else (N_BITS, 31, 0)
        col = generated(eng, O, n, c, crossing_rows(case, c))
        ids = sparse_rows(n, 4000, 101, near(n, 1 << 31, 1 << 32) if case == "rows" else near(n, X_BITS))
        ids = ids[torch.randperm(ids.numel(), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))]
    else:
        n, c, first_row = RAG, 9, (1 << 32) + 640
        col = eng.generate("splitmix", n, c, SEED[9], first_row=first_row)
        rng = rng_of("gather")
        ids = torch.from_numpy(np.concatenate([first_row + rng.integers(0, n, 3000), [first_row - 1, first_row, first_row + n - 1, first_row + n, 640, n]])).cuda()
    cap = ids.numel()
    g = Guarded(cap * 4)
    eng.gather(col, ids, cap, first_row=first_row, out=g.body.view(torch.int32))
    assert g.guards_intact()
    got = g.body.view(torch.int32).cpu().numpy().astype(np.int64)
    host_ids = ids.cpu().numpy()
    inside = (host_ids >= first_row) & (host_ids < first_row + n)
    want = np.array([int(O.gen_values("splitmix", 1, c, SEED[c], first=int(r))[0]) if ok else -1 for r, ok in zip(host_ids, inside)])
    assert np.array_equal(got, want) and (~inside).sum() == (4 if case == "first_row" else 0)
    if case != "first_row":  # and the full-size route: the values of the slices, indexed
        want_dev = torch.zeros(cap, dtype=torch.int64, device="cuda")
        for i0, i1 in slices(n):
            here = (ids >= i0) & (ids < i1)
            want_dev[here] = decoded(eng, col, i0, i1)[ids[here] - i0]
        assert torch.equal(g.body.view(torch.int32).to(torch.int64), want_dev)


@gpu
@pytest.mark.parametrize("case", CASES["mi355_aggregate_dev"])
def test_aggregate(O, eng, capped, budget, case):
    """rows: a 1-bit column of 2^32 + RAG rows, all ones but sparse zeros: count and sum pass 2^32, with and without a mask; bits:
    the 31-bit column under a random mask.  Host: the `rows` result from the rows torch cleared; bounds from the windows"""
    import torch

    e, shape = pick(case, eng, capped)
    if shape == "rows":
        n, c, rows = N_ROWS, 1, crossing_rows("rows", 1)
        zero_rows = sparse_rows(n, 10000, 102, near(n, 1 << 31, 1 << 32))
        bits = R.bitmap_of_rows(zero_rows, n, pad=256, invert=True)
        col = bit_column(bits, n)
        column = lambda i0, i1: bit_slice(bits, i0, i1).to(torch.int64)
    else:
        n, c, rows = N_BITS, 31, crossing_rows("bits", 31)
        col = shape_column(eng, O, "bits", 31)
        column = lambda i0, i1: decoded(eng, col, i0, i1)
    mask = random_bitmap(n, 103, force=near(n, *rows))
    for m in (None, mask):
        g = Guarded(32, back=64, front=64)
        e.aggregate(col, mask=m, out=as_i64(g, 4))
        assert g.guards_intact()
        acc = [0, 0, -1, 0]
        for i0, i1 in slices(n):
            acc = R.aggregate(acc, column(i0, i1), None if m is None else bit_slice(m, i0, i1))
        assert words(as_i64(g, 4)) == acc, m is None
        if shape == "rows" and m is None:
            assert acc == [n - zero_rows.numel(), n, 0, 1] and acc[0] > 1 << 32
        if shape == "bits":
            for a, ln in windows(n, rows):
                v = host(O, c, a, ln)
                if m is not None:
                    v = v[np.unpackbits(window_bitmap(m, a, ln), bitorder="little")[:ln].astype(bool)]
                assert acc[2] <= v.min() and acc[3] >= v.max() and acc[1] >= len(v)


@gpu
@pytest.mark.parametrize("case", CASES["mi355_histogram_dev"])
def test_histogram(O, eng, budget, case):
    """2^32 + RAG rows: a 1-bit column, all ones but sparse zeros (one counter passes 2^32), and the 3-bit generated column under a
    mask.  (A histogram takes at most 14 bits: the 31- and 32-bit shapes do not apply.)"""
    import torch

    n, rows = N_ROWS, crossing_rows("rows", 1)
    zero_rows = sparse_rows(n, 10000, 104, near(n, 1 << 31, 1 << 32))
    bits = R.bitmap_of_rows(zero_rows, n, pad=256, invert=True)
    g = Guarded(2 * 8, back=64, front=64)
    eng.histogram(bit_column(bits, n), out=as_i64(g, 2))
    assert g.guards_intact()
    assert words(as_i64(g, 2)) == [zero_rows.numel(), n - zero_rows.numel()] and n - zero_rows.numel() > 1 << 32
    assert R.popcount(bits) == n - zero_rows.numel()
    del bits
    col = generated(eng, O, n, 3, rows)
    mask = random_bitmap(n, 105, force=near(n, 1 << 31, 1 << 32))
    g = Guarded(8 * 8, back=64, front=64)
    eng.histogram(col, mask=mask, out=as_i64(g, 8))
    assert g.guards_intact()
    want = torch.zeros(8, dtype=torch.int64, device="cuda")
    for i0, i1 in slices(n):
        want += torch.bincount(decoded(eng, col, i0, i1)[bit_slice(mask, i0, i1)], minlength=8)
    assert torch.equal(as_i64(g, 8), want) and int(want.sum().item()) == R.popcount(mask)
    have = want.cpu().numpy()
    for a, ln in windows(n, rows):
        sel = np.unpackbits(window_bitmap(mask, a, ln), bitorder="little")[:ln].astype(bool)
        assert (have >= np.bincount(host(O, 3, a, ln)[sel], minlength=8)).all()


def two_bitmaps(n):
    return random_bitmap(n, 106, force=near(n, 1 << 31, 1 << 32)), random_bitmap(n, 107, ands=2, force=near(n, (1 << 31) + 8, (1 << 32) + 8))


@gpu
@pytest.mark.parametrize("case", CASES["mi355_bitmap_combine_dev"])
def test_bitmap_combine(O, eng, budget, case):
    """two torch-made bitmaps of 2^32 + RAG rows (byte index beyond 2^29, counts near 2^32), the four operations: every byte
    against torch's own bitwise operators, the count against a table look-up of the bytes"""
    import torch

    n = N_ROWS
    nb = (n + 7) // 8
    a, b = two_bitmaps(n)
    for op, f in (("and", lambda x, y: x & y), ("or", lambda x, y: x | y), ("xor", lambda x, y: x ^ y), ("andnot", lambda x, y: x & ~y)):
        g = Guarded(nb)
        out, count = eng.bitmap_combine(op, a, b, n, out=g.body)
        assert g.guards_intact()
        want = f(a[:nb], b[:nb])
        assert torch.equal(out, want), op
        assert words(count) == [R.popcount(want)], op
        for w0, ln in windows(n, crossing_rows("rows", 1)):
            have = window_bitmap(out, w0, ln)
            assert np.array_equal(have, f(window_bitmap(a, w0, ln), window_bitmap(b, w0, ln))), (op, w0)
        del g, out, want


@gpu
@pytest.mark.parametrize("case", CASES["mi355_bitmap_count_dev"])
def test_bitmap_count(O, eng, budget, case):
    """a torch-made bitmap of 2^32 + RAG rows with all ones but sparse zeros: the count passes 2^32; and a random one"""
    n = N_ROWS
    zero_rows = sparse_rows(n, 10000, 108, near(n, 1 << 31, 1 << 32))
    dense = R.bitmap_of_rows(zero_rows, n, invert=True)
    assert words(eng.bitmap_count(dense, n)) == [n - zero_rows.numel()] and n - zero_rows.numel() > 1 << 32
    assert R.popcount(dense) == n - zero_rows.numel()
    del dense
    a, _ = two_bitmaps(n)
    assert words(eng.bitmap_count(a, n)) == [R.popcount(a)]


@gpu
@pytest.mark.parametrize("case", CASES["mi355_pack_u32_dev"])
def test_pack_u32(O, L, eng, capped, budget, case):
    """the decoded 31-bit column packed again: the destination's bit offset crosses 2^32 inside a value.  2^32 rows of uint32
    input are 16 GiB, beyond the memory cap: the row count crosses in pack_u16's case.  Every byte against the generated column
    (itself checked against the oracle in its windows) and against torch's packing"""
    import torch

    n, c = N_BITS, 31
    col = shape_column(eng, O, "bits", c)
    values = eng.decompress(col)
    size = L.mi355_compressed_buffer_size(c, n)
    g = Guarded(size)
    rc = L.mi355_pack_u32_dev(pick(case, eng, capped)[0]._ctx, values.data_ptr(), n, c, g.ptr)
    assert rc == 0, L.mi355_last_error()
    assert g.guards_intact()
    payload_bytes = (n * c + 7) // 8
    assert torch.equal(g.body[:payload_bytes], col.data[:payload_bytes]) and not bool(g.body[payload_bytes:].any().item())
    for i0, i1 in slices(n):
        assert same_packed(g.body, c, i0, i1, R.u32(values[i0:i1])), i0


@gpu
@pytest.mark.parametrize("case", CASES["mi355_pack_u16_dev"])
def test_pack_u16(O, L, eng, budget, case):
    """2^32 + RAG uint16 values (8 GiB, made by torch) into 1 bit: the row count and the source's byte offset pass 2^32"""
    import torch

    n, c = N_ROWS, 1
    bits = random_bitmap(n, 109, force=near(n, 1 << 31, 1 << 32))
    values = torch.empty(n, dtype=torch.int16, device="cuda")
    for i0, i1 in slices(n):
        values[i0:i1] = bit_slice(bits, i0, i1).to(torch.int16)
    size = L.mi355_compressed_buffer_size(c, n)
    g = Guarded(size)
    rc = L.mi355_pack_u16_dev(eng._ctx, values.data_ptr(), n, c, g.ptr)
    assert rc == 0, L.mi355_last_error()
    assert g.guards_intact()
    nb = (n + 7) // 8
    assert torch.equal(g.body[:nb], bits[:nb]) and not bool(g.body[nb:].any().item())
    for a, ln in windows(n, crossing_rows("rows", 1)):
        assert np.array_equal(window_bitmap(g.body, a, ln), packbits(values[a: a + ln].cpu().numpy()))
