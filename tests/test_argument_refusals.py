"""What the device entry points of include/mi355_scan.h and include/mi355_columns.h refuse, and the edges they accept.

Every row of ROWS is one call with one bad argument: a width, a predicate count, a list, a layout, a comparison, a mask / combine /
bitmap op, a generator, a required pointer, a stride.  The call must answer on the host: MI355_E_INVALID, a message, an empty
launch record, and every byte of every output buffer still 0xEE.  test_refusal_names_the_argument asserts in addition that the
message of a pointer row contains the argument's name as the header spells it.

ACCEPTED: n == 0 with null column and bitmap pointers (hit counts zeroed, P words for the shared scans), an empty range
(lo > hi: zero bitmap, zero hits, no alignment requirement), a gather of capacity 0.

One column of 4096 rows at c = 9 (the shape of test_min_contract's rejection table) is enough: nothing here may reach a kernel.

No GPU needed (bottom of the file): mi355_shard_rows, mi355_device_count and mi355_ctx_create refuse their bad arguments before
they ask for a device.
"""
import ctypes as C

import numpy as np
import pytest

from support import E_INVALID as MI355_E_INVALID
from support import SENTINEL, Guarded, rt  # noqa: F401  (rt: the module-scoped runtime fixture: library, oracle, torch, two engines)

N, W = 4096, 9
NB = N // 8
LT, GT = 2, 4
HIST_MAX = 14  # kHistogramMaxBits

# RCCL calls need a communicator: tests/test_exchange_loopback.py
EXCLUDED = {"mi355_gather_bitmaps_dev", "mi355_gather_bitmaps_at_dev", "mi355_allreduce_hits_dev", "mi355_sharded_scan_eq_dev",
            "mi355_sharded_scan_range_dev"}

# the arguments of a valid call; a row overrides some.  Pointers are named by what the arena holds, None = NULL.
DEFAULTS = dict(n=N, c=W, c2=W, op=LT, op2=GT, mask_op=0, P=3, layout=0, stride=NB, capacity=8, kind=2, param=7, lo=5, hi=9, what=1,
                packed="packed", packed2="packed2", mask="mask", mask2="mask2", bitmap="bitmap", hits="hits", wide="wide", keys="keys",
                preds=((LT, 0, 5, 0), (1, 0, 7, 0), (5, 0, 9, 0)), ids="ids", count="count", values="values")

CALLS = {
    "mi355_scan_eq_dev": lambda L, x, a: L.mi355_scan_eq_dev(x, a.packed, a.n, a.c, 5, a.bitmap, a.hits),
    "mi355_scan_range_dev": lambda L, x, a: L.mi355_scan_range_dev(x, a.packed, a.n, a.c, a.lo, a.hi, a.bitmap, a.hits),
    "mi355_scan_where_dev": lambda L, x, a: L.mi355_scan_where_dev(x, a.packed, a.n, a.c, a.op, 5, 0, a.mask, a.bitmap, a.hits),
    "mi355_scan_combine_dev": lambda L, x, a: L.mi355_scan_combine_dev(x, a.packed, a.n, a.c, a.op, 5, 0, a.mask_op, a.mask, a.bitmap, a.hits),
    "mi355_scan_in_dev": lambda L, x, a: L.mi355_scan_in_dev(x, a.packed, a.n, a.c, a.keys, a.P, 0, a.mask, a.bitmap, a.hits),
    "mi355_scan2_dev": lambda L, x, a: L.mi355_scan2_dev(x, a.packed, a.c, a.op, 5, 0, a.packed2, a.c2, a.op2, 7, 0, a.n, a.mask_op, a.bitmap, a.hits),
    "mi355_scan_columns_dev": lambda L, x, a: L.mi355_scan_columns_dev(x, a.packed, a.c, a.packed2, a.c2, a.n, a.op, 0, 0, a.mask_op, a.mask, a.bitmap,
                                                                      a.hits),
    "mi355_shared_scan_eq_dev": lambda L, x, a: L.mi355_shared_scan_eq_dev(x, a.packed, a.n, a.c, a.keys, a.P, a.layout, a.bitmap, a.stride, a.hits),
    "mi355_shared_scan_where_dev": lambda L, x, a: L.mi355_shared_scan_where_dev(x, a.packed, a.n, a.c, a.preds, a.P, a.layout, a.bitmap, a.stride,
                                                                                a.hits),
    "mi355_scan_select_dev": lambda L, x, a: L.mi355_scan_select_dev(x, a.packed, a.n, a.c, a.op, 5, 0, a.mask_op, a.mask, 0, a.wide, a.capacity, a.hits),
    "mi355_bitmap_combine_dev": lambda L, x, a: L.mi355_bitmap_combine_dev(x, a.mask_op, a.mask, a.mask2, a.bitmap, a.n, a.hits),
    "mi355_bitmap_count_dev": lambda L, x, a: L.mi355_bitmap_count_dev(x, a.mask, a.n, a.hits),
    "mi355_bitmap_to_rowids_dev": lambda L, x, a: L.mi355_bitmap_to_rowids_dev(x, a.mask, a.n, 0, a.wide, a.capacity, a.hits),
    "mi355_gather_dev": lambda L, x, a: L.mi355_gather_dev(x, a.packed, a.n, a.c, 0, a.ids, a.count, a.capacity, a.wide),
    "mi355_aggregate_dev": lambda L, x, a: L.mi355_aggregate_dev(x, a.packed, a.n, a.c, a.mask, a.wide),
    "mi355_histogram_dev": lambda L, x, a: L.mi355_histogram_dev(x, a.packed, a.n, a.c, a.mask, a.wide),
    "mi355_decompress_dev": lambda L, x, a: L.mi355_decompress_dev(x, a.packed, a.n, a.c, a.wide),
    "mi355_pack_u32_dev": lambda L, x, a: L.mi355_pack_u32_dev(x, a.values, a.n, a.c, a.wide),
    "mi355_pack_u16_dev": lambda L, x, a: L.mi355_pack_u16_dev(x, a.values, a.n, a.c, a.wide),
    "mi355_generate_dev": lambda L, x, a: L.mi355_generate_dev(x, a.kind, 0, a.n, a.c, a.param, a.wide),
    "mi355_tune_dev": lambda L, x, a: L.mi355_tune_dev(x, a.packed, a.n, a.c, a.what),
}


def _rows():
    """(entry point, what is wrong, the arguments that differ from DEFAULTS, the header's name of the pointer or None)"""
    rows = []

    def add(sym, what, name=None, **kw):
        rows.append((sym, what, kw, name))

    def widths(sym, *args, extra=()):
        for arg in args:
            for v in (0, 33) + tuple(extra):
                add(sym, f"{arg}={v}", **{arg: v})

    def ops(sym, arg, bad):
        for v in bad:
            add(sym, f"{arg}={v}", **{arg: v})

    def null(sym, arg, name, **kw):
        add(sym, f"{name} null", name, **{arg: None}, **kw)

    for sym in ("mi355_scan_eq_dev", "mi355_scan_range_dev"):
        widths(sym, "c")
        null(sym, "packed", "packed_dev")
        null(sym, "bitmap", "bitmap_dev")
    for sym in ("mi355_scan_where_dev", "mi355_scan_combine_dev"):
        widths(sym, "c")
        ops(sym, "op", (-1, 8))
        null(sym, "packed", "packed_dev")
        add(sym, "bitmap and hits both null", bitmap=None, hits=None)
    ops("mi355_scan_combine_dev", "mask_op", (-1, 4))
    widths("mi355_scan_in_dev", "c")
    ops("mi355_scan_in_dev", "P", (0, 1025))
    null("mi355_scan_in_dev", "keys", "keys_host")
    null("mi355_scan_in_dev", "packed", "packed_dev")
    null("mi355_scan_in_dev", "bitmap", "bitmap_dev")
    widths("mi355_scan2_dev", "c", "c2")
    ops("mi355_scan2_dev", "op", (-1, 8))
    ops("mi355_scan2_dev", "op2", (-1, 8))
    ops("mi355_scan2_dev", "mask_op", (-1, 4))
    null("mi355_scan2_dev", "packed", "packed1_dev")
    null("mi355_scan2_dev", "packed2", "packed2_dev")
    add("mi355_scan2_dev", "bitmap and hits both null", bitmap=None, hits=None)
    widths("mi355_scan_columns_dev", "c", "c2")
    ops("mi355_scan_columns_dev", "op", (-1, 8))
    ops("mi355_scan_columns_dev", "mask_op", (-1, 4))
    null("mi355_scan_columns_dev", "packed", "packed1_dev")
    null("mi355_scan_columns_dev", "packed2", "packed2_dev")
    add("mi355_scan_columns_dev", "bitmap and hits both null", bitmap=None, hits=None)
    for sym, arg, name in (("mi355_shared_scan_eq_dev", "keys", "keys_host"), ("mi355_shared_scan_where_dev", "preds", "preds_host")):
        widths(sym, "c")
        ops(sym, "P", (0, 1025))
        null(sym, arg, name)
        ops(sym, "layout", (2,))
        null(sym, "packed", "packed_dev")
        null(sym, "bitmap", "out_dev")
        add(sym, "stride not a multiple of 16", stride=NB + 8)
        add(sym, "stride smaller than ceil(n/8)", stride=NB - 16)
    for bad in (-1, 8):
        add("mi355_shared_scan_where_dev", f"preds[1].op={bad}", preds=((LT, 0, 5, 0), (bad, 0, 7, 0), (5, 0, 9, 0)))
    add("mi355_shared_scan_where_dev", "preds[2].reserved=1", preds=((LT, 0, 5, 0), (1, 0, 7, 0), (5, 1, 9, 0)))
    widths("mi355_scan_select_dev", "c")
    ops("mi355_scan_select_dev", "op", (-1, 8))
    ops("mi355_scan_select_dev", "mask_op", (-1, 4))
    null("mi355_scan_select_dev", "hits", "count_dev")
    null("mi355_scan_select_dev", "packed", "packed_dev")
    null("mi355_scan_select_dev", "wide", "rowids_dev")
    ops("mi355_bitmap_combine_dev", "mask_op", (-1, 4))
    null("mi355_bitmap_combine_dev", "mask", "a_dev")
    null("mi355_bitmap_combine_dev", "mask2", "b_dev")
    null("mi355_bitmap_combine_dev", "bitmap", "out_dev")
    null("mi355_bitmap_count_dev", "mask", "bitmap_dev")
    null("mi355_bitmap_count_dev", "hits", "count_dev")
    null("mi355_bitmap_to_rowids_dev", "hits", "count_dev")
    null("mi355_bitmap_to_rowids_dev", "mask", "bitmap_dev")
    null("mi355_bitmap_to_rowids_dev", "wide", "rowids_dev")
    widths("mi355_gather_dev", "c")
    null("mi355_gather_dev", "count", "count_dev")
    null("mi355_gather_dev", "packed", "packed_dev")
    null("mi355_gather_dev", "ids", "rowids_dev")
    null("mi355_gather_dev", "wide", "out_dev")
    widths("mi355_aggregate_dev", "c")
    null("mi355_aggregate_dev", "wide", "out_dev")
    null("mi355_aggregate_dev", "packed", "packed_dev")
    widths("mi355_histogram_dev", "c", extra=(HIST_MAX + 3,))
    null("mi355_histogram_dev", "wide", "counts_dev")
    null("mi355_histogram_dev", "packed", "packed_dev")
    widths("mi355_decompress_dev", "c")
    null("mi355_decompress_dev", "packed", "packed_dev")
    null("mi355_decompress_dev", "wide", "out_dev")
    for sym in ("mi355_pack_u32_dev", "mi355_pack_u16_dev"):
        widths(sym, "c")
        null(sym, "wide", "packed_dev")
        null(sym, "values", "values_dev")
    widths("mi355_generate_dev", "c")
    add("mi355_generate_dev", "kind=3", kind=3)
    add("mi355_generate_dev", "modulus 0", kind=0, param=0)
    null("mi355_generate_dev", "wide", "packed_dev")
    widths("mi355_tune_dev", "c")
    null("mi355_tune_dev", "packed", "packed_dev")
    return rows


ROWS = _rows()
ROW_IDS = [f"{sym[6:]}-{what.replace(' ', '_')}" for sym, what, _, _ in ROWS]


def test_row_ids_unique_and_every_dev_symbol_has_rows():
    from shared_simd_scan_amd._capi import HEADERS

    assert len(set(ROW_IDS)) == len(ROW_IDS)
    dev = {name for name, _, _ in HEADERS["mi355_scan.h"] + HEADERS["mi355_columns.h"] if name.endswith("_dev")}
    assert dev - EXCLUDED == set(CALLS) == {sym for sym, _, _, _ in ROWS}
    assert EXCLUDED <= {name for name, _, _ in HEADERS["mi355_scan.h"]}


class Arena:
    """the inputs of every row, made once: two packed columns, two bitmaps, row ids, a count, values to pack, host lists"""

    def __init__(self, rt):
        torch = rt.torch
        vals = np.arange(N, dtype=np.uint32) % 512
        self.cols = [torch.from_numpy(rt.O.pack(vals, W)).cuda() for _ in range(2)]
        self.masks = [torch.full((NB,), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(2)]
        self.ids = torch.arange(8, dtype=torch.int64, device="cuda")
        self.count = torch.tensor([4], dtype=torch.int64, device="cuda")
        self.values = torch.zeros(N, dtype=torch.int32, device="cuda")
        self.keys = np.asarray([1, 2, 3, 0, 0, 0, 0, 0], dtype=np.int32)


@pytest.fixture(scope="module")
def arena(rt):
    return Arena(rt)


class Args:
    pass


def make_args(arena, outs, overrides):
    """DEFAULTS with `overrides` -> the ctypes arguments of a call (the Predicate array stays alive on the object)"""
    from shared_simd_scan_amd._capi import Predicate

    spec = dict(DEFAULTS, **overrides)
    where = {"packed": arena.cols[0].data_ptr(), "packed2": arena.cols[1].data_ptr(), "mask": arena.masks[0].data_ptr(),
             "mask2": arena.masks[1].data_ptr(), "ids": arena.ids.data_ptr(), "count": arena.count.data_ptr(), "values": arena.values.data_ptr(),
             "keys": arena.keys.ctypes.data, "bitmap": outs["bitmap"].ptr.value, "hits": outs["hits"].ptr.value, "wide": outs["wide"].ptr.value}
    a = Args()
    for k, v in spec.items():
        if k == "preds":
            a.pred_array = (Predicate * len(v))(*[Predicate(*p) for p in v]) if v is not None else None
            v = C.cast(a.pred_array, C.c_void_p) if v is not None else None
        elif k in where:
            v = C.c_void_p(where[v]) if v is not None else None
        setattr(a, k, v)
    return a


def fresh_outputs():
    """wide: the largest output of any entry point at these shapes (decompress: 4 bytes per row)"""
    return {"bitmap": Guarded(4096), "wide": Guarded(4 * N + 64), "hits": Guarded(64, back=64, front=64)}


def refuse(rt, arena, row):
    """the row's call -> its error message, after the checks every row passes"""
    sym, what, overrides, _ = row
    L, eng = rt.L, rt.default
    outs = fresh_outputs()
    rc = CALLS[sym](L, eng._ctx, make_args(arena, outs, overrides))
    eng.synchronize()
    msg = L.mi355_last_error()
    assert rc == MI355_E_INVALID, f"{sym}, {what}: returned {rc} ({msg})"
    assert msg, f"{sym}, {what}: no message"
    assert L.mi355_ctx_last_launch(eng._ctx) == b"", f"{sym}, {what}: something was launched"
    for name, g in outs.items():
        assert (g.fetch() == SENTINEL).all(), f"{sym}, {what}: {name} was written"
    return msg.decode()


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_refusal(rt, arena, row):
    """MI355_E_INVALID, a message, nothing launched, no output byte written"""
    refuse(rt, arena, row)


@pytest.mark.gpu
@pytest.mark.parametrize("row", [r for r in ROWS if r[3]], ids=[i for i, r in zip(ROW_IDS, ROWS) if r[3]])
def test_refusal_names_the_argument(rt, arena, row):
    """a null pointer is reported under the name the header gives the argument"""
    msg = refuse(rt, arena, row)
    assert row[3] in msg and "null" in msg, f"{row[0]}, {row[1]}: {msg!r} does not name {row[3]}"


def test_every_row_changes_an_argument():
    for sym, what, kw, _ in ROWS:
        assert kw and any(DEFAULTS[k] != v for k, v in kw.items()), (sym, what)


@pytest.mark.gpu
@pytest.mark.parametrize("sym", sorted(set(CALLS) - {"mi355_tune_dev"}))
def test_the_defaults_are_a_valid_call(rt, arena, sym):
    """the call every row of `sym` is derived from is accepted and launches: a row's refusal is its one bad argument's"""
    L, eng = rt.L, rt.default
    outs = fresh_outputs()
    rc = CALLS[sym](L, eng._ctx, make_args(arena, outs, {}))
    eng.synchronize()
    assert rc == 0, (sym, L.mi355_last_error())
    assert L.mi355_ctx_last_launch(eng._ctx) != b"", sym
    for g in outs.values():
        g.fetch()  # the guards around every output


# ---- accepted edges ---------------------------------------------------------------------------------------------------------

# n == 0, null column and bitmap pointers: (entry point, overrides, hit / count words that must read zero afterwards)
EMPTY = [
    ("mi355_scan_eq_dev", dict(packed=None, bitmap=None), 1),
    ("mi355_scan_range_dev", dict(packed=None, bitmap=None), 1),
    ("mi355_scan_where_dev", dict(packed=None, bitmap=None, mask=None), 1),
    ("mi355_scan_combine_dev", dict(packed=None, bitmap=None, mask=None), 1),
    ("mi355_scan_in_dev", dict(packed=None, bitmap=None, mask=None), 1),
    ("mi355_scan2_dev", dict(packed=None, packed2=None, bitmap=None), 1),
    ("mi355_scan_columns_dev", dict(packed=None, packed2=None, bitmap=None, mask=None), 1),
    ("mi355_shared_scan_eq_dev", dict(packed=None, bitmap=None), 3),
    ("mi355_shared_scan_where_dev", dict(packed=None, bitmap=None), 3),
    ("mi355_scan_select_dev", dict(packed=None, wide=None, mask=None), 1),
    ("mi355_bitmap_combine_dev", dict(mask=None, mask2=None, bitmap=None), 1),
    ("mi355_bitmap_count_dev", dict(mask=None), 1),
    ("mi355_bitmap_to_rowids_dev", dict(mask=None, wide=None), 1),
    ("mi355_decompress_dev", dict(packed=None, wide=None), 0),
]


@pytest.mark.gpu
@pytest.mark.parametrize("sym,overrides,words", EMPTY, ids=[e[0][6:] for e in EMPTY])
def test_zero_rows_with_null_buffers(rt, arena, sym, overrides, words):
    L, eng = rt.L, rt.default
    outs = fresh_outputs()
    rc = CALLS[sym](L, eng._ctx, make_args(arena, outs, dict(overrides, n=0)))
    eng.synchronize()
    assert rc == 0, (sym, L.mi355_last_error())
    assert L.mi355_ctx_last_launch(eng._ctx) == b"", f"{sym}: a kernel for zero rows"
    hits = outs.pop("hits").fetch()
    assert (hits[: 8 * words] == 0).all() and (hits[8 * words:] == SENTINEL).all(), f"{sym}: {words} hit words of zero expected"
    for name, g in outs.items():
        assert (g.fetch() == SENTINEL).all(), f"{sym}: {name} was written"


@pytest.mark.gpu
def test_empty_range_zeroes_bitmap_and_hits(rt, arena):
    """lo > hi: ceil(n/8) zero bytes and zero hits, at any bitmap address (no kernel runs, so nothing needs 16-byte alignment)"""
    L, eng = rt.L, rt.default
    outs = fresh_outputs()
    a = make_args(arena, outs, dict(lo=9, hi=5))
    a.bitmap = C.c_void_p(a.bitmap.value + 8)
    rc = CALLS["mi355_scan_range_dev"](L, eng._ctx, a)
    eng.synchronize()
    assert rc == 0, L.mi355_last_error()
    assert L.mi355_ctx_last_launch(eng._ctx) == b""
    bitmap, hits = outs["bitmap"].fetch(), outs["hits"].fetch()
    assert (bitmap[8: 8 + NB] == 0).all() and (bitmap[:8] == SENTINEL).all() and (bitmap[8 + NB:] == SENTINEL).all()
    assert (hits[:8] == 0).all() and (hits[8:] == SENTINEL).all()


@pytest.mark.gpu
def test_gather_of_capacity_zero(rt, arena):
    L, eng = rt.L, rt.default
    outs = fresh_outputs()
    rc = CALLS["mi355_gather_dev"](L, eng._ctx, make_args(arena, outs, dict(capacity=0, packed=None, ids=None, wide=None)))
    eng.synchronize()
    assert rc == 0, L.mi355_last_error()
    assert L.mi355_ctx_last_launch(eng._ctx) == b""
    for name, g in outs.items():
        assert (g.fetch() == SENTINEL).all(), name


@pytest.mark.gpu
def test_set_option_refusals(rt):
    L, eng = rt.L, rt.default
    num_cus = rt.torch.cuda.get_device_properties(0).multi_processor_count
    for name, value in ((b"no_such_option", 1), (None, 1), (b"llc_resident_mib", -2), (b"llc_resident_mib", 1025), (b"grid_cus", -1),
                        (b"grid_cus", num_cus + 1)):
        assert L.mi355_ctx_set_option(eng._ctx, name, value) == MI355_E_INVALID, (name, value)
        assert L.mi355_last_error(), (name, value)
    assert L.mi355_ctx_set_option(eng._ctx, b"grid_cus", num_cus) == 0 and L.mi355_ctx_set_option(eng._ctx, b"grid_cus", 0) == 0


# ---- no GPU needed: refused before the library asks for a device --------------------------------------------------------------

def test_shard_rows_refusals():
    from shared_simd_scan_amd import lib

    L = lib()
    first, count = C.c_uint64(123), C.c_uint64(456)
    for world, rank, f, n in ((0, 0, first, count), (4, 4, first, count), (4, 7, first, count), (4, 1, None, count), (4, 1, first, None)):
        assert L.mi355_shard_rows(100000, world, rank, f, n) == MI355_E_INVALID, (world, rank)
        assert L.mi355_last_error()
        assert (first.value, count.value) == (123, 456), "a refused call wrote its outputs"
    assert L.mi355_shard_rows(100000, 4, 1, first, count) == 0 and (first.value, count.value) == (32768, 32768)


def test_null_outputs_refused_without_a_device():
    from shared_simd_scan_amd import lib

    L = lib()
    assert L.mi355_device_count(None) == MI355_E_INVALID and b"count" in L.mi355_last_error()
    assert L.mi355_ctx_create(0, None, None) == MI355_E_INVALID and b"out" in L.mi355_last_error()
