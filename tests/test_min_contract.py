"""Every device entry point on a row-range view at the minimum alignment the C ABI accepts.

The contract of include/mi355_scan.h ("Conventions") that this module pins:
  1. the bytes behind a column's payload -- the pad, and the bits of the last payload byte behind value n-1 -- may hold anything;
  2. a pointer needs the documented minimum alignment only: 16 bytes, or 4 bytes for the arguments listed in MIN_ALIGN_4;
  3. a mask or bitmap operand is read up to ceil(n/8) bytes and no further.

The arena.  A view of n rows lies inside ONE packed column `hostile prefix | view | hostile suffix` (packed by the oracle,
so the view's last payload byte shares bits with the first hostile row whenever n*c % 8 != 0); masks and bitmap operands are
canonical inside [0, ceil(n/8)) and 0xFF for 256 bytes in front and behind; outputs live in fresh 0xEE guards.  Every case runs
with two hostile fills: "match" (the rows outside the view satisfy the predicate under test) and "miss" (none does, which is
what leaks through !=, NOT BETWEEN, NOT IN, XOR and ANDNOT).  Aggregate and histogram use the fills 0 and 2^c - 1 around a
view drawn from [1, 2^c - 2], so a leak moves min, max, sum, count or a counter that must stay 0; at c = 1 the view needs both
values, so only sum / count (aggregate) and the totals (histogram) can show a leak there -- min / max and the per-value
counters cannot.  Every 16-byte pointer sits at an address that is 16 mod 32, every 4-byte pointer at 4 mod 8 (asserted).

The reference is numpy over the view's own values (int64 / uint64) and np.packbits(..., bitorder="little"): integers and bits,
every comparison exact.

CPU (not gpu): every MI355_API ..._dev symbol of the two headers has a case (or a named exclusion), and every case would
notice a leak: numpy over one row more, over the last byte's bits >= n, or (masked cases) over one mask byte more gives a
different expectation in at least one fill.  Where the contract itself hides a leak no test can see it, and the check says so
(hidden()): a canonical mask has zero bits behind n, so under AND / ANDNOT -- and for the bitmap consumers, whose operands
are all canonical -- a row leaked inside the last byte changes nothing; the byte behind the mask is where those cases look.

Not covered: reads beyond mi355_compressed_buffer_size cannot be observed without provoking a fault; these tests only show
that no result depends on what lies behind a view.
"""
import ctypes as C
import os
import re
import zlib
from dataclasses import dataclass

import numpy as np
import pytest

from kernel_cases import SHARED_TILE_ROWS, family_of
from support import E_INVALID as MI355_E_INVALID
from support import HOSTILE_BYTES, SENTINEL, Guarded, base_name, packbits, parse_record, rt  # noqa: F401  (rt: the module-scoped runtime fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIDTHS = (1, 5, 9, 12, 17, 32)
HIST_WIDTHS = (1, 5, 9, 12, 14)
DECOMPRESS_TILE_ROWS = 4096   # decompress_kernel: 16 steps of 256 values
ROWID_CHUNK_ROWS = 16384      # rowid_*_kernel: 2048 bitmap bytes per wave
HOSTILE_ROWS = 256            # at least this many hostile rows in front of a view (and a whole tile + this many behind)
FIRST_ROW = (1 << 32) + 12345  # selection / gather: row ids above 2^32
FILLS = ("match", "miss")

EQ, NE, LT, LE, GT, GE, BETWEEN, NOT_BETWEEN = range(8)
AND, OR, XOR, ANDNOT = range(4)
OP_NAMES = ("eq", "ne", "lt", "le", "gt", "ge", "between", "notbetween")
MASK_NAMES = ("and", "or", "xor", "andnot")

# the pointers extras.hip accepts at 4 bytes; every other device pointer below needs 16
MIN_ALIGN_4 = {("mi355_bitmap_to_rowids_dev", "bitmap_dev"), ("mi355_gather_dev", "packed_dev"), ("mi355_aggregate_dev", "mask_dev"),
               ("mi355_histogram_dev", "mask_dev"), ("mi355_pack_u32_dev", "packed_dev"), ("mi355_pack_u16_dev", "packed_dev"),
               ("mi355_generate_dev", "packed_dev")}

# _dev symbols without a case, by name: RCCL calls need several ranks (tests/test_exchange_loopback.py), the memory helpers take
# no packed column or bitmap, and the tuner only runs the scans above on columns of >= 5e7 rows
EXCLUDED = {
    "mi355_gather_bitmaps_dev": "RCCL", "mi355_gather_bitmaps_at_dev": "RCCL", "mi355_allreduce_hits_dev": "RCCL",
    "mi355_sharded_scan_eq_dev": "RCCL", "mi355_sharded_scan_range_dev": "RCCL",
    "mi355_dev_alloc": "mi355_dev_*", "mi355_dev_free": "mi355_dev_*", "mi355_dev_upload": "mi355_dev_*",
    "mi355_dev_download": "mi355_dev_*", "mi355_dev_memset": "mi355_dev_*",
    "mi355_tune_dev": "mi355_tune_dev",
}


# (a, b) of the comparison on the difference of two columns (mi355_scan_columns_dev), per op: both outcomes exist for every
# width pair of the table, two 1-bit columns included
COLUMN_CONSTANTS = {LT: (0, 0), BETWEEN: (-3, 3), NE: (0, 0), GE: (2, 0), NOT_BETWEEN: (0, 1), EQ: (1, 0), GT: (0, 0), LE: (-1, 0)}


def vmax(c):
    return (1 << c) - 1


def mid(c):
    return 1 << (c - 1)


def scan_tile(c):
    """mi355_tile_values(c) (test_tile_sizes_are_the_librarys): 64 lanes x 128 values up to 16 bits, x 64 above"""
    return 8192 if c <= 16 else 4096


def compare(op, v, a, b=0):
    """v OP a [, b] on exact integers (int64 arrays)"""
    return {EQ: lambda: v == a, NE: lambda: v != a, LT: lambda: v < a, LE: lambda: v <= a, GT: lambda: v > a, GE: lambda: v >= a,
            BETWEEN: lambda: (v >= a) & (v <= b), NOT_BETWEEN: lambda: ~((v >= a) & (v <= b))}[op]()


def combine(mask_op, p, m):
    return {AND: lambda: p & m, OR: lambda: p | m, XOR: lambda: p ^ m, ANDNOT: lambda: m & ~p}[mask_op]()


def constants(op, c):
    """(a, b) of comparison `op` at width c: both outcomes exist at every width, c = 1 included, and the values next to the
    constants (candidates()) are where an off-by-one would show"""
    m = mid(c)
    return {EQ: (m | 1, 0), NE: (m | 1, 0), LT: (m, 0), LE: (m - 1, 0), GT: (m - 1, 0), GE: (m, 0), BETWEEN: (m // 2, m - 1),
            NOT_BETWEEN: (m // 2, m - 1)}[op]


def candidates(c):
    m, top = mid(c), vmax(c)
    return sorted({x for x in (0, 1, m // 2, m - 2, m - 1, m, m + 1, m + 2, m + 3, m | 1, (m | 1) ^ 1, top - 1, top) if 0 <= x <= top})


def key_list(c, P):
    """P keys of an IN list / shared equality scan: consecutive odd values, from mid(c) | 1 up where they fit (mid(c) is never a key); at c = 1 the key 1
    alternating with keys outside [0, 2^c), which match nothing"""
    if c == 1:
        return [1 if j % 2 == 0 else 2 + j for j in range(P)]
    first = min(mid(c) | 1, vmax(c) - 2 * (P - 1))  # (a long list at a narrow width starts lower)
    assert first >= 1
    return [first + 2 * j for j in range(P)]


def as_i32(x):
    return int(np.uint32(x).view(np.int32))


@dataclass(frozen=True)
class Case:
    id: str
    sym: str                 # the entry point
    kind: str                # scan, shared, scan2, columns, bitmap, count, rowids, gather, aggregate, histogram, decompress, pack
    c: int = 9
    c2: int = 0              # second column (scan2, columns)
    op: int = EQ
    op2: int = LT
    mask_op: int = -1        # -1: no mask operand
    inplace: bool = False    # mask_dev == bitmap_dev / out aliasing a
    count_only: bool = False
    negate: int = 0
    P: int = 1
    layout: int = 0
    hits: bool = True
    family: str = ""         # shared scans: the kernel family the call must take ("" = whatever the library names)
    select_kernel: int = 0
    extra: int = 0           # select: capacity beyond the count; generate: kind; columns: constant pair index
    masked: bool = False     # aggregate / histogram / in / select / columns: with a mask

    @property
    def widths(self):
        return {"scan2": (self.c, self.c2), "columns": (self.c, self.c2), "bitmap": (), "count": (), "rowids": (), "pack": ()}.get(self.kind, (self.c,))

    @property
    def nbitmaps(self):
        if self.kind == "bitmap":
            return 2
        if self.kind in ("count", "rowids"):
            return 1
        if self.kind == "scan2":  # mask_op is the combination of the two predicates there
            return 0
        return 1 if (self.mask_op >= 0 or self.masked) else 0

    @property
    def tile(self):
        if self.kind == "shared":
            return SHARED_TILE_ROWS
        if self.kind == "decompress":
            return DECOMPRESS_TILE_ROWS
        return min([scan_tile(w) for w in self.widths] or [8192])

    def lengths(self):
        T = self.tile
        out = [1, 77, 2 * T, 2 * T + 1, 3 * T - 1, 4 * T, 5 * T + T // 2 + 3]
        if self.kind == "rowids":
            out.append(2 * ROWID_CHUNK_ROWS + 43)
        return out


def _cases():
    out = []
    for c in WIDTHS:
        out.append(Case(f"scan_eq_c{c}", "mi355_scan_eq_dev", "scan", c, op=EQ))
        out.append(Case(f"scan_range_c{c}", "mi355_scan_range_dev", "scan", c, op=BETWEEN))
        for op in range(8):
            out.append(Case(f"where_{OP_NAMES[op]}_c{c}", "mi355_scan_where_dev", "scan", c, op=op))
        for mop in range(4):
            out.append(Case(f"combine_{MASK_NAMES[mop]}_c{c}", "mi355_scan_combine_dev", "scan", c, op=(BETWEEN, NE, GT, NOT_BETWEEN)[mop], mask_op=mop))
        out.append(Case(f"combine_inplace_c{c}", "mi355_scan_combine_dev", "scan", c, op=LE, mask_op=(OR, XOR, AND, ANDNOT, OR, XOR)[WIDTHS.index(c)],
                        inplace=True))
        out.append(Case(f"combine_count_only_c{c}", "mi355_scan_combine_dev", "scan", c, op=GE, count_only=True))
        out.append(Case(f"combine_count_only_masked_c{c}", "mi355_scan_combine_dev", "scan", c, op=NE, mask_op=XOR, count_only=True))
        for negate in (0, 1):
            for masked in (False, True):
                out.append(Case(f"in_{'chain' if c > 16 else 'bitset'}{'_not' if negate else ''}{'_masked' if masked else ''}_c{c}",
                                "mi355_scan_in_dev", "scan", c, P=5, negate=negate, masked=masked))
        for sk in (0, 1):
            out.append(Case(f"select{sk}_exact_c{c}", "mi355_scan_select_dev", "scan", c, op=(GT, NE)[sk], select_kernel=sk))
            out.append(Case(f"select{sk}_masked_roomy_c{c}", "mi355_scan_select_dev", "scan", c, op=(BETWEEN, LT)[sk], mask_op=(AND, XOR)[sk],
                            select_kernel=sk, extra=100))
        out.append(Case(f"scan2_same_c{c}", "mi355_scan2_dev", "scan2", c, c, op=GE, op2=NE, mask_op=WIDTHS.index(c) % 4))
        out.append(Case(f"gather_c{c}", "mi355_gather_dev", "gather", c))
        for masked in (False, True):
            out.append(Case(f"aggregate{'_masked' if masked else ''}_c{c}", "mi355_aggregate_dev", "aggregate", c, masked=masked))
        out.append(Case(f"decompress_c{c}", "mi355_decompress_dev", "decompress", c))
        out.append(Case(f"pack_u32_c{c}", "mi355_pack_u32_dev", "pack", c))
        if c <= 16:
            out.append(Case(f"pack_u16_c{c}", "mi355_pack_u16_dev", "pack", c))
        for kind in (0, 2):  # MI355_GEN_MOD, MI355_GEN_INDEX
            out.append(Case(f"generate_{('mod', '', 'index')[kind]}_c{c}", "mi355_generate_dev", "pack", c, extra=kind))
    for c1, c2, mop in ((5, 9, ANDNOT), (12, 17, AND), (32, 1, XOR), (17, 12, OR)):
        out.append(Case(f"scan2_c{c1}_c{c2}", "mi355_scan2_dev", "scan2", c1, c2, op=LT, op2=GE, mask_op=mop))
    for c1, c2, op2 in ((9, 9, LE), (9, 12, GE)):
        out.append(Case(f"scan2_count_only_c{c1}_c{c2}", "mi355_scan2_dev", "scan2", c1, c2, op=NE, op2=op2, mask_op=OR, count_only=True))
    for j, (c1, c2) in enumerate(((1, 1), (9, 9), (17, 17), (32, 32), (5, 12), (17, 9), (32, 1), (12, 32))):
        out.append(Case(f"columns_c{c1}_c{c2}", "mi355_scan_columns_dev", "columns", c1, c2, op=(LT, BETWEEN, NE, GE)[j % 4]))
        out.append(Case(f"columns_masked_c{c1}_c{c2}", "mi355_scan_columns_dev", "columns", c1, c2, op=(NOT_BETWEEN, EQ, GT, LE)[j % 4],
                        mask_op=(AND, XOR, ANDNOT, OR)[j % 4]))
    # shared scans: (c, P, layout, hits) -> family, as mi355_shared_scan_kernel / mi355_shared_where_kernel name it
    PAIR, LUT, MULTI, WIDE, LINEAR, GENERAL, SINGLE = ("shared_pair_kernel", "shared_lut_kernel", "shared_lut_kernel(multi-pass)", "shared_wide_kernel",
                                                        "shared_linear_kernel", "shared_general_kernel", "scan_burst_kernel")
    for c, P, layout, hits, fam in (
            (9, 1, 0, True, SINGLE), (17, 1, 1, False, SINGLE),
            (5, 2, 0, True, PAIR), (9, 2, 1, False, PAIR), (32, 2, 0, False, PAIR),
            (9, 4, 0, True, LUT), (12, 8, 0, False, LUT), (17, 7, 1, True, LUT), (1, 8, 1, False, LUT), (32, 5, 0, True, LUT),
            (17, 170, 1, False, MULTI),
            (9, 24, 0, True, WIDE), (9, 24, 0, False, WIDE), (17, 40, 0, True, WIDE), (12, 48, 0, True, WIDE), (5, 12, 0, False, WIDE),
            (9, 9, 1, True, LINEAR), (12, 16, 1, True, LINEAR), (9, 65, 1, False, LINEAR), (17, 33, 1, True, LINEAR), (5, 12, 1, True, LINEAR),
            (32, 800, 0, False, GENERAL)):
        out.append(Case(f"shared_eq_c{c}_p{P}_{'linear' if layout else 'pp'}{'' if hits else '_nohits'}", "mi355_shared_scan_eq_dev", "shared", c, P=P,
                        layout=layout, hits=hits, family=fam))
    WLUT, WMULTI, WCHAIN = "shared_where_lut_kernel", "shared_where_lut_kernel(multi-pass)", "shared_where_chain_kernel"
    for c, P, layout, hits, fam in (
            (9, 1, 0, True, SINGLE), (12, 1, 1, False, SINGLE),
            (5, 3, 0, True, WLUT), (12, 8, 1, True, WLUT), (9, 8, 0, False, WLUT), (5, 8, 1, False, WLUT),
            (9, 12, 0, True, WMULTI), (12, 20, 1, False, WMULTI), (5, 9, 1, True, WMULTI), (9, 16, 0, False, WMULTI),
            (17, 4, 0, True, WCHAIN), (32, 12, 1, True, WCHAIN), (17, 9, 1, False, WCHAIN), (32, 3, 0, False, WCHAIN)):
        out.append(Case(f"shared_where_c{c}_p{P}_{'linear' if layout else 'pp'}{'' if hits else '_nohits'}", "mi355_shared_scan_where_dev", "shared", c,
                        P=P, op=NE, layout=layout, hits=hits, family=fam))
    for mop in range(4):
        out.append(Case(f"bitmap_{MASK_NAMES[mop]}", "mi355_bitmap_combine_dev", "bitmap", mask_op=mop))
        out.append(Case(f"bitmap_{MASK_NAMES[mop]}_into_a", "mi355_bitmap_combine_dev", "bitmap", mask_op=mop, inplace=True))
    out.append(Case("bitmap_count", "mi355_bitmap_count_dev", "count"))
    out.append(Case("bitmap_to_rowids", "mi355_bitmap_to_rowids_dev", "rowids"))
    for c in HIST_WIDTHS:
        for masked in (False, True):
            out.append(Case(f"histogram{'_masked' if masked else ''}_c{c}", "mi355_histogram_dev", "histogram", c, masked=masked))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}


# ------------------------------------------------------------------------------------------------------------------------
# the numpy model: what a case computes from the value rows V (one int64 array per column) and the bit arrays B (one bool
# array per mask / bitmap operand) a kernel takes for its n rows.  n0 is the view's true length: what the row ids of gather
# are made from, whatever a leaking kernel takes n to be.
# ------------------------------------------------------------------------------------------------------------------------

def where_predicates(case):
    """the P predicates of a shared where-scan: every comparison in turn around u = mid(c), so that u fails every one"""
    u = mid(case.c)
    table = ((EQ, u + 1, 0), (NE, u, 0), (LT, u, 0), (LE, u - 1, 0), (GT, u, 0), (GE, u + 1, 0), (BETWEEN, u + 1, u + 2), (NOT_BETWEEN, u - 1, u + 1))
    return [table[(k + 1) % 8] for k in range(case.P)]  # (k + 1): a list never starts with EQ, P = 2 is never all-EQ either


def predicate_rows(case, V):
    """bool (P, n) of the unmasked predicate(s)"""
    v = V[0]
    if case.kind == "shared":
        if case.sym == "mi355_shared_scan_where_dev":
            return np.stack([compare(op, v, a, b) for op, a, b in where_predicates(case)])
        return v[None, :] == np.asarray(key_list(case.c, case.P), dtype=np.int64)[:, None]
    if case.kind == "scan2":
        p1, p2 = compare(case.op, V[0], *constants(case.op, case.c)), compare(case.op2, V[1], *constants(case.op2, case.c2))
        return {AND: p1 & p2, OR: p1 | p2, XOR: p1 ^ p2, ANDNOT: p1 & ~p2}[case.mask_op][None, :]
    if case.kind == "columns":
        a, b = COLUMN_CONSTANTS[case.op]
        return compare(case.op, V[0] - V[1], a, b)[None, :]
    if case.sym == "mi355_scan_in_dev":
        p = np.isin(v, np.asarray([k for k in key_list(case.c, case.P) if k <= vmax(case.c)], dtype=np.int64))
        return (~p if case.negate else p)[None, :]
    return compare(case.op, v, *constants(case.op, case.c))[None, :]


def and_like(case):
    """a leak behind a zero mask bit is invisible by contract: conjunctions with the mask, and the all-canonical bitmap consumers"""
    if case.kind in ("bitmap", "count", "rowids"):
        return True
    if case.kind == "scan2" or not case.nbitmaps:
        return False
    return case.masked or case.mask_op in (AND, ANDNOT)


def expect(case, V, B, n0):
    n = len(V[0]) if V else len(B[0])
    if case.kind in ("scan", "scan2", "columns", "shared"):
        p = predicate_rows(case, V)
        if case.kind != "scan2" and case.nbitmaps:
            p = combine(AND if case.masked else case.mask_op, p, B[0][None, :])
        if case.kind == "shared":
            out = {"bitmaps": np.packbits(p, axis=1, bitorder="little")}
            if case.hits:
                out["hits"] = p.sum(axis=1).astype(np.uint64)
            return out
        if case.sym == "mi355_scan_select_dev":
            return {"ids": np.nonzero(p[0])[0].astype(np.uint64) + np.uint64(FIRST_ROW), "count": int(p.sum())}
        out = {"hits": int(p.sum())}
        if not case.count_only:
            out["bitmap"] = packbits(p[0])
        return out
    if case.kind == "bitmap":
        r = {AND: B[0] & B[1], OR: B[0] | B[1], XOR: B[0] ^ B[1], ANDNOT: B[0] & ~B[1]}[case.mask_op]
        return {"bitmap": packbits(r), "hits": int(r.sum())}
    if case.kind == "count":
        return {"hits": int(B[0].sum())}
    if case.kind == "rowids":
        return {"ids": np.nonzero(B[0])[0].astype(np.uint64) + np.uint64(FIRST_ROW), "count": int(B[0].sum())}
    if case.kind == "gather":
        rows = gather_rows(case, n0)
        inside = (rows >= 0) & (rows < n)
        vals = np.where(inside, V[0][np.clip(rows, 0, n - 1)], -1)
        return {"out": vals.astype(np.uint32).view(np.int32)}
    sel = B[0] if case.masked else np.ones(n, dtype=bool)
    if case.kind == "aggregate":
        v = V[0][sel].astype(np.uint64)
        return {"agg": [int(v.sum()), len(v), int(v.min()), int(v.max())] if len(v) else [0, 0, 2 ** 64 - 1, 0]}
    if case.kind == "histogram":
        return {"counts": np.bincount(V[0][sel], minlength=1 << case.c).astype(np.uint64)}
    if case.kind == "decompress":
        return {"out": V[0].astype(np.uint32).view(np.int32)}
    raise AssertionError(case.kind)


def gather_rows(case, n0):
    """row indices (relative to the view) to fetch: random rows of the view, its edges, and rows that exist in the arena in
    front of and behind the view, which must yield -1"""
    rng = np.random.default_rng(n0)
    inside = rng.integers(0, n0, 300)
    return np.concatenate([inside, [0, n0 - 1, n0, n0 + 1, n0 + 5, n0 + 7, n0 + 8, n0 + HOSTILE_ROWS - 1, -1, -2, -HOSTILE_ROWS]]).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------------
# the arena (numpy side): values of the whole column, the view's place in it, the mask bytes
# ------------------------------------------------------------------------------------------------------------------------

def hostile_values(case, fill):
    """one sequence of hostile values per column, cycled over the rows outside the view"""
    if case.kind in ("aggregate", "histogram", "gather", "decompress"):
        return [[0] if fill == "match" else [vmax(case.c)]]
    cands = [candidates(w) + (key_list(w, case.P) if case.P > 1 and w > 1 else []) for w in case.widths]
    if len(cands) == 2:
        m = mid(min(case.widths))
        near = [x for x in (0, 1, m - 1, m, m + 1, m + 2, m + 3) if 0 <= x <= vmax(min(case.widths))]
        pairs = [(x, y) for x in near for y in near] + [(cands[0][-1], 0), (0, cands[1][-1]), (cands[0][-1], cands[1][-1])]
    else:
        pairs = [(x,) for x in cands[0]]
    P = predicate_rows(case, [np.asarray([t[j] for t in pairs], dtype=np.int64) for j in range(len(case.widths))])
    if fill == "miss":
        chosen = [t for t, hit in zip(pairs, P.any(axis=0)) if not hit]
    else:  # a satisfying row for every predicate in turn
        chosen = [pairs[int(np.argmax(row))] for row in P if row.any()]  # (a key outside [0, 2^c) has none)
    assert chosen, f"{case.id}: no {fill} value among the candidates"
    return [[t[j] for t in chosen] for j in range(len(case.widths))]


def draw_view(case, n, rng):
    """the view's own values: half of them from the values next to the constants, so that both outcomes occur"""
    V = []
    for w in case.widths:
        if case.kind in ("aggregate", "histogram") and w >= 2:
            V.append(rng.integers(1, vmax(w), n, dtype=np.int64))  # [1, 2^c - 2]
            continue
        v = rng.integers(0, vmax(w) + 1, n, dtype=np.int64)
        near = rng.random(n) < 0.5
        pool = np.asarray(candidates(w) + (key_list(w, case.P) if case.P > 1 and w > 1 else []), dtype=np.int64)
        v[near] = pool[rng.integers(0, len(pool), int(near.sum()))]
        V.append(v)
    if case.kind == "columns":  # differences near 0 in half of the rows
        near = rng.random(n) < 0.5
        V[1][near] = np.clip(V[0][near] + rng.integers(-4, 5, int(near.sum())), 0, vmax(case.c2))
    return V


class Model:
    """one (case, n, fill): the whole column of every width, the view [a, a + n) in it, the mask operands with their hostile
    bytes behind -- numpy only, nothing packed"""

    def __init__(self, case, n, fill):
        self.case, self.n, self.fill = case, n, fill
        rng = np.random.default_rng(zlib.crc32(f"{case.id}/{n}".encode()))
        self.V = draw_view(case, n, rng)
        self.B = [rng.random(n) < 0.5 for _ in range(case.nbitmaps)]
        hostile = hostile_values(case, fill) if case.widths else []
        self.columns = []
        for j, w in enumerate(case.widths):
            front = self.prefix_rows(w)
            behind = case.tile + HOSTILE_ROWS
            h = np.asarray(hostile[j], dtype=np.int64)
            # the cycle starts at the first row behind the view; in front of it, it runs backwards
            self.columns.append((np.concatenate([np.resize(h, front)[::-1], self.V[j], np.resize(h, behind)]), front))
        # bitmap operands: 0xFF behind a mask whatever the fill; the bitmap consumers flip their second operand's fill,
        # since a & ~b and a ^ b hide a leak when both neighbours are 0xFF
        self.hostile_byte = [0xFF if (j == 0 or fill == "match") else 0x00 for j in range(case.nbitmaps)]

    def prefix_rows(self, w):
        """rows in front of the view: an odd multiple of 128 rows at odd widths (16 mod 32 bytes), 288 = 32 x 9 rows for the
        4-byte pointer of gather (4 mod 8 bytes at odd widths); at even widths the whole arena is shifted instead"""
        if self.case.kind == "gather":
            return 288 if w % 2 else HOSTILE_ROWS
        return 384 if w % 2 else HOSTILE_ROWS

    def taken(self, rows, bits):
        """what a kernel sees that takes `rows` value rows and `bits` mask bits from the view's start"""
        V = [col[a: a + rows] for col, a in self.columns]
        B = []
        for b, fill in zip(self.B, self.hostile_byte):
            full = np.concatenate([np.unpackbits(packbits(b), bitorder="little").astype(bool), np.full(8 * HOSTILE_BYTES, bool(fill))])
            B.append(full[:bits])
        return V, B

    def own(self):
        return self.taken(self.n, self.n)


def differs(e0, e1):
    for k in e0:
        x, y = e0[k], e1[k]
        if isinstance(x, np.ndarray):
            w = max(x.shape[-1], y.shape[-1])
            x, y = (np.pad(z, [(0, 0)] * (z.ndim - 1) + [(0, w - z.shape[-1])]) for z in (x, y))
            if not np.array_equal(x, y):
                return True
        elif x != y:
            return True
    return False


def leak_models(case, n):
    """(name, value rows taken, mask bits taken)"""
    nb8 = (n + 7) // 8 * 8
    out = [("one row more", n + 1, n + 1)]
    if n % 8:
        out.append(("the last byte's bits >= n", nb8, nb8))
    if case.nbitmaps:
        out.append(("one mask byte more", nb8 + 8, nb8 + 8))
    return out


def hidden(case, n, name):
    """leaks the contract itself hides (see the module docstring): behind a canonical mask's zero bits"""
    return and_like(case) and name != "one mask byte more" and n % 8 != 0


# ------------------------------------------------------------------------------------------------------------------------
# CPU: the table is complete and no case passes vacuously
# ------------------------------------------------------------------------------------------------------------------------

def header_dev_symbols():
    """every MI355_API ..._dev( symbol of the two headers, read as test_capi_symbols.header_symbols reads the first"""
    names = set()
    for h in ("mi355_scan.h", "mi355_columns.h"):
        text = open(os.path.join(ROOT, "include", h)).read()
        names |= set(re.findall(r"^MI355_API [^;(]*?\b(mi355_\w+)\(", text, flags=re.M))
    return sorted(s for s in names if s.endswith("_dev") or s.startswith("mi355_dev_"))


def test_case_ids_unique():
    assert len(BY_ID) == len(CASES)


def test_every_dev_symbol_has_a_case():
    symbols = header_dev_symbols()
    assert len(symbols) >= 30 and "mi355_scan_columns_dev" in symbols, symbols  # the parse found both headers
    covered = {c.sym for c in CASES}
    missing = sorted(set(symbols) - covered - set(EXCLUDED))
    assert not missing, f"_dev symbols without a case in this module (and not in EXCLUDED): {missing}"
    stale = sorted((covered | set(EXCLUDED)) - set(symbols))
    assert not stale, f"cases / exclusions for symbols no header declares: {stale}"
    assert not covered & set(EXCLUDED)
    assert set(EXCLUDED.values()) == {"RCCL", "mi355_dev_*", "mi355_tune_dev"}


def test_tile_sizes_are_the_librarys():
    from shared_simd_scan_amd import lib

    for c in range(1, 33):
        assert lib().mi355_tile_values(c) == scan_tile(c), c
    text = open(os.path.join(ROOT, "shared_simd_scan_amd", "csrc", "kernels", "decompress.hpp")).read()
    assert f"TILE_VALUES = {DECOMPRESS_TILE_ROWS};" in text
    text = open(os.path.join(ROOT, "shared_simd_scan_amd", "csrc", "kernels", "bitmap.hpp")).read()
    assert f"kRowidChunk = {ROWID_CHUNK_ROWS // 8};" in text


def test_table_covers_the_variants_the_contract_names():
    def has(**kw):
        return any(all(getattr(c, k) == v for k, v in kw.items()) for c in CASES)

    for c in WIDTHS:
        assert all(has(sym="mi355_scan_where_dev", c=c, op=op) for op in range(8))
        assert all(has(sym="mi355_scan_combine_dev", c=c, mask_op=m, inplace=False, count_only=False) for m in range(4))
        assert has(sym="mi355_scan_combine_dev", c=c, inplace=True) and has(sym="mi355_scan_combine_dev", c=c, count_only=True)
        assert all(has(sym="mi355_scan_in_dev", c=c, negate=g, masked=m) for g in (0, 1) for m in (False, True))
        assert all(has(sym="mi355_scan_select_dev", c=c, select_kernel=k, extra=e) for k in (0, 1) for e in (0, 100))
        assert all(has(sym=s, c=c, masked=m) for s in ("mi355_aggregate_dev",) for m in (False, True))
    for c in HIST_WIDTHS:
        assert all(has(sym="mi355_histogram_dev", c=c, masked=m) for m in (False, True))
    scan2 = [c for c in CASES if c.kind == "scan2"]
    assert any(c.c == c.c2 for c in scan2) and any(c.c != c.c2 and not c.count_only for c in scan2)
    assert any(c.count_only and c.c == c.c2 for c in scan2) and any(c.count_only and c.c != c.c2 for c in scan2)
    cols = [c for c in CASES if c.kind == "columns"]
    assert all(any((c.c == c.c2) == same and (c.mask_op >= 0) == m for c in cols) for same in (False, True) for m in (False, True))
    assert all(has(kind="bitmap", mask_op=m, inplace=i) for m in range(4) for i in (False, True))
    for sym, families in (("mi355_shared_scan_eq_dev", {"scan_burst_kernel", "shared_pair_kernel", "shared_lut_kernel", "shared_lut_kernel(multi-pass)",
                                                        "shared_wide_kernel", "shared_linear_kernel", "shared_general_kernel"}),
                          ("mi355_shared_scan_where_dev", {"scan_burst_kernel", "shared_where_lut_kernel", "shared_where_lut_kernel(multi-pass)",
                                                           "shared_where_chain_kernel"})):
        mine = [c for c in CASES if c.sym == sym]
        assert {c.family for c in mine} == families
        assert {c.layout for c in mine} == {0, 1} and {c.hits for c in mine} == {False, True}
    for c in CASES:
        T = c.tile
        assert set(c.lengths()) >= {1, 77, 2 * T, 2 * T + 1, 3 * T - 1, 4 * T, 5 * T + T // 2 + 3} and max(c.lengths()) <= 70_000, c.id


def test_where_lists_are_not_handed_to_the_equality_scan():
    for c in CASES:
        if c.sym == "mi355_shared_scan_where_dev" and c.P > 1:
            assert any(op != EQ for op, _, _ in where_predicates(c)), c.id


@pytest.mark.parametrize("cid", [c.id for c in CASES if c.kind != "pack"])
def test_a_one_row_leak_would_show(cid):
    """the condition that keeps the GPU tests from passing vacuously: a kernel that takes one row too many, does not mask
    the last byte, or reads one mask byte too many computes something else than the view's own result in at least one fill.
    (min / max of the aggregate and the per-value counters of the histogram are part of the compared result, but at c = 1
    only sum / count and the totals are what differs.)"""
    case = BY_ID[cid]
    for n in case.lengths():
        models = {fill: Model(case, n, fill) for fill in FILLS}
        own = {fill: expect(case, *m.own(), n) for fill, m in models.items()}
        for name, rows, bits in leak_models(case, n):
            if hidden(case, n, name):
                continue
            shown = [fill for fill, m in models.items() if differs(own[fill], expect(case, *m.taken(rows, bits), n))]
            assert shown, f"{cid}, n = {n}: '{name}' changes nothing in either fill: the case cannot notice that leak"
        for fill, m in models.items():  # the arena holds what the docstring promises
            for (col, a), w in zip(m.columns, case.widths):
                assert a >= HOSTILE_ROWS and len(col) - a - n >= case.tile + HOSTILE_ROWS and col.max() <= vmax(w) and col.min() >= 0
    if case.kind in ("scan", "scan2", "columns", "shared") and case.P <= 8:  # both outcomes occur inside the view
        p = predicate_rows(case, Model(case, 2 * case.tile + 1, "miss").own()[0])
        if case.kind == "shared" and case.c == 1:
            p = p[::2]  # (every other key of a 1-bit list lies outside [0, 2^c) and matches nothing)
        assert p.any(axis=1).all() and (~p).any(axis=1).all(), cid


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------

def np_pack(vals, c, size):
    """values -> the packed stream (value i at bits [c*i, c*i + c), LSB first), zero padded to `size` bytes"""
    bits = ((np.asarray(vals, dtype=np.uint64)[:, None] >> np.arange(c, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8)
    out = np.zeros(size, dtype=np.uint8)
    body = np.packbits(bits.reshape(-1), bitorder="little")
    out[: len(body)] = body
    return out


def u64(g):
    return int(g.fetch().view(np.uint64)[0])


def run_case(rt, eng, case, model):
    """one call on the view; -> the outputs in the shape expect() gives them (guards checked on the way)"""
    L, ctx, n, c = rt.L, eng._ctx, model.n, case.c
    vp = C.c_void_p
    keep = []  # tensors stay alive until the results are back

    def col(j, align=16):
        t, p = rt.column(model, j, align)
        keep.append(t)
        return vp(p)

    def bm(j, align=16):
        t, p = rt.bitmap(model, j, align)
        keep.append(t)
        return vp(p)

    def ok(rc):
        assert rc == 0, L.mi355_last_error()
        eng.synchronize()

    nb = (n + 7) // 8
    want = expect(case, *model.own(), n)
    if case.kind in ("scan", "scan2", "columns") and case.sym != "mi355_scan_select_dev":
        hits = rt.word()
        mask = None
        if case.inplace:  # the mask is the result buffer: 0xFF around it inside the 0xEE guards
            out = Guarded(nb + 2 * HOSTILE_BYTES, front=4096 + 16 - HOSTILE_BYTES)
            image = np.concatenate([np.full(HOSTILE_BYTES, 0xFF, dtype=np.uint8), packbits(model.B[0]), np.full(HOSTILE_BYTES, 0xFF, dtype=np.uint8)])
            out.t[out.front: out.front + len(image)] = rt.torch.from_numpy(image).cuda()
            bitmap = mask = vp(out.ptr.value + HOSTILE_BYTES)
            assert bitmap.value % 32 == 16
        else:
            out = None if case.count_only else rt.out(nb)
            bitmap = out.ptr if out else None
            if case.kind != "scan2" and case.nbitmaps:
                mask = bm(0)
        a, b = constants(case.op, c)
        if case.sym == "mi355_scan_eq_dev":
            ok(L.mi355_scan_eq_dev(ctx, col(0), n, c, as_i32(a), bitmap, hits.ptr))
        elif case.sym == "mi355_scan_range_dev":
            ok(L.mi355_scan_range_dev(ctx, col(0), n, c, a, b, bitmap, hits.ptr))
        elif case.sym == "mi355_scan_where_dev":
            ok(L.mi355_scan_where_dev(ctx, col(0), n, c, case.op, a, b, mask, bitmap, hits.ptr))
        elif case.sym == "mi355_scan_combine_dev":
            ok(L.mi355_scan_combine_dev(ctx, col(0), n, c, case.op, a, b, max(case.mask_op, 0), mask, bitmap, hits.ptr))
        elif case.sym == "mi355_scan_in_dev":
            keys = np.asarray([as_i32(k) for k in key_list(c, case.P)], dtype=np.int32)
            ok(L.mi355_scan_in_dev(ctx, col(0), n, c, keys.ctypes.data_as(vp), case.P, case.negate, mask, bitmap, hits.ptr))
        elif case.sym == "mi355_scan2_dev":
            a2, b2 = constants(case.op2, case.c2)
            ok(L.mi355_scan2_dev(ctx, col(0), c, case.op, a, b, col(1), case.c2, case.op2, a2, b2, n, case.mask_op, bitmap, hits.ptr))
        else:
            a, b = COLUMN_CONSTANTS[case.op]
            ok(L.mi355_scan_columns_dev(ctx, col(0), c, col(1), case.c2, n, case.op, a, b, max(case.mask_op, 0), mask, bitmap, hits.ptr))
        got = {"hits": u64(hits)}
        if case.inplace:
            body = out.fetch()
            assert (body[:HOSTILE_BYTES] == 0xFF).all() and (body[HOSTILE_BYTES + nb:] == 0xFF).all(), "bytes around the in-place bitmap changed"
            got["bitmap"] = body[HOSTILE_BYTES: HOSTILE_BYTES + nb]
        elif out:
            got["bitmap"] = out.fetch()
        return got, want
    if case.sym == "mi355_scan_select_dev":
        cap = want["count"] + case.extra
        ids, cnt = Guarded(8 * cap, back=4096), rt.word()
        a, b = constants(case.op, c)
        eng.set_option("select_kernel", case.select_kernel)
        ok(L.mi355_scan_select_dev(ctx, col(0), n, c, case.op, a, b, max(case.mask_op, 0), bm(0) if case.nbitmaps else None, FIRST_ROW, ids.ptr, cap,
                                   cnt.ptr))
        rec = parse_record(L.mi355_ctx_last_launch(ctx).decode())
        assert [base_name(r[0]) for r in rec] == ["select_kernel" if case.select_kernel else "select2_kernel"], rec
        body = ids.fetch().view(np.uint64)
        assert (body[want["count"]:].view(np.uint8) == SENTINEL).all(), "ids written beyond the count"
        return {"ids": body[: want["count"]], "count": u64(cnt)}, want
    if case.kind == "shared":
        P = case.P
        stride = (nb + 15) // 16 * 16 + 16  # a guard gap behind every bitmap of the per-predicate layout
        out = rt.out(P * stride if case.layout == 0 else P * nb)
        hits = Guarded(8 * P) if case.hits else None
        if case.sym == "mi355_shared_scan_eq_dev":
            named = L.mi355_shared_scan_kernel(ctx, c, P, case.layout, int(case.hits))
            keys = np.asarray([as_i32(k) for k in key_list(c, P)], dtype=np.int32)
            ok(L.mi355_shared_scan_eq_dev(ctx, col(0), n, c, keys.ctypes.data_as(vp), P, case.layout, out.ptr, stride, hits.ptr if hits else None))
        else:
            from shared_simd_scan_amd._capi import Predicate

            named = L.mi355_shared_where_kernel(ctx, c, P, case.layout, int(case.hits))
            preds = (Predicate * P)(*[Predicate(op, 0, a, b) for op, a, b in where_predicates(case)])
            ok(L.mi355_shared_scan_where_dev(ctx, col(0), n, c, C.cast(preds, vp), P, case.layout, out.ptr, stride, hits.ptr if hits else None))
        rec = parse_record(L.mi355_ctx_last_launch(ctx).decode())
        assert named.decode() == case.family, f"{case.id}: the library names {named}"
        assert len(rec) == 1 and family_of(rec[0][0]) == case.family, rec
        body = out.fetch()
        if case.layout == 0:
            seg = body.reshape(P, stride)
            assert (seg[:, nb:] == SENTINEL).all(), "bytes between the per-predicate bitmaps overwritten"
            got = {"bitmaps": seg[:, :nb]}
        else:
            got = {"bitmaps": np.ascontiguousarray(body.reshape(nb, P).T)}
        if hits:
            got["hits"] = hits.fetch().view(np.uint64)
        return got, want
    if case.kind == "bitmap":
        hits = rt.word()
        if case.inplace:  # out aliases a
            out = Guarded(nb + 2 * HOSTILE_BYTES, front=4096 + 16 - HOSTILE_BYTES)
            image = np.concatenate([np.full(HOSTILE_BYTES, 0xFF, dtype=np.uint8), packbits(model.B[0]), np.full(HOSTILE_BYTES, 0xFF, dtype=np.uint8)])
            out.t[out.front: out.front + len(image)] = rt.torch.from_numpy(image).cuda()
            a = dst = vp(out.ptr.value + HOSTILE_BYTES)
            assert a.value % 32 == 16
        else:
            out = rt.out(nb)
            a, dst = bm(0), out.ptr
        ok(L.mi355_bitmap_combine_dev(ctx, case.mask_op, a, bm(1), dst, n, hits.ptr))
        body = out.fetch()
        if case.inplace:
            assert (body[:HOSTILE_BYTES] == 0xFF).all() and (body[HOSTILE_BYTES + nb:] == 0xFF).all(), "bytes around the in-place bitmap changed"
            body = body[HOSTILE_BYTES: HOSTILE_BYTES + nb]
        return {"bitmap": body, "hits": u64(hits)}, want
    if case.kind == "count":
        hits = rt.word()
        ok(L.mi355_bitmap_count_dev(ctx, bm(0), n, hits.ptr))
        return {"hits": u64(hits)}, want
    if case.kind == "rowids":
        ids, cnt = Guarded(8 * want["count"], back=4096), rt.word()
        ok(L.mi355_bitmap_to_rowids_dev(ctx, bm(0, align=4), n, FIRST_ROW, ids.ptr, want["count"], cnt.ptr))
        return {"ids": ids.fetch().view(np.uint64), "count": u64(cnt)}, want
    if case.kind == "gather":
        rows = (gather_rows(case, n) + FIRST_ROW).astype(np.uint64)
        drows = rt.torch.from_numpy(rows.view(np.int64)).cuda()
        dcnt = rt.torch.tensor([len(rows)], dtype=rt.torch.int64, device="cuda")
        out = Guarded(4 * len(rows))
        ok(L.mi355_gather_dev(ctx, col(0, align=4), n, c, FIRST_ROW, vp(drows.data_ptr()), vp(dcnt.data_ptr()), len(rows), out.ptr))
        return {"out": out.fetch().view(np.int32)}, want
    if case.kind == "aggregate":
        out = Guarded(32, back=64, front=64)
        ok(L.mi355_aggregate_dev(ctx, col(0), n, c, bm(0, align=4) if case.masked else None, out.ptr))
        return {"agg": out.fetch().view(np.uint64).tolist()}, want
    if case.kind == "histogram":
        out = Guarded(8 << c)
        ok(L.mi355_histogram_dev(ctx, col(0), n, c, bm(0, align=4) if case.masked else None, out.ptr))
        return {"counts": out.fetch().view(np.uint64)}, want
    if case.kind == "decompress":
        out = rt.out(4 * n)
        ok(L.mi355_decompress_dev(ctx, col(0), n, c, out.ptr))
        return {"out": out.fetch().view(np.int32)}, want
    raise AssertionError(case.kind)


def run_pack(rt, eng, case, n):
    """pack / generate: exact bytes, pad included, at a destination that is 4 mod 8"""
    L, ctx, c = rt.L, eng._ctx, case.c
    size = L.mi355_compressed_buffer_size(c, n)
    out = rt.out(size, align=4)
    rng = np.random.default_rng(n + c)
    if case.sym == "mi355_generate_dev":
        first, param = (1 << 33) + 7, 1000003
        rows = np.arange(n, dtype=np.uint64) + np.uint64(first)
        vals = rows % np.uint64(param) if case.extra == 0 else rows
        rc = L.mi355_generate_dev(ctx, case.extra, first, n, c, param, out.ptr)
    else:
        dtype = np.uint16 if case.sym == "mi355_pack_u16_dev" else np.uint32
        vals = rng.integers(0, vmax(c) + 1, n, dtype=np.uint64).astype(dtype)
        dv = rt.torch.from_numpy(vals.view(np.int16 if dtype == np.uint16 else np.int32)).cuda()
        rc = getattr(L, case.sym)(ctx, C.c_void_p(dv.data_ptr()), n, c, out.ptr)
    assert rc == 0, L.mi355_last_error()
    eng.synchronize()
    want = np_pack(vals.astype(np.uint64) & np.uint64(vmax(c)), c, size)
    assert np.array_equal(out.fetch(), want), f"{case.id}, n = {n}: packed bytes differ"


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_view_at_minimum_alignment(rt, cid):
    """both fills, every view length, the default grid and the 4-wave grid: every output equals numpy over the view alone"""
    case = BY_ID[cid]
    for n in case.lengths():
        for grid, eng in (("default", rt.default), ("4 waves", rt.capped)):
            if case.kind == "pack":
                run_pack(rt, eng, case, n)
                continue
            for fill in FILLS:
                got, want = run_case(rt, eng, case, Model(case, n, fill))
                assert set(got) == set(want)
                for k in want:
                    same = np.array_equal(got[k], want[k]) if isinstance(want[k], np.ndarray) else got[k] == want[k]
                    assert same, f"{cid}, n = {n}, fill = {fill}, grid = {grid}: {k} differs from numpy over the view"


# ---- rejection: half the minimum alignment, per pointer argument ------------------------------------------------------------

REJECT_N, REJECT_C = 77, 9
# entry point -> (call, the pointer arguments that carry an alignment requirement); p holds nominal addresses
REJECTS = {
    "mi355_scan_eq_dev": (lambda L, x, p: L.mi355_scan_eq_dev(x, p["packed"], REJECT_N, REJECT_C, 5, p["bitmap"], p["hits"]), ("packed", "bitmap")),
    "mi355_scan_range_dev": (lambda L, x, p: L.mi355_scan_range_dev(x, p["packed"], REJECT_N, REJECT_C, 5, 9, p["bitmap"], p["hits"]), ("packed", "bitmap")),
    "mi355_scan_where_dev": (lambda L, x, p: L.mi355_scan_where_dev(x, p["packed"], REJECT_N, REJECT_C, LT, 5, 0, p["mask"], p["bitmap"], p["hits"]),
                             ("packed", "mask", "bitmap")),
    "mi355_scan_combine_dev": (lambda L, x, p: L.mi355_scan_combine_dev(x, p["packed"], REJECT_N, REJECT_C, LT, 5, 0, OR, p["mask"], p["bitmap"], p["hits"]),
                               ("packed", "mask", "bitmap")),
    "mi355_scan_in_dev": (lambda L, x, p: L.mi355_scan_in_dev(x, p["packed"], REJECT_N, REJECT_C, p["keys"], 3, 0, p["mask"], p["bitmap"], p["hits"]),
                          ("packed", "mask", "bitmap")),
    "mi355_scan2_dev": (lambda L, x, p: L.mi355_scan2_dev(x, p["packed"], REJECT_C, LT, 5, 0, p["packed2"], REJECT_C, GT, 7, 0, REJECT_N, AND, p["bitmap"],
                                                          p["hits"]), ("packed", "packed2", "bitmap")),
    "mi355_scan_columns_dev": (lambda L, x, p: L.mi355_scan_columns_dev(x, p["packed"], REJECT_C, p["packed2"], REJECT_C, REJECT_N, LT, 0, 0, AND, p["mask"],
                                                                        p["bitmap"], p["hits"]), ("packed", "packed2", "mask", "bitmap")),
    "mi355_shared_scan_eq_dev": (lambda L, x, p: L.mi355_shared_scan_eq_dev(x, p["packed"], REJECT_N, REJECT_C, p["keys"], 3, 0, p["bitmap"], 16, p["hits"]),
                                 ("packed", "bitmap")),
    "mi355_shared_scan_where_dev": (lambda L, x, p: L.mi355_shared_scan_where_dev(x, p["packed"], REJECT_N, REJECT_C, p["preds"], 3, 1, p["bitmap"], 16,
                                                                                  p["hits"]), ("packed", "bitmap")),
    "mi355_scan_select_dev": (lambda L, x, p: L.mi355_scan_select_dev(x, p["packed"], REJECT_N, REJECT_C, LT, 5, 0, AND, p["mask"], 0, p["wide"], 8,
                                                                      p["hits"]), ("packed", "mask")),
    "mi355_bitmap_combine_dev": (lambda L, x, p: L.mi355_bitmap_combine_dev(x, XOR, p["mask"], p["mask2"], p["bitmap"], REJECT_N, p["hits"]),
                                 ("mask", "mask2", "bitmap")),
    "mi355_bitmap_count_dev": (lambda L, x, p: L.mi355_bitmap_count_dev(x, p["mask"], REJECT_N, p["hits"]), ("mask",)),
    "mi355_bitmap_to_rowids_dev": (lambda L, x, p: L.mi355_bitmap_to_rowids_dev(x, p["mask"], REJECT_N, 0, p["wide"], 8, p["hits"]), ("mask",)),
    "mi355_gather_dev": (lambda L, x, p: L.mi355_gather_dev(x, p["packed"], REJECT_N, REJECT_C, 0, p["ids"], p["count"], 4, p["wide"]), ("packed",)),
    "mi355_aggregate_dev": (lambda L, x, p: L.mi355_aggregate_dev(x, p["packed"], REJECT_N, REJECT_C, p["mask"], p["wide"]), ("packed", "mask")),
    "mi355_histogram_dev": (lambda L, x, p: L.mi355_histogram_dev(x, p["packed"], REJECT_N, REJECT_C, p["mask"], p["wide"]), ("packed", "mask")),
    "mi355_decompress_dev": (lambda L, x, p: L.mi355_decompress_dev(x, p["packed"], REJECT_N, REJECT_C, p["wide"]), ("packed", "wide")),
    "mi355_pack_u32_dev": (lambda L, x, p: L.mi355_pack_u32_dev(x, p["values"], REJECT_N, REJECT_C, p["wide"]), ("wide",)),
    "mi355_pack_u16_dev": (lambda L, x, p: L.mi355_pack_u16_dev(x, p["values"], REJECT_N, REJECT_C, p["wide"]), ("wide",)),
    "mi355_generate_dev": (lambda L, x, p: L.mi355_generate_dev(x, 2, 0, REJECT_N, REJECT_C, 0, p["wide"]), ("wide",)),
}
# the argument name of the header behind each slot of REJECTS, for MIN_ALIGN_4
REJECT_ARG_NAMES = {("mi355_bitmap_to_rowids_dev", "mask"): "bitmap_dev", ("mi355_gather_dev", "packed"): "packed_dev",
                    ("mi355_aggregate_dev", "mask"): "mask_dev", ("mi355_histogram_dev", "mask"): "mask_dev",
                    ("mi355_pack_u32_dev", "wide"): "packed_dev", ("mi355_pack_u16_dev", "wide"): "packed_dev", ("mi355_generate_dev", "wide"): "packed_dev"}


def test_rejection_table_is_complete():
    assert set(REJECTS) == {c.sym for c in CASES}
    assert {(s, REJECT_ARG_NAMES[(s, a)]) for (s, a) in REJECT_ARG_NAMES} == MIN_ALIGN_4
    for (s, a) in REJECT_ARG_NAMES:
        assert a in REJECTS[s][1]


@pytest.mark.gpu
@pytest.mark.parametrize("sym", sorted(REJECTS))
def test_half_the_minimum_alignment_is_rejected(rt, sym):
    """8 mod 16 (2 mod 4 for the 4-byte pointers): MI355_E_INVALID, nothing launched, every output byte still 0xEE; the same call
    with every pointer at its minimum alignment is accepted"""
    from shared_simd_scan_amd._capi import Predicate

    torch, L, eng = rt.torch, rt.L, rt.default
    call, args = REJECTS[sym]
    vals = np.arange(4096, dtype=np.uint32) % 512
    cols = [torch.from_numpy(rt.O.pack(vals, REJECT_C)).cuda() for _ in range(2)]
    masks = [torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(2)]
    ids = torch.arange(8, dtype=torch.int64, device="cuda")
    count = torch.tensor([4], dtype=torch.int64, device="cuda")
    values = torch.zeros(4096, dtype=torch.int32, device="cuda")
    keys = np.asarray([1, 2, 3, 0, 0, 0, 0, 0], dtype=np.int32)
    preds = (Predicate * 3)(Predicate(LT, 0, 5, 0), Predicate(NE, 0, 7, 0), Predicate(GE, 0, 9, 0))
    for bad in (None,) + args:
        outs = {"bitmap": Guarded(4096), "wide": Guarded((8 << REJECT_C) + 64), "hits": Guarded(64, back=64, front=64)}
        p = {"packed": cols[0].data_ptr() + 16, "packed2": cols[1].data_ptr() + 16, "mask": masks[0].data_ptr() + 16, "mask2": masks[1].data_ptr() + 16,
             "bitmap": outs["bitmap"].ptr.value + 16, "wide": outs["wide"].ptr.value + 16, "hits": outs["hits"].ptr.value}
        for (s, a) in REJECT_ARG_NAMES:
            if s == sym:
                p[a] -= 12  # the 4-byte pointers: 4 mod 8
        if bad:
            p[bad] += 2 if (sym, bad) in REJECT_ARG_NAMES else 8
        p = {k: C.c_void_p(v) for k, v in p.items()}
        p.update(keys=keys.ctypes.data_as(C.c_void_p), preds=C.cast(preds, C.c_void_p), ids=C.c_void_p(ids.data_ptr()),
                 count=C.c_void_p(count.data_ptr()), values=C.c_void_p(values.data_ptr()))
        rc = call(L, eng._ctx, p)
        eng.synchronize()
        if bad is None:
            assert rc == 0, (sym, L.mi355_last_error())
            assert L.mi355_ctx_last_launch(eng._ctx) != b"", sym
            continue
        assert rc == MI355_E_INVALID, f"{sym}: {bad} at half its minimum alignment was accepted"
        assert b"aligned" in L.mi355_last_error() or b"multiples of 16" in L.mi355_last_error(), L.mi355_last_error()
        assert L.mi355_ctx_last_launch(eng._ctx) == b"", f"{sym}: something was launched"
        for name, g in outs.items():
            assert (g.fetch() == SENTINEL).all(), f"{sym}, {bad} misaligned: {name} was written"
