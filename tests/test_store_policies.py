"""Every result-store policy of every entry point that has one.  A feature kernel that writes a packed column or a bitmap picks its
store instruction at run time, by a policy word its launcher fills from the context option "scan_nt_stores": 0 plain, 1
non-temporal, 2 write-through.  store_words_by<N> (kernels/rt_column.hpp) branches on it once per tile, and N, the lane's dword
count, decides the store width: up to nine store instructions behind one call.  semi_join and the where-scans compile the policy
into their AUX template argument instead.  With the option at its default a test-sized call runs one arm only (write-through; plain
for running_sum, delta and the runs), and non-temporal, what production runs beyond 768 MiB of output, never.  Results must not
depend on the policy: every unit below runs under 0, 1 and 2 against one image that numpy and the CPU oracle computed once.

UNITS is the table: a unit is a name, its entry point, make(width, n) -> inputs, every expected output, the call, and
expected_policy(option): what the launcher makes of -1, 0, 1 and 2 at the unit's output size, written down per unit.  Inputs stand
in hostile surroundings (support.hostile_pack / hostile_bitmap) and must be unchanged after the call; every output lives in a
support.Expected: the body compared byte for byte, 0xEE guards on both sides, the trailing bits of the last byte zero.  EXEMPT names
the entry points whose launcher reaches the option and that have no unit here, each with the test that covers it.

What ties the option to the kernel: where the policy is a template argument the launch record's label shows it, and the GPU cases
assert it.  For the run-time kernels no GPU observation can (the bytes are the same by contract): there the tie is the source check
below -- every launcher that fills an `nts` field fills it from scan_nt_stores, in the manner of
support.check_sources_read_no_flag_bits -- and the GPU cases show that each arm, once taken, writes the right bytes.

CPU: UNITS + EXEMPT is exactly what reaches the option; every __global__ of a feature directory that takes a store policy belongs to
a unit; the launchers' source; expected_policy against the rules of scan_plan.hpp (through a stand-alone program, as
test_scan_plan.py reaches them) at the unit's bytes and at 768 MiB + 1; no data recipe is vacuous; the carry at a chunk boundary;
the feature headers state the option.
GPU (-m gpu): every unit x width x option; the long tile loop on a 4-wave engine; the AUX label forms; every unit under 1, 2, 0, -1
on one context with no synchronisation in between.
"""
import contextlib
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import support
from support import (BOP, CMP, CSRC, ROOT, SENTINEL, Expected, L, base_name, combine, eng, entry_points_reaching, header_macro, header_text,  # noqa: F401
                     hostile_bitmap, hostile_pack, key_index_expect, label_matches, packbits, payload, pred, prefix_body, random_values, rng_of, top_k_expect,
                     u64s)  # (L, eng: fixtures)

gpu = pytest.mark.gpu

OPTION = "scan_nt_stores"
MIB = 1 << 20
R = 2048                       # rows per tile: 64 lanes x 32 rows
CHUNK = 16384                  # rows per chunk of the chunked kernels
N = 4 * R + 1237               # five tiles: two blocks, a ragged last tile, not a multiple of 8
N_CHUNKED = 5 * CHUNK + 4321   # six chunks: chunk boundaries inside the output
N_LONG = 40 * R + 77           # on a 4-wave engine: ten rounds of the tile loop
POLICIES = (0, 1, 2)
PACKED_WIDTHS = (9, 10, 12, 32)      # a lane's dwords: odd (4-byte stores), 2 mod 4 (8-byte), a multiple of 4, 32 (16-byte)
BITMAP_WIDTHS = (9, 24)              # the store width is the kernel's; a narrow and a wide input
SEARCH_GLOBAL_WIDTHS = (15, 18, 20, 32)  # the same four classes where positions need 15 bits
RUNNING_EXACT_WIDTHS = (17, 18, 20, 32)  # ... and where a count of N_CHUNKED rows must fit
ENDS_WIDTH = {9: 17, 10: 18, 12: 20, 32: 32}  # run_encode's second output: the same class as its first

LOOKUP_LDS_MAX = header_macro("mi355_lookup.h", "MI355_LOOKUP_LDS_MAX_BYTES")
SEARCH_LDS_MAX = header_macro("mi355_search.h", "MI355_SEARCH_LDS_MAX_BYTES")
SEMI_LDS_MAX = header_macro("mi355_semijoin.h", "MI355_SEMIJOIN_LDS_MAX_BITS")
SEARCH_GLOBAL_ROWS = SEARCH_LDS_MAX // 4 + 1


# ---- what a launcher makes of the option, one function per rule; a unit names its own ---------------------------------------------

def by_size(option, out_bytes):
    """one_pass_store_policy: write-through up to 768 MiB of output, non-temporal beyond"""
    return (1 if out_bytes > 768 * MIB else 2) if option < 0 else option


def plain_unless_named(option, out_bytes):
    """running_sum, delta, run_encode, run_decode: -1 is 0"""
    return 0 if option < 0 else option


def no_plain_form(option, out_bytes):
    """semi_join: the kernels exist with AUX 18 and 34 only, 0 runs write-through"""
    return 1 if by_size(option, out_bytes) == 1 else 2


def multi_pass(option, out_bytes):
    """the multi-pass table kernel of the where-scans: non-temporal or plain"""
    return int(out_bytes > 64 * MIB) if option < 0 else int(option != 0)


def never(option, out_bytes):
    """shared_where_chain_kernel has the plain form only"""
    return 0


# rule -> what the answers of tests/cpp/store_policy_eval.cpp (one_pass, multi_pass, in_aux, scan_aux, scan2_aux) say it is
RULES = {
    by_size: lambda option, one_pass, multi, in_aux, scan_aux, scan2_aux: one_pass,
    plain_unless_named: lambda option, *_: max(option, 0),  # (not a rule of scan_plan.hpp: the four launchers spell it, see the source test)
    no_plain_form: lambda option, one_pass, multi, in_aux, scan_aux, scan2_aux: {18: 1, 34: 2}[scan2_aux],  # (scan2's rule, by the launcher's words)
    multi_pass: lambda option, one_pass, multi, *_: multi,
    never: lambda option, *_: 0,
}
AUX_OF = {0: 2, 1: 18, 2: 34}  # scan_aux at the default dma_aux, in_aux


# ---- units ------------------------------------------------------------------------------------------------------------------------

class Unit:
    """make(width, n, key) -> dict: inputs {name: ("pack", values, c) | ("bitmap", bits) | ("scratch", nbytes)}, outs {name: body as
    the call leaves it}, tails {name of a policy-stored output: its valid bits}, policy_bytes (what the launcher hands the rule),
    call(L, ctx, i, o) -> status, more {fact: value}.  `rule(width)` -> one of the rules above; `label(width, policy)` -> the pattern
    of the launch-record label that carries the policy, for the template kernels.  `kernels`: the store-policy kernels the call may
    launch."""

    def __init__(self, name, entry, header, widths, n, make, rule, kernels, label=None):
        self.name, self.entry, self.header, self.widths, self.n, self.make, self.kernels, self.label = name, entry, header, tuple(widths), n, make, set(kernels), label
        self.rule = (lambda width: rule) if rule in RULES else rule  # (a unit whose kernel changes with the width gives width -> rule)

    def __repr__(self):
        return self.name

    @functools.lru_cache(maxsize=None)
    def data(self, width, n=None):
        n = self.n if n is None else n
        return self.make(width, n, (self.name, width, n))

    def expected_policy(self, option, width=None, out_bytes=None):
        width = self.widths[0] if width is None else width
        return self.rule(width)(option, self.data(width)["policy_bytes"] if out_bytes is None else out_bytes)


def dwords(values, c):
    return (values * c + 31) // 32 * 4


def rowid_words(n):
    """the chunk prefix of mi355_compact.h: ceil(n / 16384) + 1 + ceil(n / 16777216) words"""
    chunks = -(-n // CHUNK)
    return chunks + 1 + -(-chunks // 1024)


def make_lookup(c, table_rows):
    def make(w, n, key):
        rng = rng_of(key)
        vals, table, miss = random_values(rng, n, c), random_values(rng, table_rows, w), 5
        out = np.where(vals < table_rows, table[np.minimum(vals, table_rows - 1)], miss).astype(np.uint32)
        return dict(inputs={"col": ("pack", vals, c), "table": ("pack", table, w)}, outs={"out": payload(out, w)}, tails={"out": n * w},
                    policy_bytes=(n * w + 7) // 8, more={"rows beyond the table": int((vals >= table_rows).sum()), "shape": (c, table_rows, w)},
                    call=lambda L, ctx, i, o: L.mi355_lookup_dev(ctx, i["col"], n, c, i["table"], table_rows, w, miss, o["out"]))
    return make


def carries(before, c):
    """the bits of a dword that the rows in front of each inner chunk boundary leave to the chunk behind it"""
    return [int(b) * c % 32 for b in before]


def make_compact(w, n, key):
    rng = rng_of(key)
    vals, bits = random_values(rng, n, w), rng.random(n) < 0.4
    chosen_rows = np.nonzero(bits)[0]
    bits[chosen_rows[len(chosen_rows) - (len(chosen_rows) - 5) % 8:]] = False  # count = 5 mod 8: the last byte has trailing bits at 9, 10 and 12 bits
    chosen = vals[bits]
    m, cap = len(chosen), len(chosen) + 50
    before = np.cumsum(bits)[CHUNK - 1::CHUNK][: (n - 1) // CHUNK]
    return dict(inputs={"col": ("pack", vals, w), "bitmap": ("bitmap", bits)}, outs={"out": prefix_body(dwords(cap, w), payload(chosen, w)), "count": u64s(m)},
                tails={"out": m * w}, policy_bytes=(cap * w + 7) // 8, more={"carries": carries(before, w), "count": m},
                call=lambda L, ctx, i, o: L.mi355_compact_dev(ctx, i["col"], n, w, i["bitmap"], o["out"], cap, o["count"]))


def make_arith(checked):
    def make(w, n, key):
        rng = rng_of(key)
        c, (a, b, k, miss) = (w, (1, -1, 100, 3)) if checked else (w - 1, (1, 1, 0, 0))
        x, y = random_values(rng, n, c), random_values(rng, n, c)
        r = a * x.astype(np.int64) + b * y.astype(np.int64) + k
        ok = (r >= 0) & (r < 1 << w)
        out = np.where(ok, r, miss).astype(np.uint32)
        return dict(inputs={"x": ("pack", x, c), "y": ("pack", y, c)}, outs={"out": payload(out, w), "out_of_range": u64s(int((~ok).sum()))}, tails={"out": n * w},
                    policy_bytes=(n * w + 7) // 8, more={"replaced": int((~ok).sum()), "shape": (0, c, c, a, b, k, w)},
                    call=lambda L, ctx, i, o: L.mi355_arith_dev(ctx, 0, i["x"], c, i["y"], c, n, a, b, k, w, miss, o["out"], o["out_of_range"]))
    return make


def make_top_k(c, n, key):
    rng = rng_of(key)
    vals = (rng.integers(0, 40, n, dtype=np.uint64) * np.uint64(((1 << c) - 1) // 40)).astype(np.uint32)  # the cut goes through ties
    qual = rng.random(n) < 0.5
    k = int(qual.sum()) // 3 + 123
    bits, res = top_k_expect(vals, qual, k, True)
    return dict(inputs={"col": ("pack", vals, c), "mask": ("bitmap", qual)}, outs={"bitmap": packbits(bits), "result": u64s(*res)}, tails={"bitmap": n},
                policy_bytes=(n + 7) // 8, more={"ties kept": res[0] - res[2], "ties dropped": res[3] - (res[0] - res[2])},
                call=lambda L, ctx, i, o: L.mi355_top_k_dev(ctx, i["col"], n, c, i["mask"], k, 1, o["bitmap"], o["result"]))


def make_set_ranks(w, n, key):
    rng = rng_of(key)
    # members all over the set, a tenth of them with a rank beyond w bits (a denser set would leave every row behind the first few miss)
    bits, miss = rng.random(n) < min(0.3, 1.1 * (1 << w) / n), 5
    rank = np.cumsum(bits) - bits
    fits = bits & (rank < (1 << w))
    table = np.where(fits, rank, miss).astype(np.uint32)
    members, unfit = int(bits.sum()), int((bits & ~fits).sum())
    return dict(inputs={"set": ("bitmap", bits)}, outs={"table": payload(table, w), "counts": u64s(members, unfit)}, tails={"table": n * w},
                policy_bytes=(n * w + 7) // 8, more={"members": members},
                call=lambda L, ctx, i, o: L.mi355_set_ranks_dev(ctx, i["set"], n, w, miss, o["table"], o["counts"]))


def make_key_index(w, n, key):
    """n: the rows of the TABLE, which is what key_index_pack_kernel stores by the policy"""
    rng = rng_of(key)
    ck, rows, first_row, miss = (14, 20000, 3, 7) if n <= 1 << 14 else (17, 50000, 3, 7)
    rows = min(rows, (1 << w) + 200)  # all but the last 200 row ids fit w bits: the winners are all over the table, not only in front
    keys, qual = random_values(rng, rows, ck), rng.random(rows) < 0.6
    table, counts = key_index_expect(keys, qual, n, "first", first_row, w, miss)
    return dict(inputs={"keys": ("pack", keys, ck), "mask": ("bitmap", qual)}, outs={"table": payload(table, w), "counts": u64s(*counts)}, tails={"table": n * w},
                policy_bytes=(n * w + 7) // 8, more={"members": counts[0], "outside": counts[1]},
                call=lambda L, ctx, i, o: L.mi355_key_index_dev(ctx, i["keys"], rows, ck, i["mask"], first_row, 0, o["table"], n, w, miss, o["counts"]))


def make_search(c, rows):
    def make(w, n, key):
        rng = rng_of(key)
        table = np.sort(random_values(rng, rows, c))
        table[rows // 2] = table[rows // 2 - 1]
        x = random_values(rng, n, c)
        x[::3] = table[rng.integers(0, rows, len(x[::3]))]
        pos = np.searchsorted(table.astype(np.uint64), x.astype(np.uint64), side="left")
        found, miss = np.isin(x, table), 1
        out = np.where(found, pos, miss).astype(np.uint32)
        return dict(inputs={"col": ("pack", x, c), "table": ("pack", table, c)}, outs={"out": payload(out, w), "found": packbits(found), "hits": u64s(int(found.sum()))},
                    tails={"out": n * w, "found": n}, policy_bytes=(n * w + 7) // 8 + (n + 7) // 8, more={"found": int(found.sum()), "shape": (c, c, w, rows)},
                    call=lambda L, ctx, i, o: L.mi355_search_sorted_dev(ctx, i["col"], n, c, i["table"], c, rows, None, 0, 1, miss, o["out"], w, o["found"], o["hits"]))
    return make


def make_running_sum(checked):
    def make(w, n, key):
        rng = rng_of(key)
        ws = ("scratch", 8 * rowid_words(n))
        if not checked:  # a row's position among the selected rows: c = 1 under a mask, inclusive
            x, mask = (rng.random(n) < 0.5).astype(np.uint32), rng.random(n) < 0.7
            r = np.cumsum(np.where(mask, x, 0).astype(np.int64))
            return dict(inputs={"col": ("pack", x, 1), "mask": ("bitmap", mask), "ws": ws}, outs={"out": payload(r.astype(np.uint32), w), "result": u64s(int(r[-1]), 0)},
                        tails={"out": n * w}, policy_bytes=(n * w + 7) // 8, more={"shape": (1, n, 0, 0, w), "replaced": 0},
                        call=lambda L, ctx, i, o: L.mi355_running_sum_dev(ctx, i["col"], n, 1, i["mask"], 0, 0, 0, w, 0, o["out"], o["result"], i["ws"]))
        # 9-bit deltas around -256 whose sums swing across both ends of the output's range (below zero only at 32 bits), exclusive
        mid, amp = (1 << (w - 1), 1.3 * (1 << (w - 1))) if w <= 12 else (3000, 4000)
        s = np.rint(mid + amp * np.sin(np.arange(-1, n) / 100.0)).astype(np.int64) + np.concatenate([[0], rng.integers(-100, 101, n)])
        b, k, miss = -256, int(s[0]), 1
        x = (np.diff(s) - b).astype(np.uint32)
        t = x.astype(np.int64) + b
        r = k + np.cumsum(t) - t
        ok = (r >= 0) & (r < 1 << w)
        out = np.where(ok, r, miss).astype(np.uint32)
        return dict(inputs={"col": ("pack", x, 9), "ws": ws}, outs={"out": payload(out, w), "result": u64s(k + int(t.sum()), int((~ok).sum()))}, tails={"out": n * w},
                    policy_bytes=(n * w + 7) // 8, more={"shape": (9, n, b, k, w), "replaced": int((~ok).sum()), "kept": int(ok.sum()), "deltas": (int(x.min()), int(x.max()))},
                    call=lambda L, ctx, i, o: L.mi355_running_sum_dev(ctx, i["col"], n, 9, None, b, k, 1, w, miss, o["out"], o["result"], i["ws"]))
    return make


def make_delta(checked):
    def make(w, n, key):
        rng = rng_of(key)
        c, first, k, miss = (9, 100, 0, 2) if checked else (8, 17, 255, 0)
        x = random_values(rng, n, c)
        r = np.diff(x.astype(np.int64), prepend=first) + k
        ok = (r >= 0) & (r < 1 << w)
        out = np.where(ok, r, miss).astype(np.uint32)
        return dict(inputs={"col": ("pack", x, c)}, outs={"out": payload(out, w), "out_of_range": u64s(int((~ok).sum()))}, tails={"out": n * w},
                    policy_bytes=(n * w + 7) // 8, more={"shape": (c, k, w), "replaced": int((~ok).sum())},
                    call=lambda L, ctx, i, o: L.mi355_delta_dev(ctx, i["col"], n, c, first, k, w, miss, o["out"], o["out_of_range"]))
    return make


def make_run_encode(w, n, key):
    rng = rng_of(key)
    ce = ENDS_WIDTH[w]
    ends = np.cumsum(rng.integers(1, 7, n))
    runs = int(np.searchsorted(ends, n)) + 1
    runs -= (runs - 5) % 8  # 5 mod 8 runs: both outputs' last bytes have trailing bits at every width but 32
    ends = ends[:runs].copy()
    ends[-1] = n
    v = random_values(rng, runs, w)
    while (v[1:] == v[:-1]).any():
        v[1:][v[1:] == v[:-1]] ^= 1
    x = np.repeat(v, np.diff(ends, prepend=0))
    # the expectation, from the header's definition: row i is a tail when i == n - 1 or x_i != x_{i+1}
    tails = np.nonzero(np.append(x[1:] != x[:-1], True))[0]
    values, want_ends, r, cap = x[tails], (tails + 1).astype(np.uint32), len(tails), len(tails) + 10
    before = [int((tails < CHUNK * k).sum()) for k in range(1, (n - 1) // CHUNK + 1)]
    return dict(inputs={"col": ("pack", x, w), "ws": ("scratch", 8 * rowid_words(n))},
                outs={"values": prefix_body(dwords(cap, w), payload(values, w)), "ends": prefix_body(dwords(cap, ce), payload(want_ends, ce)), "count": u64s(r)},
                tails={"values": r * w, "ends": r * ce}, policy_bytes=(cap * w + 7) // 8, more={"carries": carries(before, w) + carries(before, ce), "count": r},
                call=lambda L, ctx, i, o: L.mi355_run_encode_dev(ctx, i["col"], n, w, ce, o["values"], o["ends"], cap, o["count"], i["ws"]))


def make_run_decode(w, n, key):
    rng = rng_of(key)
    ce, miss = 17, 6
    ends = np.cumsum(rng.integers(0, 7, n))  # (runs of length zero among them)
    runs = int(np.searchsorted(ends, n - 100))  # the last run ends in front of row n - 100: the rows behind it are uncovered
    ends, values = ends[:runs].astype(np.uint32), random_values(rng, runs, w)
    j = np.searchsorted(ends, np.arange(n), side="right")
    out = np.where(j < runs, values[np.minimum(j, runs - 1)], miss).astype(np.uint32)
    uncovered = int((j == runs).sum())
    return dict(inputs={"values": ("pack", values, w), "ends": ("pack", ends, ce)}, outs={"out": payload(out, w), "uncovered": u64s(uncovered)}, tails={"out": n * w},
                policy_bytes=(n * w + 7) // 8, more={"uncovered": uncovered, "empty runs": int((np.diff(ends) == 0).sum())},
                call=lambda L, ctx, i, o: L.mi355_run_decode_dev(ctx, i["values"], w, i["ends"], ce, runs, None, n, miss, o["out"], o["uncovered"]))


def semi_set_bits(c):
    return 500 if c == 9 else 1 << c


def make_semi_join(c, n, key):
    rng = rng_of(key)
    set_bits, negate = semi_set_bits(c), c == 9
    vals, members = random_values(rng, n, c), rng.random(set_bits) < 0.4
    inside = vals < set_bits
    bits = np.zeros(n, dtype=bool)
    bits[inside] = members[vals[inside]]
    bits = ~bits if negate else bits
    return dict(inputs={"col": ("pack", vals, c), "set": ("bitmap", members)}, outs={"bitmap": packbits(bits), "hits": u64s(int(bits.sum()))}, tails={"bitmap": n},
                policy_bytes=n // 8, more={"hits": int(bits.sum())},
                call=lambda L, ctx, i, o: L.mi355_semijoin_dev(ctx, i["col"], n, c, i["set"], set_bits, 1 if negate else 0, None, o["bitmap"], o["hits"]))


def make_scan_columns(c, n, key):
    rng = rng_of(key)
    c1, c2 = (9, 12) if c == 9 else (c, c)  # column 2 out of LDS; both columns in registers
    v1 = random_values(rng, n, c1)
    v2 = np.clip(v1.astype(np.int64) + rng.integers(-2000, 2001, n), 0, (1 << c2) - 1).astype(np.uint32)
    mask = rng.random(n) < 0.3
    d = v1.astype(np.int64) - v2.astype(np.int64)
    bits = combine((d >= -700) & (d <= 900), mask, "or")
    return dict(inputs={"col1": ("pack", v1, c1), "col2": ("pack", v2, c2), "mask": ("bitmap", mask)}, outs={"bitmap": packbits(bits), "hits": u64s(int(bits.sum()))},
                tails={"bitmap": n}, policy_bytes=n // 8, more={"hits": int(bits.sum())},
                call=lambda L, ctx, i, o: L.mi355_scan_columns_dev(ctx, i["col1"], c1, i["col2"], c2, n, CMP["between"], -700, 900, BOP["or"], i["mask"],
                                                                   o["bitmap"], o["hits"]))


def make_scan_where(c, n, key):
    rng = rng_of(key)
    vals, mask, a = random_values(rng, n, c), rng.random(n) < 0.7, (1 << c) // 3
    bits = pred(vals, "<", a) & mask
    return dict(inputs={"col": ("pack", vals, c), "mask": ("bitmap", mask)}, outs={"bitmap": packbits(bits), "hits": u64s(int(bits.sum()))}, tails={"bitmap": n},
                policy_bytes=n // 8, more={"hits": int(bits.sum())},
                call=lambda L, ctx, i, o: L.mi355_scan_where_dev(ctx, i["col"], n, c, CMP["<"], a, 0, i["mask"], o["bitmap"], o["hits"]))


def make_scan_combine(c, n, key):
    rng = rng_of(key)
    vals, mask, a, b = random_values(rng, n, c), rng.random(n) < 0.5, (1 << c) // 5, (1 << c) // 2
    bits = combine(pred(vals, "not_between", a, b), mask, "xor")
    return dict(inputs={"col": ("pack", vals, c), "mask": ("bitmap", mask)}, outs={"bitmap": packbits(bits), "hits": u64s(int(bits.sum()))}, tails={"bitmap": n},
                policy_bytes=n // 8, more={"hits": int(bits.sum())},
                call=lambda L, ctx, i, o: L.mi355_scan_combine_dev(ctx, i["col"], n, c, CMP["not_between"], a, b, BOP["xor"], i["mask"], o["bitmap"], o["hits"]))


def make_shared_where(P):
    def make(c, n, key):
        import ctypes as C

        from shared_simd_scan_amd.engine import predicates

        rng = rng_of(key)
        vals, ops, preds = random_values(rng, n, c), list(CMP), []
        for k in range(P):
            a, b = sorted(int(x) for x in rng.integers(0, 1 << c, 2))
            a = int(vals[7 * k + 1]) if ops[k % 8] == "==" else a  # (an equality that some row meets)
            preds.append((ops[k % 8], a, b) if ops[k % 8] in ("between", "not_between") else (ops[k % 8], a))
        arr = predicates(preds)
        matches = [pred(vals, *p) for p in preds]
        nb = (n + 7) // 8
        stride = (nb + 15) // 16 * 16 + 16  # a gap behind every bitmap, which stays as it was
        body = np.full((P, stride), SENTINEL, dtype=np.uint8)
        for k, m in enumerate(matches):
            body[k, :nb] = packbits(m)
        return dict(inputs={"col": ("pack", vals, c)}, outs={"out": body.reshape(-1), "hits": u64s(*[int(m.sum()) for m in matches])}, tails={"out": n},
                    policy_bytes=n // 8 * P, more={"hits": min(int(m.sum()) for m in matches), "preds": arr},
                    call=lambda L, ctx, i, o: L.mi355_shared_scan_where_dev(ctx, i["col"], n, c, C.cast(arr, C.c_void_p), P, 0, o["out"], stride, o["hits"]))
    return make


def semi_label(c, policy):
    return f"{'semijoin_lds_kernel' if c == 9 else 'semijoin_global_kernel'}<{c}, {AUX_OF[policy]}>"


def burst_label(c, policy):
    return f"scan_burst_kernel<{c}, 1, {AUX_OF[policy]}, *, *>"


def where_label(multi):
    def label(c, policy):
        return f"shared_where_lut_kernel<{c}, {AUX_OF[policy]}, 64, 0, {'true' if multi else 'false'}>" if c <= 12 else f"shared_where_chain_kernel<{c}, 2, 64>"
    return label


WHERE_KERNELS = ["shared_where_lut_kernel", "shared_where_chain_kernel"]
UNITS = [
    Unit("lookup, LDS tier", "mi355_lookup_dev", "mi355_lookup.h", PACKED_WIDTHS, N, make_lookup(12, 4000), by_size, ["lookup_lds_kernel"]),
    Unit("lookup, global tier", "mi355_lookup_dev", "mi355_lookup.h", PACKED_WIDTHS, N, make_lookup(17, 100_003), by_size, ["lookup_global_kernel"]),
    Unit("compact", "mi355_compact_dev", "mi355_compact.h", PACKED_WIDTHS, N_CHUNKED, make_compact, by_size, ["compact_kernel", "compact_edges_kernel"]),
    Unit("arith, exact", "mi355_arith_dev", "mi355_arith.h", PACKED_WIDTHS, N, make_arith(False), by_size, ["arith_exact_kernel"]),
    Unit("arith, checked", "mi355_arith_dev", "mi355_arith.h", PACKED_WIDTHS, N, make_arith(True), by_size, ["arith_checked_kernel"]),
    Unit("top_k", "mi355_top_k_dev", "mi355_topk.h", BITMAP_WIDTHS, N_CHUNKED, make_top_k, by_size, ["topk_hist_kernel", "topk_emit_kernel", "topk_trim_kernel"]),
    Unit("set_ranks", "mi355_set_ranks_dev", "mi355_distinct.h", PACKED_WIDTHS, N_CHUNKED, make_set_ranks, by_size, ["set_ranks_kernel"]),
    Unit("key_index", "mi355_key_index_dev", "mi355_keyindex.h", PACKED_WIDTHS, N, make_key_index, by_size, ["key_index_pack_kernel"]),
    Unit("search_sorted, LDS tier", "mi355_search_sorted_dev", "mi355_search.h", PACKED_WIDTHS, N, make_search(12, 300), by_size, ["search_lds_kernel"]),
    Unit("search_sorted, global tier", "mi355_search_sorted_dev", "mi355_search.h", SEARCH_GLOBAL_WIDTHS, N, make_search(24, SEARCH_GLOBAL_ROWS), by_size,
         ["search_global_kernel"]),
    Unit("running_sum, exact", "mi355_running_sum_dev", "mi355_running.h", RUNNING_EXACT_WIDTHS, N_CHUNKED, make_running_sum(False), plain_unless_named,
         ["running_sum_totals_kernel", "running_sum_exact_kernel"]),
    Unit("running_sum, checked", "mi355_running_sum_dev", "mi355_running.h", PACKED_WIDTHS, N_CHUNKED, make_running_sum(True), plain_unless_named,
         ["running_sum_totals_kernel", "running_sum_checked_kernel"]),
    Unit("delta, exact", "mi355_delta_dev", "mi355_running.h", PACKED_WIDTHS, N, make_delta(False), plain_unless_named, ["delta_exact_kernel"]),
    Unit("delta, checked", "mi355_delta_dev", "mi355_running.h", PACKED_WIDTHS, N, make_delta(True), plain_unless_named, ["delta_checked_kernel"]),
    Unit("run_encode", "mi355_run_encode_dev", "mi355_runs.h", PACKED_WIDTHS, N_CHUNKED, make_run_encode, plain_unless_named,
         ["run_count_kernel", "run_emit_kernel", "compact_edges_kernel"]),
    Unit("run_decode", "mi355_run_decode_dev", "mi355_runs.h", PACKED_WIDTHS, N, make_run_decode, plain_unless_named, ["run_decode_kernel"]),
    # semijoin and scan2 have no plain form: 0 becomes write-through; 9 bits: the LDS tier, 24 bits: the global one
    Unit("semi_join", "mi355_semijoin_dev", "mi355_semijoin.h", BITMAP_WIDTHS, N, make_semi_join, no_plain_form, ["semijoin_lds_kernel", "semijoin_global_kernel"],
         label=semi_label),
    Unit("scan_columns", "mi355_scan_columns_dev", "mi355_columns.h", BITMAP_WIDTHS, N, make_scan_columns, by_size, ["scan_columns_kernel"]),
    Unit("scan_where", "mi355_scan_where_dev", "mi355_scan.h", BITMAP_WIDTHS, N, make_scan_where, by_size, [], label=burst_label),
    Unit("scan_combine", "mi355_scan_combine_dev", "mi355_scan.h", BITMAP_WIDTHS, N, make_scan_combine, by_size, [], label=burst_label),
    # 9 bits: the table kernels; 24 bits: no table fits, the chain kernel, which has the plain form only
    Unit("shared_scan_where, one pass", "mi355_shared_scan_where_dev", "mi355_scan.h", BITMAP_WIDTHS, N, make_shared_where(5),
         lambda c: by_size if c <= 16 else never, WHERE_KERNELS, label=where_label(False)),
    Unit("shared_scan_where, multi-pass", "mi355_shared_scan_where_dev", "mi355_scan.h", BITMAP_WIDTHS, N, make_shared_where(12),
         lambda c: multi_pass if c <= 12 else never, WHERE_KERNELS, label=where_label(True)),
]
CASES = [(u, w) for u in UNITS for w in u.widths]

# entry points whose launcher reaches the option and that have no unit here: each is "covered by <test id>"
EXEMPT = {
    "mi355_scan_eq_dev": "covered by tests/test_gpu_parity.py::test_store_policy_variants_agree",
    "mi355_scan_range_dev": "covered by tests/test_gpu_parity.py::test_store_policy_variants_agree",
    "mi355_shared_scan_eq_dev": "covered by tests/test_gpu_parity.py::test_store_policy_variants_agree",
    "mi355_scan_in_dev": "covered by tests/test_kernel_paths.py::test_kernel_path",   # scan_in_nt, scan_in_plain
    "mi355_scan2_dev": "covered by tests/test_kernel_paths.py::test_kernel_path",     # scan2_nt (no plain form)
    # their scan is mi355_scan_eq_dev / mi355_scan_range_dev
    "mi355_sharded_scan_eq_dev": "covered by tests/test_gpu_parity.py::test_store_policy_variants_agree",
    "mi355_sharded_scan_range_dev": "covered by tests/test_gpu_parity.py::test_store_policy_variants_agree",
    # launches mi355_scan_eq_dev, mi355_scan_combine_dev (a unit here) and mi355_decompress_dev
    "mi355_tune_dev": "covered by tests/test_gpu_parity.py::test_store_policy_variants_agree",
    # through the width groups' launch(), which copies the option into every request; plan_decompress and plan_select read no store policy
    # (checked below), and the rules' program asserts what they do read
    "mi355_decompress_dev": "covered by tests/test_scan_plan.py::test_rules_value_by_value",
    "mi355_scan_select_dev": "covered by tests/test_scan_plan.py::test_rules_value_by_value",
}


def pid(p):
    return str(p)


def sizes_of(unit):
    return (unit.n, N_LONG)


# ------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------

def test_unit_names_unique():
    assert len({u.name for u in UNITS}) == len(UNITS)


def test_units_and_exemptions_are_exactly_what_reaches_the_option():
    """derived from csrc/**/*.hip: a future entry point whose launcher reads the option fails here until a unit or an exemption names it"""
    reaching = entry_points_reaching(OPTION)
    assert len(reaching) >= 26, reaching  # the parse found the launchers
    named = {u.entry for u in UNITS}
    assert not named & set(EXEMPT)
    assert sorted(named | set(EXEMPT)) == reaching, (sorted(set(reaching) - named - set(EXEMPT)), sorted((named | set(EXEMPT)) - set(reaching)))
    assert named >= {"mi355_lookup_dev", "mi355_compact_dev", "mi355_arith_dev", "mi355_top_k_dev", "mi355_set_ranks_dev", "mi355_key_index_dev", "mi355_search_sorted_dev",
                     "mi355_running_sum_dev", "mi355_delta_dev", "mi355_run_encode_dev", "mi355_run_decode_dev", "mi355_semijoin_dev", "mi355_scan_columns_dev",
                     "mi355_scan_where_dev", "mi355_shared_scan_where_dev", "mi355_scan_combine_dev"}


def test_exemptions_name_tests_that_exist():
    for entry, reason in EXEMPT.items():
        m = re.fullmatch(r"covered by (tests/\w+\.py)::(\w+)", reason)
        assert m, (entry, reason)
        assert re.search(rf"^def {m.group(2)}\(", open(os.path.join(ROOT, m.group(1))).read(), flags=re.M), reason
    parity = open(os.path.join(ROOT, "tests", "test_gpu_parity.py")).read()
    assert re.search(r'parametrize\("nts", \[0, 1, 2\]\)\n[^\n]*\ndef test_store_policy_variants_agree', parity)
    import kernel_cases

    ids = {c.id for c in kernel_cases.CASES if dict(c.opts).get(OPTION) is not None}
    assert {"scan_in_nt", "scan_in_plain", "scan2_nt"} <= ids
    # the two plans that the width groups' launch() reaches without a store policy
    plan = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "scan_plan.hpp")).read())
    for name in ("plan_decompress", "plan_select"):
        body = re.search(rf"inline ScanPlan {name}\([^)]*\)\n\{{\n(.*?)\n\}}", plan, flags=re.S).group(1)
        assert OPTION not in body and "store_policy" not in body, name


def test_every_store_policy_kernel_belongs_to_a_unit():
    """every __global__ of a feature directory that takes a struct with an `nts` field, or an AUX store policy"""
    derived = {k for feature in support.feature_directories() for k in support.store_policy_kernels(feature)}
    assert {"lookup_lds_kernel", "compact_kernel", "run_emit_kernel", "semijoin_global_kernel", "shared_where_lut_kernel", "scan_columns_kernel",
            "key_index_pack_kernel", "topk_emit_kernel"} <= derived, derived  # the parse found them
    named = {k for u in UNITS for k in u.kernels}
    assert derived == named, (sorted(derived - named), sorted(named - derived))
    # ... and a unit's kernels live where its entry point does, or in what that directory's launcher includes from compact/
    home = {name: os.path.dirname(path) for name, path, _ in support.hip_functions()}
    for u in UNITS:
        where = {"": "predicates"}.get(home[u.entry], home[u.entry])  # (capi.hip launches the kernels of predicates/)
        mine = support.store_policy_kernels(where) | ({"compact_edges_kernel"} if where == "runs" else set())
        assert u.kernels <= mine, (u.name, sorted(u.kernels - mine))


def test_launchers_fill_the_policy_from_the_option():
    """results are policy-independent by contract, so for the run-time kernels this source text, and no GPU observation, ties the
    option to the kernel: every `.nts = ...` of a launcher reads scan_nt_stores, the launchers of the AUX kernels hand it to the rules
    of scan_plan.hpp, and what `-1` becomes is either those rules' answer or, spelled out, plain"""
    filled = support.assignments_to("nts")
    assert len(filled) >= 12, filled
    for name, path, rhs in filled:
        assert OPTION in rhs, (name, path, rhs)
        by_rule = re.fullmatch(r"\(uint32_t\)one_pass_store_policy\(.*, ctx->scan_nt_stores\)", rhs)
        spelled = rhs == "ctx->scan_nt_stores < 0 ? 0u : (uint32_t)ctx->scan_nt_stores"
        assert by_rule or spelled, (name, path, rhs)
        units = [u for u in UNITS if u.entry == name or (name == "launch_columns" and u.entry == "mi355_scan_columns_dev")]
        assert units, (name, "fills a policy word and is no unit's entry point")
        assert {u.rule(u.widths[0]) for u in units} == {plain_unless_named if spelled else by_size}, name
    filling = {name for name, _, _ in filled}
    assert {u.entry for u in UNITS if u.rule(u.widths[0]) is plain_unless_named} <= filling
    # every call of a rule, wherever it stands, passes the option
    calls = 0
    for folder, _, files in os.walk(CSRC):
        for f in files:
            if f.endswith((".hip", ".hpp")) and f != "scan_plan.hpp":
                text = re.sub(r"//[^\n]*", "", open(os.path.join(folder, f)).read())
                for m in re.finditer(r"\b(?:one_pass_store_policy|multi_pass_nt_stores)\(((?:[^()]|\((?:[^()]|\([^()]*\))*\))*)\)", text):
                    calls += 1
                    assert re.search(r"\bscan_nt_stores$", m.group(1).strip()), (f, m.group(0))
    assert calls >= 14, calls
    # the template kernels: the rule's answer becomes the AUX, in the words expected_label uses
    semi = open(os.path.join(CSRC, "semijoin", "semijoin.hip")).read()
    assert "const bool nt = r.store_policy == 1;" in semi and semi.count("nt ? launch_tier<semijoin_") == 2 and "r.store_policy = one_pass_store_policy(n / 8, ctx->scan_nt_stores);" in semi
    where = open(os.path.join(CSRC, "predicates", "where_group.hip")).read()
    assert "in_aux(one_pass_store_policy(out_bytes, r.l.scan_nt_stores))" in where and "multi_pass_nt_stores(out_bytes, r.l.scan_nt_stores)) ? 18 : 2" in where
    assert "return WherePlan{kWhereChain, 2," in where
    assert "l.scan_nt_stores = ctx->scan_nt_stores;" in open(os.path.join(CSRC, "capi.hip")).read()


EVAL_SRC = os.path.join(ROOT, "tests", "cpp", "store_policy_eval.cpp")
EVAL_BIN = os.path.join(ROOT, "tests", "cpp", "build", "store_policy_eval")


def rules_say(rows):
    """[(out_bytes, option)] -> what scan_plan.hpp's rules answer, through a stand-alone program (test_scan_plan.py's way)"""
    header = os.path.join(CSRC, "scan_plan.hpp")
    if not os.path.exists(EVAL_BIN) or os.path.getmtime(EVAL_BIN) < max(os.path.getmtime(EVAL_SRC), os.path.getmtime(header)):
        os.makedirs(os.path.dirname(EVAL_BIN), exist_ok=True)
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, EVAL_SRC, "-o", EVAL_BIN], check=True)
    res = subprocess.run([EVAL_BIN], input="".join(f"{b} {o}\n" for b, o in rows), capture_output=True, text=True, timeout=60, check=True)
    got = [tuple(int(x) for x in ln.split()) for ln in res.stdout.splitlines()]
    assert len(got) == len(rows)
    return got


def test_expected_policy_follows_the_rules():
    rows = [(u, w, b, o) for u, w in CASES for b in (u.data(w)["policy_bytes"], 768 * MIB + 1) for o in (-1, 0, 1, 2)]
    for (u, w, b, o), answers in zip(rows, rules_say([(b, o) for _, _, b, o in rows])):
        own = u.data(w)["policy_bytes"]
        want = RULES[u.rule(w)](o, *answers)
        assert u.expected_policy(o, w, None if b == own else b) == want, (u.name, w, b, o, answers)
        assert u.expected_policy(o, w, b) in POLICIES
        assert AUX_OF[by_size(o, b)] == answers[2] == answers[3]  # in_aux; scan_aux at the default dma_aux
    for u, w in CASES:
        assert 0 < u.data(w)["policy_bytes"] < 64 * MIB
        # at test size: what the issue states
        assert [u.expected_policy(o, w) for o in (-1, 0, 1, 2)] == {by_size: [2, 0, 1, 2], plain_unless_named: [0, 0, 1, 2], no_plain_form: [2, 2, 1, 2],
                                                                    multi_pass: [0, 0, 1, 1], never: [0, 0, 0, 0]}[u.rule(w)], u.name
        if u.rule(w) in (by_size, no_plain_form, multi_pass):
            assert u.expected_policy(-1, w, 768 * MIB + 1) == 1  # what production runs beyond the Infinity Cache
    assert {u.rule(w) for u, w in CASES} == set(RULES)


def test_shapes_are_the_ones_at_which_the_arms_differ():
    assert N == 9429 and N // R == 4 and N % R and N % 8 and N_CHUNKED // CHUNK == 5 and N_CHUNKED % CHUNK and N_CHUNKED % 8 and N_LONG // R == 40 and N_LONG % 8
    chunked = {"compact", "run_encode", "running_sum, exact", "running_sum, checked", "set_ranks", "top_k"}
    bitmaps = {"top_k", "semi_join", "scan_columns", "scan_where", "scan_combine", "shared_scan_where, one pass", "shared_scan_where, multi-pass"}
    for u in UNITS:
        assert u.n == (N_CHUNKED if u.name in chunked else N), u.name
        packed_out = any(bits > u.n for bits in u.data(u.widths[0])["tails"].values())  # (a bitmap has a bit per row)
        assert packed_out == (u.name not in bitmaps), u.name
        if packed_out:  # odd, 2 mod 4, a multiple of 4, 32
            assert len(u.widths) == 4 and u.widths[0] % 2 == 1 and u.widths[1] % 4 == 2 and u.widths[2] % 4 == 0 and u.widths[2] < u.widths[3] == 32, (u.name, u.widths)
        else:
            assert u.widths == BITMAP_WIDTHS
    assert all(ce % 4 == w % 4 and (1 << ce) - 1 >= N_CHUNKED for w, ce in ENDS_WIDTH.items())
    assert all((1 << w) - 1 >= SEARCH_GLOBAL_ROWS for w in SEARCH_GLOBAL_WIDTHS) and all((1 << w) - 1 >= N_CHUNKED for w in RUNNING_EXACT_WIDTHS)


def test_tiered_units_sit_in_the_tiers_they_name(L):
    """(pure arithmetic of the library: no device)"""
    for u, w, n in [(u, w, n) for u, w in CASES for n in sizes_of(u)]:
        more = u.data(w, n)["more"]
        if u.entry == "mi355_lookup_dev":
            assert {L.mi355_lookup_kernel(*more["shape"]).decode()} == u.kernels, (u.name, w)
        if u.entry == "mi355_search_sorted_dev":
            assert {L.mi355_search_sorted_kernel(*more["shape"]).decode()} == u.kernels, (u.name, w)
        if u.entry == "mi355_arith_dev":
            assert {L.mi355_arith_kernel(*more["shape"]).decode()} == u.kernels, (u.name, w)
        if u.entry == "mi355_running_sum_dev":
            assert L.mi355_running_sum_kernel(*more["shape"]).decode() in u.kernels and L.mi355_running_sum_workspace_words(n) == rowid_words(n), (u.name, w)
        if u.entry == "mi355_delta_dev":
            assert {L.mi355_delta_kernel(*more["shape"]).decode()} == u.kernels, (u.name, w)
        if u.entry == "mi355_run_encode_dev":
            assert L.mi355_run_encode_workspace_words(n) == rowid_words(n)
        if u.entry == "mi355_semijoin_dev":
            assert L.mi355_semijoin_kernel(w, semi_set_bits(w)).decode() == base_name(u.label(w, 1)), w
    assert semi_set_bits(9) <= SEMI_LDS_MAX < semi_set_bits(24) and 4 * 4001 <= LOOKUP_LDS_MAX < 2 * 100_004 and 4 * 300 <= SEARCH_LDS_MAX < 4 * SEARCH_GLOBAL_ROWS


@pytest.mark.parametrize("unit,width", CASES, ids=pid)
def test_no_data_recipe_is_vacuous(unit, width):
    """per unit, width and size: every policy-stored output differs from all-zero and from all-0xEE, its last byte has trailing bits
    for the call to zero (no width but 32 is without), and the rows that take the other branch of the kernel exist"""
    for n in sizes_of(unit):
        host = unit.data(width, n)
        assert host["tails"] and set(host["tails"]) <= set(host["outs"])
        for name, bits in host["tails"].items():
            body = host["outs"][name]
            written = body[: (bits + 7) // 8] if name != "out" or unit.entry != "mi355_shared_scan_where_dev" else body
            assert len(written) > 4 * R // 8 and (written != 0).any() and (written != SENTINEL).any(), (unit.name, name)
            counts = np.bincount(written, minlength=256)
            assert counts.max() < 0.9 * len(written), (unit.name, name, "one byte value nearly everywhere")
            if unit.entry == "mi355_shared_scan_where_dev":
                continue  # (P bitmaps with gaps: the last byte of each is the row count's, below)
            if bits % 8:
                assert int(written[-1]) >> (bits % 8) == 0
            else:
                assert width == 32 or ENDS_WIDTH.get(width) == 32 and name == "ends", (unit.name, name, "no trailing bits to check")
        assert n % 8, "a bitmap's last byte has trailing bits"
        more = host["more"]
        for fact in ("rows beyond the table", "ties kept", "ties dropped", "members", "outside", "found", "uncovered", "empty runs", "hits", "count", "kept"):
            assert more.get(fact, 1) > 0, (unit.name, width, n, fact)
        if "replaced" in more:
            assert (more["replaced"] > 0) == ("checked" in unit.name), (unit.name, width, n, more["replaced"])
        if "deltas" in more:
            assert 0 <= more["deltas"][0] and more["deltas"][1] < 512
        for name, body in host["outs"].items():
            if name not in host["tails"] and not (len(body) == 8 and "exact" in unit.name):  # (an exact kernel's counter stays 0)
                assert (body != 0).any(), (unit.name, name)


@pytest.mark.parametrize("unit", [u for u in UNITS if u.name in ("compact", "run_encode")], ids=pid)
def test_a_carry_crosses_a_chunk_boundary(unit):
    """the rows in front of a chunk boundary end inside a dword, so the chunk behind it starts with an atomic OR into a dword that the
    policy stores of the chunk in front also reach; at 32 bits no value can"""
    for n in sizes_of(unit):
        for w in unit.widths:
            got = unit.data(w, n)["more"]["carries"]
            assert len(got) == (n - 1) // CHUNK * (2 if unit.name == "run_encode" else 1) and len(got) >= 4
            if w == 32:
                assert not any(got)
            else:
                assert sum(1 for x in got if x) >= len(got) // 2, (unit.name, w, n, got)


def test_headers_state_the_option():
    """one line per feature header whose launcher reads the option: that it governs the call's result stores, and what -1 and 0 mean there"""
    words = {by_size: r"-1 \(the default\) write-through up to 768 MiB of [\w ]+, non-temporal beyond; 0 plain",
             plain_unless_named: r"-1 \(the default\) and 0 plain",
             no_plain_form: r"-1 \(the default\) write-through up to 768 MiB of [\w ]+, non-temporal beyond; 0 write-through too"}
    for u in UNITS:
        if u.header == "mi355_scan.h":
            continue  # (documents the option itself, and that it governs the shared scans' stores)
        text = " ".join(re.sub(r"^\s*/?\*+/?", "", ln).strip() for ln in header_text(u.header).split("\n"))
        lines = re.findall(r'stores\s+option "scan_nt_stores" \(mi355_scan\.h\) governs ([^:]+): ([^.]+)\.\s+1 non-temporal, 2 write-through\.', text)
        mine = [rest for what, rest in lines if re.search(words[u.rule(u.widths[0])], rest)]
        assert mine, (u.name, u.header, lines)
        assert len(lines) == len({x.entry for x in UNITS if x.header == u.header}), (u.header, "one line per entry point")
    scan = header_text("mi355_scan.h")
    assert '"scan_nt_stores" (result stores of the scans: -1 chosen by output size' in scan and '"scan_nt_stores" also governs these result stores' in scan
    # a header that says so has a unit
    for header in sorted(os.listdir(support.INCLUDE)):
        if header.endswith(".h") and header != "mi355_scan.h" and OPTION in header_text(header):
            assert header in {u.header for u in UNITS}, header


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------

ALL_POLICY_KERNELS = {k for u in UNITS for k in u.kernels}


class Placed:
    """a unit's inputs on the device, in hostile surroundings, with a copy to hold them against, and its guarded outputs"""

    def __init__(self, unit, width, n):
        import torch

        self.unit, self.width, self.n, self.host = unit, width, n, unit.data(width, n)
        O = support.oracle()
        self.inputs, self.keep = {}, []
        for name, spec in self.host["inputs"].items():
            if spec[0] == "pack":
                self.inputs[name] = hostile_pack(O, spec[1], spec[2])
            elif spec[0] == "bitmap":
                self.inputs[name], whole = hostile_bitmap(spec[1])
                self.keep.append(whole)
            else:
                self.inputs[name] = torch.full((spec[1],), SENTINEL, dtype=torch.uint8, device="cuda")  # a workspace: it may hold anything
        self.before = {name: t.clone() for name, t in self.inputs.items() if self.host["inputs"][name][0] != "scratch"}
        self.outs = {name: Expected(body) for name, body in self.host["outs"].items()}
        self.reset()

    def reset(self):
        for o in self.outs.values():
            o.reset()

    def launch(self, L, eng):
        """enqueues the call -> the labels of its launch record"""
        i = {name: t.data_ptr() for name, t in self.inputs.items()}
        o = {name: e.ptr for name, e in self.outs.items()}
        rc = self.host["call"](L, eng._ctx, i, o)
        assert rc == 0, (self.unit.name, self.width, L.mi355_last_error())
        return [label for label, _, _, _ in support.record(L, eng)]

    def check(self, what):
        import torch

        for name, o in self.outs.items():
            o.check((self.unit.name, self.width, self.n, name, what))
        for name, t in self.before.items():
            assert torch.equal(self.inputs[name], t), (self.unit.name, self.width, name, what, "an input was written")


@functools.lru_cache(maxsize=None)
def placed(unit, width, n, copy=0):
    return Placed(unit, width, n)


@contextlib.contextmanager
def store_policy(eng, option):
    eng.set_option(OPTION, option)
    try:
        yield
    finally:
        eng.set_option(OPTION, -1)


def check_labels(unit, width, option, n, labels):
    """the call launched kernels of the unit and of no other; where the policy is a template argument, the label carries the AUX that
    expected_policy names"""
    mine = [lb for lb in labels if base_name(lb) in ALL_POLICY_KERNELS]
    assert {base_name(lb) for lb in mine} <= unit.kernels and (mine or not unit.kernels), (unit.name, labels)
    if unit.label is None:
        return None
    want = unit.label(width, unit.expected_policy(option, width, unit.data(width, n)["policy_bytes"]))
    assert [lb for lb in labels if label_matches(want, lb)], (unit.name, width, option, "expected", want, "recorded", labels)
    return want


def run_case(L, eng, unit, width, n, option):
    p = placed(unit, width, n)
    with store_policy(eng, option):
        p.reset()
        labels = p.launch(L, eng)
        eng.synchronize()
    p.check(f"under {OPTION} = {option}")
    return check_labels(unit, width, option, n, labels)


@gpu
@pytest.mark.parametrize("option", POLICIES)
@pytest.mark.parametrize("unit,width", CASES, ids=pid)
def test_every_store_policy(L, eng, unit, width, option):
    run_case(L, eng, unit, width, unit.n, option)


@pytest.fixture(scope="module")
def four_waves():
    """one block of four waves, as support.Runtime's capped engine: the stores sit inside the software-pipelined tile loop"""
    from shared_simd_scan_amd import ScanEngine

    e = ScanEngine(0)
    e.set_option("grid_cus", 1)
    e.set_option("max_blocks_per_cu", 1)
    yield e
    e.close()


@gpu
@pytest.mark.parametrize("unit", UNITS, ids=pid)
def test_long_tile_loop(L, four_waves, unit):
    for option in POLICIES:
        run_case(L, four_waves, unit, unit.widths[0], N_LONG, option)


TEMPLATE_UNITS = [u for u in UNITS if u.label is not None]


def label_forms():
    """every label the template units can carry: per unit and width, the AUX of each policy its rule can answer"""
    return {u.label(w, u.expected_policy(o, w)) for u in TEMPLATE_UNITS for w in u.widths for o in POLICIES}


def test_label_forms_are_the_issue_s():
    forms = label_forms()
    assert {"semijoin_lds_kernel<9, 18>", "semijoin_lds_kernel<9, 34>", "semijoin_global_kernel<24, 18>", "semijoin_global_kernel<24, 34>",
            "shared_where_lut_kernel<9, 2, 64, 0, false>", "shared_where_lut_kernel<9, 18, 64, 0, false>", "shared_where_lut_kernel<9, 34, 64, 0, false>",
            "shared_where_lut_kernel<9, 2, 64, 0, true>", "shared_where_lut_kernel<9, 18, 64, 0, true>", "shared_where_chain_kernel<24, 2, 64>",
            "scan_burst_kernel<9, 1, 2, *, *>", "scan_burst_kernel<9, 1, 18, *, *>", "scan_burst_kernel<24, 1, 34, *, *>"} <= forms
    assert not [f for f in forms if f.startswith("semijoin") and f.endswith(", 2>")] and len(forms) == 16, sorted(forms)


@gpu
def test_every_label_form_is_launched(L, eng):
    """each AUX form of the template kernels, launched and checked here (the cases above launch them too; this test stands alone)"""
    seen = set()
    for u in TEMPLATE_UNITS:
        for w in u.widths:
            for option in POLICIES:
                seen.add(run_case(L, eng, u, w, u.n, option))
    assert seen == label_forms(), (sorted(label_forms() - seen), sorted(seen - label_forms()))


@gpu
def test_the_policy_is_read_at_every_launch(L):
    """every unit under 1, then 2, then 0, then -1 on one context, no synchronisation between the launches, every output checked at
    the end: a launcher that kept the first policy it saw would show in the labels, one whose arms interfere in a byte"""
    import torch

    from shared_simd_scan_amd import ScanEngine

    order = (1, 2, 0, -1)
    runs = [(option, u, placed(u, u.widths[0], u.n, copy=option)) for option in order for u in UNITS]
    for _, _, p in runs:
        p.reset()
    torch.cuda.synchronize()
    e = ScanEngine(0)
    try:
        labels = []
        try:
            for option, u, p in runs:
                e.set_option(OPTION, option)
                labels.append(p.launch(L, e))
        finally:
            e.set_option(OPTION, -1)
        e.synchronize()
        for (option, u, p), got in zip(runs, labels):
            p.check(f"under {OPTION} = {option}, behind {order[: order.index(option)]}")
            check_labels(u, u.widths[0], option, u.n, got)
    finally:
        e.close()
