"""Every entry point behind every other on one context.  A context owns two pieces of device state that outlive a call and that
all its entry points share: kernel_scratch (hit-count replicas and tickets, "all zero between launches") and rowid_ws, the
grow-only selection workspace.  A feature's own test file gets a context only that feature has touched, and fresh device memory is
usually zero; here every user of either state runs behind the others, and behind calls that leave the workspace full of garbage.
DESIGN.md ("Who writes the words a call reads") is the audit these tests confirm.

UNITS is the table: a unit is a name, the state it uses, the entry points it calls, its inputs and expected outputs (numpy and the
CPU oracle only, computed once), launch(eng) (enqueues only) and check().  Every output lives in a Guarded buffer full of SENTINEL
and is compared byte for byte, guards included (support.Expected).

CPU: every exported mi355_*_dev whose launcher reaches rowid_ws_get or kernel_scratch is named by a unit; every expected count is
non-zero, no two scratch units expect the same counts, the top-k units cut through ties; the dirtiers' footprint in the workspace
covers every unit's.
GPU (-m gpu): workspace units behind a dirtier on a fresh context; every ordered pair of units of one state with no host
synchronisation in between (the scratch matrix also on a one-block grid), a refused call in the middle; a stream switch with
queued workspace work; graph replays between eager calls of other features.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import capture
from kernel_cases import CASES, WHERE_CHAIN, WHERE_COUNT_CASES, WHERE_LUT, WHERE_LUT_MULTI, column
from support import (BOP, CMP, E_INVALID, SENTINEL, Expected, Guarded, L, base_name, combine, eng, entry_points_reaching, header_macro,  # noqa: F401
                     header_text, key_index_expect, packbits, packed, parse_record, payload, pred, prefix_body, random_values, rng_of, top_k_expect,
                     u64s)

gpu = pytest.mark.gpu

N_WS = 5 * 16384 + 4321        # six chunks of 16384 rows with a ragged end
N_WS_BIG = 1025 * 16384 + 77   # two scan groups of 1024 chunks
N_WS_TWIN = 9 * 16384 + 123    # the larger input a unit runs on in front of itself
N_SCRATCH = 40 * 8192 + 4321   # more than one replica, more than one ticket group on the default grid
N_SCRATCH_TWIN = 57 * 8192 + 99
CHUNK = 16384
SCAN_GROUP = 1024

# entry points whose launcher reaches the state without being a unit, each with the reason
EXEMPT = {
    "mi355_decompress_dev": "goes through the width groups' launch(), which fills the scratch pointer of every request; decompress_kernel takes DecompArgs, "
                            "which has no such field",
    "mi355_tune_dev": "returns in front of its first launch below 5e7 rows; its launches are mi355_scan_eq_dev, mi355_scan_combine_dev and "
                      "mi355_decompress_dev",
    "mi355_sharded_scan_eq_dev": "needs a communicator; its scan is mi355_scan_eq_dev (test_exchange_loopback runs it)",
    "mi355_sharded_scan_range_dev": "needs a communicator; its scan is mi355_scan_range_dev (test_exchange_loopback runs it)",
}


# ---- the workspace's footprint per call, in 64-bit words, as the headers document it ----------------------------------------

def prefix_words(nchunks):
    """mi355_compact.h: ceil(n / 16384) + 1 + ceil(n / 16777216) for nchunks = ceil(n / 16384)"""
    return nchunks + 1 + -(-nchunks // SCAN_GROUP)


def rowid_words(n):
    return prefix_words(-(-n // CHUNK))


def top_k_words(n, c):
    """mi355_topk.h"""
    return rowid_words(n) + 8 + 4096 * -(-c // 12)


def sort_rows_words(n, capacity, c):
    """mi355_sort.h: the counters of the widest pass with their prefix, 8 words of state, min(passes - 1, 2) item buffers"""
    passes = -(-c // 8)
    return prefix_words(min(1 << c, 256) * -(-n // CHUNK)) + 8 + min(passes - 1, 2) * min(capacity, n)


def key_index_words(n, ck, table_rows):
    """mi355_keyindex.h: ceil(reach / 2), reach = min(table_rows, 2^ck), nothing without rows"""
    return -(-min(table_rows, 1 << ck) // 2) if n else 0


def select_words(n, c):
    """kernels/select.hpp select_state_words: a state word per chunk of select_tiles(c) tiles, rounded up to 16, and two lines"""
    tile = 64 * (128 if c <= 16 else 64)
    nchunks = -(-(-(-n // tile)) // (16 if c > 16 else (4 if c >= 14 else 8)))
    return -(-nchunks // 16) * 16 + 32


# ---- units ------------------------------------------------------------------------------------------------------------------

class Unit:
    """`make(n, seed)` -> dict: inputs {name: numpy array}, outs {name: body as the call leaves it}, counts [every count the call
    reports], call(L, ctx, i, o) -> status (i, o: pointers by name), words (workspace), and optionally kernel (the base name of the
    call's first launch), more {fact: value} for the data tests.  Inputs and expectations are computed once, at first use."""

    def __init__(self, name, state, entries, make, n, opts=(), seed=0, twin_n=None):
        self.name, self.state, self.entries, self.make, self.n, self.opts, self.seed = name, frozenset(state), tuple(entries), make, n, tuple(opts), seed
        self.twin_n = twin_n if twin_n is not None else (N_WS_TWIN if "ws" in self.state else N_SCRATCH_TWIN)
        self._host = self._dev = self._twin = None

    def __repr__(self):
        return self.name

    @property
    def host(self):
        if self._host is None:
            self._host = self.make(self.n, (self.name, self.seed))
        return self._host

    @property
    def counts(self):
        return [int(x) for x in self.host["counts"]]

    @property
    def words(self):
        return self.host.get("words", 0)

    def twin(self):
        """the same call on a second, larger input"""
        if self._twin is None:
            self._twin = Unit(self.name + "/larger", self.state, self.entries, self.make, self.twin_n, self.opts, seed=1)
        return self._twin

    def device(self):
        import torch

        if self._dev is None:
            inputs = {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).copy()).cuda()) for k, v in self.host["inputs"].items()}
            outs = {k: Expected(v) for k, v in self.host["outs"].items()}
            for o in outs.values():
                o.reset()
            self._dev = (inputs, outs)
        return self._dev

    def reset(self):
        """every output full of SENTINEL again (enqueued on torch's current stream)"""
        for o in self.device()[1].values():
            o.reset()

    def launch(self, L, eng):
        """enqueues the call on the engine's stream; nothing here waits for the device"""
        inputs, outs = self.device()
        i = {k: (None if t is None else t.data_ptr()) for k, t in inputs.items()}
        o = {k: e.ptr for k, e in outs.items()}
        for name, value in self.opts:
            eng.set_option(name, value)
        try:
            rc = self.host["call"](L, eng._ctx, i, o)
            assert rc == 0, (self.name, L.mi355_last_error())
            if self.host.get("kernel"):
                first = parse_record((L.mi355_ctx_last_launch(eng._ctx) or b"").decode())[0][0]
                assert base_name(first) == self.host["kernel"], (self.name, first)
        finally:
            for name, _ in self.opts:
                eng.set_option(name, 0)

    def untouched(self):
        return all(o.untouched() for o in self.device()[1].values())

    def check(self, what=""):
        for k, o in self.device()[1].items():
            o.check((self.name, k, what))


class EngineUnit(Unit):
    """a compound call of ScanEngine: the method allocates its outputs itself, so there are no guards; `run(eng, inputs)` -> the
    tensors it returns, `outs` their expected leading bytes"""

    def reset(self):
        self.device()
        self.got = None

    def device(self):
        import torch

        if self._dev is None:
            self._dev = ({k: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).copy()).cuda() for k, v in self.host["inputs"].items()}, {})
        return self._dev

    def twin(self):
        if self._twin is None:
            self._twin = EngineUnit(self.name + "/larger", self.state, self.entries, self.make, self.twin_n, self.opts, seed=1)
        return self._twin

    def launch(self, L, eng):
        self.got = self.host["run"](eng, self.device()[0])

    def untouched(self):
        return self.got is None

    def check(self, what=""):
        for k, want in self.host["outs"].items():
            have = self.got[k].contiguous().cpu().numpy().reshape(-1).view(np.uint8)[: len(want)]
            bad = np.nonzero(have != want)[0]
            assert bad.size == 0, (self.name, k, what, "byte", int(bad[0]), "of", len(want), "wrong bytes", int(bad.size))


# ---- workspace units ----

def make_rowids(density=0.3, above=True):
    def make(n, key):
        rng = rng_of(key)
        bits = rng.random(n) < density
        ids = np.nonzero(bits)[0].astype(np.uint64) + np.uint64(1000)
        cap = len(ids) + 100 if above else len(ids) // 2
        m = min(cap, len(ids))
        return dict(inputs={"bitmap": packbits(bits)}, counts=[len(ids)], words=rowid_words(n),
                    outs={"ids": prefix_body(8 * cap, ids[:m].view(np.uint8)), "count": u64s(len(ids))},
                    call=lambda L, ctx, i, o: L.mi355_bitmap_to_rowids_dev(ctx, i["bitmap"], n, 1000, o["ids"], cap, o["count"]))
    return make


def make_select(c, op, a, kernel, above):
    def make(n, key):
        rng = rng_of(key)
        vals = random_values(rng, n, c)
        ids = np.nonzero(pred(vals, op, a))[0].astype(np.uint64) + np.uint64(77)
        cap = len(ids) + 100 if above else len(ids) // 2
        m = min(cap, len(ids))
        return dict(inputs={"col": packed(vals, c)}, counts=[len(ids)], words=select_words(n, c), kernel=kernel,
                    outs={"ids": prefix_body(8 * cap, ids[:m].view(np.uint8)), "count": u64s(len(ids))},
                    call=lambda L, ctx, i, o: L.mi355_scan_select_dev(ctx, i["col"], n, c, CMP[op], a, 0, BOP["and"], None, 77, o["ids"], cap, o["count"]))
    return make


def make_compact(c, above, density=0.4):
    def make(n, key):
        rng = rng_of(key)
        vals, bits = random_values(rng, n, c), rng.random(n) < density
        chosen = vals[bits]
        cap = len(chosen) + 50 if above else len(chosen) // 2
        m = min(cap, len(chosen))
        return dict(inputs={"col": packed(vals, c), "bitmap": packbits(bits)}, counts=[len(chosen)], words=rowid_words(n),
                    outs={"out": prefix_body((cap * c + 31) // 32 * 4, payload(chosen[:m], c)), "count": u64s(len(chosen))},
                    call=lambda L, ctx, i, o: L.mi355_compact_dev(ctx, i["col"], n, c, i["bitmap"], o["out"], cap, o["count"]))
    return make


def make_top_k(c, largest):
    def make(n, key):
        rng = rng_of(key)
        # forty values spread over the whole width (every digit of the radix select has work), so the cut goes through ties
        vals = (rng.integers(0, 40, n, dtype=np.uint64) * np.uint64(((1 << c) - 1) // 40)).astype(np.uint32)
        qual = rng.random(n) < 0.5
        k = int(qual.sum()) // 3 + 123
        bits, res = top_k_expect(vals, qual, k, largest)
        return dict(inputs={"col": packed(vals, c), "mask": packbits(qual)}, counts=[res[0], res[3]], words=top_k_words(n, c),
                    more={"ties kept": res[0] - res[2], "ties dropped": res[3] - (res[0] - res[2])},
                    outs={"bitmap": packbits(bits), "result": u64s(*res)},
                    call=lambda L, ctx, i, o: L.mi355_top_k_dev(ctx, i["col"], n, c, i["mask"], k, 1 if largest else 0, o["bitmap"], o["result"]))
    return make


def make_sort_rows(c, descending, capacity="n", masked=True, spread=None):
    def make(n, key):
        rng = rng_of(key)
        vals = random_values(rng, n, c) if spread is None else (rng.integers(0, spread, n, dtype=np.uint64) * np.uint64(((1 << c) - 1) // spread)).astype(np.uint32)
        qual = rng.random(n) < 0.5 if masked else np.ones(n, dtype=bool)
        idx = np.nonzero(qual)[0]
        v = vals[idx].astype(np.int64)
        order = np.lexsort((idx, -v if descending else v))
        q = len(idx)
        cap = {"n": n, "zero": 0, "below": q - 1}[capacity]
        m = q if q <= cap else 0  # all or nothing
        ids = (idx[order[:m]].astype(np.uint64) + np.uint64(7)).view(np.uint8)
        sorted_vals = vals[idx[order[:m]]].astype(np.uint32).view(np.uint8)
        return dict(inputs={"col": packed(vals, c), "mask": packbits(qual) if masked else None}, counts=[q], words=sort_rows_words(n, cap, c),
                    more={"shape": (n, cap, c)},
                    outs={"ids": prefix_body(8 * cap, ids), "values": prefix_body(4 * cap, sorted_vals), "count": u64s(q)},
                    call=lambda L, ctx, i, o: L.mi355_sort_rows_dev(ctx, i["col"], n, c, i["mask"], 1 if descending else 0, 7, o["ids"], o["values"], cap, o["count"]))
    return make


def make_set_ranks(ct, miss):
    def make(n, key):
        rng = rng_of(key)
        bits = rng.random(n) < 0.3
        rank = np.cumsum(bits) - bits
        fits = bits & (rank < (1 << ct))
        table = np.where(fits, rank, miss).astype(np.uint32)
        members, unfit = int(bits.sum()), int((bits & ~fits).sum())
        return dict(inputs={"set": packbits(bits)}, counts=[members, unfit], words=rowid_words(n),
                    outs={"table": payload(table, ct), "counts": u64s(members, unfit)},
                    call=lambda L, ctx, i, o: L.mi355_set_ranks_dev(ctx, i["set"], n, ct, miss, o["table"], o["counts"]))
    return make


def make_key_index(ck, table_rows, keep, masked, kernel, ct=None, permutation=False):
    def make(n, key):
        rng = rng_of(key)
        keys = rng.permutation(n).astype(np.uint32) if permutation else random_values(rng, n, ck)
        qual = rng.random(n) < 0.6 if masked else np.ones(n, dtype=bool)
        first_row = 3
        width = ct or (first_row + n).bit_length()
        miss = first_row + n if first_row + n < (1 << width) else 0
        table, counts = key_index_expect(keys, qual, table_rows, keep, first_row, width, miss)
        nonzero = counts[:1] + counts[2:3] + (counts[1:2] if table_rows < 1 << ck else [])  # (a table over the whole domain has no row outside)
        return dict(inputs={"keys": packed(keys, ck), "mask": packbits(qual) if masked else None}, counts=nonzero, kernel=kernel,
                    words=key_index_words(n, ck, table_rows), outs={"table": payload(table, width), "counts": u64s(*counts)},
                    call=lambda L, ctx, i, o: L.mi355_key_index_dev(ctx, i["keys"], n, ck, i["mask"], first_row, 1 if keep == "last" else 0, o["table"],
                                                                    table_rows, width, miss, o["counts"]))
    return make


def column_of(eng, t, n, c):
    from shared_simd_scan_amd.engine import PackedColumn

    return PackedColumn(t, n, c)


def make_dense_codes(c, ct):
    def make(n, key):
        rng = rng_of(key)
        span = int(rng.integers(200, 400))  # distinct values, spread over the domain
        vals = (rng.integers(0, span, n, dtype=np.uint64) * np.uint64(((1 << c) - 1) // span)).astype(np.uint32)
        uniq, codes = np.unique(vals, return_inverse=True)
        domain = 1 << c
        return dict(inputs={"col": packed(vals, c)}, counts=[len(uniq)], words=rowid_words(domain),
                    outs={"codes": payload(codes.astype(np.uint32), ct), "values": uniq.astype(np.uint64).view(np.uint8), "count": u64s(len(uniq))},
                    run=lambda eng, i: (lambda r: {"codes": r[0].data, "values": r[1], "count": r[2]})(eng.dense_codes(column_of(eng, i["col"], n, c), ct=ct)))
    return make


def make_distinct_values(c):
    def make(n, key):
        rng = rng_of(key)
        span = int(rng.integers(400, 600))
        vals = (rng.integers(0, span, n, dtype=np.uint64) * np.uint64(((1 << c) - 1) // span)).astype(np.uint32)
        qual = rng.random(n) < 0.5
        uniq = np.unique(vals[qual])
        return dict(inputs={"col": packed(vals, c), "mask": packbits(qual)}, counts=[len(uniq)], words=rowid_words(1 << c),
                    outs={"values": uniq.astype(np.uint64).view(np.uint8), "count": u64s(len(uniq))},
                    run=lambda eng, i: (lambda r: {"values": r[0], "count": r[1]})(eng.distinct_values(column_of(eng, i["col"], n, c), mask=i["mask"])))
    return make


def make_build_table(ck, cv, table_rows, keep):
    def make(n, key):
        rng = rng_of(key)
        keys, vals = random_values(rng, n, ck), random_values(rng, n, cv)
        width = n.bit_length()
        index, counts = key_index_expect(keys, np.ones(n, dtype=bool), table_rows, keep, 0, width, n)
        table = np.where(index < n, vals[np.minimum(index, n - 1)], 5).astype(np.uint32)
        return dict(inputs={"keys": packed(keys, ck), "vals": packed(vals, cv)}, counts=counts[:1] + counts[2:3], words=key_index_words(n, ck, table_rows),
                    outs={"table": payload(table, cv), "counts": u64s(*counts)},
                    run=lambda eng, i: (lambda r: {"table": r[0].data, "counts": r[1]})(
                        eng.build_table(column_of(eng, i["keys"], n, ck), column_of(eng, i["vals"], n, cv), table_rows, keep=keep, miss=5)))
    return make


WS = "ws"
SCRATCH = "scratch"
SELECT2 = Unit("scan_select", (WS, SCRATCH), ["mi355_scan_select_dev"], make_select(9, "<", 150, "select2_kernel", above=True), N_WS)
WS_UNITS = [
    Unit("bitmap_to_rowids", [WS], ["mi355_bitmap_to_rowids_dev"], make_rowids(), N_WS),
    Unit("bitmap_to_rowids, two scan groups", [WS], ["mi355_bitmap_to_rowids_dev"], make_rowids(density=0.05), N_WS_BIG),
    SELECT2,
    Unit("scan_select, select_kernel", (WS, SCRATCH), ["mi355_scan_select_dev"], make_select(9, ">", 300, "select_kernel", above=False), N_WS, opts=(("select_kernel", 1),)),
    Unit("compact, capacity below the count", [WS], ["mi355_compact_dev"], make_compact(9, above=False), N_WS),
    Unit("compact, capacity above the count", [WS], ["mi355_compact_dev"], make_compact(13, above=True), N_WS),
    Unit("compact, two scan groups", [WS], ["mi355_compact_dev"], make_compact(9, above=True, density=0.05), N_WS_BIG),
    Unit("top_k c=9", [WS], ["mi355_top_k_dev"], make_top_k(9, True), N_WS),
    Unit("top_k c=17", [WS], ["mi355_top_k_dev"], make_top_k(17, False), N_WS),
    Unit("top_k c=32", [WS], ["mi355_top_k_dev"], make_top_k(32, True), N_WS),
    Unit("top_k, two scan groups", [WS], ["mi355_top_k_dev"], make_top_k(9, False), N_WS_BIG),
    Unit("sort_rows c=8", [WS], ["mi355_sort_rows_dev"], make_sort_rows(8, False), N_WS),
    Unit("sort_rows c=9", [WS], ["mi355_sort_rows_dev"], make_sort_rows(9, True), N_WS),
    Unit("sort_rows c=17", [WS], ["mi355_sort_rows_dev"], make_sort_rows(17, False), N_WS),
    Unit("sort_rows c=32", [WS], ["mi355_sort_rows_dev"], make_sort_rows(32, True), N_WS),
    Unit("sort_rows, capacity 0", [WS], ["mi355_sort_rows_dev"], make_sort_rows(17, False, capacity="zero"), N_WS),
    Unit("sort_rows, capacity below the count", [WS], ["mi355_sort_rows_dev"], make_sort_rows(17, True, capacity="below"), N_WS),
    Unit("set_ranks", [WS], ["mi355_set_ranks_dev"], make_set_ranks(14, 5), N_WS),
    Unit("key_index, LDS tier, first", [WS], ["mi355_key_index_dev"], make_key_index(12, 4096, "first", True, "key_index_lds_kernel"), N_WS),
    Unit("key_index, LDS tier, last", [WS], ["mi355_key_index_dev"], make_key_index(12, 4096, "last", False, "key_index_lds_kernel"), N_WS),
    Unit("key_index, global tier", [WS], ["mi355_key_index_dev"], make_key_index(17, 1 << 17, "first", True, "key_index_global_kernel"), N_WS),
    Unit("key_index, short table", [WS], ["mi355_key_index_dev"], make_key_index(17, 100_003, "last", True, "key_index_global_kernel"), N_WS),
    EngineUnit("dense_codes", [WS], ["mi355_set_ranks_dev", "mi355_bitmap_to_rowids_dev"], make_dense_codes(12, 9), N_WS),
    EngineUnit("distinct_values", [WS], ["mi355_bitmap_to_rowids_dev"], make_distinct_values(14), N_WS),
    EngineUnit("build_table", [WS], ["mi355_key_index_dev"], make_build_table(12, 9, 4096, "first"), N_WS),
]
# one variant per entry point for the pair matrix (the others run behind the dirtiers)
WS_PAIR_UNITS = [u for u in WS_UNITS if u.name in ("bitmap_to_rowids", "scan_select", "compact, capacity above the count", "top_k c=17", "sort_rows c=17", "set_ranks",
                                                   "key_index, global tier", "dense_codes", "distinct_values", "build_table")]
# the dirtiers: ordinary calls that leave the workspace full of garbage.  D1: every 32-bit slot of 2^20 words ends as ~row, non-zero
# with its high bits set; D2: more than 2^20 words of plausible small integers, prefixes and items
D1 = Unit("D1 key_index", [WS], ["mi355_key_index_dev"], make_key_index(21, 1 << 21, "first", False, "key_index_global_kernel", permutation=True), 1 << 21)
D2 = Unit("D2 sort_rows", [WS], ["mi355_sort_rows_dev"], make_sort_rows(17, False, masked=False), 1 << 19)
DIRTIERS = [D1, D2]


# ---- scratch units ----

def bitmap_and_hits(bits):
    return {"bitmap": packbits(bits), "hits": u64s(int(bits.sum()))}


def make_scan(kind):
    """the single-column scans: eq, range, where (with a mask; count only), masked combine, IN-list"""
    def make(n, key):
        rng = rng_of(key)
        c = 9
        vals = random_values(rng, n, c)
        mask = rng.random(n) < 0.7
        inputs = {"col": packed(vals, c), "mask": packbits(mask)}
        if kind == "eq":
            k = int(vals[5])
            bits, call = vals == k, lambda L, ctx, i, o: L.mi355_scan_eq_dev(ctx, i["col"], n, c, k, o["bitmap"], o["hits"])
        elif kind == "range":
            bits, call = pred(vals, "between", 40, 333), lambda L, ctx, i, o: L.mi355_scan_range_dev(ctx, i["col"], n, c, 40, 333, o["bitmap"], o["hits"])
        elif kind == "where":
            bits = pred(vals, "!=", 17) & mask
            call = lambda L, ctx, i, o: L.mi355_scan_where_dev(ctx, i["col"], n, c, CMP["!="], 17, 0, i["mask"], o["bitmap"], o["hits"])
        elif kind == "where_count":
            bits = pred(vals, ">=", 200)
            call = lambda L, ctx, i, o: L.mi355_scan_where_dev(ctx, i["col"], n, c, CMP[">="], 200, 0, None, None, o["hits"])
        elif kind == "combine":
            bits = combine(pred(vals, "not_between", 100, 400), mask, "xor")
            call = lambda L, ctx, i, o: L.mi355_scan_combine_dev(ctx, i["col"], n, c, CMP["not_between"], 100, 400, BOP["xor"], i["mask"], o["bitmap"], o["hits"])
        else:
            keys = np.ascontiguousarray(vals[rng.integers(0, n, 20)].astype(np.int32))
            bits = np.isin(vals, keys.astype(np.uint32)) & mask
            call = lambda L, ctx, i, o: L.mi355_scan_in_dev(ctx, i["col"], n, c, keys.ctypes.data, 20, 0, i["mask"], o["bitmap"], o["hits"])
        outs = bitmap_and_hits(bits)
        if kind == "where_count":
            del outs["bitmap"]
        return dict(inputs=inputs, outs=outs, counts=[int(bits.sum())], call=call, kernel="in_kernel" if kind == "in" else "scan_burst_kernel")
    return make


def make_scan2():
    def make(n, key):
        rng = rng_of(key)
        v1, v2 = random_values(rng, n, 9), random_values(rng, n, 9)
        bits = pred(v1, "<", 300) & ~pred(v2, "between", 10, 200)
        return dict(inputs={"col1": packed(v1, 9), "col2": packed(v2, 9)}, outs=bitmap_and_hits(bits), counts=[int(bits.sum())], kernel="scan2_kernel",
                    call=lambda L, ctx, i, o: L.mi355_scan2_dev(ctx, i["col1"], 9, CMP["<"], 300, 0, i["col2"], 9, CMP["between"], 10, 200, n, BOP["andnot"],
                                                                o["bitmap"], o["hits"]))
    return make


def make_scan_columns(count_only):
    def make(n, key):
        rng = rng_of(key)
        c1, c2 = (9, 12) if count_only else (12, 9)
        v1, v2 = random_values(rng, n, c1), random_values(rng, n, c2)
        mask = rng.random(n) < 0.6
        d = v1.astype(np.int64) - v2.astype(np.int64)
        bits = combine((d >= -700) & (d <= 900), mask, "or")
        outs = bitmap_and_hits(bits)
        if count_only:
            del outs["bitmap"]
        return dict(inputs={"col1": packed(v1, c1), "col2": packed(v2, c2), "mask": packbits(mask)}, outs=outs, counts=[int(bits.sum())], kernel="scan_columns_kernel",
                    call=lambda L, ctx, i, o: L.mi355_scan_columns_dev(ctx, i["col1"], c1, i["col2"], c2, n, CMP["between"], -700, 900, BOP["or"], i["mask"],
                                                                       o.get("bitmap"), o["hits"]))
    return make


def make_semi_join(c, set_bits, negate, kernel):
    def make(n, key):
        rng = rng_of(key)
        vals = random_values(rng, n, c)
        members = rng.random(set_bits) < 0.4
        inside = vals < set_bits
        bits = np.zeros(n, dtype=bool)
        bits[inside] = members[vals[inside]]
        if negate:
            bits = ~bits
        return dict(inputs={"col": packed(vals, c), "set": packbits(members)}, outs=bitmap_and_hits(bits), counts=[int(bits.sum())], kernel=kernel,
                    call=lambda L, ctx, i, o: L.mi355_semijoin_dev(ctx, i["col"], n, c, i["set"], set_bits, 1 if negate else 0, None, o["bitmap"], o["hits"]))
    return make


def make_bitmap(combine_too):
    def make(n, key):
        rng = rng_of(key)
        a, b = rng.random(n) < 0.45, rng.random(n) < 0.55
        if combine_too:
            bits = a ^ b
            return dict(inputs={"a": packbits(a), "b": packbits(b)}, outs={"out": packbits(bits), "count": u64s(int(bits.sum()))}, counts=[int(bits.sum())],
                        call=lambda L, ctx, i, o: L.mi355_bitmap_combine_dev(ctx, BOP["xor"], i["a"], i["b"], o["out"], n, o["count"]))
        return dict(inputs={"a": packbits(a)}, outs={"count": u64s(int(a.sum()))}, counts=[int(a.sum())],
                    call=lambda L, ctx, i, o: L.mi355_bitmap_count_dev(ctx, i["a"], n, o["count"]))
    return make


def shared_outs(matches, layout):
    """the outputs of a shared scan whose predicate k selects matches[k]: per predicate a bitmap every `stride` bytes with a gap that
    stays as it was, or linear rows (the byte of 8-row group g and predicate k at g P + k); and the P counts -> (outs, stride)"""
    P, n = len(matches), len(matches[0])
    nb = (n + 7) // 8
    stride = (nb + 15) // 16 * 16 + 16
    images = [packbits(m) for m in matches]
    if layout == 0:
        body = np.full((P, stride), SENTINEL, dtype=np.uint8)
        for k, img in enumerate(images):
            body[k, :nb] = img
    else:
        body = np.stack(images, axis=1)
    return {"out": body.reshape(-1), "hits": u64s(*[int(m.sum()) for m in matches])}, stride


def make_shared(case):
    """an equality shared scan with c, P, layout, column and keys of a case of kernel_cases.CASES, at this file's size"""
    def make(n, key):
        vals, keys = column(dataclasses.replace(case, n=n), rng_of(key))
        uniq = {k: vals == k for k in set(keys)}
        outs, stride = shared_outs([uniq[k] for k in keys], case.layout)
        k32 = np.ascontiguousarray(np.asarray(keys, dtype=np.uint32).view(np.int32))
        return dict(inputs={"col": packed(vals, case.c)}, outs=outs, counts=[int(uniq[k].sum()) for k in keys], kernel=base_name(case.expect[0]),
                    call=lambda L, ctx, i, o: L.mi355_shared_scan_eq_dev(ctx, i["col"], n, case.c, k32.ctypes.data, case.P, case.layout, o["out"], stride, o["hits"]))
    return make


def make_shared_where(c, P, family):
    def make(n, key):
        from shared_simd_scan_amd.engine import predicates

        rng = rng_of(key)
        vals = random_values(rng, n, c)
        ops = list(CMP)
        preds = []
        for k in range(P):
            a, b = sorted(int(x) for x in rng.integers(0, 1 << c, 2))
            preds.append((ops[k % 8], a, b) if ops[k % 8] in ("between", "not_between") else (ops[k % 8], a))
        arr = predicates(preds)
        outs, stride = shared_outs([pred(vals, *p) for p in preds], 0)
        return dict(inputs={"col": packed(vals, c)}, outs=outs, counts=[int(pred(vals, *p).sum()) for p in preds],
                    kernel=family.split("(")[0], more={"preds": arr},
                    call=lambda L, ctx, i, o: L.mi355_shared_scan_where_dev(ctx, i["col"], n, c, C.cast(arr, C.c_void_p), P, 0, o["out"], stride, o["hits"]))
    return make


def case(cid):
    return next(k for k in CASES if k.id == cid)


def where_case(c, family):
    """the smallest P of WHERE_COUNT_CASES that runs `family` at width c"""
    return min(P for w, P, f in WHERE_COUNT_CASES if w == c and f == family)


SEMI_LDS_MAX = header_macro("mi355_semijoin.h", "MI355_SEMIJOIN_LDS_MAX_BITS")
SHARED_CASES = ["pair_pp", "lut_pp", "wide3_rc1", "wide3_rc2", "wide3_rc1_big", "wide3_rc2_big", "wide2_hist", "chain_bit64", "linear_p9", "linear2_attached",
                "linear3_rc1", "linear3_rc2", "linear3_rc2_big"]
SWEEPER = dataclasses.replace(case("wide2_hist"), id="sweeper", c=16, P=1024, expect=("",))  # (whichever family the launcher takes)
SCRATCH_UNITS = [
    Unit("scan_eq", [SCRATCH], ["mi355_scan_eq_dev"], make_scan("eq"), N_SCRATCH),
    Unit("scan_range", [SCRATCH], ["mi355_scan_range_dev"], make_scan("range"), N_SCRATCH),
    Unit("scan_where", [SCRATCH], ["mi355_scan_where_dev", "mi355_scan_combine_dev"], make_scan("where"), N_SCRATCH),
    Unit("scan_where, count only", [SCRATCH], ["mi355_scan_where_dev", "mi355_scan_combine_dev"], make_scan("where_count"), N_SCRATCH),
    Unit("scan_combine, masked", [SCRATCH], ["mi355_scan_combine_dev"], make_scan("combine"), N_SCRATCH),
    Unit("scan2", [SCRATCH], ["mi355_scan2_dev"], make_scan2(), N_SCRATCH),
    Unit("scan_columns", [SCRATCH], ["mi355_scan_columns_dev"], make_scan_columns(False), N_SCRATCH),
    Unit("scan_columns, count only", [SCRATCH], ["mi355_scan_columns_dev"], make_scan_columns(True), N_SCRATCH),
    Unit("scan_in P=20", [SCRATCH], ["mi355_scan_in_dev"], make_scan("in"), N_SCRATCH),
    Unit("semi_join, LDS tier, negated", [SCRATCH], ["mi355_semijoin_dev"], make_semi_join(9, 500, True, "semijoin_lds_kernel"), N_SCRATCH),
    Unit("semi_join, global tier", [SCRATCH], ["mi355_semijoin_dev"], make_semi_join(21, 1 << 21, False, "semijoin_global_kernel"), N_SCRATCH),
    SELECT2,
    Unit("bitmap_count", [SCRATCH], ["mi355_bitmap_count_dev"], make_bitmap(False), N_SCRATCH),
    Unit("bitmap_combine, counted", [SCRATCH], ["mi355_bitmap_combine_dev"], make_bitmap(True), N_SCRATCH),
    *[Unit(f"shared_scan {cid}", [SCRATCH], ["mi355_shared_scan_eq_dev"], make_shared(case(cid)), N_SCRATCH, opts=tuple(o for o in case(cid).opts if o[0] == "kernel_flags"))
      for cid in SHARED_CASES],
    *[Unit(f"shared_scan_where {family}", [SCRATCH], ["mi355_shared_scan_where_dev"], make_shared_where(c, where_case(c, family), family), N_SCRATCH)
      for c, family in ((9, WHERE_LUT), (12, WHERE_LUT_MULTI), (17, WHERE_CHAIN))],
    # reads every hit slot of every replica
    Unit("sweeper: shared_scan P=1024", [SCRATCH], ["mi355_shared_scan_eq_dev"], make_shared(SWEEPER), N_SCRATCH),
]
UNITS = WS_UNITS + [u for u in SCRATCH_UNITS if u is not SELECT2]


def by_name(units):
    return {u.name: u for u in units}


# ------------------------------------------------------------------------------------------------------------------------
# CPU: the table is complete, its data can show a mistake, the dirtiers cover every unit
# ------------------------------------------------------------------------------------------------------------------------

def test_unit_names_unique():
    assert len(by_name(UNITS + DIRTIERS)) == len(UNITS) + len(DIRTIERS)


def test_every_state_user_is_a_unit():
    """derived from csrc/**/*.hip: a future entry point that asks for the workspace or hands the scratch to a kernel fails here until
    a unit names it"""
    ws, scratch = entry_points_reaching("rowid_ws_get("), entry_points_reaching("kernel_scratch")
    assert len(ws) >= 7 and len(scratch) >= 12, (ws, scratch)  # the parse found the launchers
    for state, derived in ((WS, ws), (SCRATCH, scratch)):
        named = {e for u in UNITS if state in u.state for e in u.entries}
        missing = sorted(set(derived) - named - set(EXEMPT))
        assert not missing, f"entry points that reach the {state} and that no unit names: {missing}"
    everything = set(ws) | set(scratch)
    assert set(EXEMPT) <= everything, sorted(set(EXEMPT) - everything)
    stale = sorted({e for u in UNITS for e in u.entries} - everything)
    assert not stale, f"units name entry points that reach neither state: {stale}"
    assert not {e for u in UNITS for e in u.entries} & set(EXEMPT)


def test_required_variants_are_in_the_table():
    names = set(by_name(UNITS))
    for width in (9, 17, 32):
        assert f"top_k c={width}" in names
    for width in (8, 9, 17, 32):
        assert f"sort_rows c={width}" in names
    assert {u.n for u in UNITS if WS in u.state} == {N_WS, N_WS_BIG} and {u.n for u in SCRATCH_UNITS if u is not SELECT2} == {N_SCRATCH}
    assert {u.name.split(",")[0] for u in UNITS if u.n == N_WS_BIG} == {"bitmap_to_rowids", "compact", "top_k"}
    assert {base_name(case(cid).expect[0]) for cid in SHARED_CASES} == {"shared_pair_kernel", "shared_lut_kernel", "shared_wide3_kernel", "shared_wide2_kernel",
                                                                         "shared_general_kernel", "shared_linear_kernel", "shared_linear2_kernel", "shared_linear3_kernel"}
    assert all(case(cid).hits for cid in SHARED_CASES)
    assert {e for u in WS_PAIR_UNITS for e in u.entries} >= set(entry_points_reaching("rowid_ws_get("))


def test_tiered_units_sit_in_the_tiers_they_name(L):
    units = by_name(SCRATCH_UNITS)
    assert L.mi355_semijoin_kernel(9, 500) == b"semijoin_lds_kernel" and 500 <= SEMI_LDS_MAX < 1 << 21
    assert L.mi355_semijoin_kernel(21, 1 << 21) == b"semijoin_global_kernel"
    assert units["semi_join, LDS tier, negated"].host["kernel"] == "semijoin_lds_kernel"
    assert L.mi355_key_index_kernel(12, 4096) == b"key_index_lds_kernel" and L.mi355_key_index_kernel(17, 100_003) == b"key_index_global_kernel"


@pytest.mark.parametrize("unit", [u for u in UNITS + DIRTIERS if u.n != N_WS_BIG], ids=repr)
def test_expected_counts_are_not_zero(unit):
    """a count of zero is what a call that did nothing, or a workspace nobody wrote, also gives"""
    assert unit.counts and all(x > 0 for x in unit.counts), (unit.name, unit.counts[:8])
    assert all(x > 0 for x in unit.twin().counts) and unit.twin().counts != unit.counts


@pytest.mark.parametrize("unit", [u for u in UNITS if u.n == N_WS_BIG], ids=repr)
def test_expected_counts_of_the_two_group_units(unit):
    assert unit.counts and all(x > 0 for x in unit.counts)
    assert -(-unit.n // CHUNK) > SCAN_GROUP and unit.n % CHUNK  # a second scan group, a ragged end


def test_no_two_scratch_units_expect_the_same_counts():
    """hits left behind by one unit would not cancel out in the next: the count vectors differ, and so do their sums"""
    seen, sums = {}, {}
    for u in SCRATCH_UNITS + [x.twin() for x in SCRATCH_UNITS]:
        assert tuple(u.counts) not in seen, (u.name, seen.get(tuple(u.counts)))
        assert sum(u.counts) not in sums, (u.name, sums.get(sum(u.counts)))
        seen[tuple(u.counts)], sums[sum(u.counts)] = u.name, u.name


def test_top_k_units_cut_through_ties():
    units = [u for u in UNITS if u.name.startswith("top_k")]
    assert len(units) == 4
    for u in units + [x.twin() for x in units if x.n == N_WS]:
        more = u.host["more"]
        assert more["ties kept"] > 0 and more["ties dropped"] > 0, (u.name, more)  # topk_trim_kernel has work


def test_dirtiers_cover_every_workspace_unit(L):
    """the workspace is grow-only with a fixed base, so a unit's words are a prefix of the dirtier's: every word a unit reads has
    been written by the dirtier in front of it"""
    assert D1.words == 1 << 20 and D2.words > 1 << 20
    for u in WS_UNITS:
        if u.n == N_WS_BIG and u.name.startswith("top_k"):
            assert u.words == rowid_words(u.n) + 8 + 4096
        assert 0 < u.words <= min(D1.words, D2.words), (u.name, u.words)
    sorts = [u for u in WS_UNITS + [D2] if "shape" in u.host.get("more", {})]
    assert len(sorts) == 7
    for u in sorts:
        n, cap, c = u.host["more"]["shape"]
        assert u.words == L.mi355_sort_rows_workspace_words(n, cap, c), (u.name, u.words)


def test_footprints_follow_the_headers():
    """the formulas above are the headers' (compare their text, whitespace aside)"""
    squeeze = lambda s: "".join(s.split())
    assert squeeze("(ceil(n / 16384) + 1 + ceil(n / 16777216)) words") in squeeze(header_text("mi355_compact.h"))
    assert squeeze("(ceil(n / 16384) + 1 + ceil(n / 16777216) + 8 + 4096 * mi355_top_k_passes(c)) words") in squeeze(header_text("mi355_topk.h"))
    assert squeeze("(ceil(set_bits / 16384) + 1 + ceil(set_bits / 16777216)) words") in squeeze(header_text("mi355_distinct.h"))
    assert squeeze("ceil(reach / 2) words") in squeeze(header_text("mi355_keyindex.h"))
    assert rowid_words(N_WS_BIG) == 1026 + 1 + 2 and CHUNK * SCAN_GROUP == 16777216


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------

def fresh_engine(opts=()):
    from shared_simd_scan_amd import ScanEngine

    e = ScanEngine(0)
    for name, value in opts:
        e.set_option(name, value)
    return e


def run_alone(L, eng, unit, what):
    unit.reset()
    unit.launch(L, eng)
    eng.synchronize()
    unit.check(what)


class Refusal:
    """a call that is refused for a misaligned column: nothing is enqueued, and the state stays as it was"""

    def __init__(self):
        import torch

        self.col = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        self.bitmap, self.word = Guarded(512), Guarded(32, back=64, front=64)

    def refuse(self, L, eng, state):
        col = self.col.data_ptr() + 4  # 4 bytes behind a 16-byte boundary: the column wants 16
        if state == WS:
            rc = L.mi355_top_k_dev(eng._ctx, col, 2000, 9, None, 10, 1, self.bitmap.ptr, self.word.ptr)
        else:
            rc = L.mi355_scan_eq_dev(eng._ctx, col, 2000, 9, 1, self.bitmap.ptr, self.word.ptr)
        assert rc == E_INVALID and b"align" in (L.mi355_last_error() or b""), (rc, L.mi355_last_error())

    def check(self):
        assert (self.bitmap.fetch() == SENTINEL).all() and (self.word.fetch() == SENTINEL).all(), "the refused call wrote"


# ---- 2. workspace users behind a dirtier ----

@gpu
@pytest.mark.parametrize("unit", WS_UNITS, ids=repr)
@pytest.mark.parametrize("dirtier", DIRTIERS, ids=repr)
def test_workspace_unit_behind_a_dirtier(L, dirtier, unit):
    e = fresh_engine()
    try:
        run_alone(L, e, dirtier, "the dirtier on a fresh context")
        run_alone(L, e, unit, f"behind {dirtier.name}")
    finally:
        e.close()


# ---- 3. every ordered pair ----

def run_pairs(L, eng, first, units, state):
    refusal = Refusal()
    refused_at = units.index(first)  # one B per A, another one for every A
    for j, second in enumerate(units):
        a = first.twin() if second is first else first
        a.reset()
        second.reset()
        a.launch(L, eng)
        if j == refused_at:
            refusal.refuse(L, eng, state)
        second.launch(L, eng)  # no host synchronisation since a.launch
        eng.synchronize()
        a.check(f"in front of {second.name}")
        second.check(f"behind {a.name}")
    refusal.check()


@gpu
@pytest.mark.parametrize("first", WS_PAIR_UNITS, ids=repr)
def test_workspace_pairs(L, eng, first):
    run_pairs(L, eng, first, WS_PAIR_UNITS, WS)


@pytest.fixture(scope="module")
def one_block():
    """an engine whose grids have one block: every ticket group but one stays empty, one replica takes every hit"""
    e = fresh_engine((("grid_cus", 1), ("max_blocks_per_cu", 1)))
    yield e
    e.close()


@gpu
@pytest.mark.parametrize("first", SCRATCH_UNITS, ids=repr)
def test_scratch_pairs(L, eng, first):
    run_pairs(L, eng, first, SCRATCH_UNITS, SCRATCH)


@gpu
@pytest.mark.parametrize("first", SCRATCH_UNITS, ids=repr)
def test_scratch_pairs_on_one_block(L, one_block, first):
    run_pairs(L, one_block, first, SCRATCH_UNITS, SCRATCH)


# ---- 4. a stream switch with queued workspace work ----

@gpu
@pytest.mark.parametrize("first", [u for u in WS_UNITS if u.n == N_WS_BIG], ids=repr)
def test_stream_switch_with_queued_workspace_work(L, first):
    """the workspace belongs to the context: mi355_ctx_set_stream orders the new stream behind what the old one still has to run"""
    import torch

    seconds = [u for u in WS_PAIR_UNITS if not isinstance(u, EngineUnit) and u.entries != first.entries]
    e = fresh_engine()
    original, side = e.stream, torch.cuda.Stream()
    try:
        for j, second in enumerate(seconds):
            for a, b, streams in ((first, second, (original, side)), (second, first, (side, original))):
                a.reset()
                b.reset()
                torch.cuda.synchronize()  # (the outputs are refilled on torch's stream, the calls run on the engine's)
                e.use_stream(streams[0])
                a.launch(L, e)
                e.use_stream(streams[1])
                b.launch(L, e)
                torch.cuda.synchronize()
                a.check(f"on the first stream, in front of {b.name}")
                b.check(f"on the second stream, behind {a.name}")
    finally:
        e.use_stream(original)
        torch.cuda.synchronize()
        e.close()


# ---- 5. replays between eager calls of other features ----

CAPTURED = ["compact, capacity above the count", "top_k c=17", "sort_rows c=17", "set_ranks", "key_index, global tier", "bitmap_to_rowids", "scan_select"]


@gpu
@pytest.mark.parametrize("name", CAPTURED, ids=str)
def test_replays_between_eager_calls(L, name):
    import torch

    unit = by_name(WS_UNITS)[name]
    others = [u for u in WS_PAIR_UNITS if not isinstance(u, EngineUnit) and u.entries != unit.entries]
    other = others[CAPTURED.index(name) % len(others)]

    def setup(e):
        # warmed with both dirtiers: the workspace never grows afterwards, the graph keeps pointing at the live buffer
        for d in DIRTIERS:
            run_alone(L, e, d, "warming the context")

        def between(r):
            run_alone(L, e, DIRTIERS[r % 2], f"eagerly in front of replay {r}")
            run_alone(L, e, other, f"eagerly in front of replay {r}, behind {DIRTIERS[r % 2].name}")

        def untouched():
            torch.cuda.current_stream().synchronize()
            assert unit.untouched()

        return capture.Steps(load=lambda r: unit.reset(), run=lambda: unit.launch(L, e), check=lambda r, what: unit.check(what), untouched=untouched,
                             between=between)

    capture.capture_replay(setup, (0, 1, 2, 3))
