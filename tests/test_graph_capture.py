"""Graph capture and replay of every device entry point (include/mi355_scan.h "graph capture").

Every case of CAPTURE_CASES goes through the protocol of capture.capture_replay, with a Trial as its buffers: three replays, each
over inputs that were overwritten in place (column, mask, row ids, device-side counts) and outputs refilled with 0xEE, each
compared byte for byte with numpy inside intact guard bytes.  The three versions' expected outputs differ pairwise (asserted on
the CPU), so a stale or an accumulated result cannot pass.  Integer work only: every comparison is exact.

generate_dev, dev_memset and the n = 0 forms take all of their inputs by value: their three replays produce the same bytes, and
only the 0xEE refill shows that each replay ran (Trial.constant).

VERDICTS is the capture contract per entry point; the CPU test holds it against the table in include/mi355_scan.h.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import capture
from kernel_cases import N_SMALL, Case, check_select, column
from support import E_INVALID, SENTINEL, Guarded, packbits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_SCAN = 3_000_077             # ragged; the equality scan's warm-up must report grid >= 17 (both ticket levels of hits_finalize contended)
N_SELECT = 65536 * 23 + 77     # 24 look-back chunks at c = 9
MIN_SCAN_GRID = 17
FRACTIONS = (0.2, 0.35, 0.5)   # share of rows that hold one of the hot keys, per version
DENSITIES = (0.4, 0.5, 0.6)    # set bits of a mask, per version
AND, OR, XOR, ANDNOT = 0, 1, 2, 3
EQ, NE, LT, LE, GT, GE, BETWEEN, NOT_BETWEEN = range(8)

gpu = pytest.mark.gpu


# ---- the capture contract ------------------------------------------------------------------------------------------------
CAPTURABLE = "capturable"
WARM = "capturable after a warm-up call of at least this size"
NEVER = "never: synchronises"
RCCL = "not covered: RCCL collectives need a communicator over several ranks; tests/test_exchange_loopback.py runs them eagerly"
# entry point -> (verdict, cases of CAPTURE_CASES that hold it to the verdict)
VERDICTS = {
    "mi355_dev_alloc": (NEVER, []),
    "mi355_dev_free": (NEVER, []),
    "mi355_dev_upload": (NEVER, []),
    "mi355_dev_download": (NEVER, []),
    "mi355_dev_memset": (CAPTURABLE, ["dev_memset"]),
    "mi355_pack_u16_dev": (CAPTURABLE, ["pack_u16"]),
    "mi355_pack_u32_dev": (CAPTURABLE, ["pack_u32"]),
    "mi355_generate_dev": (CAPTURABLE, ["generate"]),
    "mi355_decompress_dev": (CAPTURABLE, ["decompress-c9", "decompress-c1", "decompress-c32"]),
    "mi355_scan_eq_dev": (CAPTURABLE, ["scan_eq-c9", "scan_eq-c1", "scan_eq-c17", "scan_eq-c32", "n0_forms"]),
    "mi355_scan_range_dev": (CAPTURABLE, ["scan_range-c9", "scan_range-c17", "n0_forms"]),
    "mi355_shared_scan_eq_dev": ("refused while capturing when P > 8", ["shared_eq-c9-P8-pp-hits", "shared_eq-c17-P3-lin-nohits"]),
    "mi355_scan_where_dev": (CAPTURABLE, ["scan_where-c9-plain", "scan_where-c17-inplace"]),
    "mi355_scan_combine_dev": (CAPTURABLE, ["scan_combine-c9-or", "scan_combine-c17-count"]),
    "mi355_shared_scan_where_dev": ("refused while capturing when P > 8", ["shared_where-c9-P8-pp", "shared_where-c17-P2-lin"]),
    "mi355_scan_in_dev": ("refused while capturing when n > 0: every key list is uploaded per call, so the call is never capturable", []),
    "mi355_scan2_dev": ("refused while capturing when the widths differ, bitmap_dev is NULL and the context's buffer pool has to grow",
                        ["scan2-same-c9", "scan2-9+12"]),
    "mi355_scan_select_dev": (WARM, ["select-select2-mask-eq-small_grid", "select-single-nomask-gt-full_grid"]),
    "mi355_bitmap_combine_dev": (CAPTURABLE, ["bitmap_combine-xor", "bitmap_combine-and-in_a"]),
    "mi355_bitmap_count_dev": (CAPTURABLE, ["bitmap_count"]),
    "mi355_bitmap_to_rowids_dev": (WARM, ["bitmap_to_rowids"]),
    "mi355_gather_dev": (CAPTURABLE, ["gather-c9", "gather-c17"]),
    "mi355_aggregate_dev": (CAPTURABLE, ["aggregate-c9-mask", "aggregate-c17-nomask"]),
    "mi355_histogram_dev": (CAPTURABLE, ["histogram-mask", "histogram-nomask"]),
    "mi355_tune_dev": ("refused while capturing when n >= 5e7 rows (below that it measures nothing and returns)", []),
    "mi355_gather_bitmaps_dev": (RCCL, []),
    "mi355_gather_bitmaps_at_dev": (RCCL, []),
    "mi355_allreduce_hits_dev": (RCCL, []),
    "mi355_sharded_scan_eq_dev": (RCCL, []),
    "mi355_sharded_scan_range_dev": (RCCL, []),
}
VERDICT_FORMS = (r"capturable", r"capturable after a warm-up call of at least this size", r"refused while capturing when \S.*",
                 r"never: synchronises", r"not covered: \S.*")


def header_text():
    with open(os.path.join(ROOT, "include", "mi355_scan.h")) as f:
        return f.read()


def declared_dev_entry_points():
    code = re.sub(r"/\*.*?\*/", " ", header_text(), flags=re.S)
    return sorted(set(re.findall(r"\bMI355_API\s+int\s+(mi355_\w+_dev|mi355_dev_\w+)\s*\(", code)))


def header_verdicts():
    """the table in the header: lines ' *   <entry point>  <verdict>' under 'Graph capture'"""
    block = re.search(r"/\* ---- Graph capture.*?\*/", header_text(), flags=re.S)
    assert block, "include/mi355_scan.h has no 'Graph capture' comment"
    rows = {}
    name = None
    for line in block.group(0).split("\n"):
        m = re.match(r" \*   (mi355_\w+)\s+(\S.*)$", line)
        if m:
            name = m.group(1)
            rows[name] = m.group(2).strip()
        elif name and re.match(r" \*\s{8,}\S", line):  # continuation of the row above
            rows[name] += " " + line[2:].strip()
        else:
            name = None
    return rows


def test_every_dev_entry_point_has_a_capture_verdict():
    names = declared_dev_entry_points()
    assert len(names) >= 30 and "mi355_scan_eq_dev" in names and "mi355_dev_memset" in names
    assert sorted(VERDICTS) == names
    ids = set(CAPTURE_CASES)
    for name, (verdict, cases) in VERDICTS.items():
        assert any(re.fullmatch(form, verdict) for form in VERDICT_FORMS), f"{name}: {verdict!r} is no verdict"
        if verdict.startswith("not covered"):
            assert name in ("mi355_gather_bitmaps_dev", "mi355_gather_bitmaps_at_dev", "mi355_allreduce_hits_dev",
                            "mi355_sharded_scan_eq_dev", "mi355_sharded_scan_range_dev"), f"{name}: only the RCCL calls may be left out"
        if verdict.startswith("capturable"):
            assert cases, f"{name}: capturable, but no case captures it"
        if cases:  # every entry point but the refused-at-any-size ones has a path that captures: it is exercised
            assert not verdict.startswith(("never", "not covered"))
        for cid in cases:
            assert cid in ids, f"{name}: {cid} is no case of CAPTURE_CASES"
    assert header_verdicts() == {name: verdict for name, (verdict, _) in VERDICTS.items()}


# ---- data: three versions of everything, computed once ---------------------------------------------------------------------
def hot_keys(c):
    if c == 1:
        return [1] * 8
    if c == 32:
        return [0x80000000 + 37 * k + 5 for k in range(8)]  # the sign bit of the int32 key
    return [(37 * k + 5) % (1 << c) for k in range(8)]


def i32(key):
    return key - (1 << 32) if key >= 1 << 31 else key


def key_array(keys):
    return np.ascontiguousarray(np.asarray(keys, dtype=np.uint32).view(np.int32))


@functools.lru_cache(maxsize=None)
def data(c, n, salt=0):
    out = []
    for r in range(3):
        rng = np.random.default_rng([c, n, salt, r])
        vals = rng.integers(0, 1 << c, n, dtype=np.uint64).astype(np.uint32)
        hot = rng.random(n) < FRACTIONS[r]
        vals[hot] = np.asarray(hot_keys(c), dtype=np.uint32)[rng.integers(0, 8, int(hot.sum()))]
        out.append(vals)
    return tuple(out)


_packed = {}


def packed(O, c, n, salt=0):
    key = (c, n, salt)
    if key not in _packed:
        _packed[key] = tuple(O.pack(v, c) for v in data(c, n, salt))
    return _packed[key]


@functools.lru_cache(maxsize=None)
def mask_bits(n, salt=0):
    return tuple(np.random.default_rng([n, salt, r, 99]).random(n) < DENSITIES[r] for r in range(3))


def nb(n):
    return (n + 7) // 8


def u64(x):
    return np.asarray([x], dtype=np.uint64)


def compare(v, op, a, b=0):
    v = v.astype(np.int64)
    return {EQ: v == a, NE: v != a, LT: v < a, LE: v <= a, GT: v > a, GE: v >= a, BETWEEN: (v >= a) & (v <= b),
            NOT_BETWEEN: (v < a) | (v > b)}[op]


def combine(p, m, op):
    return {AND: p & m, OR: p | m, XOR: p ^ m, ANDNOT: m & ~p}[op]


def ptr(t):
    return C.c_void_p(t.data_ptr())


class Trial:
    """the buffers of one captured call: inputs with three staged versions, outputs inside guards, expectations per version"""

    def __init__(self, L, O, ctx):
        self.L, self.O, self.ctx = L, O, ctx
        self.inputs, self.outputs, self.expect = [], {}, [{}, {}, {}]
        self.constant = False   # every input travels by value: the versions are identical
        self.constant_outputs = set()  # ... or those of these outputs only
        self.on_record = None   # called with the parsed launch record of the warm-up
        self.before_capture = None  # called once the warm-up is checked, directly in front of the capture
        self.keep = []

    def inp(self, versions):
        import torch

        stage = [torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1).copy()).cuda() for v in versions]
        t = torch.empty_like(stage[0])
        self.inputs.append((t, stage))
        return t

    def col(self, c, n, salt=0):
        return self.inp(packed(self.O, c, n, salt)), data(c, n, salt)

    def mask(self, n, salt=0):
        bits = mask_bits(n, salt)
        return self.inp([packbits(b) for b in bits]), bits

    def out(self, name, nbytes, want, prefill=None, small=False, constant=False):
        """want: per version, the bytes the buffer must hold after the call; prefill: what it holds before (default 0xEE)"""
        if constant:
            self.constant_outputs.add(name)
        import torch

        g = Guarded(nbytes, back=64, front=64) if small else Guarded(nbytes)
        pre = None
        if prefill is not None:
            pre = [torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1).copy()).cuda() for v in prefill]
        self.outputs[name] = (g, pre)
        for r in range(3):
            w = np.ascontiguousarray(want[r]).view(np.uint8).reshape(-1)
            assert w.size == nbytes, (name, w.size, nbytes)
            self.expect[r][name] = w
        return g

    def result(self, preds, n, prefill=None):
        """bitmap + hit count of a scan: -> (bitmap, hits)"""
        return (self.out("bitmap", nb(n), [packbits(p) for p in preds], prefill=prefill),
                self.out("hits", 8, [u64(p.sum()) for p in preds], small=True))

    def assert_distinct(self):
        if self.constant:
            return
        for name in set(self.outputs) - self.constant_outputs:
            for r in range(3):
                for s in range(r + 1, 3):
                    assert not np.array_equal(self.expect[r][name], self.expect[s][name]), f"{name}: versions {r} and {s} expect the same bytes"

    def load(self, r):
        for t, stage in self.inputs:
            t.copy_(stage[r])
        for g, pre in self.outputs.values():
            g.t.fill_(SENTINEL)
            if pre is not None:
                g.t[g.front: g.front + g.nbytes].copy_(pre[r])

    def untouched(self, r):
        for name, (g, pre) in self.outputs.items():
            got = g.fetch()
            same = (got == SENTINEL).all() if pre is None else np.array_equal(got, pre[r].cpu().numpy())
            assert same, f"{name}: written while the call was being captured -- it ran instead of being recorded"

    def check(self, r, what):
        for name, (g, _) in self.outputs.items():
            got = g.fetch()
            want = self.expect[r][name]
            if not np.array_equal(got, want):
                at = int(np.argmax(got != want))
                raise AssertionError(f"{what}, version {r}: {name} differs at byte {at} of {want.size}: {got[at]:#x}, expected {want[at]:#x}")


def all_ok(L, rcs):
    rcs = rcs if isinstance(rcs, (list, tuple)) else [rcs]
    assert all(rc == 0 for rc in rcs), (rcs, L.mi355_last_error())


def make_ctx(L, stream, opts=()):
    ctx = C.c_void_p()
    assert L.mi355_ctx_create(0, C.c_void_p(stream.cuda_stream), C.byref(ctx)) == 0, L.mi355_last_error()
    for name, value in opts:
        assert L.mi355_ctx_set_option(ctx, name.encode(), value) == 0, L.mi355_last_error()
    return ctx


def capture_replay(L, O, setup, opts=(), between=None):
    """capture.capture_replay over a Trial, versions 0, 1, 2.  setup(T) -> the call (a function that returns one status or a list
    of them); between(T, r): eager work on the same stream and context in front of replay r"""
    def steps(eng):
        T = Trial(L, O, eng._ctx)
        call = setup(T)
        T.assert_distinct()
        return capture.Steps(load=T.load, run=lambda: all_ok(L, call()), check=T.check, untouched=lambda: T.untouched(0),
                             warmed=lambda rec: T.on_record and T.on_record(rec), before_capture=lambda: T.before_capture and T.before_capture(),
                             between=between and (lambda r: between(T, r)))

    capture.capture_replay(steps, (0, 1, 2), opts)


# ---- the cases -------------------------------------------------------------------------------------------------------------
def needs_wide_grid(T):
    def on_record(rec):
        assert rec and rec[-1][1] >= MIN_SCAN_GRID, f"n = {N_SCAN} gives grid {rec[-1][1] if rec else None}: enlarge N_SCAN"
    T.on_record = on_record


def case_decompress(T, c):
    pk, vals = T.col(c, N_SCAN)
    out = T.out("values", 4 * N_SCAN, [v.view(np.int32) for v in vals])
    return lambda: T.L.mi355_decompress_dev(T.ctx, ptr(pk), N_SCAN, c, out.ptr)


def case_scan_eq(T, c):
    pk, vals = T.col(c, N_SCAN)
    key = hot_keys(c)[0]
    bm, hits = T.result([v == key for v in vals], N_SCAN)
    needs_wide_grid(T)
    return lambda: T.L.mi355_scan_eq_dev(T.ctx, ptr(pk), N_SCAN, c, i32(key), bm.ptr, hits.ptr)


def case_scan_range(T, c):
    pk, vals = T.col(c, N_SCAN)
    lo, hi = sorted(hot_keys(c)[1:3])
    bm, hits = T.result([(v >= lo) & (v <= hi) for v in vals], N_SCAN)
    needs_wide_grid(T)
    return lambda: T.L.mi355_scan_range_dev(T.ctx, ptr(pk), N_SCAN, c, lo, hi, bm.ptr, hits.ptr)


def case_scan_where(T, c, mode):
    pk, vals = T.col(c, N_SCAN)
    a = (1 << c) // 3
    p = [compare(v, LT, a) for v in vals]
    if mode == "plain":
        bm, hits = T.result(p, N_SCAN)
        return lambda: T.L.mi355_scan_where_dev(T.ctx, ptr(pk), N_SCAN, c, LT, a, 0, None, bm.ptr, hits.ptr)
    if mode == "mask":
        m, mb = T.mask(N_SCAN)
        bm, hits = T.result([x & y for x, y in zip(p, mb)], N_SCAN)
        return lambda: T.L.mi355_scan_where_dev(T.ctx, ptr(pk), N_SCAN, c, LT, a, 0, ptr(m), bm.ptr, hits.ptr)
    mb = mask_bits(N_SCAN)  # in place: the mask is the bitmap
    bm, hits = T.result([x & y for x, y in zip(p, mb)], N_SCAN, prefill=[packbits(b) for b in mb])
    return lambda: T.L.mi355_scan_where_dev(T.ctx, ptr(pk), N_SCAN, c, LT, a, 0, bm.ptr, bm.ptr, hits.ptr)


def case_scan_combine(T, c, mask_op):
    pk, vals = T.col(c, N_SCAN)
    lo, hi = hot_keys(c)[1], (1 << c) // 2
    p = [compare(v, BETWEEN, lo, hi) for v in vals]
    if mask_op == "count":  # bitmap_dev == NULL: nothing but the count is produced
        hits = T.out("hits", 8, [u64(x.sum()) for x in p], small=True)
        return lambda: T.L.mi355_scan_combine_dev(T.ctx, ptr(pk), N_SCAN, c, BETWEEN, lo, hi, AND, None, None, hits.ptr)
    m, mb = T.mask(N_SCAN)
    bm, hits = T.result([combine(x, y, mask_op) for x, y in zip(p, mb)], N_SCAN)
    return lambda: T.L.mi355_scan_combine_dev(T.ctx, ptr(pk), N_SCAN, c, BETWEEN, lo, hi, mask_op, ptr(m), bm.ptr, hits.ptr)


def shared_image(T, preds_per_version, n, P, layout, with_hits):
    """the output image of a shared scan (per-predicate: 16 guard bytes behind every bitmap) -> (out, stride, hits)"""
    stride = (nb(n) + 15) // 16 * 16 + 16
    want = []
    for preds in preds_per_version:
        if layout == 0:
            img = np.full((P, stride), SENTINEL, dtype=np.uint8)
            for k in range(P):
                img[k, : nb(n)] = packbits(preds[k])
        else:
            img = np.stack([packbits(preds[k]) for k in range(P)], axis=1)
        want.append(img)
    out = T.out("out", P * stride if layout == 0 else P * nb(n), want)
    hits = T.out("hits", 8 * P, [np.asarray([p.sum() for p in preds], dtype=np.uint64) for preds in preds_per_version], small=True) if with_hits else None
    return out, stride, hits


def case_shared_eq(T, c, P, layout, with_hits):
    n = N_SMALL
    pk, vals = T.col(c, n)
    keys = hot_keys(c)[:P]
    out, stride, hits = shared_image(T, [[v == k for k in keys] for v in vals], n, P, layout, with_hits)
    ka = key_array(keys)
    return lambda: T.L.mi355_shared_scan_eq_dev(T.ctx, ptr(pk), n, c, ka.ctypes.data_as(C.c_void_p), P, layout, out.ptr, stride,
                                                hits.ptr if hits else None)


def mixed_predicates(c, P):
    top, hot = 1 << c, hot_keys(c)
    eight = [(LT, top // 3, 0), (GE, hot[3], 0), (BETWEEN, hot[1], top // 2), (NE, hot[0], 0), (EQ, hot[2], 0),
             (NOT_BETWEEN, hot[2], top // 4), (LE, hot[4], 0), (GT, -5, 0)]
    return eight[:P] if P <= 8 else [eight[k % 8] if k < 8 else (LT, top // 3 + k, 0) for k in range(P)]


def predicate_array(preds):
    from shared_simd_scan_amd._capi import Predicate

    arr = (Predicate * len(preds))()
    for k, (op, a, b) in enumerate(preds):
        arr[k].op, arr[k].reserved, arr[k].a, arr[k].b = op, 0, a, b
    return arr


def case_shared_where(T, c, P, layout):
    n = N_SMALL
    pk, vals = T.col(c, n)
    preds = mixed_predicates(c, P)
    out, stride, hits = shared_image(T, [[compare(v, *p) for p in preds] for v in vals], n, P, layout, True)
    arr = predicate_array(preds)
    family = T.L.mi355_shared_where_kernel(T.ctx, c, P, layout, 1)
    assert family == (b"shared_where_lut_kernel" if c <= 16 else b"shared_where_chain_kernel"), family
    return lambda: T.L.mi355_shared_scan_where_dev(T.ctx, ptr(pk), n, c, C.cast(arr, C.c_void_p), P, layout, out.ptr, stride, hits.ptr)


def case_scan2(T, c1, c2, combine_op):
    pk1, v1 = T.col(c1, N_SCAN)
    pk2, v2 = T.col(c2, N_SCAN, salt=1)
    k1, a2 = hot_keys(c1)[0], (1 << c2) // 2
    # combine_op of scan2: AND p1 & p2, OR, XOR, ANDNOT p1 & ~p2
    want = [{AND: x & y, OR: x | y, XOR: x ^ y, ANDNOT: x & ~y}[combine_op] for x, y in zip([v == k1 for v in v1], [compare(v, LT, a2) for v in v2])]
    bm, hits = T.result(want, N_SCAN)

    def on_record(rec):
        assert len(rec) == (1 if c1 == c2 else 2), rec
    T.on_record = on_record
    return lambda: T.L.mi355_scan2_dev(T.ctx, ptr(pk1), c1, EQ, k1, 0, ptr(pk2), c2, LT, a2, 0, N_SCAN, combine_op, bm.ptr, hits.ptr)


SELECT_FIRST_ROW = 1000


def select_outputs(T, sel, cap):
    """rowids (capacity cap) and count of a selection over the per-version row sets `sel`"""
    want_ids = []
    for s in sel:
        ids = np.nonzero(s)[0].astype(np.uint64) + SELECT_FIRST_ROW
        img = np.full(8 * cap, SENTINEL, dtype=np.uint8)
        k = min(cap, len(ids))
        img[: 8 * k] = ids[:k].view(np.uint8)
        want_ids.append(img)
    return T.out("rowids", 8 * cap, want_ids), T.out("count", 8, [u64(s.sum()) for s in sel], small=True)


def capacity_for(counts, kind):
    """one capacity is frozen into the graph and the count differs per replay, so "eq" is the middle version's count: that replay
    fills the buffer to the last slot, the other two run one below and one above it (overflow and room to spare in one case)"""
    return {"lt": min(counts) // 2, "eq": sorted(counts)[1], "gt": max(counts) + 100}[kind]


def case_select(T, masked, capacity, chunks_per_block):
    n, c, a = N_SELECT, 9, 170
    pk, vals = T.col(c, n)
    sel = [compare(v, LT, a) for v in vals]
    m = None
    if masked:
        m, mb = T.mask(n)
        sel = [x & y for x, y in zip(sel, mb)]
    cap = capacity_for([int(s.sum()) for s in sel], capacity)
    ids, cnt = select_outputs(T, sel, cap)

    def on_record(rec):
        assert len(rec) == 1 and "select" in rec[0][0], rec
        if chunks_per_block:  # a grid of two blocks: each walks several generations of chunks
            assert rec[0][1] == 2, rec
    T.on_record = on_record
    return lambda: T.L.mi355_scan_select_dev(T.ctx, ptr(pk), n, c, LT, a, 0, AND, ptr(m) if m is not None else None, SELECT_FIRST_ROW,
                                             ids.ptr, cap, cnt.ptr)


def case_bitmap_combine(T, op, in_place):
    n = N_SCAN
    ab, bb = mask_bits(n), mask_bits(n, 1)
    want = [{AND: x & y, OR: x | y, XOR: x ^ y, ANDNOT: x & ~y}[op] for x, y in zip(ab, bb)]
    pre = {None: None, "a": [packbits(x) for x in ab], "b": [packbits(x) for x in bb]}[in_place]
    out = T.out("bitmap", nb(n), [packbits(w) for w in want], prefill=pre)
    cnt = T.out("count", 8, [u64(w.sum()) for w in want], small=True)
    a = out.ptr if in_place == "a" else ptr(T.inp([packbits(x) for x in ab]))
    b = out.ptr if in_place == "b" else ptr(T.inp([packbits(x) for x in bb]))
    return lambda: T.L.mi355_bitmap_combine_dev(T.ctx, op, a, b, out.ptr, n, cnt.ptr)


def case_bitmap_count(T):
    m, mb = T.mask(N_SCAN)
    cnt = T.out("count", 8, [u64(x.sum()) for x in mb], small=True)
    return lambda: T.L.mi355_bitmap_count_dev(T.ctx, ptr(m), N_SCAN, cnt.ptr)


def case_bitmap_to_rowids(T):
    m, mb = T.mask(N_SCAN)
    cap = capacity_for([int(x.sum()) for x in mb], "eq")
    ids, cnt = select_outputs(T, mb, cap)
    return lambda: T.L.mi355_bitmap_to_rowids_dev(T.ctx, ptr(m), N_SCAN, SELECT_FIRST_ROW, ids.ptr, cap, cnt.ptr)


def case_gather(T, c):
    n, cap, first = N_SCAN, 3000, 1000
    pk, vals = T.col(c, n)
    counts = [cap, 0, 1234]  # read on the device at every replay
    rows, want = [], []
    for r in range(3):
        ids = np.random.default_rng([c, r, 5]).integers(0, n, cap).astype(np.uint64) + first
        ids[7], ids[1100] = first - 1, first + n  # outside the column on either side: -1
        got = np.where((ids >= first) & (ids < first + n), vals[r][np.clip(ids.astype(np.int64) - first, 0, n - 1)].astype(np.int64), -1).astype(np.int32)
        img = np.full(4 * cap, SENTINEL, dtype=np.uint8)
        img[: 4 * counts[r]] = got[: counts[r]].view(np.uint8)
        rows.append(ids)
        want.append(img)
    drows, dcnt = T.inp(rows), T.inp([u64(k) for k in counts])
    out = T.out("values", 4 * cap, want)
    return lambda: T.L.mi355_gather_dev(T.ctx, ptr(pk), n, c, first, ptr(drows), ptr(dcnt), cap, out.ptr)


def aggregate_of(v, sel):
    v = v.astype(np.uint64)[sel]
    return np.asarray([v.sum(), len(v), v.min() if len(v) else np.iinfo(np.uint64).max, v.max() if len(v) else 0], dtype=np.uint64)


def case_aggregate(T, c, masked):
    pk, vals = T.col(c, N_SCAN)
    m, mb = T.mask(N_SCAN) if masked else (None, [slice(None)] * 3)
    out = T.out("aggregate", 32, [aggregate_of(v, s) for v, s in zip(vals, mb)], small=True)
    return lambda: T.L.mi355_aggregate_dev(T.ctx, ptr(pk), N_SCAN, c, ptr(m) if masked else None, out.ptr)


def case_histogram(T, masked):
    c = 9
    pk, vals = T.col(c, N_SCAN)
    m, mb = T.mask(N_SCAN) if masked else (None, [slice(None)] * 3)
    out = T.out("counts", 8 << c, [np.bincount(v[s], minlength=1 << c).astype(np.uint64) for v, s in zip(vals, mb)])
    return lambda: T.L.mi355_histogram_dev(T.ctx, ptr(pk), N_SCAN, c, ptr(m) if masked else None, out.ptr)


def case_pack(T, bits):
    c = {16: 9, 32: 17}[bits]
    n = N_SMALL
    while T.L.mi355_compressed_buffer_size(c, n) % 4 == 0:  # the trailing 1 - 3 pad bytes are a memset node of their own
        n += 1
    assert n < N_SMALL + 8
    vals = data(c, n)
    src = T.inp([v.astype(np.uint16 if bits == 16 else np.uint32) for v in vals])
    out = T.out("packed", T.L.mi355_compressed_buffer_size(c, n), [T.O.pack(v, c) for v in vals])
    fn = T.L.mi355_pack_u16_dev if bits == 16 else T.L.mi355_pack_u32_dev
    return lambda: fn(T.ctx, ptr(src), n, c, out.ptr)


def case_generate(T):
    n, c, seed = N_SMALL, 9, 42
    T.constant = True  # kind, first_row and param are arguments: frozen with the capture
    image = T.O.pack(T.O.gen_values("splitmix", n, c, seed), c)
    out = T.out("packed", T.L.mi355_compressed_buffer_size(c, n), [image] * 3)
    return lambda: T.L.mi355_generate_dev(T.ctx, 1, 0, n, c, seed, out.ptr)


def case_dev_memset(T):
    T.constant = True
    out = T.out("bytes", 1003, [np.full(1003, 0x5A, dtype=np.uint8)] * 3)
    return lambda: T.L.mi355_dev_memset(T.ctx, out.ptr, 0x5A, 1003)


def case_n0_forms(T):
    """calls that only enqueue a memset (or, aggregate, a one-thread kernel): n = 0, and the empty range lo > hi"""
    T.constant = True
    L, ctx = T.L, T.ctx
    zero = [u64(0)] * 3
    h = {name: T.out(name, 8, zero, small=True) for name in ("eq", "range", "combine", "in", "scan2", "select", "rowids", "count", "empty_hits")}
    shared = T.out("shared", 24, [np.zeros(3, dtype=np.uint64)] * 3, small=True)
    where = T.out("where", 24, [np.zeros(3, dtype=np.uint64)] * 3, small=True)
    hist = T.out("hist", 8 << 9, [np.zeros(1 << 9, dtype=np.uint64)] * 3)
    agg = T.out("agg", 32, [np.asarray([0, 0, np.iinfo(np.uint64).max, 0], dtype=np.uint64)] * 3, small=True)
    n_empty = N_SMALL
    empty = T.out("empty_bitmap", nb(n_empty), [np.zeros(nb(n_empty), dtype=np.uint8)] * 3)
    ka = key_array([1, 2, 3])
    kp = ka.ctypes.data_as(C.c_void_p)
    arr = predicate_array(mixed_predicates(9, 3))
    return lambda: [
        L.mi355_scan_eq_dev(ctx, None, 0, 9, 5, None, h["eq"].ptr),
        L.mi355_scan_range_dev(ctx, None, 0, 9, 1, 5, None, h["range"].ptr),
        L.mi355_scan_range_dev(ctx, None, n_empty, 9, 7, 3, empty.ptr, h["empty_hits"].ptr),
        L.mi355_scan_combine_dev(ctx, None, 0, 9, LT, 5, 0, AND, None, None, h["combine"].ptr),
        L.mi355_scan_in_dev(ctx, None, 0, 9, kp, 3, 0, None, None, h["in"].ptr),
        L.mi355_scan2_dev(ctx, None, 9, EQ, 1, 0, None, 12, EQ, 1, 0, 0, AND, None, h["scan2"].ptr),
        L.mi355_scan_select_dev(ctx, None, 0, 9, LT, 5, 0, AND, None, 0, None, 0, h["select"].ptr),
        L.mi355_bitmap_to_rowids_dev(ctx, None, 0, 0, None, 0, h["rowids"].ptr),
        L.mi355_bitmap_count_dev(ctx, None, 0, h["count"].ptr),
        L.mi355_shared_scan_eq_dev(ctx, None, 0, 9, kp, 3, 0, None, 0, shared.ptr),
        L.mi355_shared_scan_where_dev(ctx, None, 0, 9, C.cast(arr, C.c_void_p), 3, 0, None, 0, where.ptr),
        L.mi355_histogram_dev(ctx, None, 0, 9, None, hist.ptr),
        L.mi355_aggregate_dev(ctx, None, 0, 9, None, agg.ptr),
    ]


SMALL_GRID = (("grid_cus", 2), ("max_blocks_per_cu", 1))
MASK_OPS = {"and": AND, "or": OR, "xor": XOR, "andnot": ANDNOT}
# id -> (setup, keyword arguments, context options)
CAPTURE_CASES = {}


def _case(cid, fn, opts=(), **kw):
    assert cid not in CAPTURE_CASES, cid
    CAPTURE_CASES[cid] = (fn, kw, opts)


for _c in (1, 9, 17, 32):
    _case(f"decompress-c{_c}", case_decompress, c=_c)
    _case(f"scan_eq-c{_c}", case_scan_eq, c=_c)
for _c in (9, 17):  # both tile geometries; byte-table / bitset kernels and compare chains
    _case(f"scan_range-c{_c}", case_scan_range, c=_c)
    for _mode in ("plain", "mask", "inplace"):
        _case(f"scan_where-c{_c}-{_mode}", case_scan_where, c=_c, mode=_mode)
    for _name, _op in MASK_OPS.items():
        _case(f"scan_combine-c{_c}-{_name}", case_scan_combine, c=_c, mask_op=_op)
    _case(f"scan_combine-c{_c}-count", case_scan_combine, c=_c, mask_op="count")
    for _P in (1, 2, 3, 8):
        for _lay in (0, 1):
            for _hits in (True, False):
                _case(f"shared_eq-c{_c}-P{_P}-{'lin' if _lay else 'pp'}-{'hits' if _hits else 'nohits'}", case_shared_eq, c=_c, P=_P, layout=_lay,
                      with_hits=_hits)
    for _P in (2, 8):
        for _lay in (0, 1):
            _case(f"shared_where-c{_c}-P{_P}-{'lin' if _lay else 'pp'}", case_shared_where, c=_c, P=_P, layout=_lay)
    _case(f"scan2-same-c{_c}", case_scan2, c1=_c, c2=_c, combine_op=AND)
    _case(f"gather-c{_c}", case_gather, c=_c)
    for _masked in (True, False):
        _case(f"aggregate-c{_c}-{'mask' if _masked else 'nomask'}", case_aggregate, c=_c, masked=_masked)
_case("scan2-9+12", case_scan2, c1=9, c2=12, combine_op=OR)
for _single in (0, 1):
    for _masked in (True, False):
        for _cap in ("lt", "eq", "gt"):
            for _small in (False, True):
                _case(f"select-{'single' if _single else 'select2'}-{'mask' if _masked else 'nomask'}-{_cap}-{'small_grid' if _small else 'full_grid'}",
                      case_select, opts=(("select_kernel", _single),) + (SMALL_GRID if _small else ()), masked=_masked, capacity=_cap,
                      chunks_per_block=_small)
for _name, _op in MASK_OPS.items():
    _case(f"bitmap_combine-{_name}", case_bitmap_combine, op=_op, in_place=None)
_case("bitmap_combine-and-in_a", case_bitmap_combine, op=AND, in_place="a")
_case("bitmap_combine-andnot-in_b", case_bitmap_combine, op=ANDNOT, in_place="b")
_case("bitmap_count", case_bitmap_count)
_case("bitmap_to_rowids", case_bitmap_to_rowids)
for _masked in (True, False):
    _case(f"histogram-{'mask' if _masked else 'nomask'}", case_histogram, masked=_masked)
_case("pack_u16", case_pack, bits=16)
_case("pack_u32", case_pack, bits=32)
_case("generate", case_generate)
_case("dev_memset", case_dev_memset)
_case("n0_forms", case_n0_forms)


# differs from support.L: says why when there is no GPU, and a missing library is an error
@pytest.fixture(scope="module")
def L():
    import torch

    from shared_simd_scan_amd import lib

    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return lib()


@gpu
@pytest.mark.parametrize("cid", list(CAPTURE_CASES))
def test_capture_replay(L, O, cid):
    fn, kw, opts = CAPTURE_CASES[cid]
    capture_replay(L, O, lambda T: fn(T, **kw), opts)


# ---- a query pipeline in one graph -----------------------------------------------------------------------------------------
PIPE_N, PIPE_C1, PIPE_C2, PIPE_SEED, PIPE_LT, PIPE_CAP = N_SELECT, 9, 17, 42, 300, 16384
PIPE_LO, PIPE_HI = 40, 47  # the IN-list call cannot be captured (every key list is uploaded): its place is taken by a range, in place on the mask


def pipeline_expectations(O):
    """generate col1 -> bm = (col1 < 300) & mask -> bm &= col1 BETWEEN lo AND hi -> row ids of bm -> take col2 at them -> aggregate col2 under bm.
    col1's generator arguments travel by value (frozen with the capture); the mask and col2 are rewritten between replays."""
    v1 = O.gen_values("splitmix", PIPE_N, PIPE_C1, PIPE_SEED).astype(np.uint32)
    v2, mb = data(PIPE_C2, PIPE_N), mask_bits(PIPE_N)
    out = []
    for r in range(3):
        sel = compare(v1, LT, PIPE_LT) & mb[r] & compare(v1, BETWEEN, PIPE_LO, PIPE_HI)
        ids = np.nonzero(sel)[0].astype(np.uint64)
        assert 0 < len(ids) < PIPE_CAP
        out.append({"bitmap": packbits(sel), "hits": len(ids), "ids": ids, "taken": v2[r][ids.astype(np.int64)].astype(np.int32),
                    "aggregate": aggregate_of(v2[r], sel)})
    return O.pack(v1, PIPE_C1), out


@gpu
def test_captured_pipeline(L, O):
    """through the C ABI"""
    col1_image, want = pipeline_expectations(O)
    n, cap = PIPE_N, PIPE_CAP

    def setup(T):
        m, _ = T.mask(n)
        pk2, _ = T.col(PIPE_C2, n)
        col1 = T.out("col1", L.mi355_compressed_buffer_size(PIPE_C1, n), [col1_image] * 3, constant=True)
        bm = T.out("bitmap", nb(n), [w["bitmap"] for w in want])
        hits = T.out("hits", 8, [u64(w["hits"]) for w in want], small=True)
        ids_img, taken_img = [], []
        for w in want:
            a, b = np.full(8 * cap, SENTINEL, dtype=np.uint8), np.full(4 * cap, SENTINEL, dtype=np.uint8)
            a[: 8 * len(w["ids"])] = w["ids"].view(np.uint8)
            b[: 4 * len(w["ids"])] = w["taken"].view(np.uint8)
            ids_img.append(a)
            taken_img.append(b)
        ids, cnt = T.out("rowids", 8 * cap, ids_img), T.out("count", 8, [u64(w["hits"]) for w in want], small=True)
        taken = T.out("taken", 4 * cap, taken_img)
        agg = T.out("aggregate", 32, [w["aggregate"] for w in want], small=True)
        return lambda: [
            L.mi355_generate_dev(T.ctx, 1, 0, n, PIPE_C1, PIPE_SEED, col1.ptr),
            L.mi355_scan_where_dev(T.ctx, col1.ptr, n, PIPE_C1, LT, PIPE_LT, 0, ptr(m), bm.ptr, None),
            L.mi355_scan_where_dev(T.ctx, col1.ptr, n, PIPE_C1, BETWEEN, PIPE_LO, PIPE_HI, bm.ptr, bm.ptr, hits.ptr),
            L.mi355_scan_select_dev(T.ctx, col1.ptr, n, PIPE_C1, GE, 0, 0, AND, bm.ptr, 0, ids.ptr, cap, cnt.ptr),
            L.mi355_gather_dev(T.ctx, ptr(pk2), n, PIPE_C2, 0, ids.ptr, cnt.ptr, cap, taken.ptr),
            L.mi355_aggregate_dev(T.ctx, ptr(pk2), n, PIPE_C2, bm.ptr, agg.ptr),
        ]

    capture_replay(L, O, setup)


# not capture.capture_replay: most outputs are allocated inside the capture, so only `hits` can show "untouched", and the eager ones are refilled by hand
@gpu
def test_captured_pipeline_through_the_engine(L, O):
    """the same pipeline through ScanEngine; outputs a method offers no argument for are allocated inside torch.cuda.graph"""
    import torch

    from shared_simd_scan_amd import ScanEngine
    from shared_simd_scan_amd.engine import PackedColumn

    col1_image, want = pipeline_expectations(O)
    n, cap = PIPE_N, PIPE_CAP
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eng = ScanEngine(0, stream=side)
        g = None
        try:
            stage_m = [torch.from_numpy(packbits(b)).cuda() for b in mask_bits(n)]
            stage_2 = [torch.from_numpy(p).cuda() for p in packed(O, PIPE_C2, n)]
            m, col2 = torch.empty_like(stage_m[0]), PackedColumn(torch.empty_like(stage_2[0]), n, PIPE_C2)
            hits = torch.empty(1, dtype=torch.int64, device="cuda")

            def run():
                col1 = eng.generate("splitmix", n, PIPE_C1, PIPE_SEED)
                bm, _ = eng.scan_where("<", PIPE_LT, col1, and_mask=m)
                eng.scan_where("between", PIPE_LO, col1, b=PIPE_HI, and_mask=bm, bitmap=bm, hits=hits)
                ids, cnt = eng.scan_select(">=", 0, col1, cap, mask=bm)
                taken = eng.gather(col2, ids, cnt)
                return {"col1": col1.data, "bitmap": bm, "hits": hits, "rowids": ids, "count": cnt, "taken": taken, "aggregate": eng.aggregate(col2, mask=bm)}

            def check(out, w, what):
                k = len(w["ids"])
                assert np.array_equal(out["col1"].cpu().numpy(), col1_image), what
                assert np.array_equal(out["bitmap"].cpu().numpy(), w["bitmap"]), what
                assert int(out["hits"].item()) == k and int(out["count"].item()) == k, what
                assert np.array_equal(out["rowids"].cpu().numpy()[:k].view(np.uint64), w["ids"]), what
                assert (out["rowids"].cpu().numpy()[k:].view(np.uint8) == SENTINEL).all(), what
                assert np.array_equal(out["taken"].cpu().numpy()[:k], w["taken"]), what
                assert (out["taken"].cpu().numpy()[k:].view(np.uint8) == SENTINEL).all(), what
                assert np.array_equal(out["aggregate"].cpu().numpy().view(np.uint64), w["aggregate"]), what

            m.copy_(stage_m[0])
            col2.data.copy_(stage_2[0])
            eager = run()
            for k in ("rowids", "taken"):  # torch.empty: only [0, count) is defined after an eager call
                eager[k][len(want[0]["ids"]):].view(torch.uint8).fill_(SENTINEL)
            check(eager, want[0], "eager warm-up")
            hits.view(torch.uint8).fill_(SENTINEL)  # the one output that exists before the capture: it shows that nothing ran
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                out = run()
            side.synchronize()
            assert (hits.cpu().numpy().view(np.uint8) == SENTINEL).all(), "written while being captured: the pipeline ran instead of being recorded"
            for t in out.values():
                t.view(torch.uint8).fill_(SENTINEL)
            side.synchronize()
            for r in range(3):
                m.copy_(stage_m[r])
                col2.data.copy_(stage_2[r])
                for t in out.values():
                    t.view(torch.uint8).fill_(SENTINEL)
                g.replay()
                side.synchronize()
                check(out, want[r], f"replay {r}")
        finally:
            side.synchronize()
            del g
            eng.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_keep_the_capture_alive(L, O):
    """what cannot be captured says so (MI355_E_INVALID, a message that names graph capture), enqueues nothing and leaves the
    capture intact: the plain scan around the refused calls replays exactly"""
    import torch

    n, c = N_SMALL, 9
    big_n = N_SELECT  # larger than anything the context has seen: workspace / pool would have to grow
    tune_n = 50_000_000

    def setup(T):
        pk, vals = T.col(c, n)
        key = hot_keys(c)[0]
        bm, hits = T.result([v == key for v in vals], n)
        stride = (nb(n) + 15) // 16 * 16
        pk17, _ = T.col(17, n, salt=2)
        refused = {name: Guarded(size) for name, size in (("shared_eq", 9 * stride), ("scan_in", nb(n)), ("where", 9 * stride), ("where_eq", 9 * stride),
                                                          ("rowids", 8 * 1024), ("count", 64), ("bitmap", nb(big_n)))}
        big9 = torch.zeros(L.mi355_compressed_buffer_size(9, big_n), dtype=torch.uint8, device="cuda")
        big12 = torch.zeros(L.mi355_compressed_buffer_size(12, big_n), dtype=torch.uint8, device="cuda")
        tune_col = torch.zeros(L.mi355_compressed_buffer_size(1, tune_n), dtype=torch.uint8, device="cuda")
        k9 = key_array(list(range(9)))
        kp = k9.ctypes.data_as(C.c_void_p)
        mixed, all_eq = predicate_array(mixed_predicates(c, 9)), predicate_array([(EQ, k, 0) for k in range(9)])
        T.keep += [big9, big12, tune_col, refused]
        state = {"capturing": False, "messages": {}}

        def refusals():
            R = refused
            return {
                "shared_scan_eq P=9": lambda: L.mi355_shared_scan_eq_dev(T.ctx, ptr(pk), n, c, kp, 9, 0, R["shared_eq"].ptr, stride, None),
                "scan_in P=9": lambda: L.mi355_scan_in_dev(T.ctx, ptr(pk), n, c, kp, 9, 0, None, R["scan_in"].ptr, None),
                # every key list of the IN-list call is uploaded: short lists too, both kernel families (c = 9 bitset, c = 17 chain),
                # plain / negated / in place on the mask
                **{f"scan_in c={w} P={P} {mode}": (lambda col=col, w=w, P=P, mode=mode: L.mi355_scan_in_dev(
                    T.ctx, ptr(col), n, w, kp, P, int(mode == "negate"), R["scan_in"].ptr if mode == "inplace" else None, R["scan_in"].ptr,
                    R["count"].ptr))
                   for w, col in ((9, pk), (17, pk17)) for P in (1, 3, 8) for mode in ("plain", "negate", "inplace")},
                "shared_scan_where P=9 mixed": lambda: L.mi355_shared_scan_where_dev(T.ctx, ptr(pk), n, c, C.cast(mixed, C.c_void_p), 9, 0,
                                                                                     R["where"].ptr, stride, None),
                "shared_scan_where P=9 all EQ": lambda: L.mi355_shared_scan_where_dev(T.ctx, ptr(pk), n, c, C.cast(all_eq, C.c_void_p), 9, 0,
                                                                                      R["where_eq"].ptr, stride, None),
                "tune": lambda: L.mi355_tune_dev(T.ctx, ptr(tune_col), tune_n, 1, 1),
                "scan_select, workspace must grow": lambda: L.mi355_scan_select_dev(T.ctx, ptr(big9), big_n, 9, LT, 5, 0, AND, None, 0, R["rowids"].ptr,
                                                                                    1024, R["count"].ptr),
                "bitmap_to_rowids, workspace must grow": lambda: L.mi355_bitmap_to_rowids_dev(T.ctx, R["bitmap"].ptr, big_n, 0, R["rowids"].ptr, 1024,
                                                                                              R["count"].ptr),
                "scan2, pool must grow": lambda: L.mi355_scan2_dev(T.ctx, ptr(big9), 9, LT, 5, 0, ptr(big12), 12, LT, 5, 0, big_n, AND, None,
                                                                   R["count"].ptr),
            }

        def call():
            rcs = [L.mi355_scan_eq_dev(T.ctx, ptr(pk), n, c, key, bm.ptr, None)]
            if state["capturing"]:  # never eagerly: tune would measure, the others would grow the context
                for what, fn in refusals().items():
                    rc = fn()
                    state["messages"][what] = (rc, (L.mi355_last_error() or b"").decode())
            rcs.append(L.mi355_bitmap_count_dev(T.ctx, bm.ptr, n, hits.ptr))
            return rcs

        def before_capture():
            state["capturing"] = True  # the next call() is the captured one: it tries the refusals too
        T.before_capture = before_capture
        T.state = state
        T.refused = refused
        return call

    holder = {}

    def setup_and_keep(T):
        holder["T"] = T
        return setup(T)

    capture_replay(L, O, setup_and_keep)
    T = holder["T"]
    assert len(T.state["messages"]) == 8 + 18
    for what, (rc, msg) in T.state["messages"].items():
        assert rc == E_INVALID, f"{what}: status {rc} ({msg})"
        assert "graph" in msg and "captur" in msg, f"{what}: the message does not name graph capture: {msg!r}"
    for name, g in T.refused.items():
        assert (g.fetch() == SENTINEL).all(), f"{name}: a refused call wrote to its output"


# ---- a graph and the context's own memory --------------------------------------------------------------------------------
@gpu
def test_graph_survives_workspace_growth(L, O):
    """a captured selection keeps the address of the context's look-back workspace, a captured two-width count-only scan2 the
    address of a pool slot: an eager call that makes either grow must not free what the graph points at (it is retired until
    mi355_ctx_destroy).  The eager call runs in front of every replay: its own result and the replay's are exact."""
    import torch

    class Eng:  # what check_select needs of an engine
        def __init__(self, ctx, stream):
            self._ctx, self.stream = ctx, stream

        def synchronize(self):
            self.stream.synchronize()

    big = Case("big", "select", (), c=9, n=4 * N_SELECT)
    big_vals, _ = column(big, np.random.default_rng(11))
    big12 = np.random.default_rng(12).integers(0, 1 << 12, big.n).astype(np.uint32)

    def select_between(T, r):
        if r == 0:
            T.big = torch.from_numpy(O.pack(big_vals, 9)).cuda()
        check_select(L, Eng(T.ctx, torch.cuda.current_stream()), T.big, big_vals, big.n, 9, 2, 170, "gt")

    capture_replay(L, O, lambda T: case_select(T, masked=True, capacity="gt", chunks_per_block=False), between=select_between)

    def scan2_count_only(T):
        n = N_SMALL
        pk1, v1 = T.col(9, n)
        pk2, v2 = T.col(12, n, salt=1)
        want = [compare(x, LT, 170) & compare(y, GE, 100) for x, y in zip(v1, v2)]
        hits = T.out("hits", 8, [u64(w.sum()) for w in want], small=True)
        return lambda: L.mi355_scan2_dev(T.ctx, ptr(pk1), 9, LT, 170, 0, ptr(pk2), 12, GE, 100, 0, n, AND, None, hits.ptr)

    def scan2_between(T, r):
        if r == 0:
            T.big = torch.from_numpy(O.pack(big_vals, 9)).cuda(), torch.from_numpy(O.pack(big12, 12)).cuda()
            T.big_hits = Guarded(8, back=64, front=64)
        rows = big.n if r == 0 else big.n // 2  # the pool grows in front of replay 0 only
        T.big_hits.t.fill_(SENTINEL)
        all_ok(L, L.mi355_scan2_dev(T.ctx, ptr(T.big[0]), 9, LT, 170, 0, ptr(T.big[1]), 12, GE, 100, 0, rows, AND, None, T.big_hits.ptr))
        torch.cuda.current_stream().synchronize()
        assert int(T.big_hits.fetch().view(np.uint64)[0]) == int((compare(big_vals[:rows], LT, 170) & compare(big12[:rows], GE, 100)).sum())

    capture_replay(L, O, scan2_count_only, between=scan2_between)


@gpu
def test_replays_interleave_with_eager_calls(L, O):
    """the shared hit-count scratch and the key ring serve eager calls between the replays of a graph that uses the scratch"""
    import torch

    n, c = N_SMALL, 9
    other = Case("other", "shared", (), c=c, n=n, P=40)
    other_vals, other_keys = column(other, np.random.default_rng(3))

    def setup(T):
        call = case_shared_eq(T, c, 8, 0, True)
        first = T.outputs["out"][0]
        cnt = T.out("first_count", 8, [T.expect[r]["hits"].view(np.uint64)[:1] for r in range(3)], small=True)
        return lambda: [call(), L.mi355_bitmap_count_dev(T.ctx, first.ptr, n, cnt.ptr)]

    def between(T, r):
        if r == 0:
            T.other = torch.from_numpy(O.pack(other_vals, c)).cuda()
        stride = int(L.mi355_bitmap_stride(n))
        out, hits, cnt = Guarded(40 * stride), Guarded(8 * 40, back=64, front=64), Guarded(8, back=64, front=64)
        ka = key_array(other_keys[r:] + other_keys[:r])  # other keys every time: the ring moves on
        keys = ka.view(np.uint32).tolist()
        all_ok(L, [L.mi355_shared_scan_eq_dev(T.ctx, ptr(T.other), n, c, ka.ctypes.data_as(C.c_void_p), 40, 0, out.ptr, stride, hits.ptr),
                   L.mi355_bitmap_count_dev(T.ctx, out.ptr, n, cnt.ptr)])
        torch.cuda.current_stream().synchronize()
        img = out.fetch().reshape(40, stride)
        for k, key in enumerate(keys):
            assert np.array_equal(img[k, : nb(n)], packbits(other_vals == key)), f"eager shared scan in front of replay {r}: bitmap {k}"
        assert hits.fetch().view(np.uint64).tolist() == [int((other_vals == key).sum()) for key in keys]
        assert int(cnt.fetch().view(np.uint64)[0]) == int((other_vals == keys[0]).sum())

    capture_replay(L, O, setup, between=between)


# not capture.capture_replay: an eager pair in front of the capture, two calls whose divisors are read inside it, eager scans between it and the replays
@gpu
def test_llc_decision_is_frozen_at_capture(L):
    """The recorded scan (csrc/llc_repeat.hpp) after a captured call.  It describes the launch that RUNS directly before the next one.  Inside one capture
    that is the call captured before it -- a graph replays its nodes in capture order -- so the second of two identical captured
    scans is a repeat and gets the divisor an eager pair gets, frozen into the node.  A captured call has not run when its capture
    ends, and the context never learns when its graph does: across the boundary of a capture nothing is a repeat -- not the first
    captured call after an identical eager one, not an eager scan after the capture, of another column or of the same."""
    import torch

    n, c, key = 56_000_077, 32, 3  # 213.6 MiB of column + 6.7 MiB of bitmap: more than the auto budget of 205 MiB holds, so a repeat gets D = 3
    moduli = (5, 7, 11)            # column version r: v[i] = i % moduli[r]

    def expected(p):
        period = np.packbits((np.arange(8 * p) % p) == key, bitorder="little")  # the bitmap repeats every p bytes
        bm = np.tile(period, nb(n) // p + 1)[: nb(n)].copy()
        bm[-1] &= (1 << (n % 8)) - 1 if n % 8 else 0xFF
        return bm, (n - key + p - 1) // p

    want = [expected(p) for p in moduli]
    assert len({w[1] for w in want}) == 3
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ctx = make_ctx(L, side)
        g = None
        try:
            size = L.mi355_compressed_buffer_size(c, n)
            col, other = (torch.empty(size, dtype=torch.uint8, device="cuda") for _ in range(2))
            bm, hits = Guarded(nb(n)), Guarded(8, back=64, front=64)

            def generate(t, p):
                all_ok(L, L.mi355_generate_dev(ctx, 0, 0, n, c, p, ptr(t)))

            def scan(t):
                all_ok(L, L.mi355_scan_eq_dev(ctx, ptr(t), n, c, key, bm.ptr, hits.ptr))
                return L.mi355_ctx_last_llc_divisor(ctx)

            def check(r, what):
                side.synchronize()
                assert np.array_equal(bm.fetch(), want[r][0]), f"{what}: bitmap differs"
                assert int(hits.fetch().view(np.uint64)[0]) == want[r][1], f"{what}: hit count differs"

            generate(col, moduli[0])
            generate(other, moduli[1])
            assert scan(col) == 0
            d = scan(col)
            assert d == 3, d  # -(-column // (205 MiB - bitmap)) | 1
            check(0, "eager pair")
            bm.t.fill_(SENTINEL)
            hits.t.fill_(SENTINEL)
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                first = scan(col)
                second = scan(col)
            assert first == 0, "the first call of a capture is no repeat of the eager call before it"
            assert second == d, "the second identical call of a capture is a repeat: it runs directly behind the first"
            side.synchronize()
            assert (bm.fetch() == SENTINEL).all() and (hits.fetch() == SENTINEL).all(), "the scans ran instead of being recorded"
            assert scan(col) == 0, "an eager scan after the capture is no repeat of the captured call: that has not run"
            assert scan(col) == d
            check(0, "eager scans after the capture")
            assert scan(other) == 0, "an eager scan of another column"
            check(1, "eager scan of the other column")
            for r in range(3):
                generate(col, moduli[r])
                bm.t.fill_(SENTINEL)
                hits.t.fill_(SENTINEL)
                g.replay()
                check(r, f"replay {r}")
        finally:
            side.synchronize()
            del g
            L.mi355_ctx_destroy(ctx)
