"""GPU (-m gpu): predicate constants at the limits of their types, against numpy on the decoded values.

Every width 1..32 gets a column of about two scan tiles and a ragged tail that holds the domain's edge values (0, 1,
2^(c-1) - 1, 2^(c-1), vmax - 1, vmax) at a lane's first value, straddling a dword and in the last rows, runs of vmax
(all-ones words) and random values.  Every comparison, range, key list and two-column predicate then runs with constants
at the int64 / int32 / uint32 limits and just outside the column's domain.  The reference is numpy on the values in exact
integer arithmetic; the only thing done to a constant first is a clamp to [-1, 2^32], which changes no comparison with a
value in [0, 2^32).

Also here: the int64 limits through the C ABI directly (the Python wrappers clamp them away), the in-place forms (mask and
result bitmap the same buffer, with several store bursts per wave), and the aggregate over columns of nothing but vmax.
Launches are batched into preallocated result slots (bitmaps at mi355_bitmap_stride inside 0xEE guard bytes) and copied
back once per width.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
OPS1 = ("==", "!=", "<", "<=", ">", ">=")
CMP = {"==": 0, "!=": 1, "<": 2, "<=": 3, ">": 4, ">=": 5, "between": 6, "not_between": 7}
MASK_OPS = {"and": lambda p, m: p & m, "or": lambda p, m: p | m, "xor": lambda p, m: p ^ m, "andnot": lambda p, m: m & ~p}
COMBINE = {"and": lambda p1, p2: p1 & p2, "or": lambda p1, p2: p1 | p2, "xor": lambda p1, p2: p1 ^ p2,
           "andnot": lambda p1, p2: p1 & ~p2}
BOP = {"and": 0, "or": 1, "xor": 2, "andnot": 3}


def np_bitmap(mask_bool):
    return np.packbits(mask_bool.astype(np.uint8), bitorder="little")


def ref_const(x):
    """the one transformation the reference applies to a constant: exact for every value in [0, 2^32)"""
    return min(max(int(x), -1), 1 << 32)


def expect_cmp(v, op, a, b=0):
    """v: int64 decoded values"""
    a, b = ref_const(a), ref_const(b)
    if op == "between":
        return (v >= a) & (v <= b)
    if op == "not_between":
        return (v < a) | (v > b)
    return {"==": v == a, "!=": v != a, "<": v < a, "<=": v <= a, ">": v > a, ">=": v >= a}[op]


def expect_key(v, k, c):
    """equality with an int32-expressible key: at c = 32 the key's unsigned pattern is the value it matches"""
    if c == 32 and -(1 << 31) <= k < 0:
        k += 1 << 32
    return v == ref_const(k)


def abi_constants(c, inside):
    """every constant the C ABI (int64) can take"""
    vmax = (1 << c) - 1
    cs = [INT64_MIN, -(1 << 32) - 1, -(1 << 31) - 1, -(1 << 31), -1, 0, 1, 1 << (c - 1), vmax - 1, vmax, vmax + 1,
          (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, INT64_MAX, inside]
    return list(dict.fromkeys(cs))


def py_constants(c, inside):
    """... and the two only a Python caller can pass"""
    return abi_constants(c, inside) + [(1 << 64) + 5, INT64_MIN - 1]


def reduced_constants(c, inside):
    vmax = (1 << c) - 1
    return list(dict.fromkeys([INT64_MIN, -1, 0, 1 << (c - 1), inside, vmax - 1, vmax, vmax + 1, 1 << 32, INT64_MAX]))


def key_ok(k, c):
    """a key the Python wrappers accept at width c (at c = 32 only [-2^31, 2^32))"""
    return c < 32 or -(1 << 31) <= k < 1 << 32


def tile_rows(c):
    return 8192 if c <= 16 else 4096


def n_rows(c):
    return tile_rows(c) * (2 if c <= 16 else 4) + 77


def edge_values(c, n, seed):
    """random values plus the domain's edges at the places a decoder gets them wrong"""
    vmax = (1 << c) - 1
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 1 << c, size=n, dtype=np.uint64)
    special = [0, 1, (1 << (c - 1)) - 1, 1 << (c - 1), vmax - 1, vmax]
    vpl = 128 if c <= 16 else 64
    for t in (0, 1):  # a lane's first value (odd lanes), in the first two tiles
        for j, s in enumerate(special):
            v[t * tile_rows(c) + (2 * j + 1) * vpl] = s
    straddle = [i for i in range(3001, 3001 + 128) if (c * i) % 32 + c > 32][:len(special)]  # empty where c divides 32
    for i, s in zip(straddle, special):
        v[i] = s
    v[5000:5400] = vmax                                     # all-ones words inside lanes
    v[tile_rows(c) - 300:tile_rows(c) + 300] = vmax         # ... across the tile boundary
    v[n - 6:] = [1, (1 << (c - 1)) - 1, 1 << (c - 1), vmax - 1, vmax, 0]  # the last rows: vmax, then 0 (the pad decodes as 0)
    return v.astype(np.uint32)


# differs from support.L: a missing library is an error here, it is not built
@pytest.fixture(scope="module")
def L():
    from shared_simd_scan_amd import lib

    return lib()


# differs from support.eng: says why when there is no GPU, takes the current device, is never closed
@pytest.fixture(scope="module")
def eng():
    import torch

    from shared_simd_scan_amd import ScanEngine

    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return ScanEngine()


@pytest.fixture(scope="module")
def eng4():
    """its own context, every persistent grid one block of 4 waves: each wave walks many tiles (several store bursts)"""
    from shared_simd_scan_amd import ScanEngine

    e = ScanEngine()
    e.set_option("grid_cus", 1)
    e.set_option("max_blocks_per_cu", 1)
    return e


def ok(L, rc):
    assert rc == 0, L.mi355_last_error()


def upload_column(O, eng, vals, c):
    import torch

    from shared_simd_scan_amd import PackedColumn

    packed = O.pack(vals, c)
    data = torch.empty(packed.shape[0], dtype=torch.uint8, device="cuda")
    data.copy_(torch.from_numpy(packed))
    return PackedColumn(data, vals.shape[0], c), packed


def upload_bitmap(bits):
    import torch

    host = np_bitmap(bits)
    dev = torch.empty(host.shape[0], dtype=torch.uint8, device="cuda")  # a fresh allocation: 16-byte aligned
    dev.copy_(torch.from_numpy(host))
    return dev


class Slots:
    """preallocated results: bitmaps mi355_bitmap_stride apart, filled with 0xEE, and hit counters; check() copies them back
    once and compares every bitmap (plus its untouched guard bytes) and count with what was expected"""

    def __init__(self, L, n, count):
        import torch

        self.n, self.nb = n, (n + 7) // 8
        self.stride = int(L.mi355_bitmap_stride(n))
        self.bm = torch.full((count, self.stride), 0xEE, dtype=torch.uint8, device="cuda")
        self.hits = torch.full((count,), -7, dtype=torch.int64, device="cuda")
        self.counts = torch.full((count,), -7, dtype=torch.int64, device="cuda")
        self.want, self.want_counts = [], []

    def bitmap(self, label, expect):
        i = len(self.want)
        assert i < self.bm.shape[0], "more results than slots"
        self.want.append((label, expect))
        return self.bm[i], self.hits[i:i + 1]

    def count(self, label, expect):
        i = len(self.want_counts)
        assert i < self.counts.shape[0], "more counts than slots"
        self.want_counts.append((label, int(expect.sum())))
        return self.counts[i:i + 1]

    def check(self):
        bm, hits, counts = self.bm.cpu().numpy(), self.hits.cpu().numpy(), self.counts.cpu().numpy()
        for i, (label, e) in enumerate(self.want):
            assert np.array_equal(bm[i, :self.nb], np_bitmap(e)), label
            assert (bm[i, self.nb:] == 0xEE).all(), ("wrote past ceil(n/8)", label)
            assert hits[i] == int(e.sum()), (label, int(hits[i]), int(e.sum()))
        for i, (label, want) in enumerate(self.want_counts):
            assert counts[i] == want, (label, int(counts[i]), want)
        return len(self.want) + len(self.want_counts)


@pytest.mark.parametrize("c", list(range(1, 33)))
def test_predicate_constants_at_type_limits(O, eng, L, c):
    """scan_where / count-only / scan_combine / scan_select / scan2 / scan / scan_range / scan_in / shared_scan with every
    edge constant, and the int64 limits through the C ABI"""
    import torch

    n = n_rows(c)
    vmax = (1 << c) - 1
    vals = edge_values(c, n, 31_000 + c)
    col, packed = upload_column(O, eng, vals, c)
    assert np.array_equal(eng.decompress(col).cpu().numpy().view(np.uint32), vals), c
    v = vals.astype(np.int64)
    inside = int(vals[1234])
    consts, pyc, red = abi_constants(c, inside), py_constants(c, inside), reduced_constants(c, inside)
    rng = np.random.default_rng(32_000 + c)
    mbits = rng.random(n) < 0.5
    mask = upload_bitmap(mbits)
    vals2 = edge_values(c, n, 33_000 + c)[::-1].copy()  # a second column of the same width
    col2, _ = upload_column(O, eng, vals2, c)
    c3 = 21 if c <= 16 else 5                            # ... and one of another tile geometry
    vals3 = rng.integers(0, 1 << c3, size=n, dtype=np.uint64).astype(np.uint32)
    col3, _ = upload_column(O, eng, vals3, c3)
    v2, v3 = vals2.astype(np.int64), vals3.astype(np.int64)
    mid2, mid3 = int(vals2[77]), int(vals3[77])

    S = Slots(L, n, 1400)
    # one-operand comparisons, every constant: bitmap + hits, and the count-only form
    cases = [(op, a, 0) for op in OPS1 for a in pyc]
    # between / not_between over every ordered pair of the reduced set (a > b included)
    cases += [(op, a, b) for op in ("between", "not_between") for a in red for b in red]
    for op, a, b in cases:
        e = expect_cmp(v, op, a, b)
        bm, h = S.bitmap(("where", op, a, b), e)
        eng.scan_where(op, a, col, b=b, bitmap=bm, hits=h)
        eng.scan_combine(op, a, col, b=b, count_only=True, hits=S.count(("count only", op, a, b), e))
    # the earlier bitmap combined inside the scan, each mask op, on a strided subset (count-only with a mask too)
    for i, (op, a, b) in enumerate(cases[::7]):
        p = expect_cmp(v, op, a, b)
        for mop, f in MASK_OPS.items():
            bm, h = S.bitmap(("combine", op, a, b, mop), f(p, mbits))
            eng.scan_combine(op, a, col, b=b, mask=mask, mask_op=mop, bitmap=bm, hits=h)
        mop = list(MASK_OPS)[i % 4]
        eng.scan_combine(op, a, col, b=b, mask=mask, mask_op=mop, count_only=True,
                         hits=S.count(("combine count only", op, a, b, mop), MASK_OPS[mop](p, mbits)))
    # fused selection: row ids and count, alternately with a mask
    selects = []
    for i, (op, a, b) in enumerate(cases[3::11]):
        p = expect_cmp(v, op, a, b)
        if i % 2:
            mop = list(MASK_OPS)[(i // 2) % 4]
            ids, cnt = eng.scan_select(op, a, col, capacity=n, b=b, mask=mask, mask_op=mop, first_row=1 << 33)
            p = MASK_OPS[mop](p, mbits)
        else:
            ids, cnt = eng.scan_select(op, a, col, capacity=n, b=b)
        selects.append(((op, a, b, i), np.flatnonzero(p) + (1 << 33 if i % 2 else 0), ids, cnt))
    # two columns: the edge constant in slot 1, then in slot 2; same width (one launch) and another width (two launches)
    ops8 = list(CMP)
    for i, a in enumerate(pyc):
        op, b, cmb = ops8[i % 8], red[i % len(red)], list(COMBINE)[i % 4]
        pe = expect_cmp(v, op, a, b)
        for other, vo, mid in ((col2, v2, mid2), (col3, v3, mid3)):
            po = vo <= mid
            bm, h = S.bitmap(("scan2 slot 1", other.c, op, a, b, cmb), COMBINE[cmb](pe, po))
            eng.scan2(col, op, a, other, "<=", mid, b1=b, combine=cmb, bitmap=bm, hits=h)
            bm, h = S.bitmap(("scan2 slot 2", other.c, op, a, b, cmb), COMBINE[cmb](po, pe))
            eng.scan2(other, "<=", mid, col, op, a, b2=b, combine=cmb, bitmap=bm, hits=h)
    # equality keys, ranges, key lists
    keys = [k for k in pyc if key_ok(k, c)]
    for k in keys:
        e = expect_key(v, k, c)
        bm, h = S.bitmap(("scan", k), e)
        eng.scan(k, col, bitmap=bm, hits=h)
        bm, h = S.bitmap(("scan_in one key", k), e)
        eng.scan_in([k], col, bitmap=bm, hits=h)
    for lo in red:
        for hi in red:
            bm, h = S.bitmap(("scan_range", lo, hi), expect_cmp(v, "between", lo, hi))
            eng.scan_range(lo, hi, col, bitmap=bm, hits=h)
    member = np.zeros(n, bool)
    for k in keys:
        member |= expect_key(v, k, c)
    bm, h = S.bitmap(("scan_in", keys), member)
    eng.scan_in(keys, col, bitmap=bm, hits=h)
    bm, h = S.bitmap(("scan_in negated", keys), ~member)
    eng.scan_in(keys, col, negate=True, bitmap=bm, hits=h)
    bm, h = S.bitmap(("scan_in masked", keys), member & mbits)
    eng.scan_in(keys, col, and_mask=mask, bitmap=bm, hits=h)
    shared = []
    for P in (1, 8, 33):
        ks = [keys[(c + i) % len(keys)] for i in range(P)]
        for layout in ("per_predicate", "linear"):
            out, hs = eng.shared_scan(ks, col, layout=layout)
            shared.append((P, layout, ks, out, hs))
    # the int64 limits straight into the C ABI: the Python wrappers clamp them, so only here do they reach normalise_predicate
    ptr, ctx = col.data.data_ptr(), eng._ctx
    for op in CMP:
        for a in (INT64_MIN, INT64_MAX):
            for b in ((INT64_MIN, INT64_MAX) if op in ("between", "not_between") else (0,)):
                e = expect_cmp(v, op, a, b)
                bm, h = S.bitmap(("C ABI where", op, a, b), e)
                ok(L, L.mi355_scan_where_dev(ctx, ptr, n, c, CMP[op], a, b, None, bm.data_ptr(), h.data_ptr()))
                ok(L, L.mi355_scan_combine_dev(ctx, ptr, n, c, CMP[op], a, b, 0, None, None,
                                               S.count(("C ABI count only", op, a, b), e).data_ptr()))
                bm, h = S.bitmap(("C ABI combine or", op, a, b), e | mbits)
                ok(L, L.mi355_scan_combine_dev(ctx, ptr, n, c, CMP[op], a, b, BOP["or"], mask.data_ptr(), bm.data_ptr(),
                                               h.data_ptr()))
                for other, vo, mid in ((col2, v2, mid2), (col3, v3, mid3)):
                    po = vo >= mid
                    bm, h = S.bitmap(("C ABI scan2 slot 1", other.c, op, a, b), e & po)
                    ok(L, L.mi355_scan2_dev(ctx, ptr, c, CMP[op], a, b, other.data.data_ptr(), other.c, CMP[">="], mid, 0, n,
                                            BOP["and"], bm.data_ptr(), h.data_ptr()))
                    bm, h = S.bitmap(("C ABI scan2 slot 2", other.c, op, a, b), po ^ e)
                    ok(L, L.mi355_scan2_dev(ctx, other.data.data_ptr(), other.c, CMP[">="], mid, 0, ptr, c, CMP[op], a, b, n,
                                            BOP["xor"], bm.data_ptr(), h.data_ptr()))
                ids = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
                cnt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
                ok(L, L.mi355_scan_select_dev(ctx, ptr, n, c, CMP[op], a, b, 0, None, 0, ids.data_ptr(), n, cnt.data_ptr()))
                selects.append((("C ABI select", op, a, b), np.flatnonzero(e), ids, cnt))
    # keys the wrappers cannot express at c = 32 are refused, not wrapped onto a value
    if c == 32:
        for k in ((1 << 32) + 5, -(1 << 31) - 1, INT64_MAX):
            for call in (lambda: eng.scan(k, col), lambda: eng.scan_in([0, k], col), lambda: eng.shared_scan([k, 1], col)):
                with pytest.raises(ValueError):
                    call()
    # copy back once
    checked = S.check()
    for label, want, ids, cnt in selects:
        k = int(cnt.item())
        assert k == want.shape[0], (label, k, want.shape[0])
        assert np.array_equal(ids[:k].cpu().numpy(), want), label
        checked += 1
    nb = (n + 7) // 8
    for P, layout, ks, out, hs in shared:
        per_key = np.stack([np_bitmap(expect_key(v, k, c)) for k in ks])
        got = out.cpu().numpy()
        if layout == "per_predicate":
            assert np.array_equal(got[:, :nb], per_key), (P, layout, ks)
        else:
            assert np.array_equal(got.reshape(nb, P), per_key.T), (P, layout, ks)
        assert hs.cpu().numpy().tolist() == [int(expect_key(v, k, c).sum()) for k in ks], (P, layout, ks)
    # the host-pointer range scan, uint32 bounds at their limits
    if c in (9, 32):
        bounds = [0, 1, vmax - 1, vmax, (1 << 31) - 1, 1 << 31, (1 << 32) - 2, (1 << 32) - 1]
        out = np.empty(L.mi355_scan_output_buffer_size(n), dtype=np.uint8)
        for lo in bounds:
            for hi in bounds:
                out[:] = 0xEE
                hits = C.c_uint64(123)
                ok(L, L.mi355_scan_range(None, packed.ctypes.data, n, c, lo, hi, out.ctypes.data, C.byref(hits)))
                e = (v >= lo) & (v <= hi)
                assert np.array_equal(out[:nb], np_bitmap(e)) and hits.value == int(e.sum()), (c, lo, hi)
    assert checked > 700, checked


@pytest.mark.parametrize("burst", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 5, 9, 12, 16, 17, 21, 32])
def test_mask_and_result_in_the_same_buffer(O, eng4, L, c, burst):
    """mask_dev == bitmap_dev (the documented in-place form; scan2 over two widths relies on it): scan_combine with each
    mask op, scan_where with and_mask, scan_in with and_mask, on a 4-wave grid where every wave walks several chunks of
    tiles -- with the width's store burst (4 tiles per burst at c = 5, 6, 9..16) and with one tile per burst"""
    n = tile_rows(c) * 45 + 77
    vmax = (1 << c) - 1
    vals = edge_values(c, n, 34_000 + c)
    col, _ = upload_column(O, eng4, vals, c)
    v = vals.astype(np.int64)
    mbits = np.random.default_rng(35_000 + c).random(n) < 0.5
    a = int(vals[999])
    p = v >= a
    keys = [int(vals[5]), int(vals[77]), 0, vmax]
    member = np.isin(v, np.array(keys, dtype=np.int64))
    k_burst = 4 if burst == 0 and (c in (5, 6) or 9 <= c <= 16) else 1
    results = []
    try:
        eng4.set_option("scan_burst", burst)
        for mop, f in MASK_OPS.items():
            m = upload_bitmap(mbits)
            _, h = eng4.scan_combine(">=", a, col, mask=m, mask_op=mop, bitmap=m)
            rec = L.mi355_ctx_last_launch(eng4._ctx).decode()
            assert "scan_burst_kernel<" in rec and f", {k_burst}> grid=1 " in rec, rec
            results.append((("combine", mop), f(p, mbits), m, h))
        m = upload_bitmap(mbits)
        _, h = eng4.scan_where(">=", a, col, and_mask=m, bitmap=m)
        results.append((("where",), p & mbits, m, h))
        m = upload_bitmap(mbits)
        _, h = eng4.scan_in(keys, col, and_mask=m, bitmap=m)
        results.append((("in",), member & mbits, m, h))
        m = upload_bitmap(mbits)
        _, h = eng4.scan_in(keys, col, negate=True, and_mask=m, bitmap=m)
        results.append((("not in",), ~member & mbits, m, h))
    finally:
        eng4.set_option("scan_burst", 0)
    for label, e, m, h in results:
        assert np.array_equal(m.cpu().numpy(), np_bitmap(e)), (c, burst, label)
        assert int(h.item()) == int(e.sum()), (c, burst, label)


@pytest.mark.parametrize("n", [1, 63, 64, 127, 128, 1000, 16384, 16385, 100_003, 1_000_003])
def test_bitmap_combine_in_place(eng, n):
    """mi355_bitmap_combine_dev: out may alias a or b"""
    rng = np.random.default_rng(36_000 + n)
    x = rng.random(n) < 0.3
    y = rng.random(n) < 0.5
    bx, by = upload_bitmap(x), upload_bitmap(y)
    results = []
    for op, f in (("and", np.logical_and), ("or", np.logical_or), ("xor", np.logical_xor), ("andnot", lambda p, q: p & ~q)):
        a = bx.clone()
        _, cnt = eng.bitmap_combine(op, a, by, n, out=a)
        results.append(((op, "out=a"), f(x, y), a, cnt))
        b = by.clone()
        _, cnt = eng.bitmap_combine(op, bx, b, n, out=b)
        results.append(((op, "out=b"), f(x, y), b, cnt))
    for label, e, out, cnt in results:
        assert np.array_equal(out.cpu().numpy(), np_bitmap(e)), (n, label)
        assert int(cnt.item()) == int(e.sum()), (n, label)


@pytest.mark.parametrize("c", [16, 17, 24, 25, 31, 32])
def test_aggregate_of_a_column_of_vmax(eng, eng4, c):
    """sum / count / min / max where every value is 2^c - 1: the worst case of the lanes' 32-bit partial sums (c <= 24) and
    of the 24-bit limbs of the wave sums -- on the default grid and on 4 waves that each add up ~180 tiles"""
    import torch

    n = 3_000_077
    vmax = (1 << c) - 1
    col = eng.compress(torch.full((n,), int(np.uint32(vmax).view(np.int32)), dtype=torch.int32, device="cuda"), c)
    pattern = np.tile(np.array([1, 0, 1, 1, 0, 1, 1, 0], bool), n // 8 + 1)[:n]
    masks = [(None, n), (upload_bitmap(np.ones(n, bool)), n), (upload_bitmap(pattern), int(pattern.sum()))]
    for e in (eng, eng4):
        outs = [(cnt, e.aggregate(col, mask=m)) for m, cnt in masks]
        for cnt, out in outs:
            assert out.cpu().numpy().view(np.uint64).tolist() == [vmax * cnt, cnt, vmax, vmax], (c, cnt, e is eng4)
