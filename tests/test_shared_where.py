"""GPU (-m gpu): shared scans over range and comparison predicates (mi355_shared_scan_where_dev / _where / _where_linear,
ScanEngine.shared_scan_where) against numpy on the source values, the reference's golden vectors, and the engine's
single-predicate and equality entry points as second opinions.

Integer / bit work: every comparison is exact, byte for byte.  Device outputs live inside 0xEE guard bytes that must stay
untouched (GUARD bytes in front and behind; per-predicate bitmaps also keep the bytes between ceil(n/8) and the stride).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import GOLDEN_SIZES, GOLDEN_WIDTHS
from kernel_cases import WHERE_CHAIN as CHAIN
from kernel_cases import WHERE_COUNT_CASES as COUNT_CASES
from kernel_cases import WHERE_LUT as LUT
from kernel_cases import WHERE_LUT_MULTI as LUT_MULTI
from kernel_cases import WHERE_SINGLE as SINGLE
from support import E_INVALID

pytestmark = pytest.mark.gpu

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
OPS = ["==", "!=", "<", "<=", ">", ">=", "between", "not_between"]
GUARD = 256


def bits(buf, n):
    return np.unpackbits(np.ascontiguousarray(buf, dtype=np.uint8), bitorder="little")[:n]


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def np_bitmap(mask):
    return np.packbits(mask.astype(np.uint8), bitorder="little")


def np_pred(v, op, a, b=0):
    """the rows a predicate selects, by int64 arithmetic on the unpacked column (v: int64 array of values in [0, 2^32))"""
    if op == "==":
        return v == a
    if op == "!=":
        return v != a
    if op == "<":
        return v < a
    if op == "<=":
        return v <= a
    if op == ">":
        return v > a
    if op == ">=":
        return v >= a
    inside = (v >= a) & (v <= b)
    return inside if op == "between" else ~inside


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


def ok(L, rc):
    assert rc == 0, L.mi355_last_error()


def make_column(eng, n, c, seed):
    """random c-bit values -> (int64 numpy values, packed column on the device)"""
    import torch

    rng = np.random.default_rng(seed)
    vals = rng.integers(0, 1 << c, size=n, dtype=np.uint64).astype(np.uint32)
    col = eng.compress(torch.from_numpy(vals.view(np.int32)), c)
    return vals.astype(np.int64), col


def guarded(eng, nbytes):
    import torch

    full = torch.full((nbytes + 2 * GUARD,), 0xEE, dtype=torch.uint8, device=eng._dev)
    return full, full[GUARD:GUARD + nbytes]


def guards_intact(full, nbytes):
    h = full.cpu().numpy()
    return bool((h[:GUARD] == 0xEE).all() and (h[GUARD + nbytes:] == 0xEE).all())


def family_of(kernel_line):
    name = kernel_line.split("<")[0]
    if name == "shared_where_lut_kernel":
        multi = kernel_line.split(">")[0].split(",")[-1].strip()
        return LUT_MULTI if multi == "true" else LUT
    return name


def run_where(L, eng, col, preds, layout, with_hits=True):
    """one device call inside guards -> (uint8 [P, ceil(n/8)] bitmaps, hits or None, launch record line)"""
    import torch

    from shared_simd_scan_amd.engine import predicates

    P, n = len(preds), col.n
    nb = (n + 7) // 8
    arr = predicates(preds)
    hits = torch.full((P + 2,), -7, dtype=torch.int64, device=eng._dev)
    if layout == "per_predicate":
        stride = int(L.mi355_bitmap_stride(n))
        full, out = guarded(eng, P * stride)
        code = 0
    else:
        stride = 0
        full, out = guarded(eng, P * nb)
        code = 1
    ok(L, L.mi355_shared_scan_where_dev(eng._ctx, col.data.data_ptr(), n, col.c, C.cast(arr, C.c_void_p), P, code, out.data_ptr(), stride,
                                        hits[1:].data_ptr() if with_hits else None))
    line = L.mi355_ctx_last_launch(eng._ctx).decode().strip()
    torch.cuda.synchronize()
    assert guards_intact(full, out.numel())
    h = hits.cpu().numpy()
    assert h[0] == -7 and h[-1] == -7
    if not with_hits:
        assert (h == -7).all()
    o = out.cpu().numpy()
    if layout == "per_predicate":
        o = o.reshape(P, stride)
        assert (o[:, nb:] == 0xEE).all()  # nothing written past ceil(n/8)
        bm = o[:, :nb]
    else:
        bm = o.reshape(nb, P).T
    return np.ascontiguousarray(bm), (h[1:-1] if with_hits else None), line


def check_against_numpy(v, n, preds, bm, hits):
    for k, p in enumerate(preds):
        mask = np_pred(v, *p)
        assert np.array_equal(bm[k], np_bitmap(mask)), (k, p)  # bits below n and the zero tail
        if hits is not None:
            assert int(hits[k]) == int(mask.sum()), (k, p)


# ---- 1. the reference's vectors -------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", GOLDEN_WIDTHS)
@pytest.mark.parametrize("n", GOLDEN_SIZES)
@pytest.mark.parametrize("P", [1, 3, 8])
def test_golden_vectors_as_between_k_and_k(L, golden, w, n, P):
    from shared_simd_scan_amd.engine import predicates

    g = golden[w]
    packed = np.ascontiguousarray(g[f"n{n}_packed"])
    keys = [int(k) for k in g[f"n{n}_shared_keys_P{P}"]]
    arr = predicates([("between", k, k) for k in keys])
    ref_std, ref_lin = g[f"n{n}_shared_std_P{P}"], g[f"n{n}_linear_std_P{P}"]
    sobs = L.mi355_scan_output_buffer_size(n)
    nb, full = (n + 7) // 8, n // 8
    outs = [np.zeros(sobs, dtype=np.uint8) for _ in range(P)]
    ptrs = (C.c_void_p * P)(*[o.ctypes.data for o in outs])
    hits = np.zeros(P, dtype=np.uint64)
    ok(L, L.mi355_shared_scan_where(None, vp(packed), n, w, C.cast(arr, C.c_void_p), P, ptrs, vp(hits)))
    rec1 = L.mi355_ctx_last_launch(None).decode()
    lin = np.zeros(P * sobs, dtype=np.uint8)
    hits2 = np.zeros(P, dtype=np.uint64)
    ok(L, L.mi355_shared_scan_where_linear(None, vp(packed), n, w, C.cast(arr, C.c_void_p), P, vp(lin), vp(hits2)))
    rec2 = L.mi355_ctx_last_launch(None).decode()
    assert np.array_equal(hits, hits2)
    for k in range(P):
        assert np.array_equal(bits(outs[k], n), bits(ref_std[k], n))
        assert hits[k] == bits(ref_std[k], n).sum()
        assert not outs[k][nb:].any()
    assert np.array_equal(lin[: full * P], ref_lin[: full * P])
    for k in range(P):
        assert np.array_equal(bits(lin[k::P][:nb], n), bits(ref_lin[k::P][:nb], n))
    assert not lin[nb * P:].any()
    if P > 1:  # equality spelled as a range stays on the kernels of csrc/predicates/
        want = "shared_where_lut_kernel<" if w <= 16 else "shared_where_chain_kernel<"
        assert want in rec1 and want in rec2, (rec1, rec2)


# ---- 2. every op at every width -------------------------------------------------------------------------------------
def every_op_list(c, rng):
    """8 predicates holding each op once; constants from inside the domain and from {-5, 2^c, 2^c + 3, INT64_MIN, INT64_MAX};
    the BETWEEN is empty (a > b), the NOT BETWEEN covers the whole domain"""
    top = 1 << c
    inside = lambda: int(rng.integers(0, top))  # noqa: E731
    outside = [-5, top, top + 3, INT64_MIN, INT64_MAX]
    pick = lambda i: outside[(i + c) % 5] if (i + c) % 3 == 0 else inside()  # noqa: E731
    preds = [("==", inside()), ("!=", pick(1)), ("<", pick(2)), ("<=", pick(3)), (">", pick(4)), (">=", pick(5)),
             ("between", max(inside(), 1), 0), ("not_between", 0, top - 1)]
    order = rng.permutation(8)
    return [preds[i] for i in order]


@pytest.mark.parametrize("c", list(range(1, 33)))
def test_every_op_every_width(L, eng, c):
    import torch

    rng = np.random.default_rng(1000 + c)
    for n in [1, 7, 8, 9, 63, 64, 65, 1000, 10 * 4096 + 77]:
        v, col = make_column(eng, n, c, 31 * c + n)
        preds = every_op_list(c, rng)
        singles = []  # what the single-predicate scan writes for each of them
        for p in preds:
            bm, h = eng.scan_where(p[0], p[1], col, b=p[2] if len(p) == 3 else 0)
            torch.cuda.synchronize()
            singles.append((bm.cpu().numpy(), int(h.item())))
        for layout in ("per_predicate", "linear"):
            for with_hits in (True, False):
                bm, hits, line = run_where(L, eng, col, preds, layout, with_hits)
                check_against_numpy(v, n, preds, bm, hits)
                for k in range(8):
                    assert np.array_equal(bm[k], singles[k][0])
                    assert hits is None or int(hits[k]) == singles[k][1]
                assert family_of(line) == (LUT if c <= 16 else CHAIN), line


# ---- 3. predicate counts --------------------------------------------------------------------------------------------
def random_ranges(c, P, rng):
    top = 1 << c
    preds = []
    for _ in range(P):
        a, b = sorted(int(x) for x in rng.integers(0, top, size=2))
        preds.append(("not_between" if rng.integers(0, 4) == 0 else "between", a, b))
    return preds


@pytest.mark.parametrize("c,P,family", COUNT_CASES)
@pytest.mark.parametrize("layout", ["per_predicate", "linear"])
def test_predicate_counts(L, eng, c, P, family, layout):
    from shared_simd_scan_amd.engine import shared_where_kernel

    n = 10 * 4096 + 77
    v, col = make_column(eng, n, c, 7 * c + P)
    preds = random_ranges(c, P, np.random.default_rng(100 * c + P))
    announced = L.mi355_shared_where_kernel(eng._ctx, c, P, 0 if layout == "per_predicate" else 1, 1).decode()
    assert announced == family == shared_where_kernel(c, P, layout)
    bm, hits, line = run_where(L, eng, col, preds, layout, True)
    assert family_of(line) == family, line
    check_against_numpy(v, n, preds, bm, hits)
    assert any(0 < int(h) < n for h in hits)  # a table of all zeros or all ones cannot pass


def test_count_cases_reach_every_family():
    fams = {f for _, _, f in COUNT_CASES}
    assert fams == {SINGLE, LUT, LUT_MULTI, CHAIN}
    assert (12, 64, LUT_MULTI) in COUNT_CASES and (12, 257, CHAIN) in COUNT_CASES and (16, 9, CHAIN) in COUNT_CASES


# ---- 4. equality is a special case ------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [9, 17])
@pytest.mark.parametrize("P", [8, 40])
@pytest.mark.parametrize("layout", ["per_predicate", "linear"])
def test_all_eq_list_equals_the_equality_scan(L, eng, c, P, layout):
    import torch

    n = 10 * 4096 + 77
    v, col = make_column(eng, n, c, 5 * c + P)
    rng = np.random.default_rng(c * P)
    keys = [int(k) for k in rng.integers(0, 1 << c, size=P)]
    keys[1], keys[P // 2], keys[-1] = 1 << c, -5, (1 << c) + 3  # out of the domain: no row
    preds = [("==", k) for k in keys]
    bm, hits, _ = run_where(L, eng, col, preds, layout, True)
    check_against_numpy(v, n, preds, bm, hits)
    out, h = eng.shared_scan(keys, col, layout=layout)
    torch.cuda.synchronize()
    nb = (n + 7) // 8
    o = out.cpu().numpy()
    eq = o[:, :nb] if layout == "per_predicate" else o.reshape(nb, P).T
    assert np.array_equal(bm, eq) and np.array_equal(hits, h.cpu().numpy())


# ---- 5. long loops ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [9, 17])
@pytest.mark.parametrize("P", [8, 40])
def test_long_per_wave_loops(L, c, P):
    """one block of four waves walks the whole column: more than 1100 tiles per wave, ragged tail"""
    import torch

    from shared_simd_scan_amd import ScanEngine

    e = ScanEngine()
    try:
        e.set_option("grid_cus", 1)
        e.set_option("max_blocks_per_cu", 1)
        n = 19_000_077
        v, col = make_column(e, n, c, 77 + c)
        preds = random_ranges(c, P, np.random.default_rng(c + P))
        preds[P // 3] = (">=", 0)  # true for every row
        bm, hits, line = run_where(L, e, col, preds, "per_predicate", True)
        assert " grid=1 " in line, line
        assert int(hits[P // 3]) == n
        check_against_numpy(v, n, preds, bm, hits)
        del col
    finally:
        e.close()
        torch.cuda.empty_cache()


def test_more_than_2_pow_32_rows(L, eng):
    """64-bit row, tile and byte offsets: 2^32 + 3 * 8192 + 77 rows of v[i] = i % 7 at c = 3, 8 predicates; hit counts exact,
    bitmaps checked over windows at the start, across row 2^32 and over the ragged end"""
    import torch

    from shared_simd_scan_amd.engine import predicates

    c, n = 3, (1 << 32) + 3 * 8192 + 77
    col = eng.generate("mod", n, c, 7)
    preds = [("==", 5), ("!=", 2), ("<", 3), ("<=", 6), (">", 4), (">=", 7), ("between", 2, 4), ("not_between", 1, 5)]
    P = len(preds)
    nb = (n + 7) // 8
    stride = int(L.mi355_bitmap_stride(n))
    full, out = guarded(eng, P * stride)
    hits = torch.zeros(P, dtype=torch.int64, device=eng._dev)
    arr = predicates(preds)
    ok(L, L.mi355_shared_scan_where_dev(eng._ctx, col.data.data_ptr(), n, c, C.cast(arr, C.c_void_p), P, 0, out.data_ptr(), stride,
                                        hits.data_ptr()))
    torch.cuda.synchronize()
    assert bool((full[:GUARD] == 0xEE).all()) and bool((full[GUARD + P * stride:] == 0xEE).all())
    o = out.view(P, stride)
    residues = np.arange(7, dtype=np.int64)
    count_of = np.array([(n - 1 - r) // 7 + 1 for r in range(7)], dtype=np.int64)
    h = hits.cpu().numpy()
    for k, p in enumerate(preds):
        assert int(h[k]) == int(count_of[np_pred(residues, *p)].sum()), p
        assert bool((o[k, nb:] == 0xEE).all())
    a0 = (1 << 32) - 8192 * 2
    for a, ln in ((0, 100_000), (a0, 8192 * 4 + 96), (n - 77 - 8192, None)):
        ln = n - a if ln is None else ln
        v = (np.arange(a, a + ln, dtype=np.uint64) % 7).astype(np.int64)
        for k, p in enumerate(preds):
            assert np.array_equal(o[k, a // 8: a // 8 + (ln + 7) // 8].cpu().numpy(), np_bitmap(np_pred(v, *p))), (a, p)
    del full, out, o, col
    torch.cuda.empty_cache()


# ---- 6. predicate lists in flight -------------------------------------------------------------------------------------
def test_many_predicate_lists_in_flight_without_synchronising(eng):
    """P > 8 lists travel through the context's ring of 8 pinned slots: 48 calls with different lists (table and chain
    widths, interleaved with equality key lists that share the ring) enqueued back to back, checked afterwards"""
    import torch

    n = 8192 * 3 + 333
    cols = {c: make_column(eng, n, c, 2468 + c) for c in (9, 17)}
    rng = np.random.default_rng(99)
    jobs = []
    for i in range(48):
        c = (9, 17)[i % 2]
        v, col = cols[c]
        P = int(rng.integers(9, 60))
        if i % 6 == 5:
            keys = [int(k) for k in rng.integers(0, 1 << c, size=P)]
            out, hits = eng.shared_scan(keys, col)
            jobs.append((v, [("==", k) for k in keys], out, hits))
        else:
            preds = random_ranges(c, P, rng)
            nb = (n + 7) // 8
            stride = (nb + 255) // 256 * 256
            full, view = guarded(eng, P * stride)
            out, hits = eng.shared_scan_where(preds, col, out=view.view(P, stride))
            jobs.append((v, preds, out, hits, full))
    torch.cuda.synchronize()
    nb = (n + 7) // 8
    for job in jobs:
        v, preds, out, hits = job[:4]
        check_against_numpy(v, n, preds, out.cpu().numpy()[:, :nb], hits.cpu().numpy())
        if len(job) == 5:
            assert guards_intact(job[4], out.numel())


# ---- 7. refusals -------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(L, eng):
    import torch

    from shared_simd_scan_amd._capi import Predicate

    n, c = 5000, 9
    _, col = make_column(eng, n, c, 1)
    stride = int(L.mi355_bitmap_stride(n))
    full, out = guarded(eng, 16 * stride)
    hits = torch.full((16,), -7, dtype=torch.int64, device=eng._dev)
    good = (Predicate * 1025)()
    for p in good:
        p.op, p.a, p.b = 6, 3, 9

    def call(preds=good, P=3, layout=0, packed=None, outp=None, stride_=stride):
        return L.mi355_shared_scan_where_dev(eng._ctx, col.data.data_ptr() if packed is None else packed, n, c,
                                             C.cast(preds, C.c_void_p) if preds is not None else None, P, layout,
                                             out.data_ptr() if outp is None else outp, stride_, hits.data_ptr())

    bad_op, bad_op2, bad_res = (Predicate * 3)(), (Predicate * 3)(), (Predicate * 3)()
    for arr in (bad_op, bad_op2, bad_res):
        for p in arr:
            p.op, p.a, p.b = 2, 100, 0
    bad_op[2].op = 8
    bad_op2[0].op = -1
    bad_res[1].reserved = 1
    refused = [call(preds=bad_op), call(preds=bad_op2), call(preds=bad_res), call(preds=None), call(P=0), call(P=1025),
               call(layout=2), call(layout=-1), call(outp=out.data_ptr() + 8), call(stride_=stride + 8), call(stride_=16),
               call(packed=col.data.data_ptr() + 4), call(layout=1, outp=out.data_ptr() + 4)]
    assert refused == [E_INVALID] * len(refused), refused
    assert L.mi355_last_error()
    for P in (1, 9):  # the single-predicate route and the uploaded lists validate first, too
        assert call(preds=bad_res, P=P if P > 1 else 2) == E_INVALID
    one = (Predicate * 1)()
    one[0].op = 9
    assert call(preds=one, P=1) == E_INVALID
    torch.cuda.synchronize()
    assert bool((full == 0xEE).all()) and bool((hits == -7).all())
    assert call() == 0  # and the same call with a valid list runs
    torch.cuda.synchronize()
    assert not bool((out[:3 * stride].view(3, stride)[:, : (n + 7) // 8] == 0xEE).all())
