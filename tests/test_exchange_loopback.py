"""The multi-rank RCCL exchange (shared_simd_scan_amd/csrc/comm.hip, RcclExchange in sharded.py) with 2..4 ranks on ONE GPU.

RCCL refuses two ranks on one device, so the ranks load tests/cpp/loopback_rccl.cpp instead (MI355_RCCL_LIB names the
library comm.hip opens): the same nine entry points over Unix sockets, staged through host memory.  It fails a receive
whose size differs from what the peer sent, and it logs every call (MI355_LOOPBACK_LOG), which the tests read to
check which lines ran: the non-root send, the root's one group of receives, roots other than rank 0, zero-byte ranks,
the side stream of scan_pipelined.  Every result is compared with the oracle over the whole column.

Only gloo-bootstrapped processes use the stand-in (a process with torch's nccl backend already runs the real librccl);
the world-1 test at the end runs the same column checks on the real library.
"""
import ctypes as C
import datetime
import os
import re
import subprocess
import time
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from support import E_INVALID, _bench_2ranks, free_port, join_or_kill

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "loopback_rccl.cpp")
LIB = os.path.join(ROOT, "tests", "cpp", "libloopback_rccl.so")
COMM_SRC = os.path.join(ROOT, "shared_simd_scan_amd", "csrc", "comm.hip")
RANK_TIMEOUT_S = 420  # per test, all ranks together; the stand-in's own socket timeouts are far shorter


def build_library() -> str:
    """tests/cpp/libloopback_rccl.so: plain g++ against the real rccl.h (which checks every signature) and libamdhip64"""
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
        subprocess.run(["g++", "-std=gnu++17", "-O1", "-Wall", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                        SRC, "-o", LIB, "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib",
                        # calls inside the library stay inside it, even where a real librccl is loaded as well
                        "-Wl,-Bsymbolic"], check=True)
    return LIB


# ------------------------------------------------------------------------------------------------
# the call log
# ------------------------------------------------------------------------------------------------

class Log:
    """the lines one rank's stand-in wrote (MI355_LOOPBACK_LOG=<base> -> <base>.<rank>)"""

    def __init__(self, base, rank):
        self.path = f"{base}.{rank}"

    def calls(self):
        if not os.path.exists(self.path):
            return []
        out = []
        with open(self.path) as f:
            for line in f:
                op, *kv = line.split()
                d = dict(x.split("=", 1) for x in kv)
                out.append(dict(op=op, peer=int(d["peer"]), bytes=int(d["bytes"]), ptr=int(d["ptr"], 16),
                                stream=int(d["stream"], 16), group=int(d["group"]), rc=int(d["rc"])))
        return out

    def mark(self):
        return len(self.calls())

    def since(self, mark):
        return self.calls()[mark:]


def p2p(calls):
    return [c for c in calls if c["op"] in ("ncclSend", "ncclRecv")]


def check_gather_log(calls, rank, world, root, sizes, offsets, local_ptr, out_ptr):
    """a gather as comm.hip must post it: each non-root rank ONE send of exactly its bytes to the root (none when it has
    none); the root ONE group holding a receive per remote rank with bytes, each at its final offset, and no sends"""
    moves = p2p(calls)
    if rank != root:
        want = [("ncclSend", root, sizes[rank], local_ptr, 0)] if sizes[rank] else []
        assert [(c["op"], c["peer"], c["bytes"], c["ptr"], c["group"]) for c in moves] == want, calls
        assert all(c["rc"] == 0 for c in calls), calls
        return
    remote = [r for r in range(world) if r != root and sizes[r]]
    starts = [c for c in calls if c["op"] == "ncclGroupStart"]
    ends = [c for c in calls if c["op"] == "ncclGroupEnd"]
    if not remote:
        assert not moves and not starts, calls
        return
    assert len(starts) == 1 and len(ends) == 1 and ends[0]["rc"] == 0, calls
    g = starts[0]["group"]
    assert g > 0 and ends[0]["group"] == g
    assert [(c["op"], c["peer"], c["bytes"], c["ptr"], c["group"]) for c in moves] == \
        [("ncclRecv", r, sizes[r], out_ptr + offsets[r], g) for r in remote], calls


# ------------------------------------------------------------------------------------------------
# rank processes
# ------------------------------------------------------------------------------------------------

def _rank_env(logbase, extra=None):
    """before the first exchange call of the process: comm.hip looks its library up once"""
    os.environ["MI355_RCCL_LIB"] = LIB
    os.environ["MI355_EXCHANGE"] = "rccl"
    os.environ["MI355_LOOPBACK_LOG"] = logbase
    os.environ.setdefault("MI355_LOOPBACK_TIMEOUT_S", "60")
    os.environ.update(extra or {})


def _entry(fn, rank, world, port, backend, args, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    try:
        dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=180))
        fn(rank, world, *args)
        q.put((rank, "ok"))
    except BaseException:
        q.put(f"rank {rank} of {world}:\n{traceback.format_exc()}")
        raise
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def run_ranks(fn, world, *args, backend="gloo", timeout=RANK_TIMEOUT_S):
    """`world` spawned rank processes running fn(rank, world, *args); every one must finish cleanly within `timeout`"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_entry, args=(fn, r, world, port, backend, args, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = join_or_kill(procs, timeout, q)
    assert sorted(m[0] for m in got if isinstance(m, tuple)) == list(range(world)), got


def _rank_bytes(seed, r, size):
    """rank r's slice in a gather test: known to every rank"""
    return np.random.default_rng(seed * 64 + r).integers(0, 256, size, dtype=np.uint8)


def capi_worker(rank, world, logbase):
    """the C ABI's exchange entry points with a communicator of `world` ranks"""
    _rank_env(logbase)
    from oracle import oracle
    from shared_simd_scan_amd import ScanEngine, lib
    from shared_simd_scan_amd.sharded import bitmap_bytes, shard_rows

    L, O, eng, log = lib(), oracle(), ScanEngine(0), Log(logbase, rank)
    dev = torch.device("cuda", 0)
    ident = (C.c_uint8 * 128)()
    if rank == 0:
        assert L.mi355_comm_get_unique_id(ident) == 0, L.mi355_last_error()
    obj = [bytes(ident)]
    dist.broadcast_object_list(obj, src=0)
    ident = (C.c_uint8 * 128).from_buffer_copy(obj[0])
    comm = C.c_void_p()
    assert L.mi355_comm_create(eng._ctx, world, rank, ident, C.byref(comm)) == 0, L.mi355_last_error()
    w, r = C.c_int(), C.c_int()
    assert L.mi355_comm_info(comm, C.byref(w), C.byref(r)) == 0 and (w.value, r.value) == (world, rank)
    u64 = C.c_uint64 * world

    # an overlapping layout is refused on EVERY rank before anything moves: nobody is left in a send (the gathers below
    # would hang or fail otherwise)
    mark = log.mark()
    ov = torch.zeros(256, dtype=torch.uint8, device=dev)
    rc = L.mi355_gather_bitmaps_at_dev(eng._ctx, comm, ov.data_ptr(), u64(*[100] * world), u64(*[50 * k for k in range(world)]),
                                       0, ov.data_ptr())
    assert rc == E_INVALID and b"overlap" in L.mi355_last_error(), (rc, L.mi355_last_error())
    assert not p2p(log.since(mark))

    # gathers: packed, at offsets with gaps in reverse rank order, a zero-byte non-root rank, a zero-byte root
    for root in sorted({0, world - 1}):
        for li, layout in enumerate(("packed", "gaps", "zero_peer", "zero_root")):
            seed = 10 * root + li
            sizes = [1000 + 37 * k + 5 * root for k in range(world)]
            if layout == "zero_peer":
                sizes[(root + 1) % world] = 0
            if layout == "zero_root":
                sizes[root] = 0
            if layout == "gaps":
                offs, at = [0] * world, 16
                for k in reversed(range(world)):
                    offs[k], at = at, at + sizes[k] + 11 * (k + 1)
            else:
                offs = [sum(sizes[:k]) for k in range(world)]
            span = max(o + s for o, s in zip(offs, sizes)) + 64
            local = torch.from_numpy(_rank_bytes(seed, rank, sizes[rank])).to(dev)
            local_ptr = local.data_ptr() if sizes[rank] else None
            out = torch.full((span,), 0xEE, dtype=torch.uint8, device=dev) if rank == root else None
            out_ptr = out.data_ptr() if out is not None else None
            mark = log.mark()
            if layout == "packed":
                rc = L.mi355_gather_bitmaps_dev(eng._ctx, comm, local_ptr, u64(*sizes), root, out_ptr)
            else:
                rc = L.mi355_gather_bitmaps_at_dev(eng._ctx, comm, local_ptr, u64(*sizes), u64(*offs), root, out_ptr)
            torch.cuda.synchronize()
            assert rc == 0, (layout, root, L.mi355_last_error())
            if rank == root:
                want = np.full(span, 0xEE, dtype=np.uint8)
                for k in range(world):
                    want[offs[k]: offs[k] + sizes[k]] = _rank_bytes(seed, k, sizes[k])
                assert np.array_equal(out.cpu().numpy(), want), (layout, root)  # slices, gaps and the tail
            check_gather_log(log.since(mark), rank, world, root, sizes, offs, local_ptr or 0, out_ptr or 0)

    # all-reduce of the hit counts: count 1 and 7, values above 2^32, the last slot wraps modulo 2^64 with 4 ranks
    for count in (1, 7):
        def vals(k):
            v = [(k + 1) * (1 << 33) + 1000 * i + k for i in range(count)]
            v[-1] = (1 << 62) + k
            return v

        want = [sum(vals(k)[i] for k in range(world)) % (1 << 64) for i in range(count)]
        t = torch.tensor(vals(rank), dtype=torch.int64, device=dev)
        mark = log.mark()
        assert L.mi355_allreduce_hits_dev(eng._ctx, comm, t.data_ptr(), count) == 0, L.mi355_last_error()
        got = [x % (1 << 64) for x in t.cpu().tolist()]
        assert got == want, (count, got, want)
        calls = log.since(mark)
        assert [(c["op"], c["bytes"], c["ptr"]) for c in calls] == [("ncclAllReduce", 8 * count, t.data_ptr())], calls

    # sharded scans: each rank generates its own shard; the root's bitmap and every rank's hit count = the whole column's
    for ci, c in enumerate((1, 9, 12, 17, 32)):
        n = 8192 * (2 * world - 1) + 8 * ci + 3  # shards of 16384 rows, a ragged last one
        ranges = shard_rows(n, world)
        rows = [b - a for a, b in ranges]
        assert rows[-1] % 8 and rows[-1] != rows[0]
        root = 0 if ci % 2 == 0 else world - 1
        col = eng.generate("splitmix", rows[rank], c, 42, first_row=ranges[rank][0])
        vals_all = O.gen_values("splitmix", n, c, 42)
        packed = O.pack(vals_all, c)
        key = int(vals_all[n // 3])
        lo, hi = (1, 1) if c == 1 else ((1 << c) // 5, (1 << c) // 3)
        nb = bitmap_bytes(n)
        for kind in ("eq", "range"):
            local = torch.empty(bitmap_bytes(rows[rank]), dtype=torch.uint8, device=dev)
            full = torch.full((nb + 64,), 0xEE, dtype=torch.uint8, device=dev) if rank == root else None
            hits = torch.zeros(1, dtype=torch.int64, device=dev)
            args = (full.data_ptr() if full is not None else None, hits.data_ptr())
            mark = log.mark()
            if kind == "eq":
                rc = L.mi355_sharded_scan_eq_dev(eng._ctx, comm, col.data.data_ptr(), c, int(np.int32(np.uint32(key))),
                                                 local.data_ptr(), u64(*rows), root, *args)
                ref, ref_hits = O.scan_eq(packed, n, c, key)
            else:
                rc = L.mi355_sharded_scan_range_dev(eng._ctx, comm, col.data.data_ptr(), c, lo, hi, local.data_ptr(), u64(*rows),
                                                    root, *args)
                ref, ref_hits = O.scan_range(packed, n, c, lo, hi)
            torch.cuda.synchronize()
            assert rc == 0, (c, kind, L.mi355_last_error())
            assert int(hits.item()) == ref_hits, (c, kind, rank, int(hits.item()), ref_hits)
            if rank == root:
                got = full.cpu().numpy()
                assert np.array_equal(got[:nb], ref), (c, kind, root)
                assert (got[nb:] == 0xEE).all(), (c, kind)
            calls = log.since(mark)
            sizes = [bitmap_bytes(x) for x in rows]
            check_gather_log(calls, rank, world, root, sizes, [sum(sizes[:k]) for k in range(world)], local.data_ptr(),
                             full.data_ptr() if full is not None else 0)
            assert [x["bytes"] for x in calls if x["op"] == "ncclAllReduce"] == [8]

    # a shard other than the last that is not a whole number of bitmap bytes: refused on every rank, nothing moves
    c, n = 9, 8192 * (2 * world - 1) + 5
    rows = [b - a for a, b in shard_rows(n, world)]
    rows[0] -= 5
    col = eng.generate("splitmix", rows[rank], c, 42)
    local = torch.empty(bitmap_bytes(rows[rank]), dtype=torch.uint8, device=dev)
    full = torch.empty(bitmap_bytes(n), dtype=torch.uint8, device=dev)
    hits = torch.zeros(1, dtype=torch.int64, device=dev)
    mark = log.mark()
    rc = L.mi355_sharded_scan_eq_dev(eng._ctx, comm, col.data.data_ptr(), c, 3, local.data_ptr(), u64(*rows), 0,
                                     full.data_ptr(), hits.data_ptr())
    assert rc == E_INVALID and b"multiples of 8 rows" in L.mi355_last_error(), (rc, L.mi355_last_error())
    assert not p2p(log.since(mark)) and not [x for x in log.since(mark) if x["op"] == "ncclAllReduce"]
    torch.cuda.synchronize()
    dist.barrier()

    assert L.mi355_comm_destroy(comm) == 0
    assert log.calls()[-1]["op"] == "ncclCommDestroy"


def check_column(sc, O, n, c, base_row, dst, rank, world, log=None, dense_rerun=False):
    """ShardedColumn end to end against the oracle over the whole column (the checks of test_sharded_gloo.gpu_worker,
    with the root at `dst`); with a call log, that scan_pipelined's gathers ran on its side stream"""
    from shared_simd_scan_amd.sharded import SHARD_ALIGN, RcclExchange, bitmap_bytes

    eng = sc.engine
    sc.generate("splitmix", 42)
    vals = O.gen_values("splitmix", n, c, 42, first=base_row)
    packed = O.pack(vals, c)
    key = int(vals[n // 2]) if n else 1
    lo, hi = (1 << c) // 4, (1 << c) // 2
    ref, ref_hits = O.scan_eq(packed, n, c, key)
    ref_r, ref_hits_r = O.scan_range(packed, n, c, lo, hi)

    def same(got, want, what):
        full, hits = got
        bm, h = want
        assert int(hits.item()) == h, (what, rank, int(hits.item()), h)  # the column-wide count, on every rank
        if rank == dst:
            assert full is not None and full.is_cuda and np.array_equal(full.cpu().numpy(), bm), (what, dst)
        else:
            assert full is None, what

    same(sc.scan(key, dst=dst), (ref, ref_hits), "scan")
    same(sc.scan_range(lo, hi, dst=dst), (ref_r, ref_hits_r), "scan_range")
    per_rank = max(b - a for a, b in sc.ranges)
    remote_bytes = sum(bitmap_bytes(b - a) for r, (a, b) in enumerate(sc.ranges) if r != dst)
    for chunks in (1, 3, -(-per_rank // SHARD_ALIGN) + 2):  # the last: more chunks than pieces
        mark = log.mark() if log else 0
        same(sc.scan_pipelined(key, dst=dst, chunks=chunks), (ref, ref_hits), f"scan_pipelined chunks={chunks}")
        if isinstance(sc.exchange, RcclExchange):
            assert sc._side is not None
            side, main = sc._side[2].cuda_stream, eng.stream.cuda_stream
            assert side != main
            if log:
                calls = log.since(mark)
                moves = p2p(calls)
                # every piece's transfer on the side stream, and together exactly this rank's bytes (sent or received)
                assert all(x["stream"] == side for x in moves), (side, main, moves)
                if rank == dst:
                    assert {x["op"] for x in moves} <= {"ncclRecv"} and sum(x["bytes"] for x in moves) == remote_bytes, moves
                else:
                    assert {x["op"] for x in moves} <= {"ncclSend"} and sum(x["bytes"] for x in moves) == bitmap_bytes(sc.rows)
                assert [x["stream"] for x in calls if x["op"] == "ncclAllReduce"] == [main], calls

    for op, a, b, want in (("==", key, 0, vals == key), ("between", lo, hi, (vals >= lo) & (vals <= hi))):
        if op == "between" and dense_rerun:
            # the first run's capacity (1 row in 16, at least 2^16) is too small for this shard: the exact re-run happens
            mine = int(want[sc.first: sc.last].sum())
            assert mine > max(1 << 16, sc.rows // 16), mine
        ids, nids = sc.select(op, a, dst=dst, b=b)
        want_ids = np.nonzero(want)[0].astype(np.int64) + base_row
        assert nids == want_ids.shape[0], (op, nids, want_ids.shape[0])
        if rank == dst:
            assert ids.is_cuda and np.array_equal(ids.cpu().numpy(), want_ids), op
        else:
            assert ids is None

    local_bm, _ = eng.scan_range(lo, hi, sc.col) if sc.rows else (None, None)
    v = vals.astype(np.uint64)
    sel = v[(v >= lo) & (v <= hi)]
    assert sc.aggregate(mask=local_bm) == ((int(sel.sum()), int(sel.shape[0]), int(sel.min()), int(sel.max()))
                                           if sel.shape[0] else (0, 0, None, 0))
    assert sc.aggregate() == ((int(v.sum()), n, int(v.min()), int(v.max())) if n else (0, 0, None, 0))


def column_worker(rank, world, n, c, base_row, dst, logbase, dense_rerun):
    _rank_env(logbase)
    from oracle import oracle
    from shared_simd_scan_amd import ScanEngine
    from shared_simd_scan_amd.sharded import RcclExchange, ShardedColumn

    sc = ShardedColumn(n, c, engine=ScanEngine(0), base_row=base_row)
    assert isinstance(sc.exchange, RcclExchange) and sc.exchange.info() == (world, rank)
    check_column(sc, oracle(), n, c, base_row, dst, rank, world, log=Log(logbase, rank), dense_rerun=dense_rerun)
    torch.cuda.synchronize()
    sc.exchange.close()


def bootstrap_worker(rank, world, mode, logbase):
    """a bootstrap that fails on one rank: ExchangeUnavailable on EVERY rank, and no communicator left behind"""
    _rank_env(logbase, {"MI355_LOOPBACK_TIMEOUT_S": "30"})
    if mode == "no_library" and rank == 1:
        os.environ["MI355_RCCL_LIB"] = "/nonexistent/no-such-librccl.so"
    if mode == "fail_init":
        os.environ["MI355_LOOPBACK_FAIL_INIT"] = "1"
    from shared_simd_scan_amd import ScanEngine
    from shared_simd_scan_amd.sharded import ExchangeUnavailable, ShardedColumn

    eng, log = ScanEngine(0), Log(logbase, rank)
    t0 = time.monotonic()
    try:
        ShardedColumn(100_000, 9, engine=eng)
    except ExchangeUnavailable as e:
        # read the log while `e` still holds the half-built exchange: what is destroyed here was destroyed by the failure
        # path itself, not by a later garbage collection
        calls = log.calls()
        inits = [x for x in calls if x["op"] == "ncclCommInitRank"]
        destroys = [x for x in calls if x["op"] == "ncclCommDestroy"]
        if mode == "no_library":
            assert not inits and not destroys, calls  # step 1 fails somewhere: no rank goes on to create a communicator
            assert ("librccl not found" in str(e)) == (rank == 1), str(e)
        elif rank == 1:
            assert len(inits) == 1 and inits[0]["rc"] != 0 and not destroys, calls
        else:
            assert len(inits) == 1 and inits[0]["rc"] == 0, calls
            assert len(destroys) == 1 and calls.index(destroys[0]) > calls.index(inits[0]), calls
        assert time.monotonic() - t0 < 30, time.monotonic() - t0
    else:
        raise AssertionError("the exchange was set up although a rank failed")


def nccl_world1_worker(rank, world, n, c):
    """torch's nccl group of ONE rank, then ShardedColumn with the exchange make_exchange picks for it: the real librccl"""
    for k in ("MI355_EXCHANGE", "MI355_RCCL_LIB", "MI355_LOOPBACK_LOG"):
        os.environ.pop(k, None)  # the exchange make_exchange chooses, on the library comm.hip finds by itself
    from oracle import oracle
    from shared_simd_scan_amd import ScanEngine
    from shared_simd_scan_amd.sharded import RcclExchange, ShardedColumn

    sc = ShardedColumn(n, c, engine=ScanEngine(0))
    assert isinstance(sc.exchange, RcclExchange) and sc.exchange.info() == (1, 0)
    check_column(sc, oracle(), n, c, 0, 0, rank, world)
    torch.cuda.synchronize()
    sc.exchange.close()


# ------------------------------------------------------------------------------------------------
# CPU: the stand-in itself
# ------------------------------------------------------------------------------------------------

def test_loopback_library_builds():
    C.CDLL(build_library())


def test_loopback_exports_exactly_what_comm_hip_resolves():
    """a new sym("nccl...") lookup in comm.hip fails here until the stand-in grows it"""
    wanted = set(re.findall(r'sym\("(nccl\w+)"\)', open(COMM_SRC).read()))
    assert len(wanted) >= 9, wanted
    res = subprocess.run(["nm", "-D", "--defined-only", build_library()], capture_output=True, text=True, check=True)
    exported = {ln.split()[-1] for ln in res.stdout.splitlines() if re.search(r"\bT nccl\w+$", ln)}
    assert exported == wanted


class _UniqueId(C.Structure):
    _fields_ = [("internal", C.c_char * 128)]


def _bind(L):
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    L.ncclGetUniqueId.argtypes = [C.POINTER(_UniqueId)]
    L.ncclCommInitRank.argtypes = [C.POINTER(vp), i, _UniqueId, i]
    L.ncclCommDestroy.argtypes = [vp]
    L.ncclSend.argtypes = [vp, sz, i, i, vp, vp]
    L.ncclRecv.argtypes = [vp, sz, i, i, vp, vp]
    L.ncclAllReduce.argtypes = [vp, vp, sz, i, i, vp, vp]
    L.ncclGetErrorString.restype = C.c_char_p
    return L


NCCL_UINT8, NCCL_UINT64, NCCL_FLOAT32, NCCL_SUM = 1, 5, 7, 0
SYSTEM_ERROR, INVALID_ARGUMENT, INVALID_USAGE = 2, 4, 5


def host_transport_worker(rank, world, ident, logbase, q):
    """the stand-in on host memory (MI355_LOOPBACK_HOST_MEM=1): mesh, grouped receives at a root other than 0,
    all-reduce with wrap-around, a size mismatch caught, the refusal of what it does not implement"""
    try:
        os.environ.update(MI355_LOOPBACK_HOST_MEM="1", MI355_LOOPBACK_TIMEOUT_S="20", MI355_LOOPBACK_LOG=logbase)
        L = _bind(C.CDLL(LIB))
        comm = C.c_void_p()
        assert L.ncclCommInitRank(C.byref(comm), world, _UniqueId.from_buffer_copy(ident), rank) == 0
        root = world - 1
        data = [bytes((r * 7 + i) % 251 for i in range(3000 + 100 * r)) for r in range(world)]
        if rank != root:
            buf = C.create_string_buffer(data[rank], len(data[rank]))
            assert L.ncclSend(buf, len(data[rank]), NCCL_UINT8, root, comm, None) == 0
        else:
            bufs = {r: C.create_string_buffer(len(data[r])) for r in range(world) if r != root}
            assert L.ncclGroupStart() == 0
            for r, b in bufs.items():
                assert L.ncclRecv(b, len(data[r]), NCCL_UINT8, r, comm, None) == 0
            assert L.ncclGroupEnd() == 0
            assert all(b.raw == data[r] for r, b in bufs.items())
        vals = (C.c_uint64 * 3)((1 << 63) + rank, 5, 1 << 40)
        assert L.ncclAllReduce(vals, vals, 3, NCCL_UINT64, NCCL_SUM, comm, None) == 0
        assert list(vals) == [((1 << 63) * world + world * (world - 1) // 2) % (1 << 64), 5 * world, world << 40]
        # rank 0 sends 10 bytes, the root expects 11: the root's receive fails, and the channel stays in step
        if rank == 0:
            assert L.ncclSend(C.create_string_buffer(10), 10, NCCL_UINT8, root, comm, None) == 0
        elif rank == root:
            assert L.ncclRecv(C.create_string_buffer(11), 11, NCCL_UINT8, 0, comm, None) == INVALID_USAGE
        one = (C.c_uint64 * 1)(1)
        assert L.ncclAllReduce(one, one, 1, NCCL_UINT64, NCCL_SUM, comm, None) == 0 and one[0] == world
        assert L.ncclAllReduce(one, one, 1, NCCL_FLOAT32, NCCL_SUM, comm, None) == INVALID_ARGUMENT
        assert L.ncclSend(one, 1, NCCL_UINT64, root, comm, None) == INVALID_ARGUMENT
        assert L.ncclSend(one, 1, NCCL_UINT8, rank, comm, None) == INVALID_ARGUMENT  # to itself
        assert L.ncclCommDestroy(comm) == 0
        q.put((rank, "ok"))
    except BaseException:
        q.put(f"rank {rank}:\n{traceback.format_exc()}")
        raise


def test_loopback_transport_on_host_memory(tmp_path):
    L = _bind(C.CDLL(build_library()))
    ident = _UniqueId()
    assert L.ncclGetUniqueId(C.byref(ident)) == 0
    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=host_transport_worker, args=(r, world, bytes(ident), str(tmp_path / "log"), q))
             for r in range(world)]
    for p in procs:
        p.start()
    got = join_or_kill(procs, 120, q)
    assert sorted(m[0] for m in got if isinstance(m, tuple)) == list(range(world)), got
    root = [ln.split()[0] for ln in open(tmp_path / f"log.{world - 1}")]
    assert root[:6] == ["ncclCommInitRank", "ncclGroupStart", "ncclRecv", "ncclRecv", "ncclGroupEnd", "ncclAllReduce"], root
    assert [ln.split()[0] for ln in open(tmp_path / "log.0")][:2] == ["ncclCommInitRank", "ncclSend"]


def test_loopback_missing_peer_is_an_error_not_a_hang(monkeypatch, capfd):
    """a world of 2 whose second rank never comes: ncclCommInitRank gives up at the deadline with ncclSystemError"""
    monkeypatch.setenv("MI355_LOOPBACK_TIMEOUT_S", "2")
    L = _bind(C.CDLL(build_library()))
    ident = _UniqueId()
    assert L.ncclGetUniqueId(C.byref(ident)) == 0
    comm = C.c_void_p()
    t0 = time.monotonic()
    assert L.ncclCommInitRank(C.byref(comm), 2, ident, 0) == SYSTEM_ERROR and not comm.value
    assert time.monotonic() - t0 < 30
    assert "never connected" in capfd.readouterr().err


# ------------------------------------------------------------------------------------------------
# GPU: 2..4 ranks on cuda:0 through the stand-in
# ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3, 4])
def test_c_abi_exchange_multi_rank(world, tmp_path):
    build_library()
    run_ranks(capi_worker, world, str(tmp_path / "calls"))


@pytest.mark.gpu
@pytest.mark.parametrize("world,n,c,base_row,dst,dense_rerun", [
    (2, 2_000_003, 12, 7_000_000_000, 1, True),   # row ids above 2^32, root = last rank, the select's exact re-run
    (3, 8192 * 7 + 77, 9, 0, 0, False),
    (4, 8192 * 13 + 5, 17, 7_000_000_000, 3, False),
    (2, 5000, 12, 0, 0, False),                    # rank 1 owns no rows
    (2, 5000, 12, 0, 1, False),                    # ... and is the root
])
def test_sharded_column_over_rccl_exchange(world, n, c, base_row, dst, dense_rerun, tmp_path):
    build_library()
    run_ranks(column_worker, world, n, c, base_row, dst, str(tmp_path / "calls"), dense_rerun)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,world", [("no_library", 2), ("fail_init", 3)])
def test_rccl_bootstrap_failure_is_seen_on_every_rank(mode, world, tmp_path):
    build_library()
    run_ranks(bootstrap_worker, world, mode, str(tmp_path / "calls"), timeout=180)


@pytest.mark.gpu
def test_bench_two_ranks_through_the_c_abi_exchange(tmp_path):
    """bench.py itself, unchanged, with the C ABI exchange on the stand-in: its own asserts check the gathered slices"""
    logbase = str(tmp_path / "calls")
    res, line = _bench_2ranks({"MI355_EXCHANGE": "rccl", "MI355_RCCL_LIB": build_library(), "MI355_LOOPBACK_LOG": logbase},
                              ("--pipelined-gather",))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert line["gather_via"] == "mi355 C ABI (RCCL)", line
    assert line["comm_world"] == 2 and line["ranks_seen"] == 2, line
    assert line["gather_ms"] > 0 and line["pipelined_scan_gather_ms"] > 0 and "gather_error" not in line, line
    calls0, calls1 = Log(logbase, 0).calls(), Log(logbase, 1).calls()
    assert [x["rc"] for x in calls0 + calls1 if x["op"] == "ncclCommInitRank"] == [0, 0]
    assert any(x["op"] == "ncclSend" and x["peer"] == 0 for x in calls1)
    assert any(x["op"] == "ncclRecv" and x["peer"] == 1 for x in calls0)


@pytest.mark.gpu
def test_sharded_column_world1_on_the_real_rccl():
    """one rank of torch's nccl backend: make_exchange picks RcclExchange on the real librccl; scan_pipelined's side
    engine and event hand-off then run with real asynchrony (the stand-in synchronises)"""
    run_ranks(nccl_world1_worker, 1, 8192 * 40 + 13, 9, backend="nccl")
