"""The kernel-path case table and what runs a case: CASES is the one list of (call, options) -> kernel (with its template
arguments) that the call must launch, as mi355_ctx_last_launch reports it.  test_kernel_paths runs it on the GPU, test_launch_plan
through the launchers' dry run (tests/cpp/launch_dry_run.cpp, built and called here), test_min_contract and test_graph_capture
borrow its sizes, columns and the selection check.  A plain module like support.py."""
import ctypes as C
import glob
import os
import subprocess
from dataclasses import dataclass

import numpy as np

from support import CSRC, ROOT, SENTINEL, Guarded, base_name

N_SMALL = 10 * 4096 + 77  # ten shared-scan wave tiles (five at 128 values per lane) and a ragged tail
N_FLUSH = 19_000_077      # 4639 tiles of 4096 rows: 1159 per wave of a 4-wave grid (> 2 x kPackedFlushTiles = 1024)
N_BYTES = 1_100_077       # 269 tiles: 67 per wave, each at least one step of the linear kernels' 8-bit counters (flush: 31)
FLUSH_TILES = 1100
BYTE_STEPS = 62
SHARED_TILE_ROWS = 4096   # 64 lanes x 64 values: the shared scans' wave tile
WAVES_PER_BLOCK = 4

LAUNCHER_SET = {0x20000: "short last table attached (shared_linear2_kernel)", 0x100000: "aligned output image (shared_linear_kernel)"}
# option bits of "kernel_flags" (DESIGN.md section 8): the shared scans' switches and the selection's
SHARED_BITS = [1, 2, 4, 8, 16, 32, 64, 128, 256, 8192, 16384, 32768, 131072, 262144, 524288, 1048576, 4194304, 8388608]
SELECT_BITS = [2048, 4096, 2048 + 4096]
TIMING_ABLATIONS = {512: "selection: no expansion (wrong ids by construction)", 1024: "selection: no look-back (wrong ids by construction)"}
UNUSED_BITS = {65536: "kernel bit 0x1000: read nowhere (reserved in csrc/switches.hpp: it stays out of the kernels' word)"}


@dataclass(frozen=True)
class Case:
    id: str
    op: str                # shared, scan_eq, scan_range, combine, in, scan2, select, decompress, generate, pack_u32,
                           # bitmap_and, bitmap_count, rowids, gather, aggregate, histogram
    expect: tuple          # one label pattern per launch, in order ("*" = any one template argument)
    c: int = 9
    n: int = N_SMALL
    P: int = 1
    layout: int = 0        # shared: 0 per-predicate, 1 linear
    hits: bool = True
    opts: tuple = ()       # (("kernel_flags", 32768), ("scan_nt_stores", 1), ...)
    set_bits: int = 0      # flags bits the (last) launch must carry
    clear_bits: int = 0    # ... and must not
    bit: int = 0           # the option bit this case is about: without it the launch record differs
    column: str = "random"  # "const": every value one key (all hits), "alt": two values alternating
    min_tiles: int = 0     # grid capped to 4 waves; every wave walks more than this many tiles

    def opt(self, name, default=0):
        return dict(self.opts).get(name, default)


def _cap(*extra):
    return (("grid_cus", 1), ("max_blocks_per_cu", 1)) + tuple(extra)


CASES = [
    # ---- shared scans, P = 2: two equality decodes; P <= 8: one-pass LUT ------------------------------------------------------
    Case("pair_pp", "shared", ("shared_pair_kernel<9, 34, 128>",), P=2),
    Case("pair_linear_nt", "shared", ("shared_pair_kernel<9, 18, 64>",), P=2, layout=1, opts=(("scan_nt_stores", 1),)),
    Case("pair_bit32_lut", "shared", ("shared_lut_kernel<9, 34, 128, 0, false>",), P=2, opts=(("kernel_flags", 32),), bit=32),
    Case("lut_pp_vpl128", "shared", ("shared_lut_kernel<9, 34, 128, 0, false>",), P=4),
    Case("lut_pp_vpl64_opt", "shared", ("shared_lut_kernel<9, 34, 64, 0, false>",), P=4, opts=(("shared_vpl", 64),)),
    Case("lut_pp", "shared", ("shared_lut_kernel<9, 34, 64, 0, false>",), P=8),
    Case("lut_pp_nt", "shared", ("shared_lut_kernel<9, 18, 64, 0, false>",), P=8, opts=(("scan_nt_stores", 1),)),
    Case("lut_pp_plain", "shared", ("shared_lut_kernel<9, 2, 64, 0, false>",), P=8, opts=(("scan_nt_stores", 0),)),
    Case("lut_linear", "shared", ("shared_lut_kernel<9, 34, 64, 1, false>",), P=8, layout=1),
    Case("lut_linear_nt", "shared", ("shared_lut_kernel<9, 18, 64, 1, false>",), P=5, layout=1, opts=(("scan_nt_stores", 1),)),
    Case("lut_linear_plain", "shared", ("shared_lut_kernel<17, 2, 64, 1, false>",), P=7, c=17, layout=1, opts=(("scan_nt_stores", 0),)),
    # byte-entry multi-pass LUT (linear rows without hit counts)
    Case("lut_multi_c17", "shared", ("shared_lut_kernel<17, 2, 64, 1, true>",), P=170, c=17, layout=1, hits=False),
    Case("lut_multi_bit2", "shared", ("shared_lut_kernel<9, 2, 64, 1, true>",), P=12, layout=1, hits=False,
         opts=(("kernel_flags", 2),), bit=2),
    # ---- per-predicate, 32 keys per lookup ---------------------------------------------------------------------------------
    Case("wide3_rc0", "shared", ("shared_wide3_kernel<9, 2, 0, false>",), P=24, hits=False),
    Case("wide3_rc1", "shared", ("shared_wide3_kernel<9, 2, 1, false>",), P=24),
    Case("wide3_rc1_nt", "shared", ("shared_wide3_kernel<9, 18, 1, false>",), P=24, opts=(("scan_nt_stores", 1),)),
    Case("wide3_rc2", "shared", ("shared_wide3_kernel<9, 2, 2, false>",), P=40),
    Case("wide3_rc0_big", "shared", ("shared_wide3_kernel<17, 2, 0, true>",), P=24, c=17, hits=False),
    Case("wide3_rc1_big", "shared", ("shared_wide3_kernel<17, 2, 1, true>",), P=24, c=17),
    Case("wide3_rc2_big", "shared", ("shared_wide3_kernel<17, 2, 2, true>",), P=40, c=17),
    Case("wide3_rc1_bit8192_bytes", "shared", ("shared_wide3_kernel<17, 2, 1, false>",), P=24, c=17,
         opts=(("kernel_flags", 8192),), bit=8192),
    Case("wide3_rc2_c12", "shared", ("shared_wide3_kernel<12, 2, 2, false>",), P=48, c=12),
    Case("wide3_unused_bit65536", "shared", ("shared_wide3_kernel<9, 2, 2, false>",), P=40, opts=(("kernel_flags", 65536),), bit=65536),
    Case("chain_bit16384", "shared", ("shared_general_kernel<17, 2, 64>",), P=16, c=17, opts=(("kernel_flags", 16384),), bit=16384),
    Case("chain_bit64", "shared", ("shared_general_kernel<9, 2, 64>",), P=24, opts=(("kernel_flags", 64),), bit=64),
    Case("chain_tables_too_big", "shared", ("shared_general_kernel<32, 2, 64>",), P=800, c=32, hits=False, n=4096 + 77),
    Case("wide2_hist", "shared", ("shared_wide2_kernel<9, 2, 64, 0, false>",), P=64),
    Case("wide2_hist_nt", "shared", ("shared_wide2_kernel<9, 18, 64, 0, false>",), P=64, opts=(("scan_nt_stores", 1),)),
    Case("wide2_big", "shared", ("shared_wide2_kernel<17, 2, 64, 0, true>",), P=100, c=17),
    Case("wide2_bit1_drain", "shared", ("shared_wide2_kernel<9, 2, 64, 0, false>",), P=64, opts=(("kernel_flags", 1),), bit=1),
    Case("wide2_bit4_rotate", "shared", ("shared_wide2_kernel<9, 2, 64, 0, false>",), P=64, opts=(("kernel_flags", 4),), bit=4),
    Case("wide2_bit8_reductions", "shared", ("shared_wide2_kernel<9, 2, 64, 0, false>",), P=24, opts=(("kernel_flags", 8),), bit=8),
    Case("wide2_rc1_bit32768", "shared", ("shared_wide2_kernel<9, 2, 64, 1, false>",), P=24, opts=(("kernel_flags", 32768),), bit=32768),
    Case("wide2_rc2_bit32768", "shared", ("shared_wide2_kernel<9, 2, 64, 2, false>",), P=40, opts=(("kernel_flags", 32768),), bit=32768),
    Case("wide_pp_bit2", "shared", ("shared_wide_kernel<9, 2, 64, 0>",), P=24, opts=(("kernel_flags", 2),), bit=2),
    Case("wide_pp_bit2_nt", "shared", ("shared_wide_kernel<9, 18, 64, 0>",), P=24, opts=(("kernel_flags", 2), ("scan_nt_stores", 1))),
    Case("wide_pp_bit1_drain", "shared", ("shared_wide_kernel<9, 2, 64, 0>",), P=24, opts=(("kernel_flags", 3),), bit=1),
    Case("wide_linear_bit2", "shared", ("shared_wide_kernel<9, 2, 64, 1>",), P=24, layout=1, opts=(("kernel_flags", 2),), bit=2),
    # ---- linear rows ---------------------------------------------------------------------------------------------------------
    Case("linear_p9", "shared", ("shared_linear_kernel<9, 2, 1>",), P=9, layout=1, clear_bits=0x100000),
    Case("linear_p16_two_rows", "shared", ("shared_linear_kernel<12, 2, 2>",), P=16, c=12, layout=1),
    Case("linear_p16_bit16", "shared", ("shared_linear_kernel<12, 2, 1>",), P=16, c=12, layout=1, opts=(("kernel_flags", 16),), bit=16),
    Case("linear_image", "shared", ("shared_linear_kernel<9, 2, 1>",), P=47, layout=1, set_bits=0x100000),
    Case("linear_p12_bit256", "shared", ("shared_linear_kernel<9, 2, 1>",), P=12, layout=1, hits=False,
         opts=(("kernel_flags", 256),), bit=256, clear_bits=0x100000),
    Case("linear_bit128_c17", "shared", ("shared_linear2_kernel<17, 2>",), P=170, c=17, layout=1, hits=False,
         opts=(("kernel_flags", 128),), bit=128, set_bits=0x20000),
    Case("linear_p33_bit131072_image", "shared", ("shared_linear_kernel<9, 2, 1>",), P=33, layout=1,
         opts=(("kernel_flags", 131072),), bit=131072, set_bits=0x100000),
    Case("linear_p33_bit262144_no_image", "shared", ("shared_linear_kernel<9, 2, 1>",), P=33, layout=1,
         opts=(("kernel_flags", 131072 + 262144),), bit=262144, clear_bits=0x100000),
    Case("linear_p121_bit8388608_image", "shared", ("shared_linear_kernel<9, 2, 1>",), P=121, layout=1,
         opts=(("kernel_flags", 8388608),), bit=8388608, set_bits=0x100000),
    Case("linear2_detached", "shared", ("shared_linear2_kernel<9, 2>",), P=12, layout=1, hits=False, clear_bits=0x20000),
    Case("linear2_attached", "shared", ("shared_linear2_kernel<9, 2>",), P=65, layout=1, set_bits=0x20000),
    Case("linear2_p33_bit524288", "shared", ("shared_linear2_kernel<9, 2>",), P=33, layout=1,
         opts=(("kernel_flags", 131072 + 524288),), bit=524288, clear_bits=0x20000),
    Case("linear_p65_bit1048576_never", "shared", ("shared_linear_kernel<9, 2, 1>",), P=65, layout=1,
         opts=(("kernel_flags", 1048576),), bit=1048576, clear_bits=0x120000),
    Case("linear2_p121_bit4194304_always", "shared", ("shared_linear2_kernel<9, 2>",), P=121, layout=1,
         opts=(("kernel_flags", 4194304),), bit=4194304, set_bits=0x20000),
    Case("linear3_rc0", "shared", ("shared_linear3_kernel<9, 2, 0, false>",), P=33, layout=1, hits=False),
    Case("linear3_rc1", "shared", ("shared_linear3_kernel<9, 2, 1, false>",), P=32, layout=1),
    Case("linear3_rc2", "shared", ("shared_linear3_kernel<9, 2, 2, false>",), P=40, layout=1),
    Case("linear3_rc2_big", "shared", ("shared_linear3_kernel<17, 2, 2, true>",), P=33, c=17, layout=1),
    Case("linear3_rc1_bit8192_bytes", "shared", ("shared_linear3_kernel<17, 2, 1, false>",), P=32, c=17, layout=1,
         opts=(("kernel_flags", 8192),), bit=8192),
    # ---- packed 16-bit hit counters: every wave flushes at least twice, all hits on one key (worst case) -------------------
    *[Case(f"flush_wide3_c{c}_p{P}", "shared", (f"shared_wide3_kernel<{c}, 18, 2, {'true' if c == 17 else 'false'}>",), P=P, c=c,
           n=N_FLUSH, column="const", opts=_cap(), min_tiles=FLUSH_TILES) for c, P in ((9, 33), (9, 48), (9, 63), (17, 33), (17, 48), (17, 64))],
    Case("flush_wide3_c9_p48_alt", "shared", ("shared_wide3_kernel<9, 18, 2, false>",), P=48, n=N_FLUSH, column="alt", opts=_cap(),
         min_tiles=FLUSH_TILES),
    *[Case(f"flush_linear3_p{P}", "shared", ("shared_linear3_kernel<9, 2, 2, false>",), P=P, layout=1, n=N_FLUSH, column="const",
           opts=_cap(), min_tiles=FLUSH_TILES) for P in (33, 40)],
    Case("flush_wide2_p33_bit32768", "shared", ("shared_wide2_kernel<9, 18, 64, 2, false>",), P=33, n=N_FLUSH, column="const",
         opts=_cap(("kernel_flags", 32768)), min_tiles=FLUSH_TILES),
    # ---- the linear kernels' 8-bit byte counters (flushed every 31 steps), all hits ------------------------------------------
    Case("bytes_linear_p9", "shared", ("shared_linear_kernel<9, 2, 1>",), P=9, layout=1, n=N_BYTES, column="const", opts=_cap(),
         min_tiles=BYTE_STEPS),
    Case("bytes_linear_p16", "shared", ("shared_linear_kernel<9, 2, 1>",), P=16, layout=1, n=N_BYTES, column="const", opts=_cap(),
         min_tiles=BYTE_STEPS),
    Case("bytes_linear_p31", "shared", ("shared_linear_kernel<9, 2, 1>",), P=31, layout=1, n=N_BYTES, column="const", opts=_cap(),
         min_tiles=BYTE_STEPS),
    Case("bytes_linear2_p65", "shared", ("shared_linear2_kernel<9, 2>",), P=65, layout=1, n=N_BYTES, column="const", opts=_cap(),
         set_bits=0x20000, min_tiles=BYTE_STEPS),
    Case("bytes_linear2_p129", "shared", ("shared_linear2_kernel<9, 2>",), P=129, layout=1, n=N_BYTES, column="const", opts=_cap(),
         set_bits=0x20000, min_tiles=BYTE_STEPS),
    Case("bytes_linear_p16_c12", "shared", ("shared_linear_kernel<12, 2, 2>",), P=16, c=12, layout=1, n=N_BYTES, column="const",
         opts=_cap(), min_tiles=BYTE_STEPS),
    # ---- equality / range scans and their consumers --------------------------------------------------------------------------
    Case("scan_eq", "scan_eq", ("scan_burst_kernel<9, 0, 34, 128, 4>",)),
    Case("scan_eq_burst1", "scan_eq", ("scan_burst_kernel<9, 0, 34, 128, 1>",), opts=(("scan_burst", 1),)),
    Case("scan_eq_nt", "scan_eq", ("scan_burst_kernel<9, 0, 18, 128, 4>",), opts=(("scan_nt_stores", 1),)),
    Case("scan_eq_plain", "scan_eq", ("scan_burst_kernel<9, 0, 2, 128, 4>",), opts=(("scan_nt_stores", 0),)),
    Case("scan_eq_dma0", "scan_eq", ("scan_burst_kernel<9, 0, 0, 128, 4>",), opts=(("dma_aux", 0),)),
    Case("scan_eq_c21", "scan_eq", ("scan_burst_kernel<21, 0, 34, 64, 1>",), c=21),
    Case("scan_range_c7", "scan_range", ("scan_burst_kernel<7, 1, 34, 128, 1>",), c=7),
    Case("combine_masked", "combine", ("scan_burst_kernel<9, 1, 34, 128, 4>",)),
    Case("scan_in", "in", ("in_kernel<9, 34, 128>",), P=20),
    Case("scan_in_nt", "in", ("in_kernel<9, 18, 128>",), P=20, opts=(("scan_nt_stores", 1),)),
    Case("scan_in_plain", "in", ("in_kernel<9, 2, 128>",), P=20, opts=(("scan_nt_stores", 0),)),
    Case("scan2", "scan2", ("scan2_kernel<9, 34, 128>",)),
    Case("scan2_nt", "scan2", ("scan2_kernel<9, 18, 128>",), opts=(("scan_nt_stores", 1),)),
    Case("select2", "select", ("select2_kernel<9, 1, 128>",)),
    Case("select_single", "select", ("select_kernel<9, 1, 128>",), opts=(("select_kernel", 1),)),
    *[Case(f"select2_bit{b}", "select", ("select2_kernel<9, 1, 128>",), opts=(("kernel_flags", b),), bit=b) for b in SELECT_BITS],
    *[Case(f"select_single_bit{b}", "select", ("select_kernel<9, 1, 128>",), opts=(("kernel_flags", b), ("select_kernel", 1)), bit=b)
      for b in SELECT_BITS],
    Case("decompress", "decompress", ("decompress_kernel<9, 18>",)),
    Case("decompress_dma0", "decompress", ("decompress_kernel<9, 0>",), opts=(("dma_aux", 0),)),
    Case("decompress_dma2", "decompress", ("decompress_kernel<9, 2>",), opts=(("dma_aux", 2),)),
    Case("decompress_dma34", "decompress", ("decompress_kernel<9, 34>",), opts=(("dma_aux", 34),)),
    Case("generate_splitmix", "generate", ("pack_kernel<3>",)),
    Case("pack_u32", "pack_u32", ("pack_tiled_kernel<1, 5>",)),
    Case("bitmap_and", "bitmap_and", ("bitmap_kernel<0>",)),
    Case("bitmap_count", "bitmap_count", ("bitmap_kernel<4>", "sum_slots_kernel")),
    Case("rowids", "rowids", ("rowid_count_kernel", "rowid_scan_kernel", "rowid_write_kernel")),
    Case("gather", "gather", ("gather_kernel",)),
    Case("aggregate", "aggregate", ("aggregate_init_kernel", "aggregate_kernel<9, 128>")),
    Case("histogram", "histogram", ("histogram_kernel<9, 128>",)),
]


def family_of(label):
    """the family mi355_shared_scan_kernel / mi355_shared_where_kernel names for the kernel of a launch-record label"""
    name = base_name(label)
    if name in ("shared_lut_kernel", "shared_where_lut_kernel") and label.split(">")[0].split(",")[-1].strip() == "true":
        return name + "(multi-pass)"
    for stem in ("shared_wide", "shared_linear"):
        if name.startswith(stem):
            return stem + "_kernel"
    return name


def column(case, rng):
    """values (uint32) and, for shared / in, the key list"""
    n, c = case.n, case.c
    top = (1 << c) if c < 32 else (1 << 32)
    if case.column == "const":
        v = int(rng.integers(0, top))
        return np.full(n, v, dtype=np.uint32), [v] * case.P
    if case.column == "alt":
        a, b = (int(x) for x in rng.choice(min(top, 1 << 16), 2, replace=False))
        vals = np.where(np.arange(n) % 2 == 0, a, b).astype(np.uint32)
        return vals, [a if k % 2 == 0 else b for k in range(case.P)]
    P = max(case.P, 1)
    keys = rng.choice(top, P, replace=False) if 2 * P <= top <= (1 << 20) else rng.integers(0, top, P)
    keys = [int(k) for k in keys]
    vals = rng.integers(0, top, n, dtype=np.uint64)
    take = rng.random(n) < 0.7
    vals[take] = np.asarray(keys, dtype=np.uint64)[rng.integers(0, P, int(take.sum()))]
    return vals.astype(np.uint32), keys


def check_select(L, eng, packed, vals, n, c, op, a, capacity_kind, first_row=1000, check_ids=True, after=None):
    """mi355_scan_select_dev with >= 4 KiB of guard behind rowids and >= 7 words behind count_dev"""
    pred = {0: vals == a, 2: vals < a, 4: vals > a}[op]
    want = np.nonzero(pred)[0].astype(np.uint64) + first_row
    cap = {"lt": len(want) // 2, "eq": len(want), "gt": len(want) + 100}[capacity_kind]
    ids, cnt = Guarded(8 * cap, back=4096), Guarded(8, back=64, front=64)
    rc = L.mi355_scan_select_dev(eng._ctx, C.c_void_p(packed.data_ptr()), n, c, op, a, 0, 0, None, first_row, ids.ptr, cap, cnt.ptr)
    assert rc == 0, L.mi355_last_error()
    eng.synchronize()
    if after:
        after()
    got, count = ids.fetch().view(np.uint64), int(cnt.fetch().view(np.uint64)[0])
    if check_ids:
        assert count == len(want)
        k = min(cap, len(want))
        assert np.array_equal(got[:k], want[:k])
        assert (ids.t[ids.front + 8 * k: ids.front + 8 * cap].cpu().numpy() == SENTINEL).all(), "ids written beyond the count"


# ---- the shared predicate scans' case table (test_shared_where runs it, test_shared_where_cpu holds it against csrc/predicates/) ---

WHERE_LUT, WHERE_LUT_MULTI, WHERE_CHAIN, WHERE_SINGLE = ("shared_where_lut_kernel", "shared_where_lut_kernel(multi-pass)", "shared_where_chain_kernel",
                                                         "scan_burst_kernel")


def where_family(c, P):
    """the documented dispatch, written down independently of the launcher: P = 1 the single-
    predicate scan; c <= 16: tables while ceil(P/8) tables of max(2^c, 4) bytes (rounded up to 16) fit into 160 KiB beside
    four tiles of 64 x 64 values (whole KiB each), 4 KiB of hit counters and 512 bytes; the compare chain elsewhere"""
    if P == 1:
        return WHERE_SINGLE
    if c > 16:
        return WHERE_CHAIN
    if P <= 8:
        return WHERE_LUT
    tables = ((P + 7) // 8 * max(1 << c, 4) + 15) // 16 * 16
    tile = (64 * 64 * c // 8 + 1023) // 1024 * 1024
    return WHERE_LUT_MULTI if tables + 4 * tile + 4096 + 512 <= 160 * 1024 else WHERE_CHAIN


# the case table of test_shared_where.test_predicate_counts: (c, P, kernel family the call must launch)
WHERE_COUNT_WIDTHS = [5, 9, 12, 16, 17, 32]
WHERE_COUNT_PS = [1, 2, 3, 5, 8, 9, 16, 33, 64, 65, 257, 1024]
WHERE_COUNT_CASES = [(c, P, where_family(c, P)) for c in WHERE_COUNT_WIDTHS for P in WHERE_COUNT_PS]


# ---- the launchers' dry run (tests/cpp/launch_dry_run.cpp) ----------------------------------------------------------------------

SRC = os.path.join(ROOT, "tests", "cpp", "launch_dry_run.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "build", "launch_dry_run")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def group_objects():
    return sorted(glob.glob(os.path.join(CSRC, "build", "width_group_*.o")))


def build_binary():
    if len(group_objects()) != 8:
        from shared_simd_scan_amd import build

        build.build()
    objs = group_objects()
    assert len(objs) == 8, objs
    newest = max(os.path.getmtime(f) for f in [SRC, os.path.join(CSRC, "dispatch.hpp"), os.path.join(CSRC, "switches.hpp")] + objs)
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < newest:
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        obj = BIN + ".o"  # (compiled on its own: hipcc would read the group objects as HIP sources next to a .cpp)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", CSRC, "-c", SRC, "-o", obj], check=True)
        subprocess.run([HIPCC, "--offload-arch=gfx950", obj, *objs, "-o", BIN], check=True)
    return BIN


def dry_run(rows):
    """rows of (op, c, P, layout, hits, n, kernel_flags, shared_vpl, scan_nt_stores, max_blocks_per_cu, dma_aux, scan_burst, select_single)
    -> [(family index or -1, launch record text)]"""
    text = "".join(" ".join(str(int(v)) for v in row) + "\n" for row in rows)
    res = subprocess.run([build_binary()], input=text, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    out = [ln.split("\t", 1) for ln in res.stdout.splitlines()]
    assert len(out) == len(rows), (len(out), len(rows))
    return [(int(fam), rec) for fam, rec in out]
