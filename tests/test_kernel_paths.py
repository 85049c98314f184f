"""Every kernel path of the launcher, by name: CASES is the one list of (call, options) -> kernel (with its template
arguments) that the call must launch, as mi355_ctx_last_launch reports it.

CPU: every __global__ kernel of csrc/kernels/*.hpp and csrc/extras/*.hpp is the expected kernel of some case; the variant
axes the launcher picks between are covered; every kernel-side `flags &` test names a switch of csrc/switches.hpp whose
option value is in the matrix, the table maps option values as the shifts it replaced did, and every option bit of the matrix has a case.
GPU (-m gpu): each case runs, its launch record matches, and every output byte equals numpy, inside 0xEE guard bytes that
must stay untouched.  A shared scan also asks mi355_shared_scan_kernel under its options: the family named is the one launched.  A case with an option bit also runs without that bit: the record must change (the launcher really
took the other path) and the results must not.  The counter-flush cases run on a 4-wave grid (grid_cus = 1,
max_blocks_per_cu = 1) so that every wave walks more than 1100 tiles: the packed 16-bit hit counters flush at least twice.
"""
import ctypes as C
import glob
import os
import re
import zlib
from dataclasses import dataclass

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shared_simd_scan_amd", "csrc")

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

EXEMPT_KERNELS = {}  # kernel name -> reason; none today

# the variant axes the launcher picks between: (regex over a case's expected label, flags set, flags clear, what)
REQUIRED_VARIANTS = [
    (r"shared_wide3_kernel<\d+, \d+, 0, false>", 0, 0, "wide3 RC 0"),
    (r"shared_wide3_kernel<\d+, \d+, 1, false>", 0, 0, "wide3 RC 1"),
    (r"shared_wide3_kernel<\d+, \d+, 2, false>", 0, 0, "wide3 RC 2"),
    (r"shared_wide3_kernel<\d+, \d+, 0, true>", 0, 0, "wide3 RC 0 BIG"),
    (r"shared_wide3_kernel<\d+, \d+, 1, true>", 0, 0, "wide3 RC 1 BIG"),
    (r"shared_wide3_kernel<\d+, \d+, 2, true>", 0, 0, "wide3 RC 2 BIG"),
    (r"shared_wide3_kernel<\d+, 2, .*>", 0, 0, "wide3 plain stores"),
    (r"shared_wide3_kernel<\d+, 18, .*>", 0, 0, "wide3 nt stores"),
    (r"shared_wide2_kernel<\d+, \d+, 64, 0, .*>", 0, 0, "wide2 RC 0"),
    (r"shared_wide2_kernel<\d+, \d+, 64, 1, .*>", 0, 0, "wide2 RC 1"),
    (r"shared_wide2_kernel<\d+, \d+, 64, 2, .*>", 0, 0, "wide2 RC 2"),
    (r"shared_wide2_kernel<\d+, \d+, 64, 0, true>", 0, 0, "wide2 BIG"),
    (r"shared_wide2_kernel<\d+, 2, .*>", 0, 0, "wide2 plain stores"),
    (r"shared_wide2_kernel<\d+, 18, .*>", 0, 0, "wide2 nt stores"),
    (r"shared_wide_kernel<\d+, 2, 64, 0>", 0, 0, "wide per-predicate plain"),
    (r"shared_wide_kernel<\d+, 18, 64, 0>", 0, 0, "wide per-predicate nt"),
    (r"shared_wide_kernel<\d+, 2, 64, 1>", 0, 0, "wide linear"),
    (r"shared_linear_kernel<\d+, 2, 1>", 0x100000, 0, "linear with the aligned image"),
    (r"shared_linear_kernel<\d+, 2, 1>", 0, 0x100000, "linear without the aligned image"),
    (r"shared_linear_kernel<\d+, 2, 2>", 0, 0, "linear, two rows per piece"),
    (r"shared_linear2_kernel<\d+, 2>", 0x20000, 0, "linear2, short table attached"),
    (r"shared_linear2_kernel<\d+, 2>", 0, 0x20000, "linear2, short table detached"),
    (r"shared_linear3_kernel<\d+, 2, 0, .*>", 0, 0, "linear3 RC 0"),
    (r"shared_linear3_kernel<\d+, 2, 1, .*>", 0, 0, "linear3 RC 1"),
    (r"shared_linear3_kernel<\d+, 2, 2, .*>", 0, 0, "linear3 RC 2"),
    (r"shared_linear3_kernel<\d+, 2, \d, true>", 0, 0, "linear3 BIG"),
    (r"shared_lut_kernel<\d+, 34, \d+, 0, false>", 0, 0, "lut per-predicate write-through"),
    (r"shared_lut_kernel<\d+, 18, \d+, 0, false>", 0, 0, "lut per-predicate nt"),
    (r"shared_lut_kernel<\d+, 2, \d+, 0, false>", 0, 0, "lut per-predicate plain"),
    (r"shared_lut_kernel<\d+, 34, \d+, 1, false>", 0, 0, "lut linear write-through"),
    (r"shared_lut_kernel<\d+, 18, \d+, 1, false>", 0, 0, "lut linear nt"),
    (r"shared_lut_kernel<\d+, 2, \d+, 1, false>", 0, 0, "lut linear plain"),
    (r"shared_lut_kernel<\d+, \d+, 128, 0, false>", 0, 0, "lut 128 values per lane"),
    (r"shared_lut_kernel<\d+, \d+, 64, 0, false>", 0, 0, "lut 64 values per lane"),
    (r"shared_lut_kernel<\d+, 2, 64, 1, true>", 0, 0, "lut multi-pass"),
    (r"shared_pair_kernel<\d+, 34, .*>", 0, 0, "pair write-through"),
    (r"shared_pair_kernel<\d+, 18, .*>", 0, 0, "pair nt"),
    (r"scan_burst_kernel<\d+, 0, 0, .*>", 0, 0, "scan default loads"),
    (r"scan_burst_kernel<\d+, 0, 2, .*>", 0, 0, "scan plain stores"),
    (r"scan_burst_kernel<\d+, 0, 18, .*>", 0, 0, "scan nt stores"),
    (r"scan_burst_kernel<\d+, 0, 34, .*>", 0, 0, "scan write-through stores"),
    (r"scan_burst_kernel<\d+, \d, \d+, \d+, 4>", 0, 0, "scan store bursts of 4 tiles"),
    (r"scan_burst_kernel<9, \d, \d+, \d+, 1>", 0, 0, "scan one tile per burst (option)"),
    (r"in_kernel<\d+, 34, .*>", 0, 0, "in write-through"),
    (r"in_kernel<\d+, 18, .*>", 0, 0, "in nt"),
    (r"in_kernel<\d+, 2, .*>", 0, 0, "in plain"),
    (r"scan2_kernel<\d+, 34, .*>", 0, 0, "scan2 write-through"),
    (r"scan2_kernel<\d+, 18, .*>", 0, 0, "scan2 nt"),
    (r"decompress_kernel<\d+, 0>", 0, 0, "decompress dma_aux 0"),
    (r"decompress_kernel<\d+, 2>", 0, 0, "decompress dma_aux 2"),
    (r"decompress_kernel<\d+, 18>", 0, 0, "decompress dma_aux 18"),
    (r"decompress_kernel<\d+, 34>", 0, 0, "decompress dma_aux 34"),
    (r"select_kernel<.*>", 0, 0, "selection, single-role kernel"),
    (r"select2_kernel<.*>", 0, 0, "selection, decoder / expander kernel"),
]


def case_by_id(cid):
    return next(c for c in CASES if c.id == cid)


def base_name(label):
    return label.split("<", 1)[0]


def family_of(label):
    """the family mi355_shared_scan_kernel / mi355_shared_where_kernel names for the kernel of a launch-record label"""
    name = base_name(label)
    if name in ("shared_lut_kernel", "shared_where_lut_kernel") and label.split(">")[0].split(",")[-1].strip() == "true":
        return name + "(multi-pass)"
    for stem in ("shared_wide", "shared_linear"):
        if name.startswith(stem):
            return stem + "_kernel"
    return name


# ------------------------------------------------------------------------------------------------------------------------
# CPU: the table covers every kernel, every variant axis and every option bit
# ------------------------------------------------------------------------------------------------------------------------

def kernel_sources():
    return sorted(glob.glob(os.path.join(CSRC, "kernels", "*.hpp")) + glob.glob(os.path.join(CSRC, "extras", "*.hpp")))


def global_kernels():
    names = set()
    for f in kernel_sources():
        text = open(f).read()
        names |= set(re.findall(r"__global__[^;{}]*?\bvoid\s+(\w+)\s*\(", text))
    return names


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def strip_debug_blocks(text):
    # the selection's look-back diagnostics exist only in -DMI355_SELECT_DEBUG builds: not a switch of the library
    return re.sub(r"#ifdef MI355_SELECT_DEBUG.*?#endif", "", text, flags=re.S)


def test_case_ids_unique():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))


def test_every_kernel_has_a_case():
    kernels = global_kernels()
    assert len(kernels) >= 20, kernels  # the parse found the kernels
    covered = {base_name(p) for c in CASES for p in c.expect}
    missing = sorted(kernels - covered - set(EXEMPT_KERNELS))
    assert not missing, f"__global__ kernels no case of CASES expects: {missing}"
    stale = sorted((covered | set(EXEMPT_KERNELS)) - kernels)
    assert not stale, f"CASES / EXEMPT_KERNELS name kernels that do not exist: {stale}"


@pytest.mark.parametrize("pattern,set_bits,clear_bits,what", REQUIRED_VARIANTS, ids=[v[3] for v in REQUIRED_VARIANTS])
def test_every_variant_has_a_case(pattern, set_bits, clear_bits, what):
    hits = [c.id for c in CASES for p in c.expect if re.fullmatch(pattern, p)
            and (c.set_bits & set_bits) == set_bits and (c.clear_bits & clear_bits) == clear_bits]
    assert hits, f"no case covers {what} ({pattern})"


def switch_table():
    """csrc/switches.hpp as tests/cpp/launch_dry_run --switches prints it: [(name, option value, kernel-side bit, receiver)]"""
    import subprocess

    from test_launch_plan import build_binary

    out = subprocess.run([build_binary(), "--switches"], capture_output=True, text=True, timeout=60, check=True).stdout
    return [(name, int(opt), int(kbit, 16), recv) for name, opt, kbit, recv in (ln.split("\t") for ln in out.splitlines())]


def switch_words(options):
    """[(shared scans' word, selection's word)] of kernel_switch_word() per option value, read from the flags=0x... of the launch
    record of an equality scan (every launch but the selection's carries the shared scans' word) and of a selection"""
    from test_launch_plan import dry_run

    recs = dry_run([(op, 9, 1, 0, 1, N_SMALL, v, 0, -1, 0, 18, 0, 0) for v in options for op in (0, 5)])
    words = [parse_record(text)[0][3] for _, text in recs]
    return list(zip(words[0::2], words[1::2]))


def test_flag_shifts_keep_the_selection_apart():
    rows = switch_table()
    assert len({r[0] for r in rows}) == len(rows) and {r[3] for r in rows} == {"shared", "select", "launcher-set", "reserved"}, rows
    options = {recv: {r[1] for r in rows if r[3] == recv} for recv in ("shared", "select", "launcher-set", "reserved")}
    kbits = {recv: {r[2] for r in rows if r[3] == recv} for recv in options}
    assert not options["select"] & options["shared"], "an option bit reaches both the shared scans and the selection"
    assert options["select"] == set(SELECT_BITS[:2]) | set(TIMING_ABLATIONS) == {512, 1024, 2048, 4096}, sorted(options["select"])
    assert options["shared"] == set(SHARED_BITS), sorted(options["shared"])
    assert options["launcher-set"] == {0}, "a launcher-set switch has an option value"
    assert kbits["launcher-set"] == set(LAUNCHER_SET), kbits["launcher-set"]
    assert options["reserved"] == set(UNUSED_BITS), options["reserved"]
    # neither the launcher's own rows (no option value) nor the reserved one give a receiver anything, and no option bit at all
    # brings about a launcher-set or reserved kernel bit, or one of the other receiver
    for v, (shared, select) in zip([0] + sorted(UNUSED_BITS), switch_words([0] + sorted(UNUSED_BITS))):
        assert shared == 0 and select == 0, f"option value {v} reaches the kernels: {shared:#x} / {select:#x}"
    singles = [1 << b for b in range(32)]
    for v, (shared, select) in zip(singles, switch_words(singles)):
        assert not shared & ~sum(kbits["shared"]) and not select & ~sum(kbits["select"]), f"option bit {v}: {shared:#x} / {select:#x}"
        assert not (shared and select), f"option bit {v} reaches both the shared scans and the selection"


# what capi.hip's launch() computed before csrc/switches.hpp held the table (recorded old behaviour): select, everything else
OLD_SWITCH_WORD = (lambda v: (v >> 8) & 0x1e, lambda v: (v & 0x1ff) | ((v >> 4) & 0xdee00))


def test_switch_word_is_what_the_shifts_gave():
    """the mapping is bitwise, so the 32 single-bit option values cover it"""
    singles = [1 << b for b in range(32)]
    for v, (shared, select) in zip(singles, switch_words(singles)):
        assert select == OLD_SWITCH_WORD[0](v), f"option bit {v}, selection: {select:#x}"
        assert shared == OLD_SWITCH_WORD[1](v), f"option bit {v}, shared scans: {shared:#x}"


FLAGS_AND = r"\bflags\s*&(?!&)"


def kernel_flag_tests():
    """(file, switch name) for every `flags & <name>` / `flags & (<name> | <name>)` of width_group.hip, shared_plan.hpp and
    kernels/*.hpp; whatever else follows a `flags &` fails here"""
    out = []
    for f in [os.path.join(CSRC, "width_group.hip"), os.path.join(CSRC, "shared_plan.hpp")] + sorted(glob.glob(os.path.join(CSRC, "kernels", "*.hpp"))):
        text = strip_comments(strip_debug_blocks(open(f).read()))
        assert not re.search(FLAGS_AND + r"[\s(]*(0x[0-9a-fA-F]+|\d)", text), f"{os.path.basename(f)}: a numeric literal next to `flags &`"
        found = re.findall(FLAGS_AND + r"\s*(?:\(([^()]*)\)|([A-Za-z_]\w*))", text)
        assert len(found) == len(re.findall(FLAGS_AND, text)), f"{os.path.basename(f)}: a `flags &` without a switch name behind it"
        for group, one in found:
            out += [(os.path.basename(f), name.strip()) for name in (group.split("|") if group else [one])]
    return out


def test_kernel_flag_tests_are_in_the_matrix():
    tests = kernel_flag_tests()
    assert len(tests) >= 20, tests  # the parse found the launcher's switches
    table = {name: (opt, kbit, recv) for name, opt, kbit, recv in switch_table()}
    documented = set(SHARED_BITS) | set(SELECT_BITS) | set(TIMING_ABLATIONS)
    for fname, name in tests:
        assert name in table, f"{fname}: `flags & {name}`: not a switch of csrc/switches.hpp"
        opt, kbit, recv = table[name]
        if fname in ("select.hpp", "select2.hpp"):
            assert recv == "select", f"{fname}: {name} is a switch of receiver {recv}"
        else:
            assert recv in ("shared", "launcher-set"), f"{fname}: {name} is a switch of receiver {recv}"
            if recv == "launcher-set":
                assert kbit in LAUNCHER_SET, f"{fname}: {name} = {kbit:#x}"
                continue
        assert opt in documented, f"{fname}: {name} = option bit {opt}: not in the option-bit matrix"


def test_design_lists_every_switch():
    """DESIGN.md's "A/B switches" section has every row of the table, name and option value on one line"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    start = text.index("**A/B switches.**")
    section = text[start:text.index("\n## 9.", start)].splitlines()
    for name, opt, kbit, recv in switch_table():
        cell = str(opt) if opt else "—"
        assert any(re.search(rf"\|\s*`{name}`\s*\|\s*{cell}\s*\|\s*{recv}\s*\|", ln) for ln in section), f"DESIGN.md section 8: no row for {name} ({cell}, {recv})"


def test_every_option_bit_has_a_case():
    for b in SHARED_BITS + list(UNUSED_BITS):
        got = [c.id for c in CASES if c.bit == b and c.opt("kernel_flags") & b and c.op == "shared"]
        assert got, f"option bit {b}: no shared-scan case"
    for b in SELECT_BITS:
        for single in (0, 1):
            got = [c.id for c in CASES if c.op == "select" and c.bit == b and c.opt("kernel_flags") == b and c.opt("select_kernel") == single]
            assert got, f"option bit {b}: no case on {'select_kernel' if single else 'select2_kernel'}"
    for c in CASES:
        if c.bit:
            assert c.opt("kernel_flags") & c.bit, c.id
            assert c.bit in SHARED_BITS + SELECT_BITS or c.bit in UNUSED_BITS, c.id


def test_flush_cases_walk_enough_tiles():
    flush = [c for c in CASES if c.min_tiles == FLUSH_TILES]
    assert {(c.c, c.P, c.layout) for c in flush} >= {(9, 33, 0), (9, 48, 0), (9, 63, 0), (17, 33, 0), (17, 48, 0), (17, 64, 0),
                                                      (9, 33, 1), (9, 40, 1)}
    for c in flush + [c for c in CASES if c.min_tiles]:
        ntiles = (c.n + SHARED_TILE_ROWS - 1) // SHARED_TILE_ROWS
        assert ntiles // WAVES_PER_BLOCK > c.min_tiles, c.id
        assert c.n % SHARED_TILE_ROWS != 0, c.id  # ragged tail
        assert c.opt("grid_cus") == 1 and c.opt("max_blocks_per_cu") == 1, c.id


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------

SENTINEL = 0xEE
RECORD_LINE = re.compile(r"(?P<label>\S.*?) grid=(?P<grid>\d+) lds=(?P<lds>\d+) flags=0x(?P<flags>[0-9a-f]+)")


def parse_record(text):
    lines = [ln for ln in text.split("\n") if ln]
    out = []
    for ln in lines:
        m = RECORD_LINE.fullmatch(ln)
        assert m, f"malformed launch record line {ln!r}"
        out.append((m["label"], int(m["grid"]), int(m["lds"]), int(m["flags"], 16)))
    return out


def label_matches(pattern, label):
    rx = re.escape(pattern).replace(r"\*", r"[^,<>]+")
    return re.fullmatch(rx, label) is not None


class Guarded:
    """a device buffer of `nbytes` inside 0xEE guard regions (`front` / `back` bytes, front a multiple of 16)"""

    def __init__(self, nbytes, back=4096, front=4096):
        import torch

        self.nbytes, self.front, self.back = int(nbytes), front, back
        self.t = torch.full((front + self.nbytes + back,), SENTINEL, dtype=torch.uint8, device="cuda")

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + self.front)

    def fetch(self):
        h = self.t.cpu().numpy()
        assert (h[: self.front] == SENTINEL).all(), "guard in front of the buffer overwritten"
        tail = h[self.front + self.nbytes:]
        assert (tail == SENTINEL).all(), f"guard behind the buffer overwritten at +{int(np.argmax(tail != SENTINEL))}"
        return h[self.front: self.front + self.nbytes]


def packbits(mask):
    return np.packbits(mask.astype(bool), bitorder="little")


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


class Runner:
    def __init__(self, L, O):
        self.L, self.O = L, O

    def ok(self, rc):
        assert rc == 0, self.L.mi355_last_error()

    def run(self, case, opts):
        """run the case with these options; check every output byte; -> the launch record"""
        import torch

        from shared_simd_scan_amd import ScanEngine

        eng = ScanEngine()
        self.last_record = ""
        try:
            for name, value in opts:
                eng.set_option(name, value)
            rng = np.random.default_rng(zlib.crc32(case.id.encode()))
            getattr(self, "op_" + case.op)(eng, case, rng, torch)  # reads the record before it checks the outputs
            return self.last_record
        finally:
            eng.close()

    def record(self, eng):
        eng.synchronize()
        self.last_record = (self.L.mi355_ctx_last_launch(eng._ctx) or b"").decode()

    def upload(self, torch, vals, c):
        return torch.from_numpy(self.O.pack(vals, c)).cuda()

    # ---- shared scans ----
    def op_shared(self, eng, case, rng, torch):
        n, c, P = case.n, case.c, case.P
        vals, keys = column(case, rng)
        packed = self.upload(torch, vals, c)
        nb = (n + 7) // 8
        stride = (nb + 15) // 16 * 16 + 16  # a guard gap behind every bitmap of the per-predicate layout
        out = Guarded(P * stride if case.layout == 0 else P * nb)
        hits = Guarded(8 * P) if case.hits else None
        k = np.ascontiguousarray(np.asarray(keys, dtype=np.uint32).view(np.int32))
        named = self.L.mi355_shared_scan_kernel(eng._ctx, c, P, case.layout, int(case.hits))  # under the case's options
        self.ok(self.L.mi355_shared_scan_eq_dev(eng._ctx, C.c_void_p(packed.data_ptr()), n, c, k.ctypes.data_as(C.c_void_p), P,
                                                case.layout, out.ptr, stride, hits.ptr if hits else None))
        self.record(eng)
        launched = parse_record(self.last_record)
        assert len(launched) == 1 and named is not None and named.decode() == family_of(launched[0][0]), \
            f"the library names {named}, launched:\n{self.last_record}"
        body = out.fetch()
        uniq = {}
        for key in keys:
            if key not in uniq:
                uniq[key] = (packbits(vals == key), int((vals == key).sum()))
        if case.layout == 0:
            seg = body.reshape(P, stride)
            for j, key in enumerate(keys):
                assert np.array_equal(seg[j, :nb], uniq[key][0]), f"bitmap of key {j} differs"
            assert (seg[:, nb:] == SENTINEL).all(), "bytes between the per-predicate bitmaps overwritten"
        else:
            lin = body.reshape(nb, P)
            for j, key in enumerate(keys):
                assert np.array_equal(lin[:, j], uniq[key][0]), f"linear column of key {j} differs"
        if hits:
            got = hits.fetch().view(np.uint64)
            assert got.tolist() == [uniq[key][1] for key in keys]

    # ---- scans ----
    def _scan(self, eng, case, rng, torch, call):
        vals, keys = column(case, rng)
        packed = self.upload(torch, vals, case.c)
        bm, hits = Guarded((case.n + 7) // 8), Guarded(8, back=64, front=64)
        expect = call(C.c_void_p(packed.data_ptr()), vals, keys, bm, hits)
        self.record(eng)
        assert np.array_equal(bm.fetch(), packbits(expect))
        assert int(hits.fetch().view(np.uint64)[0]) == int(expect.sum())

    def op_scan_eq(self, eng, case, rng, torch):
        def call(p, vals, keys, bm, hits):
            self.ok(self.L.mi355_scan_eq_dev(eng._ctx, p, case.n, case.c, keys[0], bm.ptr, hits.ptr))
            return vals == keys[0]
        self._scan(eng, case, rng, torch, call)

    def op_scan_range(self, eng, case, rng, torch):
        def call(p, vals, keys, bm, hits):
            lo, hi = sorted((keys[0], (keys[0] * 7 + 5) % (1 << case.c)))
            self.ok(self.L.mi355_scan_range_dev(eng._ctx, p, case.n, case.c, lo, hi, bm.ptr, hits.ptr))
            return (vals >= lo) & (vals <= hi)
        self._scan(eng, case, rng, torch, call)

    def op_combine(self, eng, case, rng, torch):
        mask_bits = rng.random(case.n) < 0.5
        mask = torch.from_numpy(packbits(mask_bits)).cuda()

        def call(p, vals, keys, bm, hits):
            lo, hi = 100, 300
            self.ok(self.L.mi355_scan_combine_dev(eng._ctx, p, case.n, case.c, 6, lo, hi, 0, C.c_void_p(mask.data_ptr()), bm.ptr, hits.ptr))
            return (vals >= lo) & (vals <= hi) & mask_bits
        self._scan(eng, case, rng, torch, call)

    def op_in(self, eng, case, rng, torch):
        def call(p, vals, keys, bm, hits):
            k = np.ascontiguousarray(np.asarray(keys, dtype=np.int32))
            self.ok(self.L.mi355_scan_in_dev(eng._ctx, p, case.n, case.c, k.ctypes.data_as(C.c_void_p), len(keys), 0, None, bm.ptr, hits.ptr))
            return np.isin(vals, np.asarray(keys, dtype=np.uint32))
        self._scan(eng, case, rng, torch, call)

    def op_scan2(self, eng, case, rng, torch):
        vals2 = rng.integers(0, 1 << case.c, case.n).astype(np.uint32)
        packed2 = self.upload(torch, vals2, case.c)

        def call(p, vals, keys, bm, hits):
            self.ok(self.L.mi355_scan2_dev(eng._ctx, p, case.c, 0, keys[0], 0, C.c_void_p(packed2.data_ptr()), case.c, 2, 256, 0, case.n,
                                           0, bm.ptr, hits.ptr))
            return (vals == keys[0]) & (vals2 < 256)
        self._scan(eng, case, rng, torch, call)

    # ---- selection ----
    def op_select(self, eng, case, rng, torch):
        vals, keys = column(case, rng)
        packed = self.upload(torch, vals, case.c)
        check_select(self.L, eng, packed, vals, case.n, case.c, 2, 1 << (case.c - 2), "gt", after=lambda: self.record(eng))

    # ---- decompress / pack ----
    def op_decompress(self, eng, case, rng, torch):
        vals, _ = column(case, rng)
        packed = self.upload(torch, vals, case.c)
        out = Guarded(4 * case.n)
        self.ok(self.L.mi355_decompress_dev(eng._ctx, C.c_void_p(packed.data_ptr()), case.n, case.c, out.ptr))
        self.record(eng)
        assert np.array_equal(out.fetch().view(np.int32), vals.astype(np.int32))

    def op_generate(self, eng, case, rng, torch):
        size = self.L.mi355_compressed_buffer_size(case.c, case.n)
        out = Guarded(size)
        self.ok(self.L.mi355_generate_dev(eng._ctx, 1, 0, case.n, case.c, 42, out.ptr))
        self.record(eng)
        assert np.array_equal(out.fetch(), self.O.pack(self.O.gen_values("splitmix", case.n, case.c, 42), case.c))

    def op_pack_u32(self, eng, case, rng, torch):
        vals, _ = column(case, rng)
        dv = torch.from_numpy(vals.view(np.int32)).cuda()
        out = Guarded(self.L.mi355_compressed_buffer_size(case.c, case.n))
        self.ok(self.L.mi355_pack_u32_dev(eng._ctx, C.c_void_p(dv.data_ptr()), case.n, case.c, out.ptr))
        self.record(eng)
        assert np.array_equal(out.fetch(), self.O.pack(vals, case.c))

    # ---- bitmap consumers ----
    def _bitmaps(self, case, rng, torch):
        a, b = rng.random(case.n) < 0.4, rng.random(case.n) < 0.6
        return a, b, torch.from_numpy(packbits(a)).cuda(), torch.from_numpy(packbits(b)).cuda()

    def op_bitmap_and(self, eng, case, rng, torch):
        a, b, da, db = self._bitmaps(case, rng, torch)
        out = Guarded((case.n + 7) // 8)
        self.ok(self.L.mi355_bitmap_combine_dev(eng._ctx, 0, C.c_void_p(da.data_ptr()), C.c_void_p(db.data_ptr()), out.ptr, case.n, None))
        self.record(eng)
        assert np.array_equal(out.fetch(), packbits(a & b))

    def op_bitmap_count(self, eng, case, rng, torch):
        a, _, da, _ = self._bitmaps(case, rng, torch)
        cnt = Guarded(8, back=64, front=64)
        self.ok(self.L.mi355_bitmap_count_dev(eng._ctx, C.c_void_p(da.data_ptr()), case.n, cnt.ptr))
        self.record(eng)
        assert int(cnt.fetch().view(np.uint64)[0]) == int(a.sum())

    def op_rowids(self, eng, case, rng, torch):
        a, _, da, _ = self._bitmaps(case, rng, torch)
        want = np.nonzero(a)[0].astype(np.uint64) + 5
        ids, cnt = Guarded(8 * len(want)), Guarded(8, back=64, front=64)
        self.ok(self.L.mi355_bitmap_to_rowids_dev(eng._ctx, C.c_void_p(da.data_ptr()), case.n, 5, ids.ptr, len(want), cnt.ptr))
        self.record(eng)
        assert np.array_equal(ids.fetch().view(np.uint64), want)
        assert int(cnt.fetch().view(np.uint64)[0]) == len(want)

    def op_gather(self, eng, case, rng, torch):
        vals, _ = column(case, rng)
        packed = self.upload(torch, vals, case.c)
        rows = rng.integers(0, case.n, 3000).astype(np.uint64)
        drows = torch.from_numpy(rows.view(np.int64)).cuda()
        dcnt = torch.tensor([len(rows)], dtype=torch.int64, device="cuda")
        out = Guarded(4 * len(rows))
        self.ok(self.L.mi355_gather_dev(eng._ctx, C.c_void_p(packed.data_ptr()), case.n, case.c, 0, C.c_void_p(drows.data_ptr()),
                                        C.c_void_p(dcnt.data_ptr()), len(rows), out.ptr))
        self.record(eng)
        assert np.array_equal(out.fetch().view(np.int32), vals[rows.astype(np.int64)].astype(np.int32))

    def op_aggregate(self, eng, case, rng, torch):
        vals, _ = column(case, rng)
        packed = self.upload(torch, vals, case.c)
        out = Guarded(32, back=64, front=64)
        self.ok(self.L.mi355_aggregate_dev(eng._ctx, C.c_void_p(packed.data_ptr()), case.n, case.c, None, out.ptr))
        self.record(eng)
        v = vals.astype(np.uint64)
        assert out.fetch().view(np.uint64).tolist() == [int(v.sum()), case.n, int(v.min()), int(v.max())]

    def op_histogram(self, eng, case, rng, torch):
        vals, _ = column(case, rng)
        packed = self.upload(torch, vals, case.c)
        out = Guarded(8 << case.c)
        self.ok(self.L.mi355_histogram_dev(eng._ctx, C.c_void_p(packed.data_ptr()), case.n, case.c, None, out.ptr))
        self.record(eng)
        assert np.array_equal(out.fetch().view(np.uint64), np.bincount(vals, minlength=1 << case.c).astype(np.uint64))


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


# differs from support.L: a missing library is an error here, it is not built
@pytest.fixture(scope="module")
def L():
    from shared_simd_scan_amd import lib

    return lib()


@pytest.fixture(scope="module")
def runner(L, O):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return Runner(L, O)


def expected_tiles_per_wave(case, launch):
    _, grid, _, _ = launch
    ntiles = (case.n + SHARED_TILE_ROWS - 1) // SHARED_TILE_ROWS
    return ntiles // (grid * WAVES_PER_BLOCK)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_kernel_path(runner, cid):
    case = case_by_id(cid)
    text = runner.run(case, case.opts)
    rec = parse_record(text)
    assert len(rec) == len(case.expect) and all(label_matches(p, r[0]) for p, r in zip(case.expect, rec)), \
        f"{cid}: expected {list(case.expect)}, launched:\n{text}"
    flags = rec[-1][3]
    assert flags & case.set_bits == case.set_bits and not flags & case.clear_bits, f"{cid}: flags {flags:#x}\n{text}"
    if case.min_tiles:
        assert rec[-1][1] == 1, f"{cid}: grid_cus = 1, max_blocks_per_cu = 1 should give one block:\n{text}"
        assert expected_tiles_per_wave(case, rec[-1]) > case.min_tiles
    if case.bit:
        opts = tuple((k, v & ~case.bit) if k == "kernel_flags" else (k, v) for k, v in case.opts)
        base = runner.run(case, opts)
        if case.bit in UNUSED_BITS:
            assert base == text, f"unused option bit {case.bit} changed the launch:\n{base}\n->\n{text}"
        else:
            assert base != text, f"option bit {case.bit} did not change the launch:\n{text}"


SELECT_GUARD_BITS = [0] + SHARED_BITS + SELECT_BITS + list(UNUSED_BITS) + list(TIMING_ABLATIONS)


@pytest.mark.gpu
@pytest.mark.parametrize("capacity", ["lt", "eq", "gt"])
@pytest.mark.parametrize("bit", SELECT_GUARD_BITS)
@pytest.mark.parametrize("single", [0, 1], ids=["select2", "select_single"])
def test_select_stays_inside_its_buffers(runner, O, single, bit, capacity):
    """every option bit, both kernels: nothing is written past rowids[capacity] or count_dev[0] (the timing ablations give
    wrong ids by construction: only the guards are checked under them)"""
    import torch

    from shared_simd_scan_amd import ScanEngine

    n, c = N_SMALL, 9
    vals = np.random.default_rng(bit + 7 * single).integers(0, 1 << c, n).astype(np.uint32)
    packed = torch.from_numpy(O.pack(vals, c)).cuda()
    eng = ScanEngine()
    try:
        eng.set_option("select_kernel", single)
        eng.set_option("kernel_flags", bit)
        check_select(runner.L, eng, packed, vals, n, c, 2, 200, capacity, check_ids=bit not in TIMING_ABLATIONS)
        rec = parse_record(runner.L.mi355_ctx_last_launch(eng._ctx).decode())
        assert len(rec) == 1 and base_name(rec[0][0]) == ("select_kernel" if single else "select2_kernel")
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("density", ["dense", "sparse"])
@pytest.mark.parametrize("grid_cus", [1, 2, 3])
@pytest.mark.parametrize("single", [0, 1], ids=["select2", "select_single"])
@pytest.mark.parametrize("chunks", [8, 24])
def test_select_lookback_small_grid(runner, O, chunks, single, grid_cus, density):
    """a grid of one to three blocks: every block walks several chunks (65536 rows at c = 9), the look-back crosses its own
    earlier chunks"""
    import torch

    from shared_simd_scan_amd import ScanEngine

    n, c = 65536 * (chunks - 1) + 77, 9
    vals = np.random.default_rng(grid_cus).integers(0, 1 << c, n).astype(np.uint32)
    packed = torch.from_numpy(O.pack(vals, c)).cuda()
    eng = ScanEngine()
    try:
        eng.set_option("select_kernel", single)
        eng.set_option("grid_cus", grid_cus)
        eng.set_option("max_blocks_per_cu", 1)
        op, a = (2, 300) if density == "dense" else (0, 77)
        check_select(runner.L, eng, packed, vals, n, c, op, a, "gt")
        rec = parse_record(runner.L.mi355_ctx_last_launch(eng._ctx).decode())
        assert len(rec) == 1 and rec[0][1] == min(grid_cus, (chunks + WAVES_PER_BLOCK - 1) // WAVES_PER_BLOCK), rec  # grid_for()
    finally:
        eng.close()


@pytest.mark.gpu
def test_grid_cus_option_range(runner):
    import torch

    from shared_simd_scan_amd import Mi355Error, ScanEngine

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    eng = ScanEngine()
    try:
        for bad in (-1, cus + 1):
            with pytest.raises(Mi355Error):
                eng.set_option("grid_cus", bad)
        for good in (1, cus, 0):
            eng.set_option("grid_cus", good)
    finally:
        eng.close()


@pytest.mark.gpu
def test_launch_record_scope(runner, O):
    """a call starts a new record; a compound call records all of its launches; a call that launches nothing leaves it empty"""
    import torch

    from shared_simd_scan_amd import ScanEngine

    L = runner.L
    n = N_SMALL
    rng = np.random.default_rng(5)
    v9, v12 = rng.integers(0, 512, n).astype(np.uint32), rng.integers(0, 4096, n).astype(np.uint32)
    p9, p12 = torch.from_numpy(O.pack(v9, 9)).cuda(), torch.from_numpy(O.pack(v12, 12)).cuda()
    bm, hits = Guarded((n + 7) // 8), Guarded(8, back=64, front=64)
    eng = ScanEngine()
    try:
        assert L.mi355_ctx_last_launch(eng._ctx) == b""
        runner.ok(L.mi355_scan2_dev(eng._ctx, C.c_void_p(p9.data_ptr()), 9, 0, 5, 0, C.c_void_p(p12.data_ptr()), 12, 2, 99, 0, n, 0,
                                    bm.ptr, hits.ptr))
        rec = parse_record(L.mi355_ctx_last_launch(eng._ctx).decode())
        assert [r[0] for r in rec] == ["scan_burst_kernel<9, 1, 34, 128, 4>", "scan_burst_kernel<12, 1, 34, 128, 4>"], rec
        eng.synchronize()
        assert np.array_equal(bm.fetch(), packbits((v9 == 5) & (v12 < 99)))
        eng.set_option("kernel_flags", 0)  # options leave the record alone
        assert len(parse_record(L.mi355_ctx_last_launch(eng._ctx).decode())) == 2
        runner.ok(L.mi355_scan_eq_dev(eng._ctx, C.c_void_p(p9.data_ptr()), 0, 9, 5, bm.ptr, hits.ptr))  # n = 0: nothing launched
        assert L.mi355_ctx_last_launch(eng._ctx) == b""
    finally:
        eng.close()
