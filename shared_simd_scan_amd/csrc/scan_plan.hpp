// scan_plan.hpp -- what the launches of the three group units (width_group.hip, predicates/where_group.hip, predicates/columns_group.hip)
// run with, decided ONCE and purely: the kernel's AUX word (cache policy of its loads and stores), the tiles per store burst, the blocks
// per CU, the grid and the Infinity Cache divisor are functions of the request's fields, the tile geometry (as numbers) and the
// occupancy query's answer.  Plain C++: no HIP, no project header, no static, so every rule runs on a CPU
// (tests/cpp/scan_plan_check.cpp).  launch_util.hpp and dispatch.hpp include it; the group units launch what the plans say.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace mi355 {

constexpr int kPlanWavesPerBlock = 4; // kWavesPerBlock (kernels/tile.hpp; dispatch.hpp asserts that the two agree)

// ---- grids and blocks per CU -----------------------------------------------------------------------------------------------

// Persistent grid: at most (resident blocks per CU) x (CUs) blocks of 4 waves; each wave strides
// over the wave tiles.  Small inputs get one wave per tile.
inline unsigned grid_for(uint64_t ntiles, int blocks_per_cu, int num_cus)
{
    uint64_t want = (ntiles + kPlanWavesPerBlock - 1) / kPlanWavesPerBlock;
    uint64_t cap = (uint64_t)blocks_per_cu * (uint64_t)num_cus;
    if (want < 1) want = 1;
    return (unsigned)(want < cap ? want : cap);
}

// option "max_blocks_per_cu" (0 = no cap) on top of what a kernel admits
inline int cap_bpc(int bpc, int max_blocks_per_cu) { return (max_blocks_per_cu > 0 && max_blocks_per_cu < bpc) ? max_blocks_per_cu : bpc; }

// Measured on MI355X (tools/sweep.py, 1e9 rows): the scans run fastest with ~36-48 KiB of LDS-DMA in flight per CU -- one
// 4-wave block at c=9 (4 x 9 KiB tiles) -- and lose 3-6 % at the occupancy limit (more concurrent streams, same bytes).
// So: the number of blocks whose tiles add up to ~40 KiB.  Not clamped: the streaming scans and the column scan each clamp it
// in their own order around option "max_blocks_per_cu" (scan_want_bpc, columns_want_bpc).
inline int dma_in_flight_bpc(int tile_bytes) { return (40 * 1024 + 2 * tile_bytes) / (kPlanWavesPerBlock * tile_bytes); } // rounded

// Blocks per CU the streaming scans want (the launcher takes the smaller of this and what the occupancy query admits):
// the option unclamped, else dma_in_flight_bpc, at least 1.
inline int scan_want_bpc(int tile_bytes, int max_blocks_per_cu)
{
    if (max_blocks_per_cu > 0) return max_blocks_per_cu;
    int want = dma_in_flight_bpc(tile_bytes);
    if (want < 1) want = 1;
    if (want > 4) want = 4; // c = 1, 2 (1-2 KiB tiles): four blocks per CU beat eight by 20 % / 6 % (launches back to back)
    return want;
}
// resident blocks per CU for the streaming scans: what they want (scan_want_bpc), at most what the occupancy query admits
inline int scan_bpc(int occ_bpc, int tile_bytes, int max_blocks_per_cu)
{
    const int want = scan_want_bpc(tile_bytes, max_blocks_per_cu);
    return want < occ_bpc ? want : occ_bpc;
}

// Blocks per CU the column-against-column scan wants.  Both columns in registers (`same`): the plain scans' rule on the two tiles
// together (scan2_kernel: the DMA in flight per CU is what counts, about 40 KiB).  Column 2 read from LDS (32 rows per lane, small
// tiles, LDS reads all through the decode): as many blocks as fit, up to 4 waves per SIMD.  The option is clamped to 1..4 here.
inline int columns_want_bpc(bool same, int tile_bytes, int max_blocks_per_cu)
{
    int want = same ? dma_in_flight_bpc(tile_bytes) : 4;
    if (max_blocks_per_cu > 0) want = max_blocks_per_cu;
    if (want < 1) want = 1;
    if (want > 4) want = 4;
    return want;
}

// ---- store policies: `scan_nt_stores` is the option (-1 = by size), `out_bytes` what the launch writes ------------------

// Kernels that write every output byte once, in one pass (the eq / range scans, in_kernel, scan2_kernel, the column scan,
// the pair kernel and the one-pass LUT kernels): 0 plain, 1 non-temporal, 2 write-through (sc1).
// Bitmap stores, measured with launches back to back (bench.py --store-policy, same box, 1e9 x 9 bit unless noted):
// write-through (sc1) 0.201 ms, plain 0.207, non-temporal 0.216 -- dirty bitmap lines do not pile up in L2 to be
// written back under the next launch's read stream; c = 21: 0.438 / 0.467 / 0.457; c = 5: 0.127 / 0.129 / 0.136.
// Bitmaps far beyond the 256 MiB Infinity Cache prefer non-temporal stores: 4e9 rows sc1 0.82 ms / nt 0.85,
// 8e9 rows (1 GB of bitmap) 1.74 / 1.72.
// The one-pass shared scans follow (launches back to back, P = 8: 1e8 rows sc1 0.046 ms / plain 0.047 / nt 0.049; 1e9 rows
// nt 0.353-0.383 / sc1 0.347-0.393 / plain 0.40).
inline int one_pass_store_policy(uint64_t out_bytes, int scan_nt_stores)
{
    return scan_nt_stores < 0 ? (out_bytes > (768ull << 20) ? 1 : 2) : scan_nt_stores;
}

// The multi-pass shared scans of more than 8 keys / predicates: non-temporal result stores unless the P bitmaps together
// are small.  Measured (tools/sweep.py --nts 0,1, P = 8, c = 9): 1e8 rows (100 MB of bitmaps) 0.0540 -> 0.0525 ms, 5e8
// 0.220 -> 0.214, 1e9 0.409 -> 0.372; c = 17: -1..-4 %.  Unlike the single bitmap of the plain scans, these outputs gain
// nothing from staying in the Infinity Cache.
inline bool multi_pass_nt_stores(uint64_t out_bytes, int scan_nt_stores)
{
    return scan_nt_stores < 0 ? out_bytes > (64ull << 20) : scan_nt_stores != 0;
}

// ---- the eq / range scan's own rules ---------------------------------------------------------------------------------------

// tiles per store burst of scan_burst_kernel at width C.  Same-process A/B on four MI355X boxes (tools/ab_opts.py
// --opt scan_burst=..., 1e9 rows, launches back to back; profiles/r02_burst_*.txt): K = 4 is 0-4 % faster than K = 1 at
// c = 9 (never slower), +1-2 % at c = 5, 6, 0-2 % at c = 10..16; it LOSES at c = 7 (0.171 against 0.149 ms) and c = 8
// (0.184 against 0.177), is neutral at c <= 4, and -2 % at 64 values per lane (c >= 17).
constexpr int burst_k(int c) { return (c == 5 || c == 6 || (c >= 9 && c <= 16)) ? 4 : 1; }
// "scan_burst" option: 0 = the width's default, 1 = one tile per burst (A/B)
constexpr int burst_k(int c, int scan_burst) { return scan_burst == 1 ? 1 : burst_k(c); }

// Part of a column that the eq / range scan keeps in the 256 MiB Infinity Cache between launches (option "llc_resident_mib";
// ScanArgs::llc_d): 0 none, 1 all of it, else every d-th 64 KiB granule, d odd, so that with grids of a power of two times the
// CU count every wave meets the same share in every round.  resident bytes = min(column, budget - the bitmaps the call writes
// and reads, which live in the cache too).  Measured with launches back to back on one column (tools/llc_slice.hip,
// profiles/r05_llc_slice.txt, medians), 1e9 x 9 bit, 119 MiB of bitmap, write-through stores, against 0.1985 ms with nothing
// resident: 63 / 98 MiB (d = 17 / 11) 0.1908 / 0.1900 (-3.9 / -4.3 %), 119 MiB (d = 9) 0.1986, 153 MiB 0.2031 (+2 %): the gain
// ends between 217 and 238 MiB of column part plus bitmap.  The product in one process (profiles/r05_llc_ab.txt, tools/ab_opts.py):
// budgets 190 / 205 / 220 / 240 MiB (d = 17 / 13 / 11 / 9) 0.1947 / 0.1933 / 0.1950 / 0.2048 against 0.2026 ms, hence
// kLlcAutoMiB = 205: the best measured, and a step further from the cliff than 220.  5e8 rows: 0.0983 -> 0.0893 (d = 5, what 205
// gives there); 2.5e8: 0.0492 -> 0.0460 (d = 3).  A column that fits whole gains nothing (1.25e8 rows: 0.0227 against 0.0228 ms;
// the product at 1e8 rows +3 %): auto leaves d = 1 to an explicit budget.
// When the column is NOT what the cache holds -- two 1e9-row columns scanned in turn, each into its own bitmap -- any resident
// part costs (16 / 33 / 98 MiB: +8 / +14 / +17 %: the default-policy loads push the other scan's dirty bitmap lines out to HBM),
// so auto acts only on a repeat: the context's previous launch was a scan of the same column, bitmap and mask
// (LaunchReq::llc_repeat).  An explicit budget (> 0) applies to every call.
constexpr int kLlcAutoMiB = 205;
inline uint32_t llc_divisor(int llc_resident_mib, int dma_aux, int llc_repeat, uint64_t column_bytes, uint64_t bitmap_bytes)
{
    if (llc_resident_mib == 0 || (dma_aux & 15) == 0) return 0; // off; dma_aux = 0: every load has the default policy anyway
    if (bitmap_bytes > (768ull << 20)) return 0;                // the bitmap alone is far beyond the cache (see one_pass_store_policy)
    const bool automatic = llc_resident_mib < 0;
    if (automatic && !llc_repeat) return 0;
    const uint64_t budget = (uint64_t)(automatic ? kLlcAutoMiB : llc_resident_mib) << 20;
    if (budget <= bitmap_bytes) return 0;
    const uint64_t resident = budget - bitmap_bytes;
    if (resident >= column_bytes) return automatic ? 0 : 1;
    const uint64_t d = ((column_bytes + resident - 1) / resident) | 1u; // >= 3, odd
    return d > 0x7fffffu ? 0 : (uint32_t)d;
}

// ---- AUX: the cache-policy template argument of a kernel, from option "dma_aux" and the store policy (0 plain, 1 nt, 2 sc1) -----
// 0 default loads and stores, 2 nt loads (the column is read once), 18 nt loads + nt stores, 34 nt loads + write-through stores

constexpr int scan_aux(int dma_aux, int policy) { return dma_aux == 0 ? 0 : (policy == 1 ? 18 : (policy == 2 ? 34 : 2)); }
constexpr int in_aux(int policy) { return policy == 2 ? 34 : (policy == 1 ? 18 : 2); } // (and the where-scans' one-pass table kernel)
constexpr int scan2_aux(int policy) { return policy == 1 ? 18 : 34; } // (no plain-store form: 0 runs write-through)
// default (dma_aux 18): nt loads + nt stores -- the 4 B/value output is written once (+1-2 %); 2 and 34: tools/sweep.py --aux
constexpr int decompress_aux(int dma_aux) { return (dma_aux == 0 || dma_aux == 2 || dma_aux == 34) ? dma_aux : 18; }

// ---- the plans ---------------------------------------------------------------------------------------------------------------

// the fields of a LaunchReq (dispatch.hpp) that the rules read
struct PlanReq {
    int num_cus, max_blocks_per_cu, dma_aux, scan_nt_stores, scan_burst, llc_resident_mib, llc_repeat, select_single;
};
// a wave tile, as ScanGeom / DecompGeom have it
struct PlanTile {
    int values, bytes;
};
struct ScanPlan {
    int aux = 0;         // the kernel's AUX template argument
    int k = 1;           // scan_burst_kernel: tiles per store burst
    int bpc = 1;         // blocks per CU
    unsigned grid = 1;   // blocks
    unsigned block = 64 * kPlanWavesPerBlock; // threads per block
    uint32_t llc_d = 0;  // eq / range scan: ScanArgs::llc_d
};
inline uint64_t tiles_of(uint64_t n, int tile_values) { return (n + tile_values - 1) / tile_values; }

// scan_burst_kernel<C, MODE, aux, VPL, k>; `k` is burst_k(c, scan_burst), `occ_bpc` what that K's kernel admits.
// `has_out` / `has_mask`: the bitmap the call writes and the one it reads, which share the cache with the column.
inline ScanPlan plan_scan(const PlanReq &q, PlanTile tile, int c, uint64_t n, bool has_out, bool has_mask, int k, int occ_bpc)
{
    ScanPlan p;
    p.aux = scan_aux(q.dma_aux, one_pass_store_policy(n / 8, q.scan_nt_stores));
    p.k = k;
    p.bpc = scan_bpc(occ_bpc, tile.bytes, q.max_blocks_per_cu);
    p.grid = grid_for((tiles_of(n, tile.values) + k - 1) / k, p.bpc, q.num_cus);
    p.llc_d = llc_divisor(q.llc_resident_mib, q.dma_aux, q.llc_repeat, (n * c + 7) / 8, (has_out ? (n + 7) / 8 : 0) + (has_mask ? (n + 7) / 8 : 0));
    return p;
}

// in_kernel<C, aux, VPL>.  One LDS lookup per value: a second wave per SIMD hides the lookup latency (measured, 1e9 rows, P = 40:
// c = 9 0.31 -> 0.23 ms, c = 12 0.32 -> 0.29, c = 16 0.51 -> 0.45 with two blocks per CU instead of one)
inline ScanPlan plan_in(const PlanReq &q, PlanTile tile, uint64_t n, int occ_bpc)
{
    ScanPlan p;
    p.aux = in_aux(one_pass_store_policy(n / 8, q.scan_nt_stores));
    p.bpc = scan_bpc(occ_bpc, tile.bytes, q.max_blocks_per_cu);
    if (q.max_blocks_per_cu <= 0 && p.bpc < 2 && occ_bpc >= 2) p.bpc = 2;
    p.grid = grid_for(tiles_of(n, tile.values), p.bpc, q.num_cus);
    return p;
}

// scan2_kernel<C, aux, VPL>: two columns of this width in one launch: twice the DMA per tile, so half the blocks per CU of the plain scan
inline ScanPlan plan_scan2(const PlanReq &q, PlanTile tile, uint64_t n, int occ_bpc)
{
    ScanPlan p;
    p.aux = scan2_aux(one_pass_store_policy(n / 8, q.scan_nt_stores));
    p.bpc = scan_bpc(occ_bpc, 2 * tile.bytes, q.max_blocks_per_cu);
    p.grid = grid_for(tiles_of(n, tile.values), p.bpc, q.num_cus);
    return p;
}

// decompress_kernel<C, aux>.  Blocks per CU, launches back to back, 1e9 rows.  Round 1 (one box): four blocks 0.863-0.871 ms at c = 9
// against 0.903-0.907 with one.  Round 2, every width 1..32 on two boxes (profiles/r02_decompress_bpc_sweep.txt): the best
// count differs between boxes and widths -- four blocks cost up to 16 % at c <= 8 on one box (c = 8: 0.909 / 0.948 /
// 1.055 ms with 1 / 2 / 4), one block costs 6-12 % at c <= 5 on the other -- and TWO is within 2-4 % of the best
// almost everywhere on both.
inline ScanPlan plan_decompress(const PlanReq &q, PlanTile tile, uint64_t n, int occ_bpc)
{
    ScanPlan p;
    p.aux = decompress_aux(q.dma_aux);
    p.bpc = q.max_blocks_per_cu > 0 ? cap_bpc(occ_bpc, q.max_blocks_per_cu) : (occ_bpc < 2 ? occ_bpc : 2);
    p.grid = grid_for(tiles_of(n, tile.values), p.bpc, q.num_cus);
    return p;
}

// predicate -> row ids: one block per CU (LDS: tiles + mask image + 16 KiB id stage per wave), every wave on a
// chunk of `tiles_per_chunk` tiles.  Chunks are claimed from a ticket counter, so the grid need not be resident
// as a whole (another context's kernel may hold CUs): a look-back only ever waits for running waves.
// (option "select_kernel" = 1: round 2's single-role kernel of four waves, for A/B; else the decoder / expander roles' `role_waves`)
inline ScanPlan plan_select(const PlanReq &q, PlanTile tile, uint64_t n, int tiles_per_chunk, int role_waves)
{
    ScanPlan p;
    p.bpc = 1;
    p.grid = grid_for((tiles_of(n, tile.values) + tiles_per_chunk - 1) / tiles_per_chunk, p.bpc, q.num_cus);
    p.block = q.select_single ? 64u * kPlanWavesPerBlock : 64u * (unsigned)role_waves;
    return p;
}

} // namespace mi355
