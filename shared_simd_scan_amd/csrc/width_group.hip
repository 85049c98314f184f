// width_group.hip -- instantiates the width-templated kernels for widths MI355_WLO..MI355_WHI and
// exports one launcher per group.  Compiled 8 times (4 widths each) so the build parallelises.
#include <type_traits>

#include "dispatch.hpp"
#include "kernels.hpp"
#include "launch_util.hpp"
#include "shared_plan.hpp"

#ifndef MI355_WLO
#error "compile with -DMI355_WLO=<first width> -DMI355_WHI=<last width> -DMI355_GROUP=<index>"
#endif

namespace mi355 {

namespace {

// resident blocks per CU for the streaming scans: what they want (scan_want_bpc), at most what the occupancy query admits
inline int scan_bpc(int occ_bpc, int tile_bytes, const LaunchReq &r)
{
    const int want = scan_want_bpc(tile_bytes, r.max_blocks_per_cu);
    return want < occ_bpc ? want : occ_bpc;
}

// tiles per store burst of scan_burst_kernel at width C.  Same-process A/B on four MI355X boxes (tools/ab_opts.py
// --opt scan_burst=..., 1e9 rows, launches back to back; profiles/r02_burst_*.txt): K = 4 is 0-4 % faster than K = 1 at
// c = 9 (never slower), +1-2 % at c = 5, 6, 0-2 % at c = 10..16; it LOSES at c = 7 (0.171 against 0.149 ms) and c = 8
// (0.184 against 0.177), is neutral at c <= 4, and -2 % at 64 values per lane (c >= 17).
constexpr int burst_k(int c) { return (c == 5 || c == 6 || (c >= 9 && c <= 16)) ? 4 : 1; }

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
inline uint32_t llc_divisor(const LaunchReq &r, uint64_t column_bytes, uint64_t bitmap_bytes)
{
    if (r.llc_resident_mib == 0 || (r.dma_aux & 15) == 0) return 0; // off; dma_aux = 0: every load has the default policy anyway
    if (bitmap_bytes > (768ull << 20)) return 0;                    // the bitmap alone is far beyond the cache (see one_pass_store_policy)
    const bool automatic = r.llc_resident_mib < 0;
    if (automatic && !r.llc_repeat) return 0;
    const uint64_t budget = (uint64_t)(automatic ? kLlcAutoMiB : r.llc_resident_mib) << 20;
    if (budget <= bitmap_bytes) return 0;
    const uint64_t resident = budget - bitmap_bytes;
    if (resident >= column_bytes) return automatic ? 0 : 1;
    const uint64_t d = ((column_bytes + resident - 1) / resident) | 1u; // >= 3, odd
    return d > 0x7fffffu ? 0 : (uint32_t)d;
}

template <int C, int MODE> void launch_scan(const LaunchReq &r)
{
    constexpr int VPL = scan_vpl(C, MODE);
    using G = ScanGeom<C, VPL>;
    const uint64_t ntiles = (r.scan.n + G::TILE_VALUES - 1) / G::TILE_VALUES;
    // dma_aux: cache policy of the HBM->LDS stream; 2 (non-temporal: the column is read once) is the default.
    const int policy = one_pass_store_policy(r.scan.n / 8, r.scan_nt_stores); // 0 plain, 1 nt, 2 sc1
    ScanArgs a = r.scan;
    llc_set(a, llc_divisor(r, (r.scan.n * C + 7) / 8, (r.scan.out ? (r.scan.n + 7) / 8 : 0) + (r.scan.and_mask ? (r.scan.n + 7) / 8 : 0)));
    if (r.llc_d_out) *r.llc_d_out = (int)a.llc_d;
    auto go = [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        static const int bpcK = blocks_per_cu(scan_burst_kernel<C, MODE, 34, VPL, K>);
        const dim3 grid(grid_for((ntiles + K - 1) / K, scan_bpc(bpcK, G::TILE_BYTES, r), r.num_cus));
        if (r.dma_aux == 0)
            MI355_LAUNCH(r, a.flags, (scan_burst_kernel<C, MODE, 0, VPL, K>), grid, dim3(kBlockThreads), 0, r.stream, a);
        else if (policy == 1)
            MI355_LAUNCH(r, a.flags, (scan_burst_kernel<C, MODE, 18, VPL, K>), grid, dim3(kBlockThreads), 0, r.stream, a);
        else if (policy == 2)
            MI355_LAUNCH(r, a.flags, (scan_burst_kernel<C, MODE, 34, VPL, K>), grid, dim3(kBlockThreads), 0, r.stream, a);
        else
            MI355_LAUNCH(r, a.flags, (scan_burst_kernel<C, MODE, 2, VPL, K>), grid, dim3(kBlockThreads), 0, r.stream, a);
    };
    // "scan_burst" option: 0 = the width's default, 1 = one tile per burst (A/B)
    if (burst_k(C) > 1 && r.scan_burst != 1)
        go(std::integral_constant<int, burst_k(C)>{});
    else
        go(std::integral_constant<int, 1>{});
}

// ---- equality shared scans: launch what plan_shared() decided.  The only place that names their kernel templates. ---------

// one launch of a planned kernel: the launcher's own flag bits, the dynamic-LDS limit (max_dyn > 0), the grid
template <auto Kernel> void launch_planned(const LaunchReq &r, const SharedPlan &p, int bpc, int max_dyn = 0)
{
    ScanArgs a = r.scan;
    a.flags |= p.set_flags;
    const uint64_t tile_values = 64 * (uint64_t)p.vpl;
    const dim3 grid(grid_for((a.n + tile_values - 1) / tile_values, bpc, r.num_cus));
    if (max_dyn > 0) allow_dynamic_lds<Kernel>(max_dyn, r.device);
    MI355_LAUNCH(r, a.flags, Kernel, grid, dim3(kBlockThreads), p.dyn_lds, r.stream, a);
}

// ... of the non-temporal form of a kernel if the plan says so, else of its other form
template <auto Kernel, auto NtKernel> void launch_planned_nt(const LaunchReq &r, const SharedPlan &p, int bpc, int max_dyn = 0)
{
    p.store == 1 ? launch_planned<NtKernel>(r, p, bpc, max_dyn) : launch_planned<Kernel>(r, p, bpc, max_dyn);
}

template <int C, int VPL> void launch_pair(const LaunchReq &r, const SharedPlan &p)
{
    static const int occ = blocks_per_cu(shared_pair_kernel<C, 34, VPL>);
    launch_planned_nt<shared_pair_kernel<C, 34, VPL>, shared_pair_kernel<C, 18, VPL>>(r, p, p.want_bpc < occ ? p.want_bpc : occ);
}

template <int C, int VPL, int LINEAR> void launch_lut8(const LaunchReq &r, const SharedPlan &p)
{
    static const int occ = blocks_per_cu(shared_lut_kernel<C, 2, VPL, LINEAR, false>);
    const int bpc = p.want_bpc < occ ? p.want_bpc : occ;
    if (p.store == 2)
        launch_planned<shared_lut_kernel<C, 34, VPL, LINEAR, false>>(r, p, bpc);
    else
        launch_planned_nt<shared_lut_kernel<C, 2, VPL, LINEAR, false>, shared_lut_kernel<C, 18, VPL, LINEAR, false>>(r, p, bpc);
}

template <int C> void launch_shared(const LaunchReq &r, const SharedPlan &p)
{
    constexpr int VPL = kSharedVpl;
    constexpr bool kBigWidth = shared_big_width(C);
    constexpr int max_dyn = shared_max_dyn_lds<C>();
    const bool linear = r.scan.layout != 0;
    switch (p.form) {
    case kFormPair: p.vpl == 64 ? launch_pair<C, 64>(r, p) : launch_pair<C, scan_vpl(C, kModeEq)>(r, p); break;
    case kFormLut:
        if constexpr (C <= 12) {
            if (p.vpl == 128) {
                linear ? launch_lut8<C, 128, 1>(r, p) : launch_lut8<C, 128, 0>(r, p);
                break;
            }
        }
        linear ? launch_lut8<C, 64, 1>(r, p) : launch_lut8<C, 64, 0>(r, p);
        break;
    case kFormLinear3:
        with_rc_big<2, kBigWidth>(p.rc, p.big, [&](auto rc, auto big) {
            launch_planned<shared_linear3_kernel<C, 2, rc.value, big.value>>(r, p, p.want_bpc, (int)(kCuLdsBytes - linear3_fixed_lds<C>()));
        });
        break;
    case kFormLutMulti: launch_planned<shared_lut_kernel<C, 2, VPL, 1, true>>(r, p, p.want_bpc, max_dyn); break;
    case kFormLinearTwoRows: launch_planned<shared_linear_kernel<C, 2, 2>>(r, p, p.want_bpc, max_dyn); break;
    case kFormLinear: launch_planned<shared_linear_kernel<C, 2, 1>>(r, p, p.want_bpc, max_dyn); break;
    case kFormLinear2: launch_planned<shared_linear2_kernel<C, 2>>(r, p, p.want_bpc, max_dyn); break;
    case kFormWide3:
        with_rc_big<2, kBigWidth>(p.rc, p.big, [&](auto rc, auto big) {
            launch_planned_nt<shared_wide3_kernel<C, 2, rc.value, big.value>, shared_wide3_kernel<C, 18, rc.value, big.value>>(r, p, p.want_bpc, max_dyn);
        });
        break;
    case kFormWide2: // (register counters at the single-table widths only)
        with_rc_big<(C <= 10 ? 2 : 0), kBigWidth>(p.rc, p.big, [&](auto rc, auto big) {
            launch_planned_nt<shared_wide2_kernel<C, 2, VPL, rc.value, big.value>, shared_wide2_kernel<C, 18, VPL, rc.value, big.value>>(r, p, p.want_bpc,
                                                                                                                                       max_dyn);
        });
        break;
    case kFormWideLinear: launch_planned<shared_wide_kernel<C, 2, VPL, 1>>(r, p, p.want_bpc, max_dyn); break;
    case kFormWide: launch_planned_nt<shared_wide_kernel<C, 2, VPL, 0>, shared_wide_kernel<C, 18, VPL, 0>>(r, p, p.want_bpc, max_dyn); break;
    case kFormChain: {
        static const int occ = blocks_per_cu(shared_general_kernel<C, 2, VPL>);
        launch_planned<shared_general_kernel<C, 2, VPL>>(r, p, cap_bpc(occ, p.want_bpc));
        break;
    }
    default: break;
    }
}

template <int C> hipError_t launch_width(const LaunchReq &r)
{
    switch (r.op) {
    case kOpScanEq: launch_scan<C, kModeEq>(r); break;
    case kOpScanRange: launch_scan<C, kModeRange>(r); break;
    case kOpSharedScan: {
        const SharedPlan plan = plan_shared<C>(r);
        if (r.choice_out) *r.choice_out = plan.family; // introspection (mi355_shared_scan_kernel): MI355_LAUNCH launches nothing
        launch_shared<C>(r, plan);
        break;
    }
    case kOpScanIn: {
        constexpr int VPL = scan_vpl(C, kModeEq);
        using G = ScanGeom<C, VPL>;
        static const int bpc = blocks_per_cu(in_kernel<C, 2, VPL>);
        const uint64_t ntiles = (r.scan.n + G::TILE_VALUES - 1) / G::TILE_VALUES;
        // one LDS lookup per value: a second wave per SIMD hides the lookup latency (measured, 1e9 rows, P = 40:
        // c = 9 0.31 -> 0.23 ms, c = 12 0.32 -> 0.29, c = 16 0.51 -> 0.45 with two blocks per CU instead of one)
        int want = scan_bpc(bpc, G::TILE_BYTES, r);
        if (r.max_blocks_per_cu <= 0 && want < 2 && bpc >= 2) want = 2;
        const int ipol = one_pass_store_policy(r.scan.n / 8, r.scan_nt_stores);
        if (ipol == 2)
            MI355_LAUNCH(r, r.scan.flags, (in_kernel<C, 34, VPL>), dim3(grid_for(ntiles, want, r.num_cus)), dim3(kBlockThreads), 0, r.stream, r.scan);
        else if (ipol == 1)
            MI355_LAUNCH(r, r.scan.flags, (in_kernel<C, 18, VPL>), dim3(grid_for(ntiles, want, r.num_cus)), dim3(kBlockThreads), 0, r.stream, r.scan);
        else
            MI355_LAUNCH(r, r.scan.flags, (in_kernel<C, 2, VPL>), dim3(grid_for(ntiles, want, r.num_cus)), dim3(kBlockThreads), 0, r.stream, r.scan);
        break;
    }
    case kOpSelect: {
        // predicate -> row ids: one block per CU (LDS: tiles + mask image + 16 KiB id stage per wave), every wave on a
        // chunk of select_tiles(C) tiles.  Chunks are claimed from a ticket counter, so the grid need not be resident
        // as a whole (another context's kernel may hold CUs): a look-back only ever waits for running waves
        constexpr int VPL = scan_vpl(C, kModeRange);
        using G = ScanGeom<C, VPL>;
        const uint64_t ntiles = (r.scan.n + G::TILE_VALUES - 1) / G::TILE_VALUES;
        const uint64_t nchunks = (ntiles + select_tiles(C) - 1) / select_tiles(C);
        // (option "select_kernel" = 1: round 2's single-role kernel, for A/B)
        const dim3 sgrid(grid_for(nchunks, 1, r.num_cus));
        if (r.select_single)
            MI355_LAUNCH(r, r.scan.flags, (select_kernel<C, kModeRange, VPL>), sgrid, dim3(kBlockThreads), 0, r.stream, r.scan);
        else
            MI355_LAUNCH(r, r.scan.flags, (select2_kernel<C, kModeRange, VPL>), sgrid, dim3(kSel2Waves * 64), 0, r.stream, r.scan);
        break;
    }
    case kOpScan2: {
        // two columns of this width in one launch: twice the DMA per tile, so half the blocks per CU of the plain scan
        constexpr int VPL = scan_vpl(C, kModeRange);
        using G = ScanGeom<C, VPL>;
        static const int bpc = blocks_per_cu(scan2_kernel<C, 34, VPL>);
        const uint64_t ntiles = (r.scan.n + G::TILE_VALUES - 1) / G::TILE_VALUES;
        const dim3 grid(grid_for(ntiles, scan_bpc(bpc, 2 * G::TILE_BYTES, r), r.num_cus));
        const int policy = one_pass_store_policy(r.scan.n / 8, r.scan_nt_stores);
        if (policy == 1)
            MI355_LAUNCH(r, r.scan.flags, (scan2_kernel<C, 18, VPL>), grid, dim3(kBlockThreads), 0, r.stream, r.scan);
        else
            MI355_LAUNCH(r, r.scan.flags, (scan2_kernel<C, 34, VPL>), grid, dim3(kBlockThreads), 0, r.stream, r.scan);
        break;
    }
    case kOpDecompress: {
        static const int bpc = blocks_per_cu(decompress_kernel<C, 18>);
        const uint64_t ntiles = (r.decomp.n + DecompGeom<C>::TILE_VALUES - 1) / DecompGeom<C>::TILE_VALUES;
        // Blocks per CU, launches back to back, 1e9 rows.  Round 1 (one box): four blocks 0.863-0.871 ms at c = 9 against
        // 0.903-0.907 with one.  Round 2, every width 1..32 on two boxes (profiles/r02_decompress_bpc_sweep.txt): the best
        // count differs between boxes and widths -- four blocks cost up to 16 % at c <= 8 on one box (c = 8: 0.909 / 0.948 /
        // 1.055 ms with 1 / 2 / 4), one block costs 6-12 % at c <= 5 on the other -- and TWO is within 2-4 % of the best
        // almost everywhere on both.
        const int want = bpc < 2 ? bpc : 2;
        const unsigned grid = grid_for(ntiles, r.max_blocks_per_cu > 0 ? cap_bpc(bpc, r.max_blocks_per_cu) : want, r.num_cus);
        if (r.dma_aux == 0)
            MI355_LAUNCH(r, 0, (decompress_kernel<C, 0>), dim3(grid), dim3(kBlockThreads), 0, r.stream, r.decomp);
        else if (r.dma_aux == 2) // nt DMA loads only (tools/sweep.py --aux 2)
            MI355_LAUNCH(r, 0, (decompress_kernel<C, 2>), dim3(grid), dim3(kBlockThreads), 0, r.stream, r.decomp);
        else if (r.dma_aux == 34) // nt loads + write-through stores
            MI355_LAUNCH(r, 0, (decompress_kernel<C, 34>), dim3(grid), dim3(kBlockThreads), 0, r.stream, r.decomp);
        else // default (dma_aux 18): nt loads + nt stores -- the 4 B/value output is written once (+1-2 %)
            MI355_LAUNCH(r, 0, (decompress_kernel<C, 18>), dim3(grid), dim3(kBlockThreads), 0, r.stream, r.decomp);
        break;
    }
    default:
        return hipErrorInvalidValue;
    }
    return launch_status(r);
}

} // namespace

hipError_t MI355_CAT(launch_group_, MI355_GROUP)(const LaunchReq &r)
{
    return launch_by_width<MI355_WLO, MI355_WHI>(r.c, r, [](auto c, const LaunchReq &q) { return launch_width<decltype(c)::value>(q); });
}

} // namespace mi355
