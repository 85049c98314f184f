// columns_group.hip -- instantiates scan_columns_kernel (predicates/columns.hpp) for column-1 widths MI355_WLO..MI355_WHI and
// exports one launcher per group.  Compiled 8 times (4 widths each), like where_group.hip.
//
// Per width of column 1: the same-width form, and the run-time-width form with the 32-bit comparison (C1 <= 30 only) and
// with the 64-bit one -- 94 kernels in all, not 1024.
#include <atomic>

#include "../launch_util.hpp"
#include "columns_dispatch.hpp"

#ifndef MI355_WLO
#error "compile with -DMI355_WLO=<first width> -DMI355_WHI=<last width> -DMI355_GROUP=<index>"
#endif

namespace mi355 {

template <int C1, int VPL, bool SAME, bool WIDE>
__global__ __launch_bounds__(kBlockThreads, (columns_occ<C1, VPL, SAME>())) void scan_columns_kernel(ColumnsArgs a)
{
    scan_columns_body<C1, VPL, SAME, WIDE>(a);
}

namespace {

// Blocks per CU: what the scan wants (scan_plan.hpp columns_want_bpc), inside what LDS and registers admit
template <auto Kernel> int columns_bpc(const ColumnsReq &r, bool same, int tile_bytes, size_t lds)
{
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, Kernel, kBlockThreads, lds) != hipSuccess || occ < 1) occ = 1;
    const int want = columns_want_bpc(same, tile_bytes, r.l.max_blocks_per_cu);
    return want < occ ? want : occ;
}

template <int C, int VPL, bool SAME, bool WIDE> hipError_t launch_form(const ColumnsReq &r)
{
    using G = ScanGeom<C, VPL>;
    const uint32_t c2 = r.k.c2;
    const uint64_t ntiles = (r.k.s.n + G::TILE_VALUES - 1) / G::TILE_VALUES;
    const size_t lds = columns_block_lds<C, VPL, SAME>(c2);
    const int tile_bytes = G::TILE_BYTES + (int)(64u * VPL / 8u * c2);
    allow_dynamic_lds<scan_columns_kernel<C, VPL, SAME, WIDE>>((int)columns_block_lds<C, VPL, SAME>(SAME ? C : 32), r.l.device);
    // the occupancy query depends on the dynamic LDS, i.e. on c2: asked once per width of column 2
    static std::atomic<int> bpc_of[33];
    int occ_bpc = bpc_of[c2].load(std::memory_order_relaxed);
    if (occ_bpc == 0 || r.l.max_blocks_per_cu > 0) {
        occ_bpc = columns_bpc<scan_columns_kernel<C, VPL, SAME, WIDE>>(r, SAME, tile_bytes, lds);
        if (r.l.max_blocks_per_cu <= 0) bpc_of[c2].store(occ_bpc, std::memory_order_relaxed);
    }
    const dim3 grid(grid_for(ntiles, occ_bpc, r.l.num_cus));
    MI355_LAUNCH(r.l, 0, (scan_columns_kernel<C, VPL, SAME, WIDE>), grid, dim3(kBlockThreads), lds, r.l.stream, r.k);
    return launch_status(r.l);
}

template <int C> hipError_t launch_columns(const ColumnsReq &r)
{
    const uint32_t c2 = r.k.c2;
    if (c2 == (uint32_t)C) return launch_form<C, columns_vpl(C, true), true, (C > 30)>(r);
    if constexpr (C <= 30) {
        if (c2 <= 30) return launch_form<C, columns_vpl(C, false), false, false>(r);
    }
    return launch_form<C, columns_vpl(C, false), false, true>(r);
}

} // namespace

hipError_t MI355_CAT(launch_columns_group_, MI355_GROUP)(const ColumnsReq &r)
{
    return launch_by_width<MI355_WLO, MI355_WHI>(r.l.c, r, [](auto c, const ColumnsReq &q) { return launch_columns<decltype(c)::value>(q); });
}

} // namespace mi355
