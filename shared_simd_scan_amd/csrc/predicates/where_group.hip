// where_group.hip -- instantiates the kernels of predicates/where.hpp for widths MI355_WLO..MI355_WHI and exports one
// launcher per group.  Compiled 8 times (4 widths each), like width_group.hip.
#include "../launch_util.hpp"
#include "../shared_plan.hpp"
#include "where_dispatch.hpp"

#ifndef MI355_WLO
#error "compile with -DMI355_WLO=<first width> -DMI355_WHI=<last width> -DMI355_GROUP=<index>"
#endif

namespace mi355 {

namespace {

constexpr int kWhereVpl = kSharedVpl; // 64 values per lane and tile, as the equality shared scans

// ---- the fit rule ----------------------------------------------------------------------------
// The multi-pass table kernel keeps ceil(P / 8) full tables of max(2^c, 4) bytes in dynamic LDS next to its static part:
// four tiles, the per-block hit counters, and 512 bytes for the small things (prefix carries, ticket word, padding).  A
// list goes to it when both fit into the CU's 160 KiB: every P <= 1024 at c <= 10, P <= 256 at c = 12, nothing beyond
// 8 predicates at c = 16 (two 64 KiB tables + 32 KiB of tiles).
template <int C> constexpr size_t where_static_lds() { return 4 * ScanGeom<C, kWhereVpl>::LDS_BYTES + kMaxKeys * 4 + 512; }
template <int C> constexpr size_t where_table_bytes(uint32_t P)
{
    return ((size_t)((P + 7) / 8) * WhereLutGeom<C>::TABLE_BYTES + 15) / 16 * 16;
}
template <int C> constexpr bool where_tables_fit(uint32_t P) { return where_table_bytes<C>(P) + where_static_lds<C>() <= kCuLdsBytes; }

// blocks per CU of the table kernels: shared_lut_kernel's rule (lut_want_bpc), as far as the tables leave room
template <int C> int where_lut_bpc(const WhereReq &r, bool linear, size_t lds_per_block)
{
    const int want = lut_want_bpc(ScanGeom<C, kWhereVpl>::TILE_BYTES, linear, r.l.max_blocks_per_cu);
    int fit = (int)(kCuLdsBytes / lds_per_block);
    if (fit < 1) fit = 1;
    return want < fit ? want : fit;
}

// one launch of a where-kernel: the dynamic-LDS limit (max_dyn > 0), then the launch (the kernels read no flag bits)
template <auto Kernel> void launch_where_kernel(const WhereReq &r, dim3 grid, size_t dyn_lds = 0, int max_dyn = 0)
{
    if (max_dyn > 0) allow_dynamic_lds<Kernel>(max_dyn, r.l.device);
    MI355_LAUNCH(r.l, 0, Kernel, grid, dim3(kBlockThreads), dyn_lds, r.l.stream, r.w);
}

template <int C> hipError_t launch_where(const WhereReq &r)
{
    constexpr int VPL = kWhereVpl;
    using G = ScanGeom<C, VPL>;
    const ScanArgs &s = r.w.s;
    const uint32_t P = s.nkeys;
    const bool linear = s.layout != 0;
    const uint64_t ntiles = (s.n + G::TILE_VALUES - 1) / G::TILE_VALUES;
    int choice = kWhereChain;
    if constexpr (C <= 16) choice = P <= 8 ? kWhereLut : (where_tables_fit<C>(P) ? kWhereLutMulti : kWhereChain);
    if (r.l.choice_out) *r.l.choice_out = choice; // introspection (mi355_shared_where_kernel): MI355_LAUNCH launches nothing
    if constexpr (C <= 16) {
        if (choice == kWhereLut) {
            // result stores as shared_lut_kernel's launcher: write-through below 768 MiB of output, non-temporal beyond
            const int spol = one_pass_store_policy((s.n / 8) * P, r.l.scan_nt_stores); // 0 plain, 1 nt, 2 sc1
            const size_t per_block = 4 * G::LDS_BYTES + WhereLutGeom<C>::TABLE_BYTES + (linear ? 4 * (VPL / 8) * 8 * 64 : 0) + 512;
            const dim3 grid(grid_for(ntiles, where_lut_bpc<C>(r, linear, per_block), r.l.num_cus));
            auto go = [&](auto layout) {
                constexpr int LAYOUT = decltype(layout)::value;
                if (spol == 1)
                    launch_where_kernel<shared_where_lut_kernel<C, 18, VPL, LAYOUT, false>>(r, grid);
                else if (spol == 2)
                    launch_where_kernel<shared_where_lut_kernel<C, 34, VPL, LAYOUT, false>>(r, grid);
                else
                    launch_where_kernel<shared_where_lut_kernel<C, 2, VPL, LAYOUT, false>>(r, grid);
            };
            linear ? go(std::integral_constant<int, 1>{}) : go(std::integral_constant<int, 0>{});
            return launch_status(r.l);
        }
        if constexpr (where_tables_fit<C>(9)) // (c = 16: two tables never fit, the multi-pass form is not instantiated)
        if (choice == kWhereLutMulti) {
            // per-predicate result stores: non-temporal unless the P bitmaps together are small (the rule of the equality
            // scans of more than 8 keys)
            const bool nt_stores = multi_pass_nt_stores((s.n / 8) * P, r.l.scan_nt_stores);
            const size_t dyn = where_table_bytes<C>(P);
            const int max_dyn = (int)(kCuLdsBytes - where_static_lds<C>());
            const dim3 grid(grid_for(ntiles, where_lut_bpc<C>(r, linear, dyn + where_static_lds<C>()), r.l.num_cus));
            if (linear)
                launch_where_kernel<shared_where_lut_kernel<C, 2, VPL, 1, true>>(r, grid, dyn, max_dyn);
            else if (nt_stores)
                launch_where_kernel<shared_where_lut_kernel<C, 18, VPL, 0, true>>(r, grid, dyn, max_dyn);
            else
                launch_where_kernel<shared_where_lut_kernel<C, 2, VPL, 0, true>>(r, grid, dyn, max_dyn);
            return launch_status(r.l);
        }
    }
    if constexpr (C >= 11) { // (at c <= 10 every list fits the tables)
        static const int bpc = blocks_per_cu(shared_where_chain_kernel<C, 2, VPL>);
        launch_where_kernel<shared_where_chain_kernel<C, 2, VPL>>(r, dim3(grid_for(ntiles, cap_bpc(bpc, r.l.max_blocks_per_cu), r.l.num_cus)));
        return launch_status(r.l);
    }
    return hipErrorInvalidValue;
}

} // namespace

hipError_t MI355_CAT(launch_where_group_, MI355_GROUP)(const WhereReq &r)
{
    return launch_by_width<MI355_WLO, MI355_WHI>(r.l.c, r, [](auto c, const WhereReq &q) { return launch_where<decltype(c)::value>(q); });
}

} // namespace mi355
