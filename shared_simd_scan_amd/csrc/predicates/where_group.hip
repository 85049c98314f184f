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

// ---- which kernel a where-scan of P >= 2 predicates runs, decided once: a pure function of the request, as plan_shared() ------
struct WherePlan {
    int choice;     // WhereChoice, what mi355_shared_where_kernel names
    int aux;        // the kernel's AUX: 2 plain, 18 non-temporal, 34 write-through result stores
    size_t dyn_lds; // dynamic LDS bytes
    int max_dyn;    // > 0: the most dynamic LDS the kernel is ever given
    int want_bpc;   // blocks per CU; kWhereChain: the option's cap on what the occupancy query admits, 0 = none
};

template <int C> WherePlan plan_where(const WhereReq &r)
{
    if constexpr (C <= 16) {
        using G = ScanGeom<C, kWhereVpl>;
        const uint32_t P = r.w.s.nkeys;
        const uint64_t out_bytes = (r.w.s.n / 8) * P; // the P bitmaps together
        const bool linear = r.w.s.layout != 0;
        if (P <= 8) {
            // result stores as shared_lut_kernel's launcher: write-through below 768 MiB of output, non-temporal beyond (AUX as in_kernel's)
            const size_t per_block = 4 * G::LDS_BYTES + WhereLutGeom<C>::TABLE_BYTES + (linear ? 4 * (kWhereVpl / 8) * 8 * 64 : 0) + 512;
            return WherePlan{kWhereLut, in_aux(one_pass_store_policy(out_bytes, r.l.scan_nt_stores)), 0, 0, where_lut_bpc<C>(r, linear, per_block)};
        }
        if (where_tables_fit<C>(P)) {
            // per-predicate result stores: non-temporal unless the P bitmaps together are small (the rule of the equality
            // scans of more than 8 keys); linear rows: plain
            const size_t dyn = where_table_bytes<C>(P);
            return WherePlan{kWhereLutMulti, (!linear && multi_pass_nt_stores(out_bytes, r.l.scan_nt_stores)) ? 18 : 2, dyn,
                             (int)(kCuLdsBytes - where_static_lds<C>()), where_lut_bpc<C>(r, linear, dyn + where_static_lds<C>())};
        }
    }
    return WherePlan{kWhereChain, 2, 0, 0, r.l.max_blocks_per_cu > 0 ? r.l.max_blocks_per_cu : 0};
}

// one launch of a planned where-kernel: the dynamic-LDS limit, the grid, then the launch (the kernels read no flag bits)
template <auto Kernel> void launch_where_kernel(const WhereReq &r, const WherePlan &p, int bpc)
{
    constexpr uint64_t tile_values = 64 * (uint64_t)kWhereVpl;
    const uint64_t ntiles = (r.w.s.n + tile_values - 1) / tile_values;
    if (p.max_dyn > 0) allow_dynamic_lds<Kernel>(p.max_dyn, r.l.device);
    MI355_LAUNCH(r.l, 0, Kernel, dim3(grid_for(ntiles, bpc, r.l.num_cus)), dim3(kBlockThreads), p.dyn_lds, r.l.stream, r.w);
}

// launches what plan_where() decided.  The only place that names the where-kernels' templates.
template <int C> hipError_t launch_where(const WhereReq &r)
{
    constexpr int VPL = kWhereVpl;
    const WherePlan p = plan_where<C>(r);
    const bool linear = r.w.s.layout != 0;
    if (r.l.choice_out) *r.l.choice_out = p.choice; // introspection (mi355_shared_where_kernel): MI355_LAUNCH launches nothing
    if constexpr (C <= 16) {
        if (p.choice == kWhereLut) {
            with_aux<2, 18, 34>(p.aux, [&](auto aux) {
                constexpr int AUX = decltype(aux)::value;
                linear ? launch_where_kernel<shared_where_lut_kernel<C, AUX, VPL, 1, false>>(r, p, p.want_bpc)
                       : launch_where_kernel<shared_where_lut_kernel<C, AUX, VPL, 0, false>>(r, p, p.want_bpc);
            });
            return launch_status(r.l);
        }
        if constexpr (where_tables_fit<C>(9)) // (c = 16: two tables never fit, the multi-pass form is not instantiated)
        if (p.choice == kWhereLutMulti) {
            if (linear)
                launch_where_kernel<shared_where_lut_kernel<C, 2, VPL, 1, true>>(r, p, p.want_bpc);
            else
                with_aux<2, 18>(p.aux, [&](auto aux) { launch_where_kernel<shared_where_lut_kernel<C, decltype(aux)::value, VPL, 0, true>>(r, p, p.want_bpc); });
            return launch_status(r.l);
        }
    }
    if constexpr (C >= 11) { // (at c <= 10 every list fits the tables)
        static const int occ = blocks_per_cu(shared_where_chain_kernel<C, 2, VPL>);
        launch_where_kernel<shared_where_chain_kernel<C, 2, VPL>>(r, p, cap_bpc(occ, p.want_bpc));
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
