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

// ---- the plain ops: launch what scan_plan.hpp planned.  Each occupancy query is asked once per kernel form and process, on the
// form named next to it; the plan's AUX becomes the template argument (with_aux), so every kernel has one launch line. ----------

template <typename G> constexpr PlanTile plan_tile() { return PlanTile{G::TILE_VALUES, G::TILE_BYTES}; }

template <int C, int MODE> void launch_scan(const LaunchReq &r)
{
    constexpr int VPL = scan_vpl(C, MODE);
    auto go = [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        static const int occ = blocks_per_cu(scan_burst_kernel<C, MODE, 34, VPL, K>);
        const ScanPlan p = plan_scan(plan_req(r), plan_tile<ScanGeom<C, VPL>>(), C, r.scan.n, r.scan.out != nullptr, r.scan.and_mask != nullptr, K, occ);
        ScanArgs a = r.scan;
        llc_set(a, p.llc_d);
        if (r.llc_d_out) *r.llc_d_out = (int)a.llc_d;
        with_aux<0, 2, 18, 34>(p.aux, [&](auto aux) {
            MI355_LAUNCH(r, a.flags, (scan_burst_kernel<C, MODE, decltype(aux)::value, VPL, K>), dim3(p.grid), dim3(p.block), 0, r.stream, a);
        });
    };
    burst_k(C, r.scan_burst) > 1 ? go(std::integral_constant<int, burst_k(C)>{}) : go(std::integral_constant<int, 1>{});
}

template <int C> void launch_in(const LaunchReq &r)
{
    constexpr int VPL = scan_vpl(C, kModeEq);
    static const int occ = blocks_per_cu(in_kernel<C, 2, VPL>);
    const ScanPlan p = plan_in(plan_req(r), plan_tile<ScanGeom<C, VPL>>(), r.scan.n, occ);
    with_aux<2, 18, 34>(p.aux, [&](auto aux) {
        MI355_LAUNCH(r, r.scan.flags, (in_kernel<C, decltype(aux)::value, VPL>), dim3(p.grid), dim3(p.block), 0, r.stream, r.scan);
    });
}

template <int C> void launch_select(const LaunchReq &r)
{
    constexpr int VPL = scan_vpl(C, kModeRange);
    const ScanPlan p = plan_select(plan_req(r), plan_tile<ScanGeom<C, VPL>>(), r.scan.n, select_tiles(C), kSel2Waves);
    if (r.select_single)
        MI355_LAUNCH(r, r.scan.flags, (select_kernel<C, kModeRange, VPL>), dim3(p.grid), dim3(p.block), 0, r.stream, r.scan);
    else
        MI355_LAUNCH(r, r.scan.flags, (select2_kernel<C, kModeRange, VPL>), dim3(p.grid), dim3(p.block), 0, r.stream, r.scan);
}

template <int C> void launch_scan2(const LaunchReq &r)
{
    constexpr int VPL = scan_vpl(C, kModeRange);
    static const int occ = blocks_per_cu(scan2_kernel<C, 34, VPL>);
    const ScanPlan p = plan_scan2(plan_req(r), plan_tile<ScanGeom<C, VPL>>(), r.scan.n, occ);
    with_aux<18, 34>(p.aux, [&](auto aux) {
        MI355_LAUNCH(r, r.scan.flags, (scan2_kernel<C, decltype(aux)::value, VPL>), dim3(p.grid), dim3(p.block), 0, r.stream, r.scan);
    });
}

template <int C> void launch_decompress(const LaunchReq &r)
{
    static const int occ = blocks_per_cu(decompress_kernel<C, 18>);
    const ScanPlan p = plan_decompress(plan_req(r), plan_tile<DecompGeom<C>>(), r.decomp.n, occ);
    with_aux<0, 2, 34, 18>(p.aux, [&](auto aux) {
        MI355_LAUNCH(r, 0, (decompress_kernel<C, decltype(aux)::value>), dim3(p.grid), dim3(p.block), 0, r.stream, r.decomp);
    });
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
    case kOpScanIn: launch_in<C>(r); break;
    case kOpSelect: launch_select<C>(r); break;
    case kOpScan2: launch_scan2<C>(r); break;
    case kOpDecompress: launch_decompress<C>(r); break;
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
