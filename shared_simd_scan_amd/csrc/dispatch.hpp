// dispatch.hpp -- host-side launch request shared by capi.hip and the width-group translation units.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <cstdlib>
#include <cxxabi.h>
#include <string>
#include <type_traits>
#include <typeinfo>

#include "kernels.hpp"
#include "scan_plan.hpp"

namespace mi355 {

// ---- launch record (mi355_ctx_last_launch): one line per kernel a call launched, in launch order,
//   "<name><<template args>> grid=<blocks> lds=<dynamic LDS bytes> flags=0x<ScanArgs::flags>"
// Host-side text only: no device work, no synchronisation.  The caller holds the context's lock.

// "shared_wide3_kernel<17, 2, 2, true>" out of the demangled type std::integral_constant<void (*)(mi355::ScanArgs),
// &(void mi355::shared_wide3_kernel<17, 2, 2, true>(mi355::ScanArgs))> (a plain kernel: "..., &mi355::sum_slots_kernel>")
inline std::string kernel_label_from(const char *demangled)
{
    std::string s = demangled ? demangled : "";
    const size_t at = s.find(", &");
    if (at == std::string::npos) return s;
    std::string t = s.substr(at + 3, s.size() - at - 4); // without the closing '>' of integral_constant
    if (!t.empty() && t[0] == '(') t = t.substr(1, t.size() - 2);
    if (t.compare(0, 5, "void ") == 0) t = t.substr(5);
    int depth = 0;
    for (size_t i = 0; i < t.size(); i++) { // the parameter list starts at the first '(' outside the template arguments
        if (t[i] == '<') depth++;
        else if (t[i] == '>') depth--;
        else if (t[i] == '(' && depth == 0) {
            t.resize(i);
            break;
        }
    }
    for (size_t q; (q = t.find("mi355::")) != std::string::npos;) t.erase(q, 7);
    return t;
}

template <auto Kernel> const std::string &kernel_label()
{
    static const std::string label = [] {
        int status = 0;
        char *d = abi::__cxa_demangle(typeid(std::integral_constant<decltype(Kernel), Kernel>).name(), nullptr, nullptr, &status);
        std::string s = kernel_label_from(d);
        std::free(d);
        return s;
    }();
    return label;
}

inline void note_launch(std::string *rec, const std::string &label, const dim3 &grid, size_t lds, uint32_t flags)
{
    if (!rec) return;
    char tail[96];
    snprintf(tail, sizeof tail, " grid=%u lds=%zu flags=0x%x\n", grid.x * grid.y * grid.z, lds, flags);
    *rec += label;
    *rec += tail;
}

// hipLaunchKernelGGL + the launch record.  FLAGS: the ScanArgs::flags word the kernel receives (0 for kernels without one).
// REQ: a LaunchReq -- recorded in its `record`; with `choice_out` set (a dry run) NOTHING is launched -- or, for the
// launchers that have no request, the record itself (std::string *, may be null).
#define MI355_LAUNCH(REQ, FLAGS, KERNEL, GRID, BLOCK, LDS, STREAM, ...)                                                      \
    do {                                                                                                                   \
        ::mi355::note_launch(::mi355::record_of(REQ), ::mi355::kernel_label<KERNEL>(), dim3(GRID), (size_t)(LDS), (uint32_t)(FLAGS)); \
        if (!::mi355::dry_run(REQ)) hipLaunchKernelGGL(KERNEL, GRID, BLOCK, LDS, STREAM, __VA_ARGS__);                     \
    } while (0)

enum Op { kOpScanEq = 0, kOpScanRange = 1, kOpSharedScan = 2, kOpDecompress = 3, kOpScanIn = 4, kOpSelect = 5, kOpScan2 = 6 };

struct LaunchReq {
    int op;
    unsigned c;
    hipStream_t stream;
    int device;            // the context's device (per-device kernel attributes)
    int num_cus;
    int max_blocks_per_cu; // 0 = what the occupancy query allows
    int dma_aux;           // cache policy of the HBM->LDS loads: 0 default, 2 nt
    int scan_nt_stores;    // bitmap stores of the eq / range scan: -1 by size, 0 plain, 1 non-temporal
    int scan_burst;        // eq / range scan: 0 = tiles per store burst chosen by width (burst_k), 1 = one tile per burst
    int llc_resident_mib;  // eq / range scan: Infinity Cache budget of the column's resident part, -1 auto, 0 off (scan_plan.hpp llc_divisor)
    int llc_repeat;        // eq / range scan: the context's previous call was a scan of the same column into the same bitmap (auto acts on repeats only)
    int *llc_d_out;        // eq / range scan: non-null = where the launcher reports the divisor it chose (mi355_ctx_last_llc_divisor)
    int select_single;     // kOpSelect: 1 = the older single-role kernel (option "select_kernel" = 1, A/B), 0 = decoder / expander roles
    int shared_vpl;        // shared scans of <= 8 keys: values per lane and tile, 0 = the engine's choice, 64, 128 (c <= 12)
    std::string *record;   // the context's launch record (mi355_ctx_last_launch), null = not recorded
    int *choice_out;       // introspection, the same in every group (width, where, columns): non-null = a dry run.  Nothing is
                           // launched (MI355_LAUNCH sees to it); the kernel family goes to *choice_out -- shared scans: a
                           // SharedFamily (shared_plan.hpp: one-pass LUT, byte-entry multi-pass LUT, 32 keys per lookup, compare
                           // chain, linear rows, pair), where-scans: a WhereChoice, every other op has one family and reports
                           // none -- and `record`, if set, gets the line the launch would have written
    ScanArgs scan;
    DecompArgs decomp;
};

inline std::string *record_of(std::string *rec) { return rec; }
inline std::string *record_of(const LaunchReq &r) { return r.record; }
inline bool dry_run(std::string *) { return false; }
inline bool dry_run(const LaunchReq &r) { return r.choice_out != nullptr; }

// the rules (scan_plan.hpp: grid_for, the store policies, the plans) read these fields
static_assert(kPlanWavesPerBlock == kWavesPerBlock, "scan_plan.hpp repeats kWavesPerBlock");
inline PlanReq plan_req(const LaunchReq &r)
{
    return PlanReq{r.num_cus, r.max_blocks_per_cu, r.dma_aux, r.scan_nt_stores, r.scan_burst, r.llc_resident_mib, r.llc_repeat, r.select_single};
}

constexpr int kNumGroups = 8; // widths 1..32, 4 per group
// the eight group launchers of a family of translation units (STEM##0 .. STEM##7): their declarations, and their table
#define MI355_DECLARE_GROUPS(STEM, REQ)                                                                                     \
    hipError_t STEM##0(const REQ &), STEM##1(const REQ &), STEM##2(const REQ &), STEM##3(const REQ &), STEM##4(const REQ &), \
        STEM##5(const REQ &), STEM##6(const REQ &), STEM##7(const REQ &)
#define MI355_GROUP_TABLE(STEM) {STEM##0, STEM##1, STEM##2, STEM##3, STEM##4, STEM##5, STEM##6, STEM##7}
MI355_DECLARE_GROUPS(launch_group_, LaunchReq);

} // namespace mi355
