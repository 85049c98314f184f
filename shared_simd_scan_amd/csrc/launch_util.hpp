// launch_util.hpp -- the host-side launch helpers that the translation units with a launcher share, one copy of each: capi.hip,
// extras.hip, the three group units (width_group.hip, predicates/where_group.hip, predicates/columns_group.hip) and the feature
// units (groupby/group_aggregate.hip, groupby_wide/group_aggregate_wide.hip, semijoin/semijoin.hip, lookup/lookup.hip, compact/compact.hip,
// arith/arith_kernels.hip, topk/top_k.hip, sort/sort_rows.hip; arith/arith.hip for the store policy).  No device code: kernels are only
// launched from here (launch_tier, launch_rowid_prefix).  What needs HIP or a kernel lives here; the pure rules -- grid_for, cap_bpc,
// scan_want_bpc, the store policies, the plans of the group units -- are in scan_plan.hpp, which dispatch.hpp includes.
#pragma once

#include <atomic>
#include <type_traits>

#include "dispatch.hpp"
#include "scan_plan.hpp"

namespace mi355 {

template <typename K> int blocks_per_cu(K kernel)
{
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, kBlockThreads, 0) != hipSuccess || nb < 1) nb = 1;
    return nb;
}

// Kernels that take their lookup tables as dynamic LDS may need more than the default 64 KiB: raise the limit once
// per kernel AND device (the attribute is per device; a process may hold contexts on several GPUs).
template <auto Kernel> void allow_dynamic_lds(int max_bytes, int device)
{
    static std::atomic<unsigned long long> done{0};
    const unsigned long long bit = 1ull << (device & 63);
    if (!(done.load(std::memory_order_acquire) & bit)) {
        (void)hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, max_bytes);
        done.fetch_or(bit, std::memory_order_release);
    }
}

// Blocks per CU of a kernel with `lds` bytes of dynamic LDS: what registers and LDS admit, at most four (one LDS or L2 lookup per
// value: further waves per SIMD hide the lookups' latency; the rule of group_aggregate.hip).  Shared by the kernels that size a
// lookup table in dynamic LDS to their arguments: the semi-join (its set) and lookup (its table).  The occupancy query is asked once
// per kernel and device, without dynamic LDS: that is the registers' and the static LDS's limit.  The table's share is arithmetic
// on top -- blocks of `fixed_lds` + `lds` bytes in a CU's 160 KiB -- so a caller that alternates between table sizes, or captures a
// graph, never repeats the query.  (An answer one too high would only leave a block of the persistent grid queued.)
template <auto Kernel> int table_bpc(size_t lds, size_t fixed_lds, int device)
{
    static std::atomic<signed char> by_regs[64]; // 0 = not asked on this device yet
    std::atomic<signed char> &slot = by_regs[device & 63];
    int bpc = slot.load(std::memory_order_relaxed);
    if (bpc == 0) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, Kernel, kBlockThreads, 0) != hipSuccess || bpc < 1) bpc = 1;
        if (bpc > 4) bpc = 4;
        slot.store((signed char)bpc, std::memory_order_relaxed);
    }
    const int by_lds = (int)(kCuLdsBytes / (fixed_lds + lds));
    return by_lds < 1 ? 1 : (by_lds < bpc ? by_lds : bpc);
}

// Blocks per CU of a kernel that counts into LDS next to its block's tiles (histogram_kernel, topk_hist_kernel): two while the tiles
// (`tile_lds` bytes per wave) and the `counter_bytes` of two blocks fit in the CU's LDS -- the LDS atomics want the second wave per SIMD
constexpr int counters_bpc(size_t tile_lds, size_t counter_bytes)
{
    return 2 * (kWavesPerBlock * tile_lds + counter_bytes) + 1024 <= (size_t)kCuLdsBytes ? 2 : 1;
}

// One tier of a kernel with a table in LDS, launched on a persistent grid over `ntiles` wave tiles: `lds` bytes of dynamic LDS next
// to `fixed_lds` of static, blocks per CU by table_bpc.  max_dyn > 0: the most dynamic LDS the kernel is ever given (raised once).
// Env: LaunchEnv (ctx.hpp, which the group units do not see).
template <auto Kernel, typename Env, typename Args>
void launch_tier(const Env &env, const Args &k, uint64_t ntiles, size_t lds, size_t fixed_lds, int max_dyn)
{
    if (max_dyn > 0) allow_dynamic_lds<Kernel>(max_dyn, env.device);
    const unsigned grid = grid_for(ntiles, cap_bpc(table_bpc<Kernel>(lds, fixed_lds, env.device), env.max_blocks_per_cu), env.num_cus);
    MI355_LAUNCH(env.record, 0, Kernel, dim3(grid), dim3(kBlockThreads), lds, env.stream, k);
}

// ---- the chunk prefix over a bitmap of n rows (kernels/bitmap.hpp): the prefix part of the selection workspace, its launches ----
struct RowidPlan {
    uint64_t nbytes, nchunks, ngroups; // the bitmap's bytes, its chunks of kRowidChunk bytes, their scan groups
    uint64_t words;                    // chunk counts, the total's slot, one total per scan group
};
inline RowidPlan rowid_plan(uint64_t n)
{
    RowidPlan p;
    p.nbytes = (n + 7) / 8;
    p.nchunks = (p.nbytes + kRowidChunk - 1) / kRowidChunk;
    p.ngroups = rowid_scan_groups(p.nchunks);
    p.words = rowid_prefix_words(p.nchunks);
    return p;
}
// the grid of a kernel that deals a wave per chunk: eight blocks per CU at the most
inline unsigned rowid_chunk_grid(const RowidPlan &p, int num_cus) { return grid_for(p.nchunks, 8, num_cus); }
// rowid_scan_kernel over g's chunk counts; COUNT: rowid_count_kernel in front of it, which fills them from g's bitmap.
// Env: LaunchEnv.
template <bool COUNT, typename Env> void launch_rowid_prefix(const Env &env, const RowidPlan &p, const RowidArgs &g)
{
    if constexpr (COUNT) MI355_LAUNCH(env.record, 0, rowid_count_kernel, dim3(rowid_chunk_grid(p, env.num_cus)), dim3(256), 0, env.stream, g);
    MI355_LAUNCH(env.record, 0, rowid_scan_kernel, dim3((unsigned)p.ngroups), dim3(256), 0, env.stream, g);
}

// ---- compile-time fan-out ------------------------------------------------------------------------------------------------

// The width ladder of a group translation unit: f(std::integral_constant<int, C>{}, r) for the C in LO .. HI that c names.
template <int LO, int HI, typename Req, typename F> hipError_t launch_by_width(unsigned c, const Req &r, F f)
{
    if (c == (unsigned)LO) return f(std::integral_constant<int, LO>{}, r);
    if constexpr (LO < HI)
        return launch_by_width<LO + 1, HI>(c, r, f);
    else
        return hipErrorInvalidValue;
}

// launch_group_3, launch_where_group_3, ...: MI355_CAT(launch_group_, MI355_GROUP)
#define MI355_CAT2(a, b) a##b
#define MI355_CAT(a, b) MI355_CAT2(a, b)

// A run-time (rc, big) pair as template arguments: f(std::integral_constant<int, rc>{}, std::bool_constant<big>{}).
// Only what a kernel can use is instantiated: rc counts as 0 unless kMaxRc is 2, and BIG = true exists at kBigWidth widths only.
template <int kMaxRc, bool kBigWidth, typename F> void with_rc_big(int rc, bool big, F f)
{
    auto with_big = [&](auto rc_c) {
        if constexpr (kBigWidth) {
            if (big) return f(rc_c, std::true_type{});
        }
        f(rc_c, std::false_type{});
    };
    if constexpr (kMaxRc >= 2) {
        if (rc == 1) return with_big(std::integral_constant<int, 1>{});
        if (rc == 2) return with_big(std::integral_constant<int, 2>{});
    }
    with_big(std::integral_constant<int, 0>{});
}

// A planned AUX word (scan_plan.hpp) as a template argument: f(std::integral_constant<int, aux>{}) for the one of kAux, kMore... that
// `aux` names -- the forms a kernel is instantiated in, and no other; the plans give nothing else (the last stands for "none of the others")
template <int kAux, int... kMore, typename F> void with_aux(int aux, F f)
{
    if constexpr (sizeof...(kMore) > 0) {
        if (aux != kAux) return with_aux<kMore...>(aux, f);
    }
    f(std::integral_constant<int, kAux>{});
}

// what a launcher returns: in a dry run (LaunchReq::choice_out) nothing was launched, so nothing can have failed
inline hipError_t launch_status(const LaunchReq &r) { return r.choice_out ? hipSuccess : hipGetLastError(); }

} // namespace mi355
