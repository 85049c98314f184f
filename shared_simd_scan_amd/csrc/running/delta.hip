// delta.hip -- mi355_delta_dev of include/mi355_running.h: argument checks, the rule that chooses between delta_exact_kernel and
// delta_checked_kernel (running/running.hpp), and the one launch of a call by output width.  No workspace and nothing of the
// context's: capturable whatever its arguments.  Its own translation unit, beside running_sum.hip: the two sets of 64 kernels build
// side by side.
#include "../ctx.hpp"

#include "../../../include/mi355_running.h"
#include "../checks.hpp"
#include "../dispatch.hpp"
#include "../launch_util.hpp"
#include "running.hpp"

using namespace mi355;

namespace {

struct DeltaLaunch {
    DeltaArgs k;
    LaunchEnv env;
};

enum DeltaPlan { kDeltaRefused = 0, kDeltaExact, kDeltaChecked };

// x_i - x_{i-1} + k spans [k - (2^c - 1), k + 2^c - 1] over all rows: exact when that lies within [0, 2^co - 1]
DeltaPlan delta_plan(unsigned c, int64_t k, unsigned co)
{
    if (c < 1 || c > 32 || co < 1 || co > 32) return kDeltaRefused;
    const __int128 X = ((__int128)1 << c) - 1;
    return (__int128)k - X >= 0 && (__int128)k + X <= ((__int128)1 << co) - 1 ? kDeltaExact : kDeltaChecked;
}

template <int CO, bool CHECKED> hipError_t launch_delta(const DeltaLaunch &r)
{
    const uint64_t ntiles = rt_ntiles(r.k.n);
    const size_t lds = running_block_lds(r.k.c);
    const int max_dyn = (int)running_block_lds(32);
    if constexpr (CHECKED)
        launch_tier<delta_checked_kernel<CO>>(r.env, r.k, ntiles, lds, 0, max_dyn);
    else
        launch_tier<delta_exact_kernel<CO>>(r.env, r.k, ntiles, lds, 0, max_dyn);
    return hipGetLastError();
}

} // namespace

const char *mi355_delta_kernel(unsigned c, int64_t k, unsigned co)
{
    switch (delta_plan(c, k, co)) {
    case kDeltaExact: return "delta_exact_kernel";
    case kDeltaChecked: return "delta_checked_kernel";
    default: return nullptr;
    }
}

int mi355_delta_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, uint32_t first, int64_t k, unsigned co, uint32_t miss, void *out_dev,
                    uint64_t *out_of_range_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(c, "c"));
    MI355_CHECK(check_width(co, "co"));
    if (c < 32 && (first >> c)) return fail(MI355_E_INVALID, "first=%u is no value of c=%u bits", first, c);
    if (co < 32 && (miss >> co)) return fail(MI355_E_INVALID, "miss=%u is no value of co=%u bits", miss, co);
    const DeltaPlan plan = delta_plan(c, k, co);
    MI355_CHECK(check_aligned(out_of_range_dev, 8, "out_of_range_dev"));
    const uint64_t out_bytes = packed_bytes(n, co);
    if (n) {
        MI355_CHECK(check_dev(packed_dev, 16, "packed_dev"));
        MI355_CHECK(check_dev(out_dev, 16, "out_dev"));
        MI355_CHECK(check_no_overlap(out_dev, out_bytes, "out_dev", packed_dev, packed_bytes(n, c), "packed_dev", "column"));
    }
    // the counter starts from 0: all the exact kernel and an empty column leave in it
    if (out_of_range_dev) HIP_TRY(hipMemsetAsync(out_of_range_dev, 0, sizeof(uint64_t), ctx->stream));
    if (n == 0) return MI355_OK;
    DeltaLaunch r{};
    r.k.packed = (const uint8_t *)packed_dev;
    r.k.n = n;
    r.k.out = (uint8_t *)out_dev;
    r.k.out_of_range = (unsigned long long *)out_of_range_dev;
    r.k.k = k;
    r.k.c = c;
    r.k.first = first;
    r.k.miss = miss;
    // plain stores unless option "scan_nt_stores" names a policy: a lane writes up to 128 contiguous bytes, and at the even wide widths the
    // non-temporal and write-through forms cost 2 - 6 x (profiles/r21_running_sum.txt), whatever the size of the result
    r.k.nts = ctx->scan_nt_stores < 0 ? 0u : (uint32_t)ctx->scan_nt_stores;
    r.env = launch_env(ctx);
    hipError_t err;
    if (plan == kDeltaChecked)
        err = launch_by_width<1, 32>(co, r, [](auto w, const DeltaLaunch &q) { return launch_delta<decltype(w)::value, true>(q); });
    else
        err = launch_by_width<1, 32>(co, r, [](auto w, const DeltaLaunch &q) { return launch_delta<decltype(w)::value, false>(q); });
    if (err != hipSuccess) return fail(MI355_E_HIP, "delta launch: %s", hipGetErrorString(err));
    return MI355_OK;
}
