// running_sum.hip -- mi355_running_sum_dev of include/mi355_running.h: argument checks, the range rule that chooses between
// running_sum_exact_kernel and running_sum_checked_kernel (running/running.hpp), and the three launches of a call --
// running_sum_totals_kernel, rowid_scan_kernel (kernels/bitmap.hpp, through launch_rowid_prefix<false> of launch_util.hpp) over the
// chunk totals, then the emitting kernel by output width.  The chunk prefix lives in the CALLER's workspace: the call takes nothing
// from the context, so it is capturable whatever its arguments.  Its own translation unit: neither the other entry points nor the
// width groups rebuild with it.
#include "../ctx.hpp"

#include "../../../include/mi355_running.h"
#include "../checks.hpp"
#include "../dispatch.hpp"
#include "../launch_util.hpp"
#include "running.hpp"

using namespace mi355;

namespace {

static_assert(kRunningInclusive == MI355_RUNNING_INCLUSIVE && kRunningExclusive == MI355_RUNNING_EXCLUSIVE, "the header's flags are the kernels'");

struct RunningLaunch {
    RunningArgs k;
    LaunchEnv env;
};

enum RunningPlan { kRunningRefused = 0, kRunningExact, kRunningChecked };

// The range rule: every partial sum of up to n terms lies in [k + n lo_t, k + n hi_t], in 128 bits.  `why` (nullable) gets the refusal.
RunningPlan running_plan(unsigned c, uint64_t n, int64_t b, int64_t k, unsigned co, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = nullptr;
    if (c < 1 || c > 32 || co < 1 || co > 32) *why = "a bit width (c, co) outside 1..32";
    else if (n >> 62) *why = "n beyond 2^62 rows";
    if (*why) return kRunningRefused;
    const __int128 top = (((__int128)1 << c) - 1) + b;
    const __int128 lo_t = b < 0 ? (__int128)b : 0, hi_t = top > 0 ? top : 0; // |.| < 2^64, n < 2^62: the products stay inside 128 bits
    const __int128 lo = (__int128)k + (__int128)n * lo_t, hi = (__int128)k + (__int128)n * hi_t;
    if (lo < (__int128)INT64_MIN || hi > (__int128)INT64_MAX) {
        *why = "the sums' range [k + n min(0, b), k + n max(0, 2^c - 1 + b)] leaves int64: 64-bit arithmetic would not be exact";
        return kRunningRefused;
    }
    return lo >= 0 && hi <= ((__int128)1 << co) - 1 ? kRunningExact : kRunningChecked;
}

// all of a block's LDS is dynamic, sized to the input width: the waves' two images of the column
template <int CO, bool CHECKED> hipError_t launch_running_sum(const RunningLaunch &r)
{
    const size_t lds = running_block_lds(r.k.c);
    const int max_dyn = (int)running_block_lds(32);
    if constexpr (CHECKED)
        launch_tier<running_sum_checked_kernel<CO>>(r.env, r.k, r.k.nchunks, lds, 0, max_dyn);
    else
        launch_tier<running_sum_exact_kernel<CO>>(r.env, r.k, r.k.nchunks, lds, 0, max_dyn);
    return hipGetLastError();
}

} // namespace

const char *mi355_running_sum_kernel(unsigned c, uint64_t n, int64_t b, int64_t k, unsigned co)
{
    switch (running_plan(c, n, b, k, co, nullptr)) {
    case kRunningExact: return "running_sum_exact_kernel";
    case kRunningChecked: return "running_sum_checked_kernel";
    default: return nullptr;
    }
}

uint64_t mi355_running_sum_workspace_words(uint64_t n)
{
    return rowid_plan(n).words; // the chunk prefix over n rows: a chunk of a bitmap of n rows is a chunk of the column
}

int mi355_running_sum_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const void *mask_dev, int64_t b, int64_t k, unsigned flags,
                          unsigned co, uint32_t miss, void *out_dev, uint64_t *result_dev, uint64_t *ws_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(c, "c"));
    MI355_CHECK(check_width(co, "co"));
    if (flags != MI355_RUNNING_INCLUSIVE && flags != MI355_RUNNING_EXCLUSIVE)
        return fail(MI355_E_INVALID, "flags=%u is neither MI355_RUNNING_INCLUSIVE nor MI355_RUNNING_EXCLUSIVE", flags);
    if (co < 32 && (miss >> co)) return fail(MI355_E_INVALID, "miss=%u is no value of co=%u bits", miss, co);
    const char *why = nullptr;
    const RunningPlan plan = running_plan(c, n, b, k, co, &why);
    if (plan == kRunningRefused) return fail(MI355_E_INVALID, "running_sum (b=%lld, k=%lld, c=%u, n=%llu): %s", (long long)b, (long long)k, c, (unsigned long long)n, why);
    MI355_CHECK(check_aligned(result_dev, 8, "result_dev"));
    MI355_CHECK(check_aligned(mask_dev, 4, "mask_dev"));
    const uint64_t out_bytes = packed_bytes(n, co), ws_bytes = mi355_running_sum_workspace_words(n) * sizeof(uint64_t);
    if (n) {
        MI355_CHECK(check_dev(packed_dev, 16, "packed_dev"));
        MI355_CHECK(check_dev(out_dev, 16, "out_dev"));
        MI355_CHECK(check_dev(ws_dev, 8, "ws_dev"));
        MI355_CHECK(check_no_overlap(out_dev, out_bytes, "out_dev", packed_dev, packed_bytes(n, c), "packed_dev", "column"));
        MI355_CHECK(check_no_overlap(out_dev, out_bytes, "out_dev", mask_dev, mask_dev ? bitmap_bytes(n) : 0, "mask_dev", "mask"));
        MI355_CHECK(check_no_overlap(out_dev, out_bytes, "out_dev", ws_dev, ws_bytes, "ws_dev", "workspace"));
    }
    if (n == 0) {
        // no kernel: word 0 is k, word 1 is 0 -- three memset nodes, so even this is capturable
        if (result_dev) {
            HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)result_dev, (int)(uint32_t)(uint64_t)k, 1, ctx->stream));
            HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)((uint32_t *)result_dev + 1), (int)(uint32_t)((uint64_t)k >> 32), 1, ctx->stream));
            HIP_TRY(hipMemsetAsync(result_dev + 1, 0, sizeof(uint64_t), ctx->stream));
        }
        return MI355_OK;
    }
    // the counter starts from 0 (all the exact kernel leaves in it); word 0 is stored by the wave that owns the last tile
    if (result_dev) HIP_TRY(hipMemsetAsync(result_dev, 0, 2 * sizeof(uint64_t), ctx->stream));
    const RowidPlan p = rowid_plan(n);
    RowidArgs g{};
    g.nchunks = p.nchunks;
    g.chunk_counts = (unsigned long long *)ws_dev;
    RunningLaunch r{};
    r.k.packed = (const uint8_t *)packed_dev;
    r.k.mask = (const uint8_t *)mask_dev;
    r.k.n = n;
    r.k.out = (uint8_t *)out_dev;
    r.k.chunk_totals = g.chunk_counts;
    r.k.nchunks = p.nchunks;
    r.k.result = (unsigned long long *)result_dev;
    r.k.b = b;
    r.k.k = k;
    r.k.c = c;
    r.k.miss = miss;
    r.k.exclusive = flags == MI355_RUNNING_EXCLUSIVE ? 1u : 0u;
    // plain stores unless option "scan_nt_stores" names a policy: a lane writes up to 128 contiguous bytes, and at the even wide widths the
    // non-temporal and write-through forms cost 2 - 6 x (profiles/r21_running_sum.txt), whatever the size of the result
    r.k.nts = ctx->scan_nt_stores < 0 ? 0u : (uint32_t)ctx->scan_nt_stores;
    r.env = launch_env(ctx);
    // 1: the chunks' totals; 2: their prefix, every word of which the emitting kernel reads is written here or by launch 1
    launch_tier<running_sum_totals_kernel>(r.env, r.k, p.nchunks, running_block_lds(c), 0, (int)running_block_lds(32));
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) {
        launch_rowid_prefix<false>(r.env, p, g);
        err = hipGetLastError();
    }
    if (err == hipSuccess) {
        if (plan == kRunningChecked)
            err = launch_by_width<1, 32>(co, r, [](auto w, const RunningLaunch &q) { return launch_running_sum<decltype(w)::value, true>(q); });
        else
            err = launch_by_width<1, 32>(co, r, [](auto w, const RunningLaunch &q) { return launch_running_sum<decltype(w)::value, false>(q); });
    }
    if (err != hipSuccess) return fail(MI355_E_HIP, "running_sum launch: %s", hipGetErrorString(err));
    return MI355_OK;
}
