// run_decode.hip -- mi355_run_decode_dev of include/mi355_runs.h: argument checks and the one launch of a call,
// run_decode_kernel<CV> (runs/runs.hpp) by the values' width.  No workspace, no LDS and nothing of the context's: capturable
// whatever its arguments.  Its own translation unit, beside run_encode.hip: the two sets of 32 kernels build side by side.
#include "../ctx.hpp"

#include "../../../include/mi355_runs.h"
#include "../checks.hpp"
#include "../dispatch.hpp"
#include "../launch_util.hpp"
#include "runs.hpp"

using namespace mi355;

namespace {

struct RunDecodeLaunch {
    RunDecodeArgs k;
    LaunchEnv env;
};

// Blocks per CU: what the registers admit, at most eight.  The kernel holds no LDS and waits on dependent table reads (the tile
// search), which further waves per SIMD hide.  Asked once per width and device, so a captured call never repeats the query.
template <int CV> int run_decode_bpc(int device)
{
    static std::atomic<signed char> asked[64]; // 0 = not asked on this device yet
    std::atomic<signed char> &slot = asked[device & 63];
    int bpc = slot.load(std::memory_order_relaxed);
    if (bpc == 0) {
        bpc = blocks_per_cu(run_decode_kernel<CV>);
        if (bpc > 8) bpc = 8;
        slot.store((signed char)bpc, std::memory_order_relaxed);
    }
    return bpc;
}

template <int CV> hipError_t launch_run_decode(const RunDecodeLaunch &r)
{
    const unsigned grid = grid_for(rt_ntiles(r.k.n), cap_bpc(run_decode_bpc<CV>(r.env.device), r.env.max_blocks_per_cu), r.env.num_cus);
    MI355_LAUNCH(r.env.record, 0, run_decode_kernel<CV>, dim3(grid), dim3(kBlockThreads), 0, r.env.stream, r.k);
    return hipGetLastError();
}

// a table of `runs` entries of w bits, in the whole dwords the kernel reads
uint64_t table_bytes(uint64_t runs, unsigned w) { return ((runs * w + 31) / 32) * 4; }

} // namespace

const char *mi355_run_decode_kernel(unsigned cv, unsigned ce)
{
    return cv >= 1 && cv <= 32 && ce >= 1 && ce <= 32 ? "run_decode_kernel" : nullptr;
}

int mi355_run_decode_dev(mi355_ctx *ctx, const void *values_dev, unsigned cv, const void *ends_dev, unsigned ce, uint64_t runs, const uint64_t *runs_dev,
                         uint64_t n, uint32_t miss, void *out_dev, uint64_t *uncovered_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(cv, "cv"));
    MI355_CHECK(check_width(ce, "ce"));
    if (cv < 32 && (miss >> cv)) return fail(MI355_E_INVALID, "miss=%u is no value of cv=%u bits", miss, cv);
    if (runs > 0xffffffffull) return fail(MI355_E_INVALID, "runs=%llu beyond 2^32 - 1", (unsigned long long)runs);
    MI355_CHECK(check_aligned(runs_dev, 8, "runs_dev"));
    MI355_CHECK(check_aligned(uncovered_dev, 8, "uncovered_dev"));
    MI355_CHECK(check_aligned(values_dev, 4, "values_dev"));
    MI355_CHECK(check_aligned(ends_dev, 4, "ends_dev"));
    if (n) {
        MI355_CHECK(check_dev(out_dev, 16, "out_dev"));
        if (runs) {
            MI355_CHECK(check_ptr(values_dev, "values_dev"));
            MI355_CHECK(check_ptr(ends_dev, "ends_dev"));
            const uint64_t out_bytes = packed_bytes(n, cv);
            MI355_CHECK(check_no_overlap(out_dev, out_bytes, "out_dev", values_dev, table_bytes(runs, cv), "values_dev", "table of values"));
            MI355_CHECK(check_no_overlap(out_dev, out_bytes, "out_dev", ends_dev, table_bytes(runs, ce), "ends_dev", "table of ends"));
        }
    }
    // the counter starts from 0: all an empty column leaves in it
    if (uncovered_dev) HIP_TRY(hipMemsetAsync(uncovered_dev, 0, sizeof(uint64_t), ctx->stream));
    if (n == 0) return MI355_OK;
    RunDecodeLaunch r{};
    r.k.values = (const uint32_t *)values_dev;
    r.k.ends = (const uint32_t *)ends_dev;
    r.k.runs_dev = (const unsigned long long *)runs_dev;
    r.k.runs = runs;
    r.k.n = n;
    r.k.out = (uint8_t *)out_dev;
    r.k.uncovered = (unsigned long long *)uncovered_dev;
    r.k.ce = ce;
    r.k.miss = miss;
    // plain stores unless option "scan_nt_stores" names a policy: running_sum's finding (profiles/r21_running_sum.txt)
    r.k.nts = ctx->scan_nt_stores < 0 ? 0u : (uint32_t)ctx->scan_nt_stores;
    r.env = launch_env(ctx);
    const hipError_t err = launch_by_width<1, 32>(cv, r, [](auto w, const RunDecodeLaunch &q) { return launch_run_decode<decltype(w)::value>(q); });
    if (err != hipSuccess) return fail(MI355_E_HIP, "run_decode launch: %s", hipGetErrorString(err));
    return MI355_OK;
}
