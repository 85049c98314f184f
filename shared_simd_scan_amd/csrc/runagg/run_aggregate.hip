// run_aggregate.hip -- implementation of include/mi355_run_aggregate.h: argument checks, the size of the waves' span tables and the
// two launches of a call, run_aggregate_init_kernel and run_aggregate_kernel (runagg/run_aggregate.hpp).  No workspace and nothing
// of the context's: capturable whatever its arguments.  Its own translation unit: neither the other entry points nor the width
// groups rebuild with it.  What it takes from the context is a LaunchEnv (ctx.hpp), as in groupby_wide/ and runs/.
#include "../ctx.hpp"

#include "../../../include/mi355_run_aggregate.h"
#include "../checks.hpp"
#include "../dispatch.hpp"
#include "../launch_util.hpp"
#include "run_aggregate.hpp"

using namespace mi355;

namespace {

// the most dynamic LDS any width asks for
constexpr uint32_t run_agg_max_lds()
{
    uint32_t most = 0;
    for (uint32_t cv = 1; cv <= 32; cv++) {
        const uint32_t b = run_agg_block_lds(cv, run_agg_span_slots(cv));
        most = b > most ? b : most;
    }
    return most;
}
static_assert(run_agg_max_lds() <= (uint32_t)kCuLdsBytes / (kRunAggResidentBlocks < 2 ? kRunAggResidentBlocks : 2u), "LDS budget: two blocks at every width");

// a table of `runs` entries of w bits, in the whole dwords the kernel reads
uint64_t table_bytes(uint64_t runs, unsigned w) { return ((runs * w + 31) / 32) * 4; }

// every entry to the empty result and the counter to 0: all an empty column takes, and what the aggregation starts from
void launch_init(const LaunchEnv &env, const RunAggArgs &k)
{
    const uint64_t blocks = (k.runs + 255u) / 256u;
    MI355_LAUNCH(env.record, 0, run_aggregate_init_kernel, dim3((unsigned)(blocks ? blocks : 1u)), dim3(256), 0, env.stream, k.out, k.runs, k.uncovered);
}

} // namespace

const char *mi355_run_aggregate_kernel(unsigned cv, unsigned ce)
{
    return cv >= 1 && cv <= 32 && ce >= 1 && ce <= 32 ? "run_aggregate_kernel" : nullptr;
}

uint32_t mi355_run_aggregate_span_slots(unsigned cv)
{
    if (cv < 1 || cv > 32) return 0;
    return run_agg_span_slots(cv);
}

int mi355_run_aggregate_dev(mi355_ctx *ctx, const void *values_dev, unsigned cv, uint64_t n, const void *mask_dev, const void *ends_dev, unsigned ce,
                            uint64_t runs, const uint64_t *runs_dev, uint64_t *out_dev, uint64_t *uncovered_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(cv, "cv"));
    MI355_CHECK(check_width(ce, "ce"));
    if (runs > 0xffffffffull) return fail(MI355_E_INVALID, "runs=%llu beyond 2^32 - 1", (unsigned long long)runs);
    if (runs) MI355_CHECK(check_ptr(out_dev, "out_dev"));
    MI355_CHECK(check_aligned(out_dev, 8, "out_dev"));
    MI355_CHECK(check_aligned(uncovered_dev, 8, "uncovered_dev"));
    MI355_CHECK(check_aligned(runs_dev, 8, "runs_dev"));
    MI355_CHECK(check_aligned(values_dev, 16, "values_dev"));
    MI355_CHECK(check_aligned(mask_dev, 4, "mask_dev"));
    MI355_CHECK(check_aligned(ends_dev, 4, "ends_dev"));
    if (n) {
        MI355_CHECK(check_ptr(values_dev, "values_dev"));
        if (runs) MI355_CHECK(check_ptr(ends_dev, "ends_dev"));
    }
    const uint64_t out_bytes = 32 * runs;
    if (n) {
        MI355_CHECK(check_no_overlap(out_dev, out_bytes, "out_dev", values_dev, packed_bytes(n, cv), "values_dev", "column"));
        if (mask_dev) MI355_CHECK(check_no_overlap(out_dev, out_bytes, "out_dev", mask_dev, bitmap_bytes(n), "mask_dev", "mask"));
        if (ends_dev) MI355_CHECK(check_no_overlap(out_dev, out_bytes, "out_dev", ends_dev, table_bytes(runs, ce), "ends_dev", "table of ends"));
    }
    if (runs_dev) MI355_CHECK(check_no_overlap(out_dev, out_bytes, "out_dev", runs_dev, sizeof(uint64_t), "runs_dev", "run count"));
    if (uncovered_dev) MI355_CHECK(check_no_overlap(out_dev, out_bytes, "out_dev", uncovered_dev, sizeof(uint64_t), "uncovered_dev", "other output"));
    RunAggArgs k{};
    k.values = (const uint8_t *)values_dev;
    k.n = n;
    k.mask = (const uint8_t *)mask_dev;
    k.ends = (const uint32_t *)ends_dev;
    k.runs_dev = (const unsigned long long *)runs_dev;
    k.runs = runs;
    k.out = (unsigned long long *)out_dev;
    k.uncovered = (unsigned long long *)uncovered_dev;
    k.cv = cv;
    k.ce = ce;
    k.slots = run_agg_span_slots(cv);
    const LaunchEnv env = launch_env(ctx);
    launch_init(env, k);
    // a wave per chunk of 8 tiles.  Blocks per CU: what registers and this width's LDS admit (table_bpc: the occupancy query is
    // asked once per device, the LDS share is arithmetic, so a capture never repeats the query)
    if (n) launch_tier<run_aggregate_kernel>(env, k, (rt_ntiles(n) + kRunsChunkTiles - 1) / kRunsChunkTiles, run_agg_block_lds(cv, k.slots), 0, (int)run_agg_max_lds());
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(MI355_E_HIP, "run_aggregate launch: %s", hipGetErrorString(err));
    return MI355_OK;
}
