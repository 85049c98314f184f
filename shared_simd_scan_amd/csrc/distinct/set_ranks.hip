// set_ranks.hip -- the mi355_set_ranks_dev half of include/mi355_distinct.h: argument checks, the selection workspace, and the
// three launches of a call -- rowid_count_kernel and rowid_scan_kernel (kernels/bitmap.hpp, through launch_rowid_prefix of
// launch_util.hpp) over the set, then set_ranks_kernel<CT> (distinct/set_ranks.hpp) by the table's width.  Its own translation
// unit: neither the other entry points nor the width groups rebuild with it.
#include "../ctx.hpp"

#include "../../../include/mi355_distinct.h"
#include "../checks.hpp"
#include "../dispatch.hpp"
#include "../launch_util.hpp"
#include "set_ranks.hpp"

using namespace mi355;

namespace {

struct SetRanksLaunch {
    SetRanksArgs k;
    RowidPlan plan;
    LaunchEnv env;
};

template <int CT> hipError_t launch_set_ranks(const SetRanksLaunch &r)
{
    MI355_LAUNCH(r.env.record, 0, set_ranks_kernel<CT>, dim3(rowid_chunk_grid(r.plan, r.env.num_cus)), dim3(kBlockThreads), 0, r.env.stream, r.k);
    return hipGetLastError();
}

} // namespace

int mi355_set_ranks_dev(mi355_ctx *ctx, const void *set_dev, uint64_t set_bits, unsigned ct, uint32_t miss, void *table_dev, uint64_t *out_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(ct, "ct"));
    if (ct < 32 && miss >> ct) return fail(MI355_E_INVALID, "miss=%u is no value of ct=%u bits", miss, ct);
    if (set_bits > (1ull << 32)) return fail(MI355_E_INVALID, "set_bits=%llu beyond 2^32", (unsigned long long)set_bits);
    MI355_CHECK(check_dev(out_dev, 8, "out_dev"));
    MI355_CHECK(check_aligned(set_dev, 4, "set_dev"));
    MI355_CHECK(check_aligned(table_dev, 16, "table_dev"));
    const uint64_t set_bytes = (set_bits + 7) / 8, table_bytes = packed_bytes(set_bits, ct);
    if (set_bits) {
        MI355_CHECK(check_ptr(set_dev, "set_dev"));
        MI355_CHECK(check_ptr(table_dev, "table_dev"));
        MI355_CHECK(check_no_overlap(table_dev, table_bytes, "table_dev", set_dev, set_bytes, "set_dev", "set"));
        if (ranges_overlap(out_dev, 2 * sizeof(uint64_t), table_dev, table_bytes)) return fail(MI355_E_INVALID, "out_dev overlaps table_dev");
        if (ranges_overlap(out_dev, 2 * sizeof(uint64_t), set_dev, set_bytes)) return fail(MI355_E_INVALID, "out_dev overlaps set_dev");
    }
    SetRanksLaunch r{};
    if (set_bits) { // the chunk prefix over the set (launch_util.hpp rowid_plan): refused under capture when it would have to grow
        r.plan = rowid_plan(set_bits);
        MI355_CHECK(rowid_ws_get(ctx, r.plan.words, "mi355_set_ranks_dev"));
    }
    HIP_TRY(hipMemsetAsync(out_dev, 0, 2 * sizeof(uint64_t), ctx->stream));
    if (set_bits == 0) return MI355_OK;
    RowidArgs g{};
    g.bitmap = (const uint8_t *)set_dev;
    g.nbytes = r.plan.nbytes;
    g.nchunks = r.plan.nchunks;
    g.chunk_counts = ctx->rowid_ws;
    r.k.set = g.bitmap;
    r.k.set_bits = set_bits;
    r.k.nbytes = g.nbytes;
    r.k.chunk_counts = g.chunk_counts;
    r.k.nchunks = g.nchunks;
    r.k.table = (uint8_t *)table_dev;
    r.k.out = (unsigned long long *)out_dev;
    r.k.miss = miss;
    r.k.nts = (uint32_t)one_pass_store_policy(table_bytes, ctx->scan_nt_stores);
    r.env = launch_env(ctx);
    launch_rowid_prefix<true>(r.env, r.plan, g);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = launch_by_width<1, 32>(ct, r, [](auto w, const SetRanksLaunch &q) { return launch_set_ranks<decltype(w)::value>(q); });
    if (err != hipSuccess) return fail(MI355_E_HIP, "set_ranks launch: %s", hipGetErrorString(err));
    return MI355_OK;
}
