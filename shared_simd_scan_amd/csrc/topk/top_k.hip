// top_k.hip -- implementation of include/mi355_topk.h: argument checks, the selection workspace, and the launches of a call --
// per digit topk_hist_kernel<C> and topk_pick_kernel, then topk_emit_kernel<C>, rowid_scan_kernel (kernels/bitmap.hpp, through
// launch_rowid_prefix of launch_util.hpp) and topk_trim_kernel<C> (topk/top_k.hpp).  Its own translation unit: neither the other
// entry points nor the width groups rebuild with it.  The grids come from a LaunchEnv (ctx.hpp), as in semijoin/, lookup/ and compact/.
#include "../ctx.hpp"

#include "../../../include/mi355_topk.h"
#include "../checks.hpp"
#include "../dispatch.hpp"
#include "../launch_util.hpp"
#include "top_k.hpp"

using namespace mi355;

namespace {

struct TopkLaunch {
    TopkArgs k;
    TopkPickArgs pick;
    RowidArgs scan;
    RowidPlan plan;
    LaunchEnv env;
    unsigned passes;
};

template <int C> hipError_t launch_top_k(const TopkLaunch &r)
{
    constexpr int VPL = topk_vpl<C>();
    using G = ScanGeom<C, VPL>;
    std::string *const rec = r.env.record;
    const uint64_t ntiles = (r.k.n + G::TILE_VALUES - 1) / G::TILE_VALUES;
    const unsigned hist_grid = grid_for(ntiles, cap_bpc(counters_bpc(G::LDS_BYTES, 4u * kTopkBuckets), r.env.max_blocks_per_cu), r.env.num_cus);
    const unsigned emit_grid = grid_for(ntiles, scan_want_bpc(G::TILE_BYTES, r.env.max_blocks_per_cu), r.env.num_cus);
    const unsigned trim_grid = grid_for(r.k.nchunks, cap_bpc(2, r.env.max_blocks_per_cu), r.env.num_cus);
    const uint32_t vmask = C == 32 ? 0xffffffffu : ((1u << (C & 31)) - 1u);
    TopkArgs k = r.k;
    TopkPickArgs p = r.pick;
    for (unsigned d = 0; d < r.passes; d++) {
        // digit d from the top: the top one takes what 12-bit digits leave of C
        const uint32_t shift = kTopkDigitBits * (r.passes - 1 - d);
        const uint32_t bits = d == 0 ? C - shift : kTopkDigitBits;
        k.hist = p.hist = r.k.hist + (size_t)d * kTopkBuckets;
        k.shift = p.shift = shift;
        k.dmask = (1u << bits) - 1u;
        k.himask = d == 0 ? 0u : (vmask & ~((1u << (shift + kTopkDigitBits)) - 1u));
        p.nb = 1u << bits;
        p.first = d == 0;
        p.last = d + 1 == r.passes;
        MI355_LAUNCH(rec, 0, topk_hist_kernel<C>, dim3(hist_grid), dim3(kBlockThreads), 0, r.env.stream, k);
        MI355_LAUNCH(rec, 0, topk_pick_kernel, dim3(1), dim3(256), 0, r.env.stream, p);
    }
    MI355_LAUNCH(rec, 0, topk_emit_kernel<C>, dim3(emit_grid), dim3(kBlockThreads), 0, r.env.stream, k);
    launch_rowid_prefix<false>(r.env, r.plan, r.scan); // topk_emit_kernel has counted the ties per chunk
    MI355_LAUNCH(rec, 0, topk_trim_kernel<C>, dim3(trim_grid), dim3(kBlockThreads), 0, r.env.stream, k);
    return hipGetLastError();
}

} // namespace

unsigned mi355_top_k_passes(unsigned c) { return topk_passes(c); }

int mi355_top_k_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const void *mask_dev, uint64_t k, int largest, void *bitmap_dev,
                    uint64_t *result_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(c));
    MI355_CHECK(check_dev(result_dev, 8, "result_dev"));
    MI355_CHECK(check_aligned(packed_dev, 16, "packed_dev"));
    MI355_CHECK(check_aligned(mask_dev, 4, "mask_dev"));
    MI355_CHECK(check_aligned(bitmap_dev, 4, "bitmap_dev"));
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(result_dev, 0, 4 * sizeof(uint64_t), ctx->stream));
        return MI355_OK;
    }
    MI355_CHECK(check_ptr(packed_dev, "packed_dev"));
    MI355_CHECK(check_ptr(bitmap_dev, "bitmap_dev"));
    const uint64_t nbytes = bitmap_bytes(n), col_bytes = packed_bytes(n, c);
    MI355_CHECK(check_no_overlap(bitmap_dev, nbytes, "bitmap_dev", packed_dev, col_bytes, "packed_dev", "column"));
    if (mask_dev && bitmap_dev != mask_dev && ranges_overlap(bitmap_dev, nbytes, mask_dev, nbytes))
        return fail(MI355_E_INVALID, "bitmap_dev overlaps mask_dev without being it: only bitmap_dev == mask_dev works in place");
    MI355_CHECK(check_no_overlap(result_dev, 4 * sizeof(uint64_t), "result_dev", packed_dev, col_bytes, "packed_dev", "column"));
    MI355_CHECK(check_no_overlap(result_dev, 4 * sizeof(uint64_t), "result_dev", mask_dev, mask_dev ? nbytes : 0, "mask_dev", "mask"));
    if (ranges_overlap(result_dev, 4 * sizeof(uint64_t), bitmap_dev, nbytes))
        return fail(MI355_E_INVALID, "result_dev overlaps bitmap_dev");
    // the chunk prefix of the ties (launch_util.hpp rowid_plan); the state; the counters
    const RowidPlan plan = rowid_plan(n);
    const uint64_t nchunks = plan.nchunks, front = plan.words;
    const unsigned passes = topk_passes(c);
    const uint64_t words = front + kTopkStateWords + (uint64_t)passes * kTopkBuckets;
    MI355_CHECK(rowid_ws_get(ctx, words, "mi355_top_k_dev"));
    unsigned long long *const ws = ctx->rowid_ws;
    TopkLaunch r{};
    r.k.packed = (const uint8_t *)packed_dev;
    r.k.n = n;
    r.k.mask = (const uint8_t *)mask_dev;
    r.k.bitmap = (uint8_t *)bitmap_dev;
    r.k.chunk_counts = ws;
    r.k.nchunks = nchunks;
    r.k.state = ws + front;
    r.k.hist = ws + front + kTopkStateWords;
    r.k.flip = largest ? 0u : (c == 32 ? 0xffffffffu : ((1u << c) - 1u));
    r.k.in_place = mask_dev != nullptr && bitmap_dev == mask_dev;
    r.k.nts = (uint32_t)one_pass_store_policy(nbytes, ctx->scan_nt_stores);
    r.pick.state = r.k.state;
    r.pick.k = k;
    r.pick.result = result_dev;
    r.pick.flip = r.k.flip;
    r.scan.chunk_counts = ws;
    r.scan.nchunks = nchunks;
    r.plan = plan;
    r.passes = passes;
    r.env = launch_env(ctx);
    HIP_TRY(hipMemsetAsync(ws, 0, words * sizeof(unsigned long long), ctx->stream));
    const hipError_t err = launch_by_width<1, 32>(c, r, [](auto w, const TopkLaunch &q) { return launch_top_k<decltype(w)::value>(q); });
    if (err != hipSuccess) return fail(MI355_E_HIP, "top_k launch: %s", hipGetErrorString(err));
    return MI355_OK;
}
