// compact.hip -- implementation of include/mi355_compact.h: argument checks, the selection workspace, and the four launches of a
// call -- rowid_count_kernel and rowid_scan_kernel (kernels/bitmap.hpp, through launch_rowid_prefix of launch_util.hpp), then
// compact_edges_kernel and compact_kernel<C> (compact/compact.hpp) by width.  Its own translation unit: neither the other entry
// points nor the width groups rebuild with it.  The last launch is launch_tier (launch_util.hpp) on a LaunchEnv (ctx.hpp), shared
// with semijoin/ and lookup/.
#include "../ctx.hpp"

#include "../../../include/mi355_compact.h"
#include "../checks.hpp"
#include "../dispatch.hpp"
#include "../launch_util.hpp"
#include "compact.hpp"

using namespace mi355;

namespace {

struct CompactLaunch {
    CompactArgs k;
    LaunchEnv env;
};

// all of a block's LDS is dynamic, sized to the width: the waves' two images and their stages
template <int C> hipError_t launch_compact(const CompactLaunch &r)
{
    launch_tier<compact_kernel<C>>(r.env, r.k, r.k.nchunks, compact_lds(C), 0, (int)compact_lds(C));
    return hipGetLastError();
}

} // namespace

const char *mi355_compact_kernel(unsigned c) { return c >= 1 && c <= 32 ? "compact_kernel" : nullptr; }

int mi355_compact_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const void *bitmap_dev, void *out_dev, uint64_t capacity,
                      uint64_t *count_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(c));
    MI355_CHECK(check_ptr(count_dev, "count_dev"));
    MI355_CHECK(check_aligned(packed_dev, 16, "packed_dev"));
    MI355_CHECK(check_aligned(bitmap_dev, 4, "bitmap_dev"));
    MI355_CHECK(check_aligned(out_dev, 16, "out_dev"));
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(count_dev, 0, sizeof(uint64_t), ctx->stream));
        return MI355_OK;
    }
    MI355_CHECK(check_ptr(packed_dev, "packed_dev"));
    MI355_CHECK(check_ptr(bitmap_dev, "bitmap_dev"));
    if (capacity) {
        MI355_CHECK(check_ptr(out_dev, "out_dev"));
        const uint64_t most = capacity < n ? capacity : n;          // values the call can write
        const uint64_t out_bytes = ((most * c + 31) / 32) * 4;      // in whole dwords
        MI355_CHECK(check_no_overlap(out_dev, out_bytes, "out_dev", packed_dev, packed_bytes(n, c), "packed_dev", "column"));
        MI355_CHECK(check_no_overlap(out_dev, out_bytes, "out_dev", bitmap_dev, bitmap_bytes(n), "bitmap_dev", "bitmap"));
    }
    // counts and prefix: the chunk prefix over the bitmap (launch_util.hpp rowid_plan)
    const RowidPlan p = rowid_plan(n);
    MI355_CHECK(rowid_ws_get(ctx, p.words, "mi355_compact_dev"));
    RowidArgs g{};
    g.bitmap = (const uint8_t *)bitmap_dev;
    g.nbytes = p.nbytes;
    g.nchunks = p.nchunks;
    g.chunk_counts = ctx->rowid_ws;
    CompactLaunch r{};
    r.k.packed = (const uint8_t *)packed_dev;
    r.k.n = n;
    r.k.bitmap = g.bitmap;
    r.k.nbytes = g.nbytes;
    r.k.chunk_counts = g.chunk_counts;
    r.k.nchunks = g.nchunks;
    r.k.out = (uint32_t *)out_dev;
    r.k.capacity = capacity;
    r.k.c = c;
    r.k.nts = (uint32_t)one_pass_store_policy(packed_bytes(capacity < n ? capacity : n, c), ctx->scan_nt_stores);
    r.env = launch_env(ctx);
    std::string *const rec = r.env.record;
    launch_rowid_prefix<true>(r.env, p, g);
    // also with capacity == 0: it leaves the total where the copy below takes it from
    MI355_LAUNCH(rec, 0, compact_edges_kernel, dim3((unsigned)((g.nchunks + 255) / 256)), dim3(256), 0, ctx->stream, r.k);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess && capacity)
        err = launch_by_width<1, 32>(c, r, [](auto w, const CompactLaunch &q) { return launch_compact<decltype(w)::value>(q); });
    if (err != hipSuccess) return fail(MI355_E_HIP, "compact launch: %s", hipGetErrorString(err));
    HIP_TRY(hipMemcpyAsync(count_dev, g.chunk_counts + g.nchunks, sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream));
    return MI355_OK;
}
