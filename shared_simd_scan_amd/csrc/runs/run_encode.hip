// run_encode.hip -- mi355_run_encode_dev of include/mi355_runs.h: argument checks and the launches of a call -- run_count_kernel
// (runs/runs.hpp), rowid_scan_kernel (kernels/bitmap.hpp, through launch_rowid_prefix<false> of launch_util.hpp) over the chunks'
// tail counts, compact_edges_kernel (compact/compact.hpp, as it stands) once per output given, then run_emit_kernel<C> by the
// column's width.  The chunk prefix lives in the CALLER's workspace: the call takes nothing from the context, so it is capturable
// whatever its arguments.  Its own translation unit: neither the other entry points nor the width groups rebuild with it.
#include "../ctx.hpp"

#include "../../../include/mi355_runs.h"
#include "../checks.hpp"
#include "../dispatch.hpp"
#include "../launch_util.hpp"
#include "runs.hpp"

using namespace mi355;

namespace {

struct RunEncodeLaunch {
    RunEncodeArgs k;
    LaunchEnv env;
};

// all of a block's LDS is dynamic, sized to both widths: the waves' two images of the column and their two stages
template <int C> hipError_t launch_run_emit(const RunEncodeLaunch &r)
{
    launch_tier<run_emit_kernel<C>>(r.env, r.k, r.k.nchunks, run_emit_block_lds(C, r.k.ce), 0, (int)run_emit_block_lds(C, 32));
    return hipGetLastError();
}

// an output of up to `most` values of w bits, in the whole dwords the call stores
uint64_t output_bytes(uint64_t most, unsigned w) { return ((most * w + 31) / 32) * 4; }

} // namespace

const char *mi355_run_encode_kernel(unsigned c, unsigned ce)
{
    return c >= 1 && c <= 32 && ce >= 1 && ce <= 32 ? "run_emit_kernel" : nullptr;
}

uint64_t mi355_run_encode_workspace_words(uint64_t n)
{
    return rowid_plan(n).words; // the chunk prefix over n rows: a chunk of a bitmap of n rows is a chunk of the column
}

int mi355_run_encode_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, unsigned ce, void *values_dev, void *ends_dev, uint64_t capacity,
                         uint64_t *count_dev, uint64_t *ws_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(c, "c"));
    MI355_CHECK(check_width(ce, "ce"));
    if (n > (ce >= 32 ? 0xffffffffull : (1ull << ce) - 1))
        return fail(MI355_E_INVALID, "n=%llu beyond 2^ce - 1: an end of ce=%u bits cannot hold it", (unsigned long long)n, ce);
    MI355_CHECK(check_dev(count_dev, 8, "count_dev"));
    MI355_CHECK(check_aligned(values_dev, 16, "values_dev"));
    MI355_CHECK(check_aligned(ends_dev, 16, "ends_dev"));
    if (capacity && !values_dev && !ends_dev) return fail(MI355_E_INVALID, "values_dev and ends_dev are both null with capacity > 0: nothing to write");
    if (n) {
        MI355_CHECK(check_dev(packed_dev, 16, "packed_dev"));
        MI355_CHECK(check_dev(ws_dev, 8, "ws_dev"));
        const uint64_t most = capacity < n ? capacity : n; // runs the call can write
        const uint64_t vbytes = values_dev ? output_bytes(most, c) : 0, ebytes = ends_dev ? output_bytes(most, ce) : 0;
        const uint64_t col_bytes = packed_bytes(n, c), ws_bytes = mi355_run_encode_workspace_words(n) * sizeof(uint64_t);
        MI355_CHECK(check_no_overlap(values_dev, vbytes, "values_dev", packed_dev, col_bytes, "packed_dev", "column"));
        MI355_CHECK(check_no_overlap(ends_dev, ebytes, "ends_dev", packed_dev, col_bytes, "packed_dev", "column"));
        MI355_CHECK(check_no_overlap(values_dev, vbytes, "values_dev", ws_dev, ws_bytes, "ws_dev", "workspace"));
        MI355_CHECK(check_no_overlap(ends_dev, ebytes, "ends_dev", ws_dev, ws_bytes, "ws_dev", "workspace"));
        MI355_CHECK(check_no_overlap(values_dev, vbytes, "values_dev", ends_dev, ebytes, "ends_dev", "other output"));
    }
    // the count starts from 0: all an empty column leaves in it; the waves of run_count_kernel add their chunks' tails
    HIP_TRY(hipMemsetAsync(count_dev, 0, sizeof(uint64_t), ctx->stream));
    if (n == 0) return MI355_OK;
    const RowidPlan p = rowid_plan(n);
    RowidArgs g{};
    g.nchunks = p.nchunks;
    g.chunk_counts = (unsigned long long *)ws_dev;
    RunEncodeLaunch r{};
    r.k.packed = (const uint8_t *)packed_dev;
    r.k.n = n;
    r.k.chunk_counts = g.chunk_counts;
    r.k.nchunks = p.nchunks;
    r.k.values = capacity ? (uint32_t *)values_dev : nullptr;
    r.k.ends = capacity ? (uint32_t *)ends_dev : nullptr;
    r.k.capacity = capacity;
    r.k.count = (unsigned long long *)count_dev;
    r.k.c = c;
    r.k.ce = ce;
    // plain stores unless option "scan_nt_stores" names a policy: running_sum's finding (profiles/r21_running_sum.txt)
    r.k.nts = ctx->scan_nt_stores < 0 ? 0u : (uint32_t)ctx->scan_nt_stores;
    r.env = launch_env(ctx);
    std::string *const rec = r.env.record;
    // 1: the chunks' tail counts; 2: their prefix, every word of which the later kernels read is written here or by launch 1
    launch_tier<run_count_kernel>(r.env, r.k, p.nchunks, run_count_block_lds(c), 0, (int)run_count_block_lds(32));
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) {
        launch_rowid_prefix<false>(r.env, p, g);
        err = hipGetLastError();
    }
    // 3: the dwords of each output that chunks share, zeroed: compact's kernel on that output's width and pointer
    for (int which = 0; which < 2 && err == hipSuccess && capacity; which++) {
        CompactArgs e{};
        e.chunk_counts = g.chunk_counts;
        e.nchunks = p.nchunks;
        e.out = which ? r.k.ends : r.k.values;
        e.capacity = capacity;
        e.c = which ? ce : c;
        if (!e.out) continue;
        MI355_LAUNCH(rec, 0, compact_edges_kernel, dim3((unsigned)((p.nchunks + 255) / 256)), dim3(256), 0, ctx->stream, e);
        err = hipGetLastError();
    }
    if (err == hipSuccess && capacity) err = launch_by_width<1, 32>(c, r, [](auto w, const RunEncodeLaunch &q) { return launch_run_emit<decltype(w)::value>(q); });
    if (err != hipSuccess) return fail(MI355_E_HIP, "run_encode launch: %s", hipGetErrorString(err));
    return MI355_OK;
}
