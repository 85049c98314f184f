// sort_rows.hip -- implementation of include/mi355_sort.h: argument checks, the selection workspace, and the launches of a call --
// per digit a count kernel, rowid_scan_kernel (kernels/bitmap.hpp, through launch_rowid_prefix of launch_util.hpp),
// sort_offsets_kernel and a scatter kernel (sort/sort_rows.hpp).  Its own translation unit: neither the other entry points nor the
// width groups rebuild with it.  The grids come from a LaunchEnv (ctx.hpp), as in compact/ and topk/.
#include "../ctx.hpp"

#include "../../../include/mi355_sort.h"
#include "../checks.hpp"
#include "../dispatch.hpp"
#include "../launch_util.hpp"
#include "sort_rows.hpp"

using namespace mi355;

namespace {

constexpr uint64_t kSortMaxRows = 1ull << 32; // a row index inside the view fits 32 bits

// the workspace: the widest pass's counters in RowidArgs' layout, the state, then the item buffers
struct SortPlan {
    uint64_t most;     // rows the call can write: min(capacity, n)
    uint64_t prefix;   // words of the counters and their prefix
    unsigned buffers;  // item buffers of `most` words each: passes - 1, at most 2 (ping-pong)
    uint64_t words;
};
SortPlan sort_plan(uint64_t n, uint64_t capacity, unsigned c)
{
    SortPlan p{};
    const unsigned passes = sort_passes(c);
    p.most = capacity < n ? capacity : n;
    p.prefix = rowid_prefix_words((uint64_t)sort_max_buckets(c) * sort_spans(n)); // (the item passes have no more spans than pass 0)
    p.buffers = passes > 2 ? 2 : (passes > 1 ? 1 : 0);
    p.words = p.prefix + kSortStateWords + p.buffers * p.most;
    return p;
}

// the prefix over a pass's counters
void launch_prefix(const LaunchEnv &env, const SortArgs &k)
{
    RowidPlan p{};
    p.nchunks = (uint64_t)(1u << k.dbits) * k.nspans;
    p.ngroups = rowid_scan_groups(p.nchunks);
    p.words = rowid_prefix_words(p.nchunks);
    RowidArgs g{};
    g.chunk_counts = k.counts;
    g.nchunks = p.nchunks;
    launch_rowid_prefix<false>(env, p, g);
    MI355_LAUNCH(env.record, 0, sort_offsets_kernel, dim3(1), dim3(256), 0, env.stream, k);
}

} // namespace

unsigned mi355_sort_rows_passes(unsigned c) { return sort_passes(c); }

uint64_t mi355_sort_rows_workspace_words(uint64_t n, uint64_t capacity, unsigned c)
{
    if (sort_passes(c) == 0 || n > kSortMaxRows || n == 0) return 0;
    return sort_plan(n, capacity, c).words;
}

int mi355_sort_rows_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const void *mask_dev, int descending, uint64_t first_row,
                        uint64_t *rowids_dev, uint32_t *values_dev, uint64_t capacity, uint64_t *count_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(c));
    if (n > kSortMaxRows) return fail(MI355_E_INVALID, "n=%llu beyond 2^32 rows: a row index inside the view must fit 32 bits", (unsigned long long)n);
    MI355_CHECK(check_dev(count_dev, 8, "count_dev"));
    MI355_CHECK(check_aligned(packed_dev, 16, "packed_dev"));
    MI355_CHECK(check_aligned(mask_dev, 4, "mask_dev"));
    MI355_CHECK(check_aligned(rowids_dev, 8, "rowids_dev"));
    MI355_CHECK(check_aligned(values_dev, 4, "values_dev"));
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(count_dev, 0, sizeof(uint64_t), ctx->stream));
        return MI355_OK;
    }
    MI355_CHECK(check_ptr(packed_dev, "packed_dev"));
    if (capacity) MI355_CHECK(check_ptr(rowids_dev, "rowids_dev"));
    const SortPlan plan = sort_plan(n, capacity, c);
    const uint64_t col_bytes = packed_bytes(n, c), mask_bytes = mask_dev ? bitmap_bytes(n) : 0;
    const uint64_t ids_bytes = rowids_dev ? plan.most * sizeof(uint64_t) : 0, vals_bytes = values_dev ? plan.most * sizeof(uint32_t) : 0;
    MI355_CHECK(check_no_overlap(rowids_dev, ids_bytes, "rowids_dev", packed_dev, col_bytes, "packed_dev", "column"));
    MI355_CHECK(check_no_overlap(rowids_dev, ids_bytes, "rowids_dev", mask_dev, mask_bytes, "mask_dev", "mask"));
    MI355_CHECK(check_no_overlap(values_dev, vals_bytes, "values_dev", packed_dev, col_bytes, "packed_dev", "column"));
    MI355_CHECK(check_no_overlap(values_dev, vals_bytes, "values_dev", mask_dev, mask_bytes, "mask_dev", "mask"));
    MI355_CHECK(check_no_overlap(count_dev, sizeof(uint64_t), "count_dev", packed_dev, col_bytes, "packed_dev", "column"));
    MI355_CHECK(check_no_overlap(count_dev, sizeof(uint64_t), "count_dev", mask_dev, mask_bytes, "mask_dev", "mask"));
    if (ranges_overlap(rowids_dev, ids_bytes, values_dev, vals_bytes)) return fail(MI355_E_INVALID, "rowids_dev overlaps values_dev");
    if (ranges_overlap(count_dev, sizeof(uint64_t), rowids_dev, ids_bytes)) return fail(MI355_E_INVALID, "count_dev overlaps rowids_dev");
    if (ranges_overlap(count_dev, sizeof(uint64_t), values_dev, vals_bytes)) return fail(MI355_E_INVALID, "count_dev overlaps values_dev");
    MI355_CHECK(rowid_ws_get(ctx, plan.words, "mi355_sort_rows_dev"));
    unsigned long long *const ws = ctx->rowid_ws;
    unsigned long long *const buffers[2] = {ws + plan.prefix + kSortStateWords, ws + plan.prefix + kSortStateWords + plan.most};

    SortArgs k{};
    k.packed = (const uint8_t *)packed_dev;
    k.n = n;
    k.mask = (const uint8_t *)mask_dev;
    k.counts = ws;
    k.state = ws + plan.prefix;
    k.capacity = capacity;
    k.first_row = first_row;
    k.rowids = rowids_dev;
    k.values = values_dev;
    k.c = c;
    k.flip = descending ? rt_vmask(c) : 0u;
    const LaunchEnv env = launch_env(ctx);
    std::string *const rec = env.record;
    const unsigned passes = sort_passes(c);
    const unsigned item_grid = grid_for(sort_spans(plan.most), cap_bpc(8, env.max_blocks_per_cu), env.num_cus);
    for (unsigned p = 0; p < passes; p++) {
        // digit p from the bottom: the top one takes what 8-bit digits leave of c
        k.shift = kSortDigitBits * p;
        k.dbits = p + 1 == passes ? c - k.shift : (uint32_t)kSortDigitBits;
        k.last = p + 1 == passes;
        k.items_in = p ? buffers[(p - 1) & 1] : nullptr;
        k.items_out = k.last ? nullptr : buffers[p & 1];
        if (p == 0) {
            k.nspans = sort_spans(n);
            k.count_out = count_dev;
            launch_tier<sort_count_kernel>(env, k, k.nspans, sort_lds(c, false), 0, (int)sort_lds(32, false));
            launch_prefix(env, k);
            if (capacity == 0) break; // the count is all the caller asked for
            launch_tier<sort_scatter_kernel>(env, k, k.nspans, sort_lds(c, true), 0, (int)sort_lds(32, true));
        } else {
            k.nspans = sort_spans(plan.most);
            k.count_out = nullptr;
            MI355_LAUNCH(rec, 0, sort_item_count_kernel, dim3(item_grid), dim3(kBlockThreads), 0, env.stream, k);
            launch_prefix(env, k);
            launch_tier<sort_item_scatter_kernel>(env, k, k.nspans, kSortItemLds, 0, (int)kSortItemLds); // (the stage: two blocks per CU)
        }
    }
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(MI355_E_HIP, "sort_rows launch: %s", hipGetErrorString(err));
    return MI355_OK;
}
