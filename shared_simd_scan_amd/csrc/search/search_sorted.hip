// search_sorted.hip -- implementation of include/mi355_search.h: argument checks, the choice between the two tiers and the launch
// of search_lds_kernel / search_global_kernel (search/search.hpp) by output width.  Its own translation unit: neither the other
// entry points nor the width groups rebuild with it.  The launch itself is launch_tier (launch_util.hpp) on a LaunchEnv (ctx.hpp),
// shared with lookup/ and semijoin/.  Nothing of the context's is taken: no workspace, no counter scratch.
#include "../ctx.hpp"

#include "../../../include/mi355_search.h"
#include "../checks.hpp"
#include "../dispatch.hpp"
#include "../launch_util.hpp"
#include "search.hpp"

using namespace mi355;

namespace {

static_assert(kSearchLdsMaxBytes == MI355_SEARCH_LDS_MAX_BYTES, "the header's limit is the kernels'");

constexpr uint64_t kSearchMaxRows = 0xffffffffull;

struct SearchLaunch {
    SearchArgs k;
    bool in_lds;
    LaunchEnv env;
};

// all of a block's LDS is dynamic: the waves' images and the samples
template <int CO> hipError_t launch_search(const SearchLaunch &r)
{
    const uint64_t ntiles = rt_ntiles(r.k.n);
    const int max_dyn = (int)(search_images_lds(32) + kSearchLdsMaxBytes + 16u);
    const size_t lds = search_images_lds(r.k.c) + search_samples_lds(r.k.rows);
    if (r.in_lds)
        launch_tier<search_lds_kernel<CO>>(r.env, r.k, ntiles, lds, 0, max_dyn);
    else
        launch_tier<search_global_kernel<CO>>(r.env, r.k, ntiles, lds, 0, max_dyn);
    return hipGetLastError();
}

bool search_args_ok(unsigned c, unsigned ct, unsigned co, uint64_t rows)
{
    return c >= 1 && c <= 32 && ct >= 1 && ct <= 32 && co >= 1 && co <= 32 && rows <= kSearchMaxRows;
}

// a table of `rows` entries of w bits, in the whole dwords the kernel reads
uint64_t table_bytes(uint64_t rows, unsigned w) { return ((rows * w + 31) / 32) * 4; }

uint32_t log2_of(uint64_t pow2)
{
    uint32_t lg = 0;
    while ((1ull << lg) < pow2) lg++;
    return lg;
}

} // namespace

const char *mi355_search_sorted_kernel(unsigned c, unsigned ct, unsigned co, uint64_t rows)
{
    if (!search_args_ok(c, ct, co, rows)) return nullptr;
    return search_in_lds(rows) ? "search_lds_kernel" : "search_global_kernel";
}

uint64_t mi355_search_sorted_stride(uint64_t rows)
{
    return search_stride(rows);
}

int mi355_search_sorted_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const void *table_dev, unsigned ct, uint64_t rows,
                            const uint64_t *rows_dev, int side, int exact, uint32_t miss, void *out_dev, unsigned co, void *found_dev,
                            uint64_t *hits_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(c));
    MI355_CHECK(check_width(ct, "ct"));
    MI355_CHECK(check_width(co, "co"));
    if (side != MI355_SEARCH_LEFT && side != MI355_SEARCH_RIGHT) return fail(MI355_E_INVALID, "side=%d is neither MI355_SEARCH_LEFT nor MI355_SEARCH_RIGHT", side);
    if (rows > kSearchMaxRows) return fail(MI355_E_INVALID, "rows=%llu beyond 2^32 - 1", (unsigned long long)rows);
    if (n && !out_dev && !found_dev && !hits_dev) return fail(MI355_E_INVALID, "out_dev, found_dev and hits_dev are all null: nothing to compute");
    if (out_dev) {
        if (co < 32 && (rows >> co)) return fail(MI355_E_INVALID, "rows=%llu beyond 2^co - 1: a position is no value of co=%u bits", (unsigned long long)rows, co);
        if (co < 32 && (miss >> co)) return fail(MI355_E_INVALID, "miss=%u is no value of co=%u bits", miss, co);
    }
    MI355_CHECK(check_aligned(packed_dev, 16, "packed_dev"));
    MI355_CHECK(check_aligned(table_dev, 4, "table_dev"));
    MI355_CHECK(check_aligned(rows_dev, 8, "rows_dev"));
    MI355_CHECK(check_aligned(out_dev, 16, "out_dev"));
    MI355_CHECK(check_aligned(found_dev, 4, "found_dev"));
    MI355_CHECK(check_aligned(hits_dev, 8, "hits_dev"));
    if (rows) MI355_CHECK(check_ptr(table_dev, "table_dev"));
    // (n == 0: the column and the results are empty ranges, which overlap nothing)
    const uint64_t out_bytes = out_dev ? packed_bytes(n, co) : 0, found_bytes = found_dev ? bitmap_bytes(n) : 0;
    const uint64_t col_bytes = packed_bytes(n, c), tab_bytes = table_dev ? table_bytes(rows, ct) : 0;
    if (n) {
        MI355_CHECK(check_ptr(packed_dev, "packed_dev"));
        MI355_CHECK(check_no_overlap(out_dev, out_bytes, "out_dev", packed_dev, col_bytes, "packed_dev", "column"));
        MI355_CHECK(check_no_overlap(out_dev, out_bytes, "out_dev", table_dev, tab_bytes, "table_dev", "table"));
        MI355_CHECK(check_no_overlap(found_dev, found_bytes, "found_dev", packed_dev, col_bytes, "packed_dev", "column"));
        MI355_CHECK(check_no_overlap(found_dev, found_bytes, "found_dev", table_dev, tab_bytes, "table_dev", "table"));
        if (ranges_overlap(out_dev, out_bytes, found_dev, found_bytes)) return fail(MI355_E_INVALID, "out_dev overlaps found_dev: two results of one call");
    }
    // the counter is a result too, zeroed below whatever n is; *rows_dev is read while the results are written
    const uint64_t word = sizeof(uint64_t), hits_bytes = hits_dev ? word : 0, rows_bytes = rows_dev ? word : 0;
    MI355_CHECK(check_no_overlap(hits_dev, hits_bytes, "hits_dev", packed_dev, col_bytes, "packed_dev", "column"));
    MI355_CHECK(check_no_overlap(hits_dev, hits_bytes, "hits_dev", table_dev, tab_bytes, "table_dev", "table"));
    MI355_CHECK(check_no_overlap(hits_dev, hits_bytes, "hits_dev", rows_dev, rows_bytes, "rows_dev", "row count"));
    MI355_CHECK(check_no_overlap(out_dev, out_bytes, "out_dev", rows_dev, rows_bytes, "rows_dev", "row count"));
    MI355_CHECK(check_no_overlap(found_dev, found_bytes, "found_dev", rows_dev, rows_bytes, "rows_dev", "row count"));
    if (ranges_overlap(hits_dev, hits_bytes, out_dev, out_bytes)) return fail(MI355_E_INVALID, "hits_dev overlaps out_dev: two results of one call");
    if (ranges_overlap(hits_dev, hits_bytes, found_dev, found_bytes)) return fail(MI355_E_INVALID, "hits_dev overlaps found_dev: two results of one call");
    // the counter starts from 0: all an empty column leaves in it
    if (hits_dev) HIP_TRY(hipMemsetAsync(hits_dev, 0, sizeof(uint64_t), ctx->stream));
    if (n == 0) return MI355_OK;
    SearchLaunch r{};
    r.k.packed = (const uint8_t *)packed_dev;
    r.k.n = n;
    r.k.table = (const uint32_t *)table_dev;
    r.k.rows_dev = (const unsigned long long *)rows_dev;
    r.k.out = (uint8_t *)out_dev;
    r.k.found = (uint8_t *)found_dev;
    r.k.hits = (unsigned long long *)hits_dev;
    r.k.rows = (uint32_t)rows;
    uint32_t top = 0;
    if (rows)
        for (top = 1; (uint64_t)top * 2 <= rows; top *= 2) {}
    r.k.top = top;
    r.in_lds = search_in_lds(rows);
    r.k.lg = log2_of(search_stride(rows));
    r.k.c = c;
    r.k.ct = ct;
    r.k.right = side == MI355_SEARCH_RIGHT;
    r.k.exact = exact != 0;
    r.k.miss = miss;
    r.k.nts = (uint32_t)one_pass_store_policy((out_dev ? packed_bytes(n, co) : 0) + (found_dev ? bitmap_bytes(n) : 0), ctx->scan_nt_stores);
    r.env = launch_env(ctx);
    const hipError_t err = launch_by_width<1, 32>(co, r, [](auto w, const SearchLaunch &q) { return launch_search<decltype(w)::value>(q); });
    if (err != hipSuccess) return fail(MI355_E_HIP, "search_sorted launch: %s", hipGetErrorString(err));
    return MI355_OK;
}
