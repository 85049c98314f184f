// lookup.hip -- implementation of include/mi355_lookup.h: argument checks, the choice between the two tiers and the launch of
// lookup_lds_kernel / lookup_global_kernel (lookup/lookup.hpp) by output width.  Its own translation unit: neither the other
// entry points nor the width groups rebuild with it.  The launch itself is launch_tier (launch_util.hpp) on a LaunchEnv (ctx.hpp),
// shared with semijoin/.
#include "../ctx.hpp"

#include "../../../include/mi355_lookup.h"
#include "../checks.hpp"
#include "../dispatch.hpp"
#include "../launch_util.hpp"
#include "lookup.hpp"

using namespace mi355;

namespace {

static_assert(kLookupLdsMaxBytes == MI355_LOOKUP_LDS_MAX_BYTES, "the header's limit is the kernels'");

constexpr uint64_t kLookupMaxTableRows = 1ull << 32;

struct LookupLaunch {
    LookupArgs k;
    bool in_lds;
    LaunchEnv env;
};

// all of a block's LDS is dynamic: the waves' images, and the table in the LDS tier
template <int CT> hipError_t launch_lookup(const LookupLaunch &r)
{
    const uint64_t ntiles = rt_ntiles(r.k.n);
    const int max_dyn = (int)(lookup_images_lds(32) + kLookupLdsMaxBytes);
    if (r.in_lds)
        launch_tier<lookup_lds_kernel<CT>>(r.env, r.k, ntiles, lookup_images_lds(r.k.c) + lookup_table_lds(r.k.reach, CT), 0, max_dyn);
    else
        launch_tier<lookup_global_kernel<CT>>(r.env, r.k, ntiles, lookup_images_lds(r.k.c), 0, max_dyn);
    return hipGetLastError();
}

bool lookup_args_ok(unsigned c, uint64_t table_rows, unsigned ct) { return c >= 1 && c <= 32 && ct >= 1 && ct <= 32 && table_rows <= kLookupMaxTableRows; }

} // namespace

const char *mi355_lookup_kernel(unsigned c, uint64_t table_rows, unsigned ct)
{
    if (!lookup_args_ok(c, table_rows, ct)) return nullptr;
    return lookup_in_lds(c, table_rows, ct) ? "lookup_lds_kernel" : "lookup_global_kernel";
}

int mi355_lookup_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const void *table_dev, uint64_t table_rows, unsigned ct,
                     uint32_t miss, void *out_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(c));
    MI355_CHECK(check_width(ct, "ct"));
    if (table_rows > kLookupMaxTableRows) return fail(MI355_E_INVALID, "table_rows=%llu beyond 2^32", (unsigned long long)table_rows);
    if (ct < 32 && (miss >> ct)) return fail(MI355_E_INVALID, "miss=%u is no value of ct=%u bits", miss, ct);
    if (table_rows) MI355_CHECK(check_ptr(table_dev, "table_dev"));
    MI355_CHECK(check_aligned(table_dev, 4, "table_dev"));
    MI355_CHECK(check_aligned(packed_dev, 16, "packed_dev"));
    MI355_CHECK(check_aligned(out_dev, 16, "out_dev"));
    if (n == 0) return MI355_OK;
    MI355_CHECK(check_ptr(packed_dev, "packed_dev"));
    MI355_CHECK(check_ptr(out_dev, "out_dev"));
    const uint64_t out_bytes = packed_bytes(n, ct);
    MI355_CHECK(check_no_overlap(out_dev, out_bytes, "out_dev", packed_dev, packed_bytes(n, c), "packed_dev", "column"));
    if (table_dev) MI355_CHECK(check_no_overlap(out_dev, out_bytes, "out_dev", table_dev, packed_bytes(table_rows, ct), "table_dev", "table"));
    const uint64_t reach = value_reach(c, table_rows); // what a c-bit value can address of the table
    LookupLaunch r{};
    r.k.packed = (const uint8_t *)packed_dev;
    r.k.n = n;
    r.k.table = (const uint32_t *)table_dev;
    r.k.out = (uint8_t *)out_dev;
    r.k.c = c;
    r.in_lds = lookup_in_lds(c, table_rows, ct);
    r.k.reach = r.in_lds ? (uint32_t)reach : 0u;
    r.k.limit = reach ? (uint32_t)(reach - 1) : 0u;
    r.k.last_word = reach ? (uint32_t)((reach * ct - 1) >> 5) : 0u;
    r.k.miss = miss;
    r.k.nts = (uint32_t)one_pass_store_policy(out_bytes, ctx->scan_nt_stores);
    r.env = launch_env(ctx);
    const hipError_t err = launch_by_width<1, 32>(ct, r, [](auto w, const LookupLaunch &q) { return launch_lookup<decltype(w)::value>(q); });
    if (err != hipSuccess) return fail(MI355_E_HIP, "lookup launch: %s", hipGetErrorString(err));
    return MI355_OK;
}
