// key_index.hip -- include/mi355_keyindex.h: argument checks, the slots in the selection workspace and their clear, the choice between
// the two tiers and the two launches of a call -- key_index_lds_kernel / key_index_global_kernel by the keys' width, then
// key_index_pack_kernel by the table's (keyindex/key_index.hpp).  Its own translation unit: neither the other entry points nor the
// width groups rebuild with it.  The tier's launch is launch_tier (launch_util.hpp) on a LaunchEnv (ctx.hpp), shared with distinct/,
// semijoin/ and lookup/.
#include "../ctx.hpp"

#include "../../../include/mi355_keyindex.h"
#include "../checks.hpp"
#include "../dispatch.hpp"
#include "../launch_util.hpp"
#include "key_index.hpp"

using namespace mi355;

namespace {

static_assert(kKeyIndexLdsMaxRows == MI355_KEY_INDEX_LDS_MAX_ROWS, "the header's limit is the kernels'");
static_assert(MI355_KEY_INDEX_FIRST == 0 && MI355_KEY_INDEX_LAST == 1, "KeyIndexArgs::last is the constant itself");

constexpr uint64_t kKeyIndexMaxRows = 1ull << 32;

struct KeyIndexLaunch {
    KeyIndexArgs k;
    bool in_lds;
    LaunchEnv env;
};

struct KeyIndexPackLaunch {
    KeyIndexPackArgs k;
    LaunchEnv env;
};

template <int C> hipError_t launch_key_index(const KeyIndexLaunch &r)
{
    using G = ScanGeom<C, scan_vpl(C, kModeEq)>;
    const uint64_t ntiles = (r.k.n + G::TILE_VALUES - 1) / G::TILE_VALUES;
    constexpr size_t fixed = key_index_static_lds<C>() + 16u;
    if (r.in_lds) {
        constexpr int max_dyn = (int)key_index_dyn_lds((uint32_t)kKeyIndexLdsMaxRows);
        launch_tier<key_index_lds_kernel<C>>(r.env, r.k, ntiles, key_index_dyn_lds(r.k.nslots), fixed, max_dyn);
    } else {
        if constexpr (C >= kKeyIndexGlobalMinBits)
            launch_tier<key_index_global_kernel<C>>(r.env, r.k, ntiles, 0, fixed, 0);
        else
            return hipErrorInvalidValue; // key_index_in_lds() is true below kKeyIndexGlobalMinBits
    }
    return hipGetLastError();
}

// a wave per 2048 entries of the table, eight blocks per CU at the most
template <int CT> hipError_t launch_key_index_pack(const KeyIndexPackLaunch &r)
{
    const uint64_t nsteps = (r.k.table_rows + kKeyIndexPackRows - 1) / kKeyIndexPackRows;
    const unsigned grid = grid_for(nsteps, cap_bpc(8, r.env.max_blocks_per_cu), r.env.num_cus);
    MI355_LAUNCH(r.env.record, 0, key_index_pack_kernel<CT>, dim3(grid), dim3(kBlockThreads), 0, r.env.stream, r.k);
    return hipGetLastError();
}

} // namespace

const char *mi355_key_index_kernel(unsigned ck, uint64_t table_rows)
{
    if (ck < 1 || ck > 32 || table_rows > kKeyIndexMaxRows) return nullptr;
    return key_index_in_lds(ck, table_rows) ? "key_index_lds_kernel" : "key_index_global_kernel";
}

int mi355_key_index_dev(mi355_ctx *ctx, const void *keys_dev, uint64_t n, unsigned ck, const void *mask_dev, uint64_t first_row, int keep,
                        void *table_dev, uint64_t table_rows, unsigned ct, uint32_t miss, uint64_t *out_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(ck, "ck"));
    MI355_CHECK(check_width(ct, "ct"));
    if (ct < 32 && miss >> ct) return fail(MI355_E_INVALID, "miss=%u is no value of ct=%u bits", miss, ct);
    if (table_rows > kKeyIndexMaxRows) return fail(MI355_E_INVALID, "table_rows=%llu beyond 2^32", (unsigned long long)table_rows);
    if (n >= (1ull << 32)) return fail(MI355_E_INVALID, "n=%llu beyond 2^32 - 1: a slot holds a 32-bit row", (unsigned long long)n);
    if (first_row >= (1ull << 32)) return fail(MI355_E_INVALID, "first_row=%llu beyond 2^32 - 1", (unsigned long long)first_row);
    if (keep != MI355_KEY_INDEX_FIRST && keep != MI355_KEY_INDEX_LAST) return fail(MI355_E_INVALID, "unknown keep %d", keep);
    MI355_CHECK(check_dev(out_dev, 8, "out_dev"));
    MI355_CHECK(check_aligned(keys_dev, 16, "keys_dev"));
    MI355_CHECK(check_aligned(mask_dev, 4, "mask_dev"));
    MI355_CHECK(check_aligned(table_dev, 16, "table_dev"));
    if (n) MI355_CHECK(check_ptr(keys_dev, "keys_dev"));
    const uint64_t table_bytes = packed_bytes(table_rows, ct);
    if (table_rows) {
        MI355_CHECK(check_ptr(table_dev, "table_dev"));
        MI355_CHECK(check_no_overlap(table_dev, table_bytes, "table_dev", keys_dev, keys_dev ? packed_bytes(n, ck) : 0, "keys_dev", "key column"));
        MI355_CHECK(check_no_overlap(table_dev, table_bytes, "table_dev", mask_dev, mask_dev ? bitmap_bytes(n) : 0, "mask_dev", "mask"));
        if (ranges_overlap(table_dev, table_bytes, out_dev, 4 * sizeof(uint64_t))) return fail(MI355_E_INVALID, "table_dev overlaps out_dev");
    }
    // what a ck-bit key can address of the table; with no rows nothing is addressed and the table is all miss
    const uint64_t reach = n ? value_reach(ck, table_rows) : 0;
    // the slots: two per word of the selection workspace (refused under capture when it would have to grow)
    if (reach) MI355_CHECK(rowid_ws_get(ctx, (reach + 1) / 2, "mi355_key_index_dev"));
    HIP_TRY(hipMemsetAsync(out_dev, 0, 4 * sizeof(uint64_t), ctx->stream));
    // zeroed at every call: no winner of an earlier call, or of another entry point that uses the workspace, survives
    if (reach) HIP_TRY(hipMemsetAsync(ctx->rowid_ws, 0, reach * sizeof(uint32_t), ctx->stream));
    hipError_t err = hipSuccess;
    if (n) {
        KeyIndexLaunch r{};
        r.k.packed = (const uint8_t *)keys_dev;
        r.k.n = n;
        r.k.mask = (const uint8_t *)mask_dev;
        r.k.slots = (uint32_t *)ctx->rowid_ws;
        r.k.out = (unsigned long long *)out_dev;
        r.in_lds = key_index_in_lds(ck, table_rows);
        r.k.bound = r.in_lds ? (uint32_t)reach : (uint32_t)(reach - 1);
        r.k.nslots = r.in_lds ? (uint32_t)reach : 0u;
        r.k.last = keep == MI355_KEY_INDEX_LAST ? 1u : 0u;
        r.env = launch_env(ctx);
        err = launch_by_width<1, 32>(ck, r, [](auto w, const KeyIndexLaunch &q) { return launch_key_index<decltype(w)::value>(q); });
    }
    if (err == hipSuccess && table_rows) {
        KeyIndexPackLaunch p{};
        p.k.slots = (const uint32_t *)ctx->rowid_ws;
        p.k.reach = reach;
        p.k.table_rows = table_rows;
        p.k.first_row = first_row;
        p.k.table = (uint8_t *)table_dev;
        p.k.out = (unsigned long long *)out_dev;
        p.k.miss = miss;
        p.k.last = keep == MI355_KEY_INDEX_LAST ? 1u : 0u;
        p.k.nts = (uint32_t)one_pass_store_policy(table_bytes, ctx->scan_nt_stores);
        p.env = launch_env(ctx);
        err = launch_by_width<1, 32>(ct, p, [](auto w, const KeyIndexPackLaunch &q) { return launch_key_index_pack<decltype(w)::value>(q); });
    }
    if (err != hipSuccess) return fail(MI355_E_HIP, "key_index launch: %s", hipGetErrorString(err));
    return MI355_OK;
}
