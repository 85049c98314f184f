// group_aggregate_wide.hip -- implementation of include/mi355_groupby_wide.h: argument checks, the size of the LDS front and the
// launch of group_aggregate_wide_kernel (groupby_wide/group_aggregate_wide.hpp).  Its own translation unit: neither the other
// entry points nor the width groups rebuild with it.  What it takes from the context is a LaunchEnv (ctx.hpp), as in groupby/,
// semijoin/ and lookup/.
#include "../ctx.hpp"

#include "../../../include/mi355_groupby_wide.h"
#include "../checks.hpp"
#include "../dispatch.hpp"
#include "../launch_util.hpp"
#include "group_aggregate_wide.hpp"

using namespace mi355;

namespace {

static_assert(kGroupWideMaxGroups == MI355_GROUP_WIDE_MAX_GROUPS, "the header's limit is the kernel's");

// the most dynamic LDS any pair of widths asks for
constexpr uint32_t group_wide_max_lds()
{
    uint32_t most = 0;
    for (uint32_t ck = 1; ck <= 32; ck++)
        for (uint32_t cv = 1; cv <= 32; cv++) {
            const uint32_t b = group_wide_block_lds(group_wide_front_slots(ck, cv), ck, cv);
            most = b > most ? b : most;
        }
    return most;
}
static_assert(group_wide_max_lds() <= (uint32_t)kCuLdsBytes, "LDS budget");

// every group to its neutral element and the counter to 0: all an empty column takes, and what the aggregation starts from
void launch_init(const LaunchEnv &env, const GroupWideArgs &k)
{
    MI355_LAUNCH(env.record, 0, group_aggregate_wide_init_kernel, dim3((k.groups + 255u) / 256u), dim3(256), 0, env.stream, k.out, k.groups, k.dropped);
}

} // namespace

uint32_t mi355_group_wide_front_slots(unsigned ck, unsigned cv)
{
    if (ck < 1 || ck > 32 || cv < 1 || cv > 32) return 0;
    return group_wide_front_slots(ck, cv);
}

int mi355_group_aggregate_wide_dev(mi355_ctx *ctx, const void *keys_dev, unsigned ck, const void *values_dev, unsigned cv, uint64_t n,
                                   const void *mask_dev, uint64_t groups, uint64_t *out_dev, uint64_t *dropped_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(ck, "ck"));
    MI355_CHECK(check_width(cv, "cv"));
    if (groups == 0) return fail(MI355_E_INVALID, "groups=0: the key domain [0, groups) is empty");
    if (groups > kGroupWideMaxGroups)
        return fail(MI355_E_INVALID, "groups=%llu beyond MI355_GROUP_WIDE_MAX_GROUPS=%llu", (unsigned long long)groups, (unsigned long long)kGroupWideMaxGroups);
    if (groups > value_reach(ck, groups)) return fail(MI355_E_INVALID, "groups=%llu beyond 2^ck, ck=%u", (unsigned long long)groups, ck);
    MI355_CHECK(check_dev(out_dev, 8, "out_dev"));
    MI355_CHECK(check_aligned(dropped_dev, 8, "dropped_dev"));
    if (n) {
        MI355_CHECK(check_ptr(keys_dev, "keys_dev"));
        MI355_CHECK(check_ptr(values_dev, "values_dev"));
    }
    MI355_CHECK(check_aligned(keys_dev, 16, "keys_dev"));
    MI355_CHECK(check_aligned(values_dev, 16, "values_dev"));
    MI355_CHECK(check_aligned(mask_dev, 4, "mask_dev"));
    GroupWideArgs k{};
    k.keys = (const uint8_t *)keys_dev;
    k.values = (const uint8_t *)values_dev;
    k.n = n;
    k.mask = (const uint8_t *)mask_dev;
    k.out = (unsigned long long *)out_dev;
    k.dropped = (unsigned long long *)dropped_dev;
    k.groups = (uint32_t)groups;
    k.ck = ck;
    k.cv = cv;
    k.slots = group_wide_front_slots(ck, cv);
    const LaunchEnv env = launch_env(ctx);
    launch_init(env, k);
    if (n) {
        const uint64_t ntiles = rt_ntiles(n);
        const size_t lds = group_wide_block_lds(k.slots, ck, cv);
        allow_dynamic_lds<group_aggregate_wide_kernel>((int)group_wide_max_lds(), env.device);
        // Blocks per CU: what registers and this launch's LDS admit, at most four (table_bpc: the occupancy query is asked once
        // per device, the LDS share is arithmetic, so a capture never repeats the query).
        unsigned grid = grid_for(ntiles, cap_bpc(table_bpc<group_aggregate_wide_kernel>(lds, 0, env.device), env.max_blocks_per_cu), env.num_cus);
        // a block's counts are 32-bit words in LDS: no block may see 2^32 rows (a grid beyond what is resident simply queues)
        const uint64_t min_grid = (n >> 31) + 1;
        if (grid < min_grid) grid = (unsigned)min_grid;
        MI355_LAUNCH(env.record, 0, group_aggregate_wide_kernel, dim3(grid), dim3(kBlockThreads), lds, env.stream, k);
    }
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(MI355_E_HIP, "group_aggregate_wide launch: %s", hipGetErrorString(err));
    return MI355_OK;
}
