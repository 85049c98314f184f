// group_aggregate.hip -- implementation of include/mi355_groupby.h: argument checks and the launch of
// group_aggregate_kernel (groupby/group_aggregate.hpp) by key width.  Its own translation unit: neither the other entry points nor the
// width groups rebuild with it.  What it takes from the context is a LaunchEnv (ctx.hpp), as in semijoin/ and lookup/.
#include "../ctx.hpp"

#include <atomic>

#include "../../../include/mi355_groupby.h"
#include "../checks.hpp"
#include "../dispatch.hpp"
#include "../launch_util.hpp"
#include "group_aggregate.hpp"

using namespace mi355;

namespace {

static_assert(kGroupMaxBits == MI355_GROUP_MAX_KEY_BITS, "the header's limit is the kernel's");

struct GroupLaunch {
    GroupArgs k;
    unsigned ck;
    LaunchEnv env;
};

// every group's slot to its neutral element: all an empty column takes, and what group_aggregate_kernel starts from
void launch_init(const LaunchEnv &env, unsigned long long *out, unsigned ck)
{
    MI355_LAUNCH(env.record, 0, group_aggregate_init_kernel, dim3(((1u << ck) + 255u) / 256u), dim3(256), 0, env.stream, out, 1u << ck);
}

template <int CK> hipError_t launch_group(const GroupLaunch &r)
{
    using G = ScanGeom<CK, kRtVpl>;
    const uint32_t cv = r.k.cv;
    const uint64_t ntiles = (r.k.n + G::TILE_VALUES - 1) / G::TILE_VALUES;
    const size_t lds = group_block_lds<CK>(cv);
    allow_dynamic_lds<group_aggregate_kernel<CK>>((int)group_block_lds<CK>(32), r.env.device);
    // Blocks per CU: small tiles, LDS reads and atomics all through a tile -- as many blocks as LDS and registers admit, up to
    // 4 waves per SIMD (the rule of scan_columns_kernel's run-time-width form).  The query depends on the dynamic LDS, i.e.
    // on cv: asked once per value width.
    static std::atomic<int> bpc_of[33];
    int bpc = bpc_of[cv].load(std::memory_order_relaxed);
    if (bpc == 0) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, group_aggregate_kernel<CK>, kBlockThreads, lds) != hipSuccess || bpc < 1) bpc = 1;
        if (bpc > 4) bpc = 4;
        bpc_of[cv].store(bpc, std::memory_order_relaxed);
    }
    unsigned grid = grid_for(ntiles, cap_bpc(bpc, r.env.max_blocks_per_cu), r.env.num_cus);
    // a block's counts are 32-bit words in LDS: no block may see 2^32 rows (a grid beyond what is resident simply queues)
    const uint64_t min_grid = (r.k.n >> 31) + 1;
    if (grid < min_grid) grid = (unsigned)min_grid;
    launch_init(r.env, r.k.out, CK);
    MI355_LAUNCH(r.env.record, 0, (group_aggregate_kernel<CK>), dim3(grid), dim3(kBlockThreads), lds, r.env.stream, r.k);
    return hipGetLastError();
}

} // namespace

int mi355_group_aggregate_dev(mi355_ctx *ctx, const void *keys_dev, unsigned ck, const void *values_dev, unsigned cv, uint64_t n,
                              const void *mask_dev, uint64_t *out_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(ck, "ck", kGroupMaxBits, " (group_aggregate: the groups' state lives in LDS)"));
    MI355_CHECK(check_width(cv, "cv"));
    MI355_CHECK(check_dev(out_dev, 8, "out_dev"));
    if (n) MI355_CHECK(check_ptr(keys_dev, "keys_dev"));
    if (n && !values_dev) return fail(MI355_E_INVALID, "pointer values_dev is null (count(*) per value of one column: mi355_histogram_dev)");
    MI355_CHECK(check_aligned(keys_dev, 16, "keys_dev"));
    MI355_CHECK(check_aligned(values_dev, 16, "values_dev"));
    MI355_CHECK(check_aligned(mask_dev, 4, "mask_dev"));
    GroupLaunch r{};
    r.k.keys = (const uint8_t *)keys_dev;
    r.k.values = (const uint8_t *)values_dev;
    r.k.n = n;
    r.k.mask = (const uint8_t *)mask_dev;
    r.k.out = (unsigned long long *)out_dev;
    r.k.cv = cv;
    r.ck = ck;
    r.env = launch_env(ctx);
    if (n == 0) {
        launch_init(r.env, r.k.out, ck);
        HIP_TRY(hipGetLastError());
        return MI355_OK;
    }
    const hipError_t err = launch_by_width<1, kGroupMaxBits>(ck, r, [](auto c, const GroupLaunch &q) { return launch_group<decltype(c)::value>(q); });
    if (err != hipSuccess) return fail(MI355_E_HIP, "group_aggregate launch: %s", hipGetErrorString(err));
    return MI355_OK;
}
