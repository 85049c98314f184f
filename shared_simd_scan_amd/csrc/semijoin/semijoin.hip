// semijoin.hip -- implementation of include/mi355_semijoin.h: argument checks, the choice between the two tiers and the launch
// of semijoin_lds_kernel / semijoin_global_kernel (semijoin/semijoin.hpp) by width.  Its own translation unit: neither the other
// entry points nor the width groups rebuild with it.  The launch itself is launch_tier (launch_util.hpp) on a LaunchEnv (ctx.hpp),
// shared with lookup/.
#include "../ctx.hpp"

#include "../../../include/mi355_semijoin.h"
#include "../checks.hpp"
#include "../dispatch.hpp"
#include "../launch_util.hpp"
#include "semijoin.hpp"

using namespace mi355;

namespace {

static_assert(semijoin_lds_max_bits() == MI355_SEMIJOIN_LDS_MAX_BITS, "the header's limit is the kernels'");

constexpr uint64_t kSemiMaxSetBits = 1ull << 32;

struct SemiLaunch {
    SemiArgs k;
    unsigned c;
    bool in_lds;
    int store_policy; // one_pass_store_policy: 1 non-temporal, else write-through
    LaunchEnv env;
};

template <int C> hipError_t launch_semijoin(const SemiLaunch &r)
{
    using G = ScanGeom<C, scan_vpl(C, kModeEq)>;
    const uint64_t ntiles = (r.k.s.n + G::TILE_VALUES - 1) / G::TILE_VALUES;
    const bool nt = r.store_policy == 1;
    constexpr size_t fixed = semijoin_static_lds<C>() + 16u; // tiles, mask images, hits_finalize's flag
    if (r.in_lds) {
        const size_t lds = semijoin_dyn_lds(r.k.set_bytes);
        const int max_dyn = (int)(kCuLdsBytes - fixed);
        nt ? launch_tier<semijoin_lds_kernel<C, 18>>(r.env, r.k, ntiles, lds, fixed, max_dyn) : launch_tier<semijoin_lds_kernel<C, 34>>(r.env, r.k, ntiles, lds, fixed, max_dyn);
    } else {
        if constexpr (C >= kSemiGlobalMinBits)
            nt ? launch_tier<semijoin_global_kernel<C, 18>>(r.env, r.k, ntiles, 0, fixed, 0) : launch_tier<semijoin_global_kernel<C, 34>>(r.env, r.k, ntiles, 0, fixed, 0);
        else
            return hipErrorInvalidValue; // semijoin_in_lds() is true below kSemiGlobalMinBits
    }
    return hipGetLastError();
}

} // namespace

const char *mi355_semijoin_kernel(unsigned c, uint64_t set_bits)
{
    if (c < 1 || c > 32 || set_bits > kSemiMaxSetBits) return nullptr;
    return semijoin_in_lds(c, set_bits) ? "semijoin_lds_kernel" : "semijoin_global_kernel";
}

int mi355_semijoin_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const void *set_dev, uint64_t set_bits, int negate,
                       const void *and_mask_dev, void *bitmap_dev, uint64_t *hits_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(c));
    if (set_bits > kSemiMaxSetBits) return fail(MI355_E_INVALID, "set_bits=%llu beyond 2^32", (unsigned long long)set_bits);
    MI355_CHECK(check_some_output(bitmap_dev, hits_dev));
    if (set_bits) MI355_CHECK(check_ptr(set_dev, "set_dev"));
    MI355_CHECK(check_aligned(set_dev, 4, "set_dev"));
    MI355_CHECK(check_aligned(bitmap_dev, 16, "bitmap_dev"));
    MI355_CHECK(check_aligned(and_mask_dev, 16, "and_mask_dev"));
    MI355_CHECK(check_aligned(hits_dev, 8, "hits_dev"));
    if (set_dev && ranges_overlap(set_dev, (set_bits + 7) / 8, bitmap_dev, bitmap_bytes(n)))
        return fail(MI355_E_INVALID, "set_dev overlaps bitmap_dev: the set is read while the bitmap is written");
    if (n == 0) {
        if (hits_dev) HIP_TRY(hipMemsetAsync(hits_dev, 0, sizeof(uint64_t), ctx->stream));
        return MI355_OK;
    }
    MI355_CHECK(check_dev(packed_dev, 16, "packed_dev"));
    const uint64_t reach = value_reach(c, set_bits); // what a c-bit value can address of the set
    SemiLaunch r{};
    r.k.s.packed = (const uint8_t *)packed_dev;
    r.k.s.n = n;
    r.k.s.out = (uint8_t *)bitmap_dev;
    r.k.s.hits = (unsigned long long *)hits_dev;
    r.k.s.scratch = ctx->kernel_scratch;
    r.k.s.nkeys = 1;
    r.k.s.and_mask = (const uint8_t *)and_mask_dev;
    r.k.s.invert = negate ? 0xffffffffu : 0u;
    r.k.set = (const uint8_t *)set_dev;
    r.k.set_bytes = (uint32_t)((reach + 7) / 8);
    r.k.limit = reach ? (uint32_t)(reach - 1) : 0u;
    r.k.last_keep = (reach & 7) ? ((1u << (reach & 7)) - 1u) : 0xffu;
    r.c = c;
    r.in_lds = semijoin_in_lds(c, set_bits);
    r.store_policy = one_pass_store_policy(n / 8, ctx->scan_nt_stores);
    r.env = launch_env(ctx);
    const hipError_t err = launch_by_width<1, 32>(c, r, [](auto w, const SemiLaunch &q) { return launch_semijoin<decltype(w)::value>(q); });
    if (err != hipSuccess) return fail(MI355_E_HIP, "semijoin launch: %s", hipGetErrorString(err));
    return MI355_OK;
}
