// value_set.hip -- the mi355_value_set_dev half of include/mi355_distinct.h: argument checks, the clear, the choice between the two
// tiers and the launch of value_set_lds_kernel / value_set_global_kernel (distinct/value_set.hpp) by width.  Its own translation
// unit: neither the other entry points nor the width groups rebuild with it.  The launch itself is launch_tier (launch_util.hpp) on
// a LaunchEnv (ctx.hpp), shared with semijoin/ and lookup/.
#include "../ctx.hpp"

#include "../../../include/mi355_distinct.h"
#include "../checks.hpp"
#include "../dispatch.hpp"
#include "../launch_util.hpp"
#include "value_set.hpp"

using namespace mi355;

namespace {

static_assert(kValueSetLdsMaxBits == MI355_VALUE_SET_LDS_MAX_BITS, "the header's limit is the kernels'");
static_assert(MI355_VALUE_SET_LDS_MAX_BITS >= (1 << 16) && MI355_VALUE_SET_LDS_MAX_BITS <= 753152, "between a 16-bit domain and the semi-join's ceiling");

constexpr uint64_t kValueSetMaxSetBits = 1ull << 32;

struct ValueSetLaunch {
    ValueSetArgs k;
    bool in_lds;
    LaunchEnv env;
};

template <int C> hipError_t launch_value_set(const ValueSetLaunch &r)
{
    using G = ScanGeom<C, scan_vpl(C, kModeEq)>;
    const uint64_t ntiles = (r.k.n + G::TILE_VALUES - 1) / G::TILE_VALUES;
    constexpr size_t fixed = value_set_static_lds<C>() + 16u;
    if (r.in_lds) {
        constexpr int max_dyn = (int)value_set_dyn_lds((uint32_t)(kValueSetLdsMaxBits / 32));
        launch_tier<value_set_lds_kernel<C>>(r.env, r.k, ntiles, value_set_dyn_lds(r.k.words), fixed, max_dyn);
    } else {
        if constexpr (C >= kValueSetGlobalMinBits)
            launch_tier<value_set_global_kernel<C>>(r.env, r.k, ntiles, 0, fixed, 0);
        else
            return hipErrorInvalidValue; // value_set_in_lds() is true below kValueSetGlobalMinBits
    }
    return hipGetLastError();
}

} // namespace

const char *mi355_value_set_kernel(unsigned c, uint64_t set_bits)
{
    if (c < 1 || c > 32 || set_bits > kValueSetMaxSetBits) return nullptr;
    return value_set_in_lds(c, set_bits) ? "value_set_lds_kernel" : "value_set_global_kernel";
}

int mi355_value_set_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const void *mask_dev, void *set_dev, uint64_t set_bits,
                        int accumulate, uint64_t *out_dev)
{
    MI355_ENTER(ctx);
    MI355_CHECK(check_width(c));
    if (set_bits > kValueSetMaxSetBits) return fail(MI355_E_INVALID, "set_bits=%llu beyond 2^32", (unsigned long long)set_bits);
    MI355_CHECK(check_dev(out_dev, 8, "out_dev"));
    if (set_bits) MI355_CHECK(check_ptr(set_dev, "set_dev"));
    MI355_CHECK(check_aligned(set_dev, 4, "set_dev"));
    MI355_CHECK(check_aligned(packed_dev, 16, "packed_dev"));
    MI355_CHECK(check_aligned(mask_dev, 4, "mask_dev"));
    if (n) MI355_CHECK(check_ptr(packed_dev, "packed_dev"));
    const uint64_t set_bytes = (set_bits + 7) / 8;
    if (set_dev) {
        MI355_CHECK(check_no_overlap(set_dev, set_bytes, "set_dev", packed_dev, packed_dev ? packed_bytes(n, c) : 0, "packed_dev", "column"));
        MI355_CHECK(check_no_overlap(set_dev, set_bytes, "set_dev", mask_dev, mask_dev ? bitmap_bytes(n) : 0, "mask_dev", "mask"));
        if (ranges_overlap(set_dev, set_bytes, out_dev, 2 * sizeof(uint64_t))) return fail(MI355_E_INVALID, "set_dev overlaps out_dev");
    }
    if (!accumulate && set_bytes) HIP_TRY(hipMemsetAsync(set_dev, 0, set_bytes, ctx->stream));
    HIP_TRY(hipMemsetAsync(out_dev, 0, 2 * sizeof(uint64_t), ctx->stream));
    if (n == 0) return MI355_OK;
    const uint64_t reach = value_reach(c, set_bits); // what a c-bit value can address of the set
    ValueSetLaunch r{};
    r.k.packed = (const uint8_t *)packed_dev;
    r.k.n = n;
    r.k.mask = (const uint8_t *)mask_dev;
    r.k.set = (uint32_t *)set_dev;
    r.k.out = (unsigned long long *)out_dev;
    r.in_lds = value_set_in_lds(c, set_bits);
    r.k.bound = r.in_lds ? (uint32_t)reach : (uint32_t)(reach - 1);
    r.k.words = r.in_lds ? (uint32_t)((reach + 31) / 32) : 0u;
    r.env = launch_env(ctx);
    const hipError_t err = launch_by_width<1, 32>(c, r, [](auto w, const ValueSetLaunch &q) { return launch_value_set<decltype(w)::value>(q); });
    if (err != hipSuccess) return fail(MI355_E_HIP, "value_set launch: %s", hipGetErrorString(err));
    return MI355_OK;
}
