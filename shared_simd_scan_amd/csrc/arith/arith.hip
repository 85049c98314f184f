// arith.hip -- implementation of include/mi355_arith.h: argument checks and the range rule that chooses between
// arith_exact_kernel and arith_checked_kernel (arith/arith.hpp).  Its own translation unit: neither the other entry points nor the
// width groups rebuild with it.  Host code only: the 32 widths of each kernel are compiled and launched by arith_kernels.hip, once
// per kernel (arith_launch.hpp) -- ten forms of the expression in each of 64 kernels are four minutes of compile time in one unit.
#include "../ctx.hpp"

#include "../../../include/mi355_arith.h"
#include "../checks.hpp"
#include "../launch_util.hpp" // one_pass_store_policy
#include "arith_launch.hpp"

using namespace mi355;

namespace {

static_assert(kArithLinear == MI355_ARITH_LINEAR && kArithMul == MI355_ARITH_MUL, "the header's operations are the kernels'");

enum ArithPlan { kArithRefused = 0, kArithExact, kArithChecked };

// The range rule: [lo, hi] bounds r over all x < 2^c1, y < 2^c2, in 128 bits (|a X Y| < 2^31 2^64).  `why` (nullable) gets the refusal.
ArithPlan arith_plan(int op, unsigned c1, unsigned c2, int32_t a, int32_t b, int64_t k, unsigned co, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = nullptr;
    if (op != MI355_ARITH_LINEAR && op != MI355_ARITH_MUL) *why = "op is neither MI355_ARITH_LINEAR nor MI355_ARITH_MUL";
    else if (c1 < 1 || c1 > 32 || c2 < 1 || c2 > 32 || co < 1 || co > 32) *why = "a bit width (c1, c2, co) outside 1..32";
    else if (op == MI355_ARITH_MUL && b != 0) *why = "b must be 0 with MI355_ARITH_MUL";
    if (*why) return kArithRefused;
    const __int128 X = ((__int128)1 << c1) - 1, Y = ((__int128)1 << c2) - 1;
    __int128 lo = k, hi = k;
    auto term = [&](__int128 t) { (t < 0 ? lo : hi) += t; };
    if (op == MI355_ARITH_MUL) {
        term((__int128)a * X * Y);
    } else {
        term((__int128)a * X);
        term((__int128)b * Y);
    }
    if (lo < (__int128)INT64_MIN || hi > (__int128)INT64_MAX) {
        *why = "the result's range [lo, hi] over all inputs leaves int64: 64-bit arithmetic would not be exact";
        return kArithRefused;
    }
    return lo >= 0 && hi <= ((__int128)1 << co) - 1 ? kArithExact : kArithChecked;
}

} // namespace

const char *mi355_arith_kernel(int op, unsigned c1, unsigned c2, int32_t a, int32_t b, int64_t k, unsigned co)
{
    switch (arith_plan(op, c1, c2, a, b, k, co, nullptr)) {
    case kArithExact: return "arith_exact_kernel";
    case kArithChecked: return "arith_checked_kernel";
    default: return nullptr;
    }
}

int mi355_arith_dev(mi355_ctx *ctx, int op, const void *packed1_dev, unsigned c1, const void *packed2_dev, unsigned c2, uint64_t n, int32_t a,
                    int32_t b, int64_t k, unsigned co, uint32_t miss, void *out_dev, uint64_t *out_of_range_dev)
{
    MI355_ENTER(ctx);
    if (op != MI355_ARITH_LINEAR && op != MI355_ARITH_MUL) return fail(MI355_E_INVALID, "op=%d is neither MI355_ARITH_LINEAR nor MI355_ARITH_MUL", op);
    MI355_CHECK(check_width(c1, "c1"));
    MI355_CHECK(check_width(c2, "c2"));
    MI355_CHECK(check_width(co, "co"));
    if (co < 32 && (miss >> co)) return fail(MI355_E_INVALID, "miss=%u is no value of co=%u bits", miss, co);
    const char *why = nullptr;
    const ArithPlan plan = arith_plan(op, c1, c2, a, b, k, co, &why);
    if (plan == kArithRefused) return fail(MI355_E_INVALID, "arith (a=%d, b=%d, k=%lld, c1=%u, c2=%u): %s", a, b, (long long)k, c1, c2, why);
    MI355_CHECK(check_aligned(out_of_range_dev, 8, "out_of_range_dev"));
    if (n) {
        MI355_CHECK(check_dev(packed1_dev, 16, "packed1_dev"));
        MI355_CHECK(check_dev(packed2_dev, 16, "packed2_dev"));
        MI355_CHECK(check_dev(out_dev, 16, "out_dev"));
    }
    const uint64_t out_bytes = packed_bytes(n, co);
    MI355_CHECK(check_no_overlap(out_dev, out_bytes, "out_dev", packed1_dev, packed_bytes(n, c1), "packed1_dev", "column"));
    MI355_CHECK(check_no_overlap(out_dev, out_bytes, "out_dev", packed2_dev, packed_bytes(n, c2), "packed2_dev", "column"));
    // the counter starts from 0: all the exact kernel and an empty column leave in it
    if (out_of_range_dev) HIP_TRY(hipMemsetAsync(out_of_range_dev, 0, sizeof(uint64_t), ctx->stream));
    if (n == 0) return MI355_OK;
    ArithLaunch r{};
    r.k.packed1 = (const uint8_t *)packed1_dev;
    r.k.packed2 = (const uint8_t *)packed2_dev;
    r.k.n = n;
    r.k.out = (uint8_t *)out_dev;
    r.k.out_of_range = (unsigned long long *)out_of_range_dev;
    r.k.k = k;
    r.k.a = a;
    r.k.b = b;
    r.k.c1 = c1;
    r.k.c2 = c2;
    r.k.mode = arith_mode((uint32_t)op, a, b);
    r.k.miss = miss;
    r.k.nts = (uint32_t)one_pass_store_policy(out_bytes, ctx->scan_nt_stores);
    r.env = launch_env(ctx);
    const hipError_t err = plan == kArithChecked ? launch_arith_checked(co, r) : launch_arith_exact(co, r);
    if (err != hipSuccess) return fail(MI355_E_HIP, "arith launch: %s", hipGetErrorString(err));
    return MI355_OK;
}
