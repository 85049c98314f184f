// predicate_norm.hpp -- (op, a, b) -> what the kernels compare with.  Host arithmetic only: no HIP, no kernel argument
// structs; capi.hip copies the results into ScanArgs / ColumnsArgs / WhereReq, tests/cpp/predicate_norm_check.cpp checks them
// against plain int64 comparisons with g++.
//
// Every kernel tests one inclusive range, possibly negated: ((uint32)(x - lo) <= span) != invert.
#pragma once

#include <stdint.h>

#include "../../include/mi355_scan.h"

namespace mi355 {

struct OpRange {
    int64_t lo, hi; // inclusive, clipped to the domain; lo > hi: the comparison holds for no value of the domain
    bool invert;
};

// the one switch over the comparisons: `x OP a [, b]` over the domain [dmin, dmax] as a range of x and a negation.
// a and b are clamped to [limit_lo, limit_hi] first: limits outside the domain on both sides change no comparison and keep
// a - 1 / a + 1 from overflowing.
inline OpRange op_range(int op, int64_t a, int64_t b, int64_t dmin, int64_t dmax, int64_t limit_lo, int64_t limit_hi)
{
    a = a < limit_lo ? limit_lo : (a > limit_hi ? limit_hi : a);
    b = b < limit_lo ? limit_lo : (b > limit_hi ? limit_hi : b);
    OpRange r{dmin, dmax, false};
    switch (op) {
    case MI355_CMP_EQ: r.lo = r.hi = a; break;
    case MI355_CMP_NE: r.lo = r.hi = a; r.invert = true; break;
    case MI355_CMP_LT: r.hi = a - 1; break;
    case MI355_CMP_LE: r.hi = a; break;
    case MI355_CMP_GT: r.lo = a + 1; break;
    case MI355_CMP_GE: r.lo = a; break;
    case MI355_CMP_BETWEEN: r.lo = a; r.hi = b; break;
    case MI355_CMP_NOT_BETWEEN: r.lo = a; r.hi = b; r.invert = true; break;
    }
    if (r.lo < dmin) r.lo = dmin;
    if (r.hi > dmax) r.hi = dmax;
    return r;
}

inline int64_t width_max(unsigned c) { return c == 32 ? 0xffffffffll : ((1ll << c) - 1); }

// ---- one column: x in [0, 2^c) ----
struct ValueTest {
    uint32_t lo, span, invert; // invert: 0 or 0xffffffff
};

// a and b may be any int64: clamped to [-1, 2^32], which changes no comparison with a value in [0, 2^32)
inline ValueTest normalise_predicate(unsigned c, int op, int64_t a, int64_t b)
{
    const OpRange r = op_range(op, a, b, 0, width_max(c), -1, 1ll << 32);
    if (r.lo <= r.hi) return {(uint32_t)r.lo, (uint32_t)(r.hi - r.lo), r.invert ? 0xffffffffu : 0u};
    // matches nothing (or, negated, everything).  lo above every value: x - lo is never <= span 0 unless x == 0xffffffff,
    // which needs c == 32 ...
    if (c < 32) return {0xffffffffu, 0u, r.invert ? 0xffffffffu : 0u};
    return {0u, 0xffffffffu, r.invert ? 0u : 0xffffffffu}; // ... so there the full range with the negation flipped
}

// ---- the row-wise difference of two columns: d = v1 - v2 in [-(2^c2 - 1), 2^c1 - 1] ----
struct DifferenceTest {
    int64_t lo64;      // the 64-bit test: every width pair
    uint64_t span64;
    uint32_t lo, span; // the 32-bit test: exact when both widths are <= 30 (lo fits an int32, the span 31 bits)
    uint32_t invert;
};

// a and b may be any int64: clamped to [-2^33, 2^33], outside every domain on both sides.  A range that misses the domain
// is the full range with the negation flipped, so lo <= hi always and hi - lo <= 2^33 - 2: no encoding of "empty".
inline DifferenceTest normalise_difference(unsigned c1, unsigned c2, int op, int64_t a, int64_t b)
{
    const int64_t dmin = -((1ll << c2) - 1), dmax = (1ll << c1) - 1;
    OpRange r = op_range(op, a, b, dmin, dmax, -(1ll << 33), 1ll << 33);
    if (r.lo > r.hi) r = {dmin, dmax, !r.invert};
    // lo: two's complement low word, (int32)lo when both widths are <= 30
    return {r.lo, (uint64_t)(r.hi - r.lo), (uint32_t)(uint64_t)r.lo, (uint32_t)(r.hi - r.lo), r.invert ? 0xffffffffu : 0u};
}

// ---- a list of predicates through the equality machinery (mi355_shared_scan_where_dev) ----
// Is `x OP a` an equality that an int32 key of the shared equality scan can carry, and which key?  A constant outside the
// column's domain matches nothing: key -1, which is no value below c = 32 (at c = 32 it is one, so such a list is not routed).
inline bool equality_key(unsigned c, int op, int64_t a, int32_t *key)
{
    if (op != MI355_CMP_EQ) return false;
    const bool outside = a < 0 || a > width_max(c);
    if (outside ? c == 32 : a > 0x7fffffffll) return false;
    *key = outside ? -1 : (int32_t)a;
    return true;
}

} // namespace mi355
