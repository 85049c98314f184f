// predicate_norm_check.cpp -- csrc/predicate_norm.hpp against plain int64 comparisons.  Stand-alone: plain g++, no HIP, built
// and run under -fsanitize=undefined,address by tests/test_predicate_norm.py.
//
// For every width, every comparison and constants at every boundary of the arithmetic, the test the kernels make,
// ((uint32)(x - lo) <= span) != invert, must give what `x OP a [, b]` gives on int64; the same for the difference of two columns
// (64-bit test at every width pair, 32-bit test where both widths are <= 30); and a predicate goes to the equality-key path only
// with a key that the equality kernel's compare, (uint32)key == x, answers as the predicate.
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "predicate_norm.hpp"

using namespace mi355;

static unsigned long long g_checked = 0, g_failed = 0;

static bool truth(int op, int64_t x, int64_t a, int64_t b)
{
    switch (op) {
    case MI355_CMP_EQ: return x == a;
    case MI355_CMP_NE: return x != a;
    case MI355_CMP_LT: return x < a;
    case MI355_CMP_LE: return x <= a;
    case MI355_CMP_GT: return x > a;
    case MI355_CMP_GE: return x >= a;
    case MI355_CMP_BETWEEN: return x >= a && x <= b;
    default: return !(x >= a && x <= b);
    }
}

static void expect(bool ok, const char *what, unsigned c1, unsigned c2, int op, int64_t a, int64_t b, int64_t x)
{
    g_checked++;
    if (ok) return;
    if (g_failed++ < 20) fprintf(stderr, "%s: c1=%u c2=%u op=%d a=%lld b=%lld x=%lld\n", what, c1, c2, op, (long long)a, (long long)b, (long long)x);
}

// constants around every boundary of the clamps and of the domain [dmin, dmax]
static std::vector<int64_t> constants(int64_t dmin, int64_t dmax)
{
    const int64_t p33 = 1ll << 33, p32 = 1ll << 32, p31 = 1ll << 31;
    std::set<int64_t> s = {INT64_MIN, INT64_MIN + 1, -p33 - 1, -p33, -p33 + 1, p33 - 1, p33, p33 + 1, -p32, -2, -1, 0, 1, 2,
                           dmax / 2, dmax - 1, dmax, dmax + 1, dmax + 2, p31 - 1, p31, p32 - 2, p32 - 1, p32, p32 + 1, INT64_MAX - 1, INT64_MAX,
                           dmin - 1, dmin, dmin + 1};
    return std::vector<int64_t>(s.begin(), s.end());
}

// values at 0, 1, 2, the middle +- 1 and the top three, shifted to start at dmin
static std::vector<int64_t> values(int64_t dmin, int64_t dmax)
{
    const int64_t mid = dmin + (dmax - dmin) / 2;
    std::set<int64_t> s;
    for (int64_t x : {dmin, dmin + 1, dmin + 2, mid - 1, mid, mid + 1, dmax - 2, dmax - 1, dmax, (int64_t)0, (int64_t)-1, (int64_t)1})
        if (x >= dmin && x <= dmax) s.insert(x);
    return std::vector<int64_t>(s.begin(), s.end());
}

static void check_value_tests()
{
    for (unsigned c = 1; c <= 32; c++) {
        const int64_t vmax = width_max(c);
        const std::vector<int64_t> ks = constants(0, vmax), xs = values(0, vmax);
        for (int op = MI355_CMP_EQ; op <= MI355_CMP_NOT_BETWEEN; op++)
            for (int64_t a : ks)
                for (int64_t b : ks) {
                    if (op < MI355_CMP_BETWEEN && b != ks[0]) break; // b is read by the two BETWEENs only
                    const ValueTest t = normalise_predicate(c, op, a, b);
                    expect(t.invert == 0 || t.invert == 0xffffffffu, "invert word", c, 0, op, a, b, 0);
                    for (int64_t x : xs) {
                        const bool got = ((uint32_t)((uint32_t)x - t.lo) <= t.span) != (t.invert != 0);
                        expect(got == truth(op, x, a, b), "value test", c, 0, op, a, b, x);
                    }
                    // the equality-key rule
                    int32_t key = 0;
                    if (equality_key(c, op, a, &key)) {
                        expect(op == MI355_CMP_EQ, "key for a non-equality", c, 0, op, a, b, 0);
                        for (int64_t x : xs) expect(((uint32_t)key == (uint32_t)x) == truth(op, x, a, b), "equality key", c, 0, op, a, b, x);
                    }
                }
    }
}

static void check_difference_tests()
{
    for (unsigned c1 = 1; c1 <= 32; c1++)
        for (unsigned c2 : std::set<unsigned>{1, 2, c1, 30, 31, 32}) {
            const int64_t dmin = -((1ll << c2) - 1), dmax = (1ll << c1) - 1;
            const std::vector<int64_t> ks = constants(dmin, dmax), ds = values(dmin, dmax);
            for (int op = MI355_CMP_EQ; op <= MI355_CMP_NOT_BETWEEN; op++)
                for (int64_t a : ks)
                    for (int64_t b : ks) {
                        if (op < MI355_CMP_BETWEEN && b != ks[0]) break;
                        const DifferenceTest t = normalise_difference(c1, c2, op, a, b);
                        expect(t.lo64 >= dmin && (uint64_t)(dmax - t.lo64) >= t.span64, "lo <= hi inside the domain", c1, c2, op, a, b, 0);
                        for (int64_t d : ds) {
                            const bool want = truth(op, d, a, b);
                            const bool wide = ((uint64_t)(d - t.lo64) <= t.span64) != (t.invert != 0);
                            expect(wide == want, "64-bit difference test", c1, c2, op, a, b, d);
                            if (c1 <= 30 && c2 <= 30) {
                                const bool narrow = ((uint32_t)((uint32_t)(uint64_t)d - t.lo) <= t.span) != (t.invert != 0);
                                expect(narrow == want, "32-bit difference test", c1, c2, op, a, b, d);
                            }
                        }
                    }
        }
}

int main()
{
    check_value_tests();
    check_difference_tests();
    printf("%llu comparisons, %llu failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
