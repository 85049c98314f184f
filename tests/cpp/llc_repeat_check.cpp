// llc_repeat_check.cpp -- csrc/llc_repeat.hpp driven through scripted call sequences.  Stand-alone: plain g++, no HIP, built and
// run under -fsanitize=undefined,address by tests/test_llc_repeat.py.
//
// Host stands in for a context as ctx.hpp and capi.hip use the struct: a launch record that grows by a line per kernel launch, an
// outermost compute call that reports the record's length and clears it, an eq / range scan that asks "repeat?" in front of its
// launch and reports its divisor behind it (kD for a repeat, 0 for anything else, as option "llc_resident_mib" = -1 gives on a
// column beyond the budget).  After every step: was the scan a repeat, and what does the introspection call report.
#include <cstdint>
#include <cstdio>

#include "llc_repeat.hpp"

using namespace mi355;

static int g_checked = 0, g_failed = 0;
#define EXPECT(cond)                                                                  \
    do {                                                                              \
        g_checked++;                                                                  \
        if (!(cond) && g_failed++ < 50) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
    } while (0)

constexpr int kD = 3;

struct Host {
    LlcRepeat llc;
    size_t record = 0; // the launch record's length
    int depth = 0;
    // MI355_ENTER(ctx) ... the entry point's return; `transparent`: kKeepRecord (memory helpers, synchronize) or Locked (options, accessors)
    void enter(bool transparent = false)
    {
        if (depth == 0 && !transparent) {
            llc.call_begins(record);
            record = 0;
        }
        if (!transparent) depth++;
    }
    void leave() { depth--; }
    void other_launch() { record += 61; } // MI355_LAUNCH of any kernel but the eq / range scan
    // capi.hip launch() of an eq / range scan, inside a call
    bool scan_launch(const LlcScan &s, bool known = true, unsigned long long capture = 0)
    {
        const bool repeat = llc.is_repeat(s, known, capture, record);
        record += 74;
        llc.launched(s, known, capture, repeat ? kD : 0, record);
        return repeat;
    }
    // a whole mi355_scan_eq_dev
    bool scan(const LlcScan &s, bool known = true, unsigned long long capture = 0)
    {
        enter();
        const bool repeat = scan_launch(s, known, capture);
        leave();
        return repeat;
    }
    // the host-pointer flavour: the outer call copies, then nests the _dev call, then copies back
    bool scan_host(const LlcScan &s)
    {
        enter();
        const bool repeat = scan(s);
        leave();
        return repeat;
    }
    void other_call() { enter(), other_launch(), leave(); }
    void empty_call() { enter(), leave(); } // refused, or n == 0
    void transparent_call() { enter(true); }
    int divisor() const { return llc.last_divisor(record); }
};

static char col_a[1], col_b[1], bits_a[1], bits_b[1], mask_a[1];
static const LlcScan A{col_a, bits_a, nullptr, 1000, 9};

// after `between`, is an identical scan a repeat; and what the divisor reads directly behind `between`
template <typename F> static void after(F between, bool repeat_expected, int divisor_expected)
{
    Host h;
    EXPECT(!h.scan(A));
    EXPECT(h.scan(A));
    EXPECT(h.divisor() == kD);
    between(h);
    EXPECT(h.divisor() == divisor_expected);
    EXPECT(h.scan(A) == repeat_expected);
    EXPECT(h.divisor() == (repeat_expected ? kD : 0));
    EXPECT(h.scan(A)); // and the one after it is a repeat again
    EXPECT(h.divisor() == kD);
}

int main()
{
    { // before any call
        Host h;
        EXPECT(h.divisor() == -1);
        h.transparent_call();
        EXPECT(h.divisor() == -1);
        h.other_call();
        EXPECT(h.divisor() == -1);
    }
    { // a first scan, an identical one, a third
        Host h;
        EXPECT(!h.scan(A));
        EXPECT(h.divisor() == 0);
        EXPECT(h.scan(A));
        EXPECT(h.divisor() == kD);
        EXPECT(h.scan(A));
        EXPECT(h.divisor() == kD);
    }
    { // one property changed: no repeat, and the changed scan is what the next one repeats
        LlcScan v[5] = {A, A, A, A, A};
        v[0].column = col_b, v[1].bitmap = bits_b, v[2].mask = mask_a, v[3].n = 1001, v[4].c = 10;
        for (const LlcScan &s : v) {
            Host h;
            EXPECT(!h.scan(A));
            EXPECT(h.scan(A));
            EXPECT(!h.scan(s));
            EXPECT(h.divisor() == 0);
            EXPECT(h.scan(s));
            EXPECT(h.divisor() == kD);
            EXPECT(!h.scan(A));
        }
        Host h; // a count-only scan (no bitmap) repeats like any other
        LlcScan count_only = A;
        count_only.bitmap = nullptr;
        EXPECT(!h.scan(count_only));
        EXPECT(h.scan(count_only));
    }
    // an identical scan after ...
    after([](Host &h) { h.other_call(); }, false, -1);          // another launch in a call of its own
    after([](Host &h) { h.empty_call(); }, false, -1);          // a call that launched nothing: ends the repeat too
    after([](Host &h) { h.transparent_call(); }, true, kD);     // kKeepRecord / Locked: transparent
    after([](Host &h) { h.transparent_call(), h.transparent_call(); }, true, kD);
    after([](Host &h) { h.other_call(), h.transparent_call(); }, false, -1);
    after([](Host &h) { h.empty_call(), h.empty_call(); }, false, -1);
    after([](Host &h) { h.scan_host(A); }, true, kD);           // the same scan through the host-pointer flavour
    after([](Host &h) { // another launch later in the scan's own outermost call (a compound call: scan, then a consumer)
              h.enter();
              EXPECT(h.scan(A));
              h.other_launch();
              h.leave();
          },
          false, -1);
    after([](Host &h) { // ... and in front of it: the call ends with the scan, but the scan was no repeat
              h.enter();
              h.other_launch();
              EXPECT(!h.scan(A));
              h.leave();
          },
          true, 0);
    { // a nested scan (outer call -> _dev call) repeated
        Host h;
        EXPECT(!h.scan_host(A));
        EXPECT(h.divisor() == 0);
        EXPECT(h.scan_host(A));
        EXPECT(h.divisor() == kD);
        EXPECT(h.scan(A)); // the _dev call on the same buffers directly behind it
        h.other_call();
        EXPECT(!h.scan_host(A));
        h.empty_call();
        EXPECT(!h.scan_host(A));
        EXPECT(h.scan_host(A));
    }
    { // identical scans inside one outermost call (mi355_tune_dev's bursts), with and without a launch between them
        Host h;
        h.enter();
        EXPECT(!h.scan(A));
        EXPECT(h.scan(A));
        EXPECT(h.scan(A));
        h.other_launch();
        EXPECT(!h.scan(A));
        EXPECT(h.scan(A));
        h.leave();
        EXPECT(h.divisor() == kD);
        EXPECT(h.scan(A)); // the call ended with the scan
        h.enter();
        EXPECT(h.scan(A));
        h.other_launch();
        h.leave();
        EXPECT(h.divisor() == -1);
        EXPECT(!h.scan(A));
    }
    { // graph capture: a repeat only on the same side of a capture's boundary
        Host h;
        EXPECT(!h.scan(A));                 // eager
        EXPECT(!h.scan(A, true, 7));        // the first call of a capture
        EXPECT(h.scan(A, true, 7));         // the id stays: the call captured before it runs directly before it
        EXPECT(h.divisor() == kD);
        EXPECT(!h.scan(A, true, 8));        // the id changes: another capture
        EXPECT(h.scan(A, true, 8));
        EXPECT(!h.scan(A));                 // eager after captured
        EXPECT(h.scan(A));
        EXPECT(!h.scan(A, false));          // unknown: no repeat ...
        EXPECT(h.divisor() == 0);
        EXPECT(!h.scan(A));                 // ... and nothing to repeat
        EXPECT(h.scan(A));
        EXPECT(!h.scan(A, false, 7));
        EXPECT(!h.scan(A, true, 7));
        h.enter();                          // two identical scans inside one capture and one call
        EXPECT(!h.scan(A, true, 9));
        EXPECT(h.scan(A, true, 9));
        h.leave();
    }
    printf("%d checks, %d failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
