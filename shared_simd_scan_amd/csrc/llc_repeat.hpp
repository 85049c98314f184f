// llc_repeat.hpp -- is this eq / range scan a repeat of the launch that runs directly before it?  The one place that decides: option
// "llc_resident_mib" = -1 keeps part of a column in the Infinity Cache only for a repeat, and mi355_ctx_last_llc_divisor reports a
// divisor only while the scan that chose it is the context's most recent launch.  Host bookkeeping only: no HIP, no header of the
// project; ctx.hpp holds one LlcRepeat per context, tests/cpp/llc_repeat_check.cpp drives it with g++.
//
// "Directly before" is read off the launch record (mi355_ctx_last_launch), which every kernel launch of the library extends by a line
// (MI355_LAUNCH) and the outermost compute call clears when it begins.  Two callers: Entry (ctx.hpp), outermost and kNewRecord, says
// call_begins in front of the clear; the eq / range path of capi.hip launch() asks is_repeat in front of its launch and says launched
// behind it.  No other launcher has anything to remember: its record lines, or its call, end the repeat.  Calls that neither count nor
// clear the record (kKeepRecord: memory helpers, mi355_ctx_synchronize; Locked: options, accessors) never get here: transparent.
// A compute call that launches nothing -- a refused call, n == 0 -- is still "the call directly before" and ends the repeat as well:
// the next scan runs once with D = 0.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace mi355 {

struct LlcScan {
    const void *column, *bitmap, *mask;
    uint64_t n;
    unsigned c;
    bool operator==(const LlcScan &o) const { return column == o.column && bitmap == o.bitmap && mask == o.mask && n == o.n && c == o.c; }
};

struct LlcRepeat {
    LlcScan scan = {nullptr, nullptr, nullptr, 0, 0}; // the most recent eq / range scan; column == null: not one to repeat
    unsigned long long capture = 0;                   // id of the graph capture it was recorded into, 0 = it ran eagerly
    int divisor = -1;                                 // ScanArgs::llc_d it was launched with
    uint64_t calls = 0, scan_call = 0;                // outermost compute calls so far; the one that launched that scan (0: none yet) ...
    size_t scan_end = 0;                              // ... and the length of its record right behind the scan's line

    // an outermost compute call begins; record_len: what the call that just ended left in the record
    void call_begins(size_t record_len)
    {
        if (scan_call != calls || scan_end != record_len) scan_call = 0; // that call did not end with the scan
        calls++;
    }
    // nothing was launched since the scan: no line since in its own outermost call (two scans of mi355_tune_dev), or it ended the call
    // directly before and this one is still empty (a query loop; a host-pointer flavour, whose outer call copies, then nests the _dev call)
    bool scan_is_latest(size_t record_len) const
    {
        return scan_call != 0 && (scan_call == calls ? scan_end == record_len : (scan_call + 1 == calls && record_len == 0));
    }
    // An eq / range scan is about to be launched.  The recorded scan RUNS directly before it only on the same side of a capture's
    // boundary -- a graph replays its nodes in capture order, but a captured call has not run when the capture ends and the context
    // never learns when its graph does -- so capture_id (0 = eager) must match, and nothing is a repeat while the runtime would not say.
    bool is_repeat(const LlcScan &s, bool capture_known, unsigned long long capture_id, size_t record_len) const
    {
        return capture_known && scan_is_latest(record_len) && scan.column && scan == s && capture == capture_id;
    }
    // ... and has been, with divisor d: record_len now includes its line.  Capture unknown: nothing to repeat.
    void launched(const LlcScan &s, bool capture_known, unsigned long long capture_id, int d, size_t record_len)
    {
        scan = s;
        if (!capture_known) scan.column = nullptr;
        capture = capture_id, divisor = d, scan_call = calls, scan_end = record_len;
    }
    // mi355_ctx_last_llc_divisor, asked between calls: the divisor while that scan is the context's most recent launch, else -1
    int last_divisor(size_t record_len) const { return scan_call != 0 && scan_call == calls && scan_end == record_len ? divisor : -1; }
};

} // namespace mi355
