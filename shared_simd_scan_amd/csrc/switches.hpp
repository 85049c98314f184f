// switches.hpp -- the A/B switches of option "kernel_flags" (env MI355_KERNEL_FLAGS), every one once: what a caller sets (the option
// value), the bit of ScanArgs::flags its receiver tests, and what it selects.  They never change a result (but the two timing
// ablations of the selection).  The selection's kernel bits coincide with four of the shared scans': a launch carries one
// receiver's word only, select*.hpp use only the kSel names and everything else only kSw / kSet.  Host and device code.
#pragma once

#include <stdint.h>

namespace mi355 {

enum SwitchReceiver { kRecvShared, kRecvSelect, kRecvLauncherSet, kRecvReserved };
constexpr const char *kSwitchReceiverName[] = {"shared", "select", "launcher-set", "reserved"};

// X(name, option value, kernel-side bit, receiver, meaning); option value 0: no caller sets it, the launcher does (SharedPlan::flag)
#define MI355_SWITCHES(X)                                                                                                                 \
    X(kSwDrainEveryTile, 1, 0x1, kRecvShared, "shared_wide_kernel / shared_wide2_kernel drain their stores every tile")                   \
    X(kSwPerGroupKernels, 2, 0x2, kRecvShared, "the per-group kernels instead of shared_wide2 / shared_linear")                           \
    X(kSwRotateRounds, 4, 0x4, kRecvShared, "rotate the 32-key rounds between waves")                                                     \
    X(kSwCountsByReduction, 8, 0x8, kRecvShared, "hit counts by per-tile wave reductions / the histogram instead of registers")           \
    X(kSwP16OneRowPerPiece, 16, 0x10, kRecvShared, "P = 16 linear: one row per piece")                                                    \
    X(kSwPairOnLut, 32, 0x20, kRecvShared, "P = 2 on the LUT kernel")                                                                     \
    X(kSwCompareChain, 64, 0x40, kRecvShared, "compare chain instead of the tables")                                                      \
    X(kSwLinearAnyWidth, 128, 0x80, kRecvShared, "the row-per-lane linear kernel whatever the width")                                     \
    X(kSwLinearRound2, 256, 0x100, kRecvShared, "round 2's shared_linear_kernel instead of shared_linear2_kernel")                        \
    X(kSwByteDigits, 8192, 0x200, kRecvShared, "byte digits instead of the wider ones (BIG off)")                                         \
    X(kSwChainRuleRound2, 16384, 0x400, kRecvShared, "round 2's chain rule at c >= 17")                                                   \
    X(kSwWide2, 32768, 0x800, kRecvShared, "shared_wide2_kernel instead of shared_wide3_kernel")                                          \
    X(kSwReserved, 65536, 0x1000, kRecvReserved, "read nowhere, reaches no kernel")                                                       \
    X(kSwNoLinear3, 131072, 0x2000, kRecvShared, "no shared_linear3_kernel")                                                              \
    X(kSwNoImage, 262144, 0x4000, kRecvShared, "no aligned output image")                                                                 \
    X(kSwLinear2Short, 524288, 0x8000, kRecvShared, "shared_linear2_kernel attached for rows of 33 .. 56 keys")                           \
    X(kSwShortNeverAttached, 1048576, 0x10000, kRecvShared, "the short last table never attached")                                        \
    X(kSwShortAlwaysAttached, 4194304, 0x40000, kRecvShared, "the short last table always attached")                                      \
    X(kSwImageAnyLength, 8388608, 0x80000, kRecvShared, "the aligned image at every row length")                                          \
    X(kSetShortAttached, 0, 0x20000, kRecvLauncherSet, "the short last table attached (shared_linear2_kernel)")                           \
    X(kSetImage, 0, 0x100000, kRecvLauncherSet, "the aligned output image (shared_linear_kernel)")                                        \
    X(kSelNoExpansion, 512, 0x2, kRecvSelect, "timing ablation: no expansion (wrong ids by construction)")                                \
    X(kSelNoLookBack, 1024, 0x4, kRecvSelect, "timing ablation: no look-back (wrong ids by construction)")                                \
    X(kSelByBlockIndex, 2048, 0x8, kRecvSelect, "select_kernel: chunks dealt out by block index")                                         \
    X(kSelNoBarrier, 4096, 0x10, kRecvSelect, "select_kernel: no per-generation barrier (with kSelByBlockIndex)")

#define MI355_SWITCH_CONSTANT(name, option, kbit, receiver, meaning) constexpr uint32_t name = kbit;
MI355_SWITCHES(MI355_SWITCH_CONSTANT)
#undef MI355_SWITCH_CONSTANT

struct SwitchRow {
    const char *name;
    uint32_t option, kbit;
    SwitchReceiver receiver;
    const char *meaning;
};
#define MI355_SWITCH_ROW(name, option, kbit, receiver, meaning) {#name, option, kbit, receiver, meaning},
constexpr SwitchRow kSwitches[] = {MI355_SWITCHES(MI355_SWITCH_ROW)};
#undef MI355_SWITCH_ROW

// the word a receiver's kernels and launcher see for an option value: the one place where option value and kernel bit differ.
// Option bits of no row, of the reserved row or of the other receiver reach nothing.
constexpr uint32_t kernel_switch_word(unsigned option, bool select)
{
    uint32_t word = 0;
    for (const SwitchRow &s : kSwitches)
        if (s.receiver == (select ? kRecvSelect : kRecvShared) && (option & s.option)) word |= s.kbit;
    return word;
}

} // namespace mi355
