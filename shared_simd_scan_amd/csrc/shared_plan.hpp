// shared_plan.hpp -- which kernel an equality shared scan of P >= 2 keys runs, decided ONCE: plan_shared<C>() is a pure
// function of the request (no HIP call, no static), read top to bottom in priority order.  launch_shared<C>() in
// width_group.hip launches what the plan says; mi355_shared_scan_kernel reports the plan's family.
#pragma once

#include "kernels.hpp"
#include "launch_util.hpp"

namespace mi355 {

// kernel families of a shared scan, as mi355_shared_scan_kernel names them (P = 1 never comes here: scan_burst_kernel)
enum SharedFamily { kFamLut = 0, kFamLutMulti = 1, kFamWide = 2, kFamGeneral = 3, kFamLinear = 4, kFamPair = 5 };
constexpr const char *kSharedFamilyName[] = {"shared_lut_kernel",     "shared_lut_kernel(multi-pass)", "shared_wide_kernel",
                                             "shared_general_kernel", "shared_linear_kernel",          "shared_pair_kernel"};

// the concrete forms, in the priority order of plan_shared(): shared_pair_kernel; shared_lut_kernel in one pass; shared_linear3_kernel;
// shared_lut_kernel with byte-entry tables in several passes; shared_general_kernel; shared_linear_kernel with two rows per 32-byte
// piece / with or without the aligned output image; shared_linear2_kernel with the short last table attached or detached;
// shared_wide3_kernel; shared_wide2_kernel; shared_wide_kernel for per-predicate bitmaps / for linear rows
enum SharedForm { kFormPair, kFormLut, kFormLinear3, kFormLutMulti, kFormChain, kFormLinearTwoRows, kFormLinear, kFormLinear2,
                  kFormWide3, kFormWide2, kFormWide, kFormWideLinear, kNumSharedForms };
// the one table form -> public family
constexpr SharedFamily kSharedFamilyOf[kNumSharedForms] = {kFamPair,   kFamLut,    kFamLinear, kFamLutMulti, kFamGeneral, kFamLinear,
                                                           kFamLinear, kFamLinear, kFamWide,   kFamWide,     kFamWide,    kFamWide};

struct SharedPlan {
    SharedForm form;
    SharedFamily family;
    int want_bpc;           // blocks per CU; where the launch asks the occupancy query, the smaller of the two; 0 = what that admits
    int vpl;                // values per lane and tile
    int rc = 0;             // hit counts in registers: 0 no, 1 one 32-key round in 32-bit registers, 2 two rounds in packed 16-bit halves
    bool big = false;       // wider table digits (WideLutGeom<C, true>)
    int store = 0;          // result stores: 0 plain, 1 non-temporal, 2 write-through
    size_t dyn_lds = 0;     // dynamic LDS bytes
    uint32_t set_flags = 0; // the launcher's own switch for the kernel: kSetShortAttached or kSetImage (switches.hpp)
    SharedPlan &lds(size_t bytes) { dyn_lds = bytes; return *this; }
    SharedPlan &stores(int policy) { store = policy; return *this; }
    SharedPlan &counters(int rc_, bool big_) { rc = rc_, big = big_; return *this; }
    SharedPlan &flag(uint32_t bits) { set_flags = bits; return *this; }
};
inline SharedPlan make_plan(SharedForm form, int want_bpc, int vpl = 64) { return SharedPlan{form, kSharedFamilyOf[form], want_bpc, vpl}; }

// ---- LDS budgets ---------------------------------------------------------------------------------------------------------

constexpr int kSharedVpl = scan_vpl(0, kModeShared); // 64 values per lane and tile, but for the pair and the one-pass LUT kernels

// static LDS of the multi-pass LUT kernel: four tiles, the per-block hit counters, ticket word and slack
template <int C, int VPL> constexpr size_t lut_static_lds()
{
    // + the hit-count histogram
    return 4 * ScanGeom<C, VPL>::LDS_BYTES + kMaxKeys * 4 + 512 + (C <= 12 ? (size_t)(4u << C) : 16);
}
// what the kernels with tables in dynamic LDS may be given
template <int C> constexpr int shared_max_dyn_lds() { return (int)(kCuLdsBytes - lut_static_lds<C, kSharedVpl>()); }

// one dword-entry table per 32 keys (WideLutGeom) / one byte-entry table per 8 keys (LutGeom<C, true>), in dynamic LDS
template <int C, bool BIG = false> constexpr size_t wide_table_bytes(uint32_t P) { return (size_t)((P + 31) / 32) * WideLutGeom<C, BIG>::TABLE_BYTES; }
template <int C> constexpr size_t lut8_table_bytes(uint32_t P) { return ((size_t)((P + 7) / 8) * LutGeom<C, true>::TABLE_BYTES + 15) / 16 * 16; }

// the 32-keys-per-lookup kernels need ceil(P/32) tables next to the static part in the CU's 160 KiB of LDS
template <int C, int VPL> constexpr bool lut_fits(uint32_t P) { return wide_table_bytes<C>(P) + lut_static_lds<C, VPL>() <= kCuLdsBytes; }
// ... and the byte-entry multi-pass kernel ceil(P/8) tables
template <int C, int VPL> constexpr bool lut8_fits(uint32_t P) { return lut8_table_bytes<C>(P) + lut_static_lds<C, VPL>() <= kCuLdsBytes; }

// shared_linear3_kernel: four tiles and the 33 KiB row stage next to the tables
template <int C> constexpr size_t linear3_fixed_lds() { return 4 * ScanGeom<C, 64>::LDS_BYTES + 33 * 1024; }

// widths of three or four byte digits, where wider digits (BIG) save a lookup per value
constexpr bool shared_big_width(int c) { return (c >= 17 && c <= 20) || (c >= 25 && c <= 30); }

// ---- the rules -----------------------------------------------------------------------------------------------------------

// which shared scans of <= 8 keys run with 128 values per lane by default (A/B on MI355X: see DESIGN.md section 3.1b)
inline bool shared_lut_prefers_vpl128(int c, uint32_t P, bool linear)
{
    // launches back to back, 1e9 x 9 bit, same box (tools/sweep_p.py --vpl 64,128): per-predicate P = 2 0.296 -> 0.265 ms,
    // P = 4 0.301 -> 0.272 (16-byte stores, 1 KiB per wave and key), P = 8 equal (0.349); linear LOSES (P = 2 0.244 ->
    // 0.367, P = 8 0.365 -> 0.470: twice the row stage, one wave per SIMD)
    (void)c;
    return !linear && P <= 4;
}

// blocks per CU of the LUT kernels.  Measured (tools/tune_scan.hip, 1e9 x 9 bit, P = 8): one block per CU 0.41 ms, two 0.46,
// three 0.49 (tools/sweep.py: c = 5, 2.5 KiB tiles, is the exception -- two blocks 0.30 ms against 0.37).
// The linear layout (word-wise transposition + LDS row stage) wants a second block per CU on random data: launches back to
// back, 1e9 x 9 bit, P = 8, random column 0.36-0.37 ms against 0.417 with one block; equal on the i % 8 column; per-predicate
// prefers one (0.35-0.38 against 0.37-0.40).
inline int lut_want_bpc(int tile_bytes, bool linear, int max_blocks_per_cu)
{
    return max_blocks_per_cu > 0 ? max_blocks_per_cu : ((tile_bytes < 4096 || linear) ? 2 : 1);
}

// linear rows: does the short last table (R = P mod 32 keys behind Tf = P / 32 full ones) ride on the lane of the row's last full
// piece (shared_linear2_kernel's attached mode) instead of getting a lane of its own (shared_linear_kernel)?  Attached, a
// wave-step covers 64 / Tf rows instead of 64 / (Tf + 1) and pays the short piece's instructions with 1 / Tf of the lanes in
// use.  Measured at every Tf = 2 .. 8, 12, 15 and R = 1 .. 31 (2.5e8 x 9 bit, profiles/r03_linear_attach_ab.txt): where the row
// gain is >= 1.19 x it wins at (almost) every R -- 1.0 - 1.4 x; where it is 1.10 .. 1.18 x only for R <= 8; where the row
// count does not change (Tf = 11, 13 .. 15, ...) it loses 10 - 20 %.  (kSwShortNeverAttached / kSwShortAlwaysAttached, for A/B)
inline bool attach_short(unsigned P, unsigned flags, bool hits)
{
    const unsigned Tf = P / 32, R = P % 32;
    if (Tf < 2 || R == 0) return false;
    if (flags & kSwShortAlwaysAttached) return true;
    if (flags & kSwShortNeverAttached) return false;
    const unsigned rows_attached = 64 / Tf, rows_own_lane = 64 / (Tf + 1);
    if (rows_attached * 100 >= rows_own_lane * 119) return !(Tf == 3 && R > 24);
    // (Tf = 7 with hit counts: the old mapping's eight lanes per row count one value each with a single LDS atomic)
    if (rows_attached * 100 >= rows_own_lane * 110) return R <= 8 && !(Tf == 7 && hits);
    return false;
}

// Reads only the key count, the layout, whether hit counts are wanted, the row count, the kernel-side switch word and the options
// shared_vpl, scan_nt_stores and max_blocks_per_cu.
template <int C> SharedPlan plan_shared(const LaunchReq &r)
{
    constexpr int VPL = kSharedVpl;
    using G = ScanGeom<C, VPL>;
    constexpr bool kBigWidth = shared_big_width(C);
    const uint32_t P = r.scan.nkeys, flags = r.scan.flags;
    const bool linear = r.scan.layout != 0, hits = r.scan.hits != nullptr;
    const int max_bpc = r.max_blocks_per_cu;
    const uint64_t out_bytes = (r.scan.n / 8) * P; // the P bitmaps together

    // ---- 1. two keys: the equality scan's decode twice (kSwPairOnLut: the LUT kernel, A/B)
    if (P == 2 && !(flags & kSwPairOnLut)) {
        // per-predicate: the scan's geometry (128 values per lane at c <= 16: a 16-byte store per key and lane); linear:
        // 64 values per lane, so that the lane's 16 row bytes are ONE store and an instruction writes 1 KiB of whole
        // lines (with 128 the lane's 32 bytes left as two instructions of half lines: write-through stores turned
        // them into partial-line writes -- c = 12: 4.7 TB/s against 5.5 for the LUT kernel it was to replace)
        // result stores as the one-pass LUT kernels': write-through below 768 MiB of output, non-temporal beyond (the kernel
        // has no plain-store form: 0 runs write-through)
        constexpr int kEqVpl = scan_vpl(C, kModeEq);
        return make_plan(kFormPair, scan_want_bpc(linear ? ScanGeom<C, 64>::TILE_BYTES : ScanGeom<C, kEqVpl>::TILE_BYTES, max_bpc), linear ? 64 : kEqVpl)
            .stores(one_pass_store_policy(out_bytes, r.scan_nt_stores));
    }

    // ---- 2. P <= 8: LDS lookup table, one pass, deferred stores
    if (P <= 8) {
        // 128 values per lane (16-byte result stores, 1 KiB per wave and key) where the tile, the table and the linear
        // stage fit in LDS and the registers hold 2 x 32 result dwords: c <= 12
        const bool vpl128 = C <= 12 && (r.shared_vpl == 128 || (r.shared_vpl == 0 && shared_lut_prefers_vpl128(C, P, linear)));
        return make_plan(kFormLut, lut_want_bpc(vpl128 ? ScanGeom<C, 128>::TILE_BYTES : G::TILE_BYTES, linear, max_bpc), vpl128 ? 128 : 64)
            .stores(one_pass_store_policy(out_bytes, r.scan_nt_stores));
    }

    // ---- 3. linear rows of 32 .. 40 keys: the per-predicate machinery + an LDS stage (shared_linear3_kernel; kSwNoLinear3: the
    // row-per-lane kernels below, for A/B).  Hit counts in registers: one round (P <= 32) or two packed.  Where it pays
    // (2.5e8 rows, TB/s with hit counts, against the row-per-lane kernels on the same box): c = 9, P = 32 / 33 / 40:
    // 4.67 / 3.54 / 3.52 against 4.05 / 3.29 / 3.24; c = 5, P = 32: 4.49 against 3.28; c = 12: 4.54 against 4.06; c = 17:
    // 4.64 against 4.32.  Where it does not: fewer keys (no VALU to save: P = 9 2.55 against 2.92, P = 16 3.94 against
    // 4.33, P = 24 / 31 equal), a long second round (its 32-byte pieces complete the first round's half-written lines a
    // whole round later: P = 48 3.01 against 3.41, P = 64 2.29 against 3.94), and widths whose tiles leave room for one
    // block per CU only (c = 25, P = 32: 2.95 against 4.40).
    if (linear && P >= 32 && P <= 40 && !(flags & kSwNoLinear3) && 2 * (wide_table_bytes<C>(P) + linear3_fixed_lds<C>()) <= kCuLdsBytes) {
        bool big = false;
        if constexpr (kBigWidth) big = !(flags & kSwByteDigits) && 2 * (wide_table_bytes<C, true>(P) + linear3_fixed_lds<C>()) <= kCuLdsBytes;
        const size_t dyn3 = big ? wide_table_bytes<C, true>(P) : wide_table_bytes<C>(P);
        const int fit = (int)(kCuLdsBytes / (dyn3 + linear3_fixed_lds<C>()));
        return make_plan(kFormLinear3, cap_bpc(fit > 2 ? 2 : (fit < 1 ? 1 : fit), max_bpc)).lds(dyn3).counters(hits ? (P <= 32 ? 1 : 2) : 0, big);
    }

    // linear rows of 9 .. 1024 keys: lanes in memory order (shared_linear_kernel).  It needs two blocks per CU to hide its
    // lookups: tables too big for that -- P = 1024 at c <= 10 -- stay on the per-group kernel unless hit counts are
    // wanted (2.5e8 x 9 bit, P = 1024: 13.5 against 10.2 ms without, 15.6 against 17.8 with).  (kSwPerGroupKernels: the older kernels, A/B)
    // Digit-table widths (c > 10) leave it to the per-group kernel beyond 320 keys (beyond 160 without hit counts at c > 16):
    // every lane of a row decodes the row again and looks up ceil(c/8) digits, and the tables leave room for two blocks
    // per CU only (2.5e8 rows, with / without hit counts, TB/s, shared_linear_kernel against the per-group kernel: c = 13,
    // P = 300: 2.6 / 2.9 against 2.2 / 2.2, P = 400: 2.1 / 2.3 against 2.4 / 2.7, P = 600: 1.7 / 1.8 against 2.4 / 2.6;
    // c = 17, P = 150: 2.6 / 2.8 against 1.4 / 1.8, P = 200: 2.6 / 2.8 against 1.5 / 3.0, P = 300: 2.1 / 2.2 against 1.5 / 2.5;
    // c = 9, P = 300: 3.6 / 4.1 against 2.2 / 2.3).
    const bool lin_pays = C <= 10 || (C <= 16 ? P <= 320 : P <= (hits ? 320u : 160u)) || (flags & kSwLinearAnyWidth); // (always, A/B)
    const bool lin_rows = linear && lut_fits<C, VPL>(P) && !(flags & kSwPerGroupKernels) && lin_pays &&
                          (2 * (wide_table_bytes<C>(P) + lut_static_lds<C, VPL>()) <= kCuLdsBytes || (hits && WideLutGeom<C>::SINGLE));

    // ---- 4. linear rows of fewer than ~200 keys without hit counts, where the row-per-lane kernels do not run: byte-entry
    // tables, 16 output bytes per round (measured, tools/sweep_p.py, 2.5e8 x 9 bit: P = 16 / 32 / 64 / 128 0.21 / 0.43 / 0.72 /
    // 1.45 ms against 0.41 / 0.58 / 0.91 / 1.50 for the dword-entry kernel, which wins from P = 256: 2.80 against 3.16 ms)
    if (linear && !hits && P < 192 && lut8_fits<C, VPL>(P) && !lin_rows) {
        const int want = lut_want_bpc(G::TILE_BYTES, linear, max_bpc);
        return make_plan(kFormLutMulti, want < 8 ? want : 8).lds(lut8_table_bytes<C>(P));
    }

    // Per-predicate bitmaps at the widths of three or four table digits with few keys: round 2 sent them to the compare chain
    // (16 v_cmp + v_addc per value beat three or four lookups + ANDs per value in shared_wide2_kernel at ONE wave per SIMD).
    // shared_wide3_kernel turns that around (2.5e8 rows, with hit counts, TB/s, tables against chain: c = 17, P = 16: 4.39
    // against 2.92; c = 21: 3.61 against 3.27; c = 29: 4.77 against 3.56, P = 24: 4.74), so the chain keeps only the key
    // counts whose tables do not fit (kSwChainRuleRound2: round 2's rule, for A/B).
    const bool chain_pays = !linear && C >= 17 && P <= (C >= 25 ? 24u : 16u) && (flags & kSwChainRuleRound2);

    // ---- 5. more keys than the tables hold: compare chain, ceil(P/8) passes over the registers (kSwCompareChain: always, for A/B)
    if (!lut_fits<C, VPL>(P) || (flags & kSwCompareChain) || chain_pays) return make_plan(kFormChain, max_bpc > 0 ? max_bpc : 0);

    // ---- everything below: one dword-entry lookup table per 32 keys, in dynamic LDS
    const size_t dyn = wide_table_bytes<C>(P);

    // ---- 6. linear rows, a row per lane
    if (lin_rows) {
        const int want = max_bpc > 0 ? max_bpc : 4;
        // P = 16: two rows per 32-byte piece only with the digit tables (c > 10: 4.0 / 4.8 TB/s against 3.2 / 4.2 with one
        // row per piece at c = 12); at c <= 10 one row per piece wins (c = 5: 3.0 / 4.7 against 2.0 / 4.1, c = 9: 3.9 /
        // 4.8 against 3.5 / 4.9 with / without hit counts).  (kSwP16OneRowPerPiece: everywhere, for A/B)
        if (P == 16 && C > 10 && !(flags & kSwP16OneRowPerPiece)) return make_plan(kFormLinearTwoRows, want).lds(dyn);
        // everything else: full tables in memory order, the short last table on its own (shared_linear2_kernel;
        // kSwLinearRound2: round 2's kernel, which gives the short table a whole lane per row, for A/B)
        // shared_linear2_kernel (the short last table on the full piece's lane / in steps of its own) is the product only for
        // rows below 32 keys without hit counts (2.5e8 x 9 bit, same box: P = 12: 4.09 against 3.77 TB/s; with hit counts
        // 2.87 against 3.43).  For rows of 33 .. 63 keys it beat round 2's kernel (P = 33: 3.10 against 2.59) until that kernel
        // learnt to write such rows through an aligned LDS image (P = 47 / 52 / 56: 3.02 / 3.30 / 3.46 against 2.82 / 2.84 /
        // 2.85; kSwLinear2Short brings it back for A/B), and its short-table steps LOSE behind two or more full tables -- P = 100:
        // 2.26 against 3.18, P = 300: 2.45 against 3.58: a step that writes 4 bytes of each of 64 rows is 64 partial-line
        // transactions, where the old mapping's short lane sits in the same store instruction as its row's full pieces.
        // Rows of 65 and more keys with a short last table: attach_short() above decides between the two mappings.
        const bool attached = attach_short(P, flags, hits);
        if (!(flags & kSwLinearRound2) && (((flags & kSwLinear2Short) && P / 32 == 1 && P % 32 >= 1 && P % 32 <= 24) || (P < 32 && !hits) || attached))
            return make_plan(kFormLinear2, want).lds(dyn).flag(attached ? kSetShortAttached : 0u);
        // rows of 33 .. 63 keys whose length is not a multiple of 16 bytes, single-table widths: through the wave-private
        // aligned output image (dynamic LDS behind the tables; kSwNoImage: never, kSwImageAnyLength: at every row length, A/B)
        const size_t with_image = dyn + (size_t)kWavesPerBlock * kLinearImageBytes;
        const bool image = C <= 10 && (P & 15u) != 0 && !(flags & kSwNoImage) && ((P + 31) / 32 == 2 || (flags & kSwImageAnyLength)) &&
                           with_image <= (size_t)shared_max_dyn_lds<C>();
        return make_plan(kFormLinear, want).lds(image ? with_image : dyn).flag(image ? kSetImage : 0u);
    }

    const int want = max_bpc > 0 ? max_bpc : 2;
    // result stores of the per-predicate bitmaps: non-temporal unless the P bitmaps together are small
    const int store = (!linear && multi_pass_nt_stores(out_bytes, r.scan_nt_stores)) ? 1 : 0;

    // ---- 7. per-predicate bitmaps (kSwPerGroupKernels: the per-group kernel, for A/B)
    if (!linear && !(flags & kSwPerGroupKernels)) {
        // Hit counts in registers (kSwCountsByReduction: per-tile wave reductions / the histogram instead, for A/B): one 32-key
        // round in 32-bit registers (P <= 32: 2.5e8 x 9 bit, same box, P = 16 0.200 -> 0.158 ms, P = 32 0.298 -> 0.249),
        // two rounds in packed 16-bit halves (P <= 64, round 3: c = 9, P = 33 / 40 / 48 3.50 / 3.96 / 4.12 -> 4.44 / 4.81 /
        // 4.87 TB/s; not where the histogram counts -- c <= 12, P >= 64: 4.99 against 4.66).
        // Wider digits (BIG; kSwByteDigits: byte digits, for A/B) at the widths of three or four byte digits while two
        // blocks per CU still fit.
        const bool hist_counts = C <= 12 && P >= 64;
        const int rc = (hits && !(flags & kSwCountsByReduction)) ? (P <= 32 ? 1 : ((P <= 64 && !hist_counts) ? 2 : 0)) : 0;
        bool big = false;
        if constexpr (kBigWidth) big = !(flags & kSwByteDigits) && 2 * (wide_table_bytes<C, true>(P) + lut_static_lds<C, VPL>()) <= kCuLdsBytes;
        const size_t bdyn = big ? wide_table_bytes<C, true>(P) : dyn;
        // a 32-value word at a time (shared_wide3_kernel: half the registers, several waves per SIMD -- what the digit-table
        // widths need, and 0-20 % ahead at c <= 10 too: 2.5e8 x 9 bit, P = 9 / 24 / 63, TB/s with / without hit counts:
        // 3.63 / 4.41, 5.13 / 5.43, 5.21 / 5.56 against 3.44 / 3.58, 4.49 / 4.58, 4.39 / 4.49) for every scan it can count:
        // without hit counts, or up to 64 keys (kSwWide2: shared_wide2_kernel, A/B)
        if ((!hits || rc != 0) && !(flags & kSwWide2)) {
            const int waves = (rc == 0 || C <= 10) ? 3 : 2; // the kernel's launch bound
            const int fit = (int)(kCuLdsBytes / (bdyn + 4 * ScanGeom<C, 64>::LDS_BYTES + 256));
            return make_plan(kFormWide3, cap_bpc(fit > waves ? waves : (fit < 1 ? 1 : fit), max_bpc)).lds(bdyn).counters(rc, big).stores(store);
        }
        // (register counters in shared_wide2_kernel only at the single-table widths: the digit-table widths that come here
        // -- more than 64 keys with hit counts, or the A/B switch -- have no registers to spare for them)
        return make_plan(kFormWide2, want).lds(bdyn).counters(C <= 10 ? rc : 0, big).stores(store);
    }

    // ---- 8. the per-group kernel: the linear rows it keeps (lin_pays), either layout under kSwPerGroupKernels
    return make_plan(linear ? kFormWideLinear : kFormWide, want).lds(dyn).stores(store);
}

} // namespace mi355
