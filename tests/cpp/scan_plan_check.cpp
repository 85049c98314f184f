// scan_plan_check.cpp -- the launch rules of csrc/scan_plan.hpp, checked value by value.  Stand-alone: plain g++, no HIP, built and
// run under -fsanitize=undefined,address by tests/test_scan_plan.py.
//
// What is asserted comes from the rules' own comments (the divisors the measurements name), from the table of AUX words that the
// launchers instantiate, and from each rule's exits taken one by one; nothing here is read back from the code under test.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "scan_plan.hpp"

using namespace mi355;

static int g_checked = 0, g_failed = 0;
#define EXPECT(cond)                                                                  \
    do {                                                                              \
        g_checked++;                                                                  \
        if (!(cond) && g_failed++ < 50) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
    } while (0)

constexpr uint64_t MiB = 1ull << 20;
constexpr int kCus = 256;

// a request with nothing set but the CU count: every option at its default
static PlanReq req(int max_bpc = 0, int dma_aux = 18, int nts = -1)
{
    PlanReq q{};
    q.num_cus = kCus;
    q.max_blocks_per_cu = max_bpc;
    q.dma_aux = dma_aux;
    q.scan_nt_stores = nts;
    q.llc_resident_mib = -1;
    return q;
}

// the eq / range scan of `rows` x 9 bit, one bitmap written, `masks` bitmaps read
static uint32_t d9(uint64_t rows, int mib, int repeat, int masks = 0, int dma_aux = 18)
{
    return llc_divisor(mib, dma_aux, repeat, (rows * 9 + 7) / 8, (1 + masks) * ((rows + 7) / 8));
}

static void check_llc_divisor()
{
    // the values the rule's comment states: 1e9 x 9 bit, one bitmap, no mask
    EXPECT(kLlcAutoMiB == 205);
    EXPECT(d9(1000000000, 190, 0) == 17);
    EXPECT(d9(1000000000, 205, 0) == 13);
    EXPECT(d9(1000000000, 220, 0) == 11);
    EXPECT(d9(1000000000, 240, 0) == 9);
    EXPECT(d9(1000000000, -1, 1) == 13);
    EXPECT(d9(500000000, -1, 1) == 5);
    EXPECT(d9(250000000, -1, 1) == 3);
    // every exit.  Budget 0: off
    EXPECT(d9(1000000000, 0, 1) == 0);
    // default-policy loads (dma_aux & 15 == 0): nothing to decide
    EXPECT(d9(1000000000, 205, 1, 0, 0) == 0);
    EXPECT(d9(1000000000, 205, 1, 0, 16) == 0);
    EXPECT(d9(1000000000, 205, 1, 0, 32) == 0);
    EXPECT(d9(1000000000, 205, 1, 0, 2) == 13);
    EXPECT(d9(1000000000, 205, 1, 0, 34) == 13);
    // a bitmap beyond 768 MiB: '>', not '>='
    EXPECT(llc_divisor(1024, 18, 1, 16ull << 30, 768 * MiB) == 65);       // 256 MiB resident of 16 GiB: 64 | 1
    EXPECT(llc_divisor(1024, 18, 1, 16ull << 30, 768 * MiB + 1) == 0);
    // auto acts on a repeat only; an explicit budget on every call
    EXPECT(d9(1000000000, -1, 0) == 0);
    EXPECT(d9(1000000000, 205, 0) == d9(1000000000, 205, 1));
    // budget <= bitmap
    EXPECT(llc_divisor(100, 18, 1, 1000 * MiB, 100 * MiB) == 0);
    EXPECT(llc_divisor(100, 18, 1, 1000 * MiB, 101 * MiB) == 0);
    EXPECT(llc_divisor(100, 18, 1, 1000 * MiB, 100 * MiB - 1) == 0);      // one resident byte: a divisor beyond 0x7fffff
    // resident >= column: nothing in auto, all of it with an explicit budget
    EXPECT(d9(100000000, -1, 1) == 0);                                    // 107 MiB of column, 193 MiB left of 205
    EXPECT(d9(100000000, 205, 1) == 1);
    EXPECT(llc_divisor(101, 18, 1, 100 * MiB, 1 * MiB) == 1);             // resident == column
    EXPECT(llc_divisor(-1, 18, 1, 204 * MiB, 1 * MiB) == 0);
    EXPECT(llc_divisor(101, 18, 1, 100 * MiB + 1, 1 * MiB) == 3);         // one byte more: the smallest divisor
    // otherwise always odd and >= 3
    for (uint64_t rows = 130000000; rows <= 6000000000ull; rows += 97000001)
        for (int mib : {-1, 64, 150, 205, 255, 4000})
            for (int masks = 0; masks <= 1; masks++) {
                const uint32_t d = d9(rows, mib, 1, masks);
                EXPECT(d == 0 || d == 1 || (d >= 3 && (d & 1)));
                if (d == 1) EXPECT(mib > 0);
            }
    // a divisor above 0x7fffff: one resident byte
    EXPECT(llc_divisor(1, 18, 1, 0x7fffff, MiB - 1) == 0x7fffff);
    EXPECT(llc_divisor(1, 18, 1, 0x800000, MiB - 1) == 0);
    EXPECT(llc_divisor(1, 18, 1, 1ull << 40, MiB - 1) == 0);
    // a mask's bytes count with the bitmap's: 1e9 rows, 205 MiB - 2 x 119.2 MiB is negative
    EXPECT(d9(1000000000, 205, 1, 1) == 0);
    EXPECT(d9(500000000, 205, 1, 1) == 7);                                // 562.5e6 / (214958080 - 125e6) = 6.25 -> 7
    EXPECT(d9(500000000, -1, 1, 1) == 7);
    // ... as plan_scan passes them
    const PlanTile t{8192, 9216};
    PlanReq q = req();
    q.llc_repeat = 1;
    EXPECT(plan_scan(q, t, 9, 500000000, true, false, 4, 1).llc_d == 5);
    EXPECT(plan_scan(q, t, 9, 500000000, true, true, 4, 1).llc_d == 7);
    EXPECT(plan_scan(q, t, 9, 500000000, false, true, 4, 1).llc_d == 5);
    EXPECT(plan_scan(q, t, 9, 500000000, false, false, 4, 1).llc_d == 3);  // count only: 562.5e6 / 214958080 = 2.6 -> 3
    q.llc_repeat = 0;
    EXPECT(plan_scan(q, t, 9, 500000000, true, false, 4, 1).llc_d == 0);
    q.llc_resident_mib = 190;
    EXPECT(plan_scan(q, t, 9, 1000000000, true, false, 4, 1).llc_d == 17);
    q.dma_aux = 0;
    EXPECT(plan_scan(q, t, 9, 1000000000, true, false, 4, 1).llc_d == 0);
}

static void check_burst_k()
{
    for (int c = 1; c <= 32; c++) {
        const bool four = c == 5 || c == 6 || (c >= 9 && c <= 16);
        EXPECT(burst_k(c) == (four ? 4 : 1));
        EXPECT(burst_k(c, 0) == burst_k(c));
        EXPECT(burst_k(c, 1) == 1);
    }
}

static void check_store_policies()
{
    EXPECT(one_pass_store_policy(768 * MiB, -1) == 2);
    EXPECT(one_pass_store_policy(768 * MiB + 1, -1) == 1);
    EXPECT(one_pass_store_policy(0, -1) == 2);
    for (uint64_t bytes : {(uint64_t)0, 768 * MiB, 768 * MiB + 1}) {
        EXPECT(one_pass_store_policy(bytes, 0) == 0);
        EXPECT(one_pass_store_policy(bytes, 1) == 1);
    }
    EXPECT(multi_pass_nt_stores(64 * MiB, -1) == false);
    EXPECT(multi_pass_nt_stores(64 * MiB + 1, -1) == true);
    for (uint64_t bytes : {(uint64_t)0, 64 * MiB, 64 * MiB + 1}) {
        EXPECT(multi_pass_nt_stores(bytes, 0) == false);
        EXPECT(multi_pass_nt_stores(bytes, 1) == true);
    }
}

// the AUX words, row by row: what the launchers instantiate, and what each (dma_aux, store policy) maps to
static void check_aux()
{
    // scan_burst_kernel: dma_aux == 0 -> 0; else policy 1 -> 18, 2 -> 34, 0 -> 2
    for (int policy = 0; policy <= 2; policy++) EXPECT(scan_aux(0, policy) == 0);
    for (int dma : {2, 18, 34}) {
        EXPECT(scan_aux(dma, 0) == 2);
        EXPECT(scan_aux(dma, 1) == 18);
        EXPECT(scan_aux(dma, 2) == 34);
    }
    // in_kernel: policy 2 -> 34, 1 -> 18, else 2; dma_aux is not read
    EXPECT(in_aux(0) == 2 && in_aux(1) == 18 && in_aux(2) == 34);
    // scan2_kernel: policy 1 -> 18, else 34 (policy 0 runs write-through)
    EXPECT(scan2_aux(0) == 34 && scan2_aux(1) == 18 && scan2_aux(2) == 34);
    // decompress_kernel: 0 -> 0, 2 -> 2, 34 -> 34, anything else -> 18
    EXPECT(decompress_aux(0) == 0 && decompress_aux(2) == 2 && decompress_aux(34) == 34 && decompress_aux(18) == 18);
    for (int dma : {1, 3, 16, 17, 32, 33, 35, 50, -1}) EXPECT(decompress_aux(dma) == 18);

    // ... through the plans, by size (768 MiB of bitmap = 6 Gi rows + 8 rows more) and by option
    const PlanTile t{8192, 9216};
    const uint64_t small = 4099, edge = 768 * MiB * 8, big = edge + 8;
    for (int dma : {0, 2, 18, 34}) {
        const int on = dma != 0;
        EXPECT(plan_scan(req(0, dma, -1), t, 9, small, true, false, 4, 1).aux == (on ? 34 : 0));
        EXPECT(plan_scan(req(0, dma, -1), t, 9, edge, true, false, 4, 1).aux == (on ? 34 : 0));
        EXPECT(plan_scan(req(0, dma, -1), t, 9, big, true, false, 4, 1).aux == (on ? 18 : 0));
        EXPECT(plan_scan(req(0, dma, 0), t, 9, big, true, false, 4, 1).aux == (on ? 2 : 0));
        EXPECT(plan_scan(req(0, dma, 1), t, 9, small, true, false, 4, 1).aux == (on ? 18 : 0));
        EXPECT(plan_in(req(0, dma, -1), t, small, 1).aux == 34);
        EXPECT(plan_in(req(0, dma, -1), t, big, 1).aux == 18);
        EXPECT(plan_in(req(0, dma, 0), t, small, 1).aux == 2);
        EXPECT(plan_in(req(0, dma, 1), t, small, 1).aux == 18);
        EXPECT(plan_scan2(req(0, dma, -1), t, small, 1).aux == 34);
        EXPECT(plan_scan2(req(0, dma, -1), t, big, 1).aux == 18);
        EXPECT(plan_scan2(req(0, dma, 0), t, small, 1).aux == 34);
        EXPECT(plan_scan2(req(0, dma, 1), t, small, 1).aux == 18);
        for (int nts = -1; nts <= 1; nts++) EXPECT(plan_decompress(req(0, dma, nts), PlanTile{4096, 4608}, big, 4).aux == (dma == 0 ? 0 : dma));
    }
    EXPECT(plan_decompress(req(0, 7, -1), PlanTile{4096, 4608}, small, 4).aux == 18);
    // tiles per burst pass through
    EXPECT(plan_scan(req(), t, 9, small, true, false, 4, 1).k == 4 && plan_scan(req(), t, 9, small, true, false, 1, 1).k == 1);
}

static void check_blocks_per_cu()
{
    // the 40 KiB rule: (40 KiB + half a block's tiles) / a block's tiles.  9 KiB tiles (c = 9, 128 values per lane): one block
    EXPECT(dma_in_flight_bpc(9216) == 1);
    EXPECT(dma_in_flight_bpc(5120) == 2);  // c = 5: 20 KiB per block
    EXPECT(dma_in_flight_bpc(1024) == 10); // c = 1
    EXPECT(dma_in_flight_bpc(32768) == 0); // c = 32: 128 KiB per block
    // scan_want_bpc: the cap unclamped when one is set, else clamped to 1 .. 4
    for (int cap : {1, 2, 3, 4, 5, 6, 8, 100})
        for (int tile : {1024, 9216, 32768}) EXPECT(scan_want_bpc(tile, cap) == cap);
    EXPECT(scan_want_bpc(1024, 0) == 4);
    EXPECT(scan_want_bpc(2048, 0) == 4);
    EXPECT(scan_want_bpc(5120, 0) == 2);
    EXPECT(scan_want_bpc(9216, 0) == 1);
    EXPECT(scan_want_bpc(32768, 0) == 1);
    EXPECT(scan_want_bpc(9216, -1) == 1);
    // ... inside what the occupancy query admits
    EXPECT(scan_bpc(8, 1024, 0) == 4 && scan_bpc(3, 1024, 0) == 3 && scan_bpc(8, 1024, 6) == 6 && scan_bpc(4, 1024, 6) == 4);
    // the column scan clamps the cap to 4 as well; run-time width of column 2: four blocks
    EXPECT(columns_want_bpc(true, 9216, 0) == 1 && columns_want_bpc(true, 1024, 0) == 4 && columns_want_bpc(true, 65536, 0) == 1);
    EXPECT(columns_want_bpc(false, 9216, 0) == 4 && columns_want_bpc(false, 65536, 0) == 4);
    for (int same = 0; same <= 1; same++) {
        EXPECT(columns_want_bpc(same, 9216, 1) == 1 && columns_want_bpc(same, 9216, 3) == 3 && columns_want_bpc(same, 9216, 4) == 4);
        EXPECT(columns_want_bpc(same, 9216, 5) == 4 && columns_want_bpc(same, 9216, 6) == 4 && columns_want_bpc(same, 9216, 100) == 4);
    }
    EXPECT(scan_want_bpc(9216, 6) == 6); // where the two differ
    // cap_bpc
    EXPECT(cap_bpc(4, 0) == 4 && cap_bpc(4, -1) == 4 && cap_bpc(4, 2) == 2 && cap_bpc(4, 4) == 4 && cap_bpc(4, 6) == 4);

    const PlanTile t9{8192, 9216}, t1{8192, 1024};
    const uint64_t n = 3000000000ull;
    // the eq / range scan: min(want, occ)
    EXPECT(plan_scan(req(), t9, 9, n, true, false, 4, 3).bpc == 1);
    EXPECT(plan_scan(req(), t1, 1, n, true, false, 1, 8).bpc == 4);
    EXPECT(plan_scan(req(), t1, 1, n, true, false, 1, 2).bpc == 2);
    EXPECT(plan_scan(req(6), t9, 9, n, true, false, 4, 3).bpc == 3);
    EXPECT(plan_scan(req(6), t9, 9, n, true, false, 4, 8).bpc == 6);
    // the IN-list: raised to 2 only when no cap is set and occ >= 2
    EXPECT(plan_in(req(), t9, n, 1).bpc == 1);
    EXPECT(plan_in(req(), t9, n, 2).bpc == 2);
    EXPECT(plan_in(req(), t9, n, 5).bpc == 2);
    EXPECT(plan_in(req(1), t9, n, 5).bpc == 1);
    EXPECT(plan_in(req(3), t9, n, 5).bpc == 3);
    EXPECT(plan_in(req(6), t9, n, 5).bpc == 5);
    EXPECT(plan_in(req(), t1, n, 8).bpc == 4);
    // scan2: on two tiles together
    EXPECT(plan_scan2(req(), PlanTile{8192, 5120}, n, 4).bpc == 1); // 10 KiB per wave: one block, where the plain scan takes two
    EXPECT(plan_scan2(req(), t1, n, 8).bpc == 4);                   // 2 KiB per wave: 5 -> 4
    EXPECT(plan_scan2(req(), PlanTile{8192, 3072}, n, 8).bpc == 2);  // 6 KiB per wave: 52 / 24
    EXPECT(plan_scan2(req(3), t9, n, 2).bpc == 2);
    // decompress: min(occ, 2) against cap_bpc(occ, max)
    const PlanTile td{4096, 4608};
    EXPECT(plan_decompress(req(), td, n, 1).bpc == 1);
    EXPECT(plan_decompress(req(), td, n, 2).bpc == 2);
    EXPECT(plan_decompress(req(), td, n, 5).bpc == 2);
    EXPECT(plan_decompress(req(1), td, n, 5).bpc == 1);
    EXPECT(plan_decompress(req(3), td, n, 5).bpc == 3);
    EXPECT(plan_decompress(req(6), td, n, 5).bpc == 5);
    EXPECT(plan_decompress(req(6), td, n, 1).bpc == 1);
}

static void check_grids()
{
    // grid_for: ntiles of 0, 1, exactly cap x waves and one more
    EXPECT(kPlanWavesPerBlock == 4);
    EXPECT(grid_for(0, 1, kCus) == 1);
    EXPECT(grid_for(1, 1, kCus) == 1);
    EXPECT(grid_for(4, 1, kCus) == 1);
    EXPECT(grid_for(5, 1, kCus) == 2);
    for (int bpc : {1, 2, 4}) {
        const uint64_t cap = (uint64_t)bpc * kCus;
        EXPECT(grid_for(cap * 4 - 4, bpc, kCus) == cap - 1);
        EXPECT(grid_for(cap * 4 - 3, bpc, kCus) == cap);
        EXPECT(grid_for(cap * 4, bpc, kCus) == cap);
        EXPECT(grid_for(cap * 4 + 1, bpc, kCus) == cap);
        EXPECT(grid_for(1ull << 40, bpc, kCus) == cap);
    }
    EXPECT(grid_for(1000, 2, 304) == 250);
    EXPECT(tiles_of(0, 8192) == 0 && tiles_of(1, 8192) == 1 && tiles_of(8192, 8192) == 1 && tiles_of(8193, 8192) == 2);

    const PlanTile t9{8192, 9216};
    // the scan deals bursts of K tiles: 3 000 077 rows are 367 tiles, 92 bursts of four, 23 blocks
    EXPECT(plan_scan(req(), t9, 9, 3000077, true, false, 4, 1).grid == 23);
    EXPECT(plan_scan(req(), t9, 9, 3000077, true, false, 1, 1).grid == 92);
    EXPECT(plan_scan(req(), t9, 9, 1000000000, true, false, 4, 1).grid == 256); // 122 071 tiles: the cap
    EXPECT(plan_scan(req(), t9, 9, 4099, true, false, 4, 1).grid == 1);
    EXPECT(plan_scan(req(), t9, 9, 0, true, false, 4, 1).grid == 1);
    EXPECT(plan_in(req(), t9, 3000077, 2).grid == 92);
    EXPECT(plan_in(req(), t9, 1000000000, 2).grid == 512);
    EXPECT(plan_scan2(req(), t9, 3000077, 2).grid == 92);
    EXPECT(plan_decompress(req(), PlanTile{4096, 4608}, 3000077, 2).grid == 184); // 733 tiles
    EXPECT(plan_decompress(req(), PlanTile{4096, 4608}, 1000000000, 4).grid == 512);
    EXPECT(plan_scan(req(), t9, 9, 4099, true, false, 4, 1).block == 256 && plan_decompress(req(), PlanTile{4096, 4608}, 1, 1).block == 256);
    // the selection: a grid over chunks of tiles, one block per CU; twelve waves but for the single-role kernel's four
    PlanReq q = req(6);
    EXPECT(plan_select(q, t9, 3000077, 8, 12).grid == 12); // 367 tiles, 46 chunks
    EXPECT(plan_select(q, t9, 1000000000, 8, 12).grid == 256);
    EXPECT(plan_select(q, t9, 1, 8, 12).grid == 1);
    EXPECT(plan_select(q, t9, 3000077, 8, 12).block == 768 && plan_select(q, t9, 3000077, 8, 12).bpc == 1);
    q.select_single = 1;
    EXPECT(plan_select(q, t9, 3000077, 8, 12).block == 256 && plan_select(q, t9, 3000077, 8, 12).grid == 12);
}

int main()
{
    check_llc_divisor();
    check_burst_k();
    check_store_policies();
    check_aux();
    check_blocks_per_cu();
    check_grids();
    printf("%d checks, %d failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
