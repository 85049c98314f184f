// arith/arith.hpp -- the device code of mi355_arith_dev: a packed column computed row by row from two others,
//   LINEAR  r_i = a x_i + b y_i + k        MUL  r_i = a x_i y_i + k        out_i = 0 <= r_i < 2^CO ? r_i : miss,
// packed in and packed out -- the composite key of GROUP BY a, b, the product under sum(price * discount), the difference
// that histogram / lookup / group_aggregate consume.  gfx950 only; part of libmi355scan.so through arith/arith.hip.
//
// Pipeline.  The run-time-width tile stream of kernels/rt_column.hpp, twice in and packed out: a wave owns tiles of 64 x 32
// consecutive rows, lane l rows [32 l, 32 l + 32) of BOTH columns.  The kernels are templates of the OUTPUT width CO only
// (2 x 32 instantiations): a lane's 32 results are exactly CO dwords, assembled by rt_insert<CO, K> and stored at byte
// 4 CO lane of the tile's 256 CO output bytes.  Both input widths are wave-uniform run-time numbers: both tiles travel by
// non-temporal LDS-DMA, stay in LDS and are decoded from there (columns_lds_value), so a wave has two
// alternating images of EACH column -- the next tiles land in one pair while the other is decoded.  A full tile's dwords leave
// one tile late, in front of the next DMA (rt_store); the ragged tile writes exactly the bytes it owns (rt_store_tail).
// The geometry, the decode, rt_insert, the two stores and wave_sum64 are rt_column.hpp's, not copies; the DMA loop is the kernels' own.  The same buffer as both
// inputs fills both image sets like any other pair.
//
// Arithmetic.  The host (arith.hip, arith_plan) has bounded r over ALL x < 2^c1, y < 2^c2 in 128 bits:
//   arith_exact_kernel    [lo, hi] lies within [0, 2^CO - 1]: no row can be out of range -- rows >= n of the ragged tile
//                         included, whose stale LDS still decodes to values below 2^c1 / 2^c2.  The true result lies in
//                         [0, 2^32), so 32-bit wrap-around arithmetic on a, b, k reduced mod 2^32 yields it.  No test, no
//                         counter.
//   arith_checked_kernel  [lo, hi] lies within int64: 64-bit wrap-around arithmetic yields the exact r, (uint64)r < 2^CO is
//                         the range test (a negative r is a huge unsigned one), `miss` is selected without a branch.  A
//                         lane collects its tile's out-of-range rows as a 32-bit mask -- the ragged tile masks the rows
//                         >= n away before they are counted --, a wave adds its total with ONE vector atomic at its end.
// op and the cheap operands (a == 1, b == 0, b == +-1) are wave-uniform and no template arguments of the kernels: the launcher
// folds them into ArithArgs::mode, ONE switch per tile picks among ten straight-line bodies of 32 rows (decode, compute, test,
// insert per row, so no value waits in a register for a branch), each with only the multiplications its form needs.
// The kernels test no switch bit.
#pragma once

#include "../kernels.hpp"
#include "../kernels/rt_column.hpp" // the tile stream of a column of run-time width, and the packed-out half

namespace mi355 {

constexpr uint32_t kArithLinear = 0, kArithMul = 1; // MI355_ARITH_LINEAR, MI355_ARITH_MUL

struct ArithArgs {
    const uint8_t *packed1, *packed2; // n values of c1 / c2 bits, 16 B aligned
    uint64_t n;
    uint8_t *out;                     // n values of CO bits, 16 B aligned; exactly ceil(n CO / 8) bytes are written
    unsigned long long *out_of_range; // checked kernel, nullable: zeroed in front of the launch, one add per wave
    int64_t k;
    int32_t a, b;
    uint32_t c1, c2;
    uint32_t mode; // arith_mode(op, a, b): the form of the expression, wave-uniform
    uint32_t miss; // < 2^CO
    uint32_t nts;  // result stores: 0 plain, 1 non-temporal, 2 write-through (one uniform branch per tile)
};

// a wave's images: two of each column
constexpr uint32_t arith_wave_lds(uint32_t c1, uint32_t c2) { return 2u * rt_image(c1) + 2u * rt_image(c2); }
// + 16: the dword behind the last lane's run is read (and not used)
constexpr uint32_t arith_block_lds(uint32_t c1, uint32_t c2) { return kWavesPerBlock * arith_wave_lds(c1, c2) + 16u; }
static_assert(arith_block_lds(32, 32) <= kCuLdsBytes, "LDS budget");

// ---- the form of the expression, decided by the launcher: op and the cheap operands, one number per launch ----
// mode = 8 (op == MUL) + 4 (a != 1) + how b enters (LINEAR only)
constexpr uint32_t kArithBZero = 0, kArithBPlus = 1, kArithBMinus = 2, kArithBAny = 3;
constexpr uint32_t kArithAAny = 4, kArithModeMul = 8;
constexpr uint32_t arith_mode(uint32_t op, int32_t a, int32_t b)
{
    const uint32_t am = a == 1 ? 0u : kArithAAny;
    if (op == kArithMul) return kArithModeMul + am;
    return am + (b == 0 ? kArithBZero : b == 1 ? kArithBPlus : b == -1 ? kArithBMinus : kArithBAny);
}

// one result in wrap-around arithmetic of T: uint32_t (exact kernel: a, b, k reduced mod 2^32) or uint64_t (checked kernel:
// a, b sign-extended)
template <int MODE, typename T> __device__ __forceinline__ T arith_one(T a, T b, T k, uint32_t x, uint32_t y)
{
    T r;
    if constexpr (MODE & kArithModeMul) {
        r = (T)x * (T)y;
        if constexpr (MODE & kArithAAny) r *= a;
    } else {
        if constexpr (MODE & kArithAAny) r = a * (T)x;
        else r = (T)x;
        if constexpr ((MODE & 3) == kArithBPlus) r += (T)y;
        else if constexpr ((MODE & 3) == kArithBMinus) r -= (T)y;
        else if constexpr ((MODE & 3) == kArithBAny) r += b * (T)y;
    }
    return r + k;
}

// ---- the lane's 32 rows of a tile, straight-line: decode both values, compute, (test,) insert -- row K at compile-time
// output offsets, at scalar input offsets.  CHECKED: bit K of `bad` = row K is out of range. ----
template <int CO, bool CHECKED, int MODE, int K = 0>
__device__ __forceinline__ void arith_rows(const ArithArgs &q, const uint8_t *base1, uint32_t c1, uint32_t vmask1, const uint8_t *base2, uint32_t c2,
                                           uint32_t vmask2, uint32_t (&res)[CO], uint32_t &bad)
{
    const uint32_t x = columns_lds_value<K>(base1, c1, vmask1), y = columns_lds_value<K>(base2, c2, vmask2);
    if constexpr (CHECKED) {
        // 64-bit wrap-around is exact under the range rule; (uint64)r < 2^CO also sends a negative r to `miss`
        const uint64_t t = arith_one<MODE, uint64_t>((uint64_t)(int64_t)q.a, (uint64_t)(int64_t)q.b, (uint64_t)q.k, x, y);
        const bool in = (t >> CO) == 0;
        rt_insert<CO, K>(res, in ? (uint32_t)t : q.miss);
        bad |= in ? 0u : (1u << K);
    } else {
        // the true result lies in [0, 2^CO) within [0, 2^32): 32-bit wrap-around yields it
        rt_insert<CO, K>(res, arith_one<MODE, uint32_t>((uint32_t)q.a, (uint32_t)q.b, (uint32_t)q.k, x, y));
    }
    if constexpr (K + 1 < kRtVpl) arith_rows<CO, CHECKED, MODE, K + 1>(q, base1, c1, vmask1, base2, c2, vmask2, res, bad);
}

template <int CO, bool CHECKED> __device__ __forceinline__ void arith_body(const ArithArgs &a)
{
    constexpr int VPL = kRtVpl;
    constexpr int AUX = 2; // both columns are streamed once: non-temporal DMA
    constexpr uint32_t OUT_TILE = rt_tile_bytes(CO); // output bytes of a tile
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t c1 = a.c1, c2 = a.c2;
    const uint32_t tile_bytes1 = rt_tile_bytes(c1), tile_bytes2 = rt_tile_bytes(c2); // multiples of 256
    const uint32_t image1 = rt_image(c1), image2 = rt_image(c2);
    uint8_t *cur1 = mi355_dyn_lds + (uint32_t)wave * arith_wave_lds(c1, c2); // the images being decoded ...
    uint8_t *nxt1 = cur1 + image1;                                           // ... and where the next tiles land
    uint8_t *cur2 = cur1 + 2u * image1;
    uint8_t *nxt2 = cur2 + image2;
    const uint32_t vmask1 = rt_vmask(c1), vmask2 = rt_vmask(c2);

    const uint64_t n = a.n;
    const uint64_t ntiles = rt_ntiles(n), nfull = rt_nfull(n);
    const uint64_t data_bytes1 = (n * c1 + 7) / 8, data_bytes2 = (n * c2 + 7) / 8;
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock;
    uint64_t tile = (uint64_t)blockIdx.x * kWavesPerBlock + wave;
    const uint32_t nts = a.nts, mode = a.mode;

    // tile t of one column: LDS-DMA into `dst` (the last tile: only 16-byte chunks that start inside the payload).  The kernels' own
    // copy of rt_issue_tile's loop, as their store dispatch is of store_words_by and `left` of lane_valid_rows (kernels/rt_column.hpp):
    // with the shared forms 43 of the 64 instantiations take other register counts
    auto issue_column = [&](const uint8_t *packed, uint64_t data_bytes, uint32_t tile_bytes, uint64_t t, uint8_t *dst) {
        const uint64_t first = t * tile_bytes;
        const uint8_t *src = packed + first;
        const uint64_t left = data_bytes - first; // t < ntiles: at least one byte
        const uint32_t lim = left < tile_bytes ? (uint32_t)left : tile_bytes;
#pragma unroll
        for (int j = 0; j < kRtDmaInstrs; j++) {
            const uint32_t o = j * 1024 + lane * 16;
            if ((uint32_t)j * 1024u < tile_bytes && o < lim) __builtin_amdgcn_global_load_lds(MI355_GPTR(src + o), MI355_LPTR(dst + j * 1024), 16, 0, AUX);
        }
    };
    auto issue = [&](uint64_t t, uint8_t *dst1, uint8_t *dst2) {
        issue_column(a.packed1, data_bytes1, tile_bytes1, t, dst1);
        issue_column(a.packed2, data_bytes2, tile_bytes2, t, dst2);
    };

    if (tile < ntiles) issue(tile, cur1, cur2);

    uint32_t res[CO];
    uint64_t prev = ~0ull;
    unsigned long long outside = 0; // CHECKED: the lane's out-of-range rows so far
    uint8_t *const out_lane = a.out + (uint32_t)lane * (4u * CO);
    auto store_prev = [&]() {
        uint8_t *dst = out_lane + prev * OUT_TILE;
        if (nts == 2)
            rt_store<CO, 2>(dst, res);
        else if (nts == 1)
            rt_store<CO, 1>(dst, res);
        else
            rt_store<CO, 0>(dst, res);
    };
    while (tile < ntiles) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // both tiles have landed
        if (prev != ~0ull) store_prev();
        const uint64_t next = tile + stride;
        if (next < ntiles) issue(next, nxt1, nxt2);

        const uint8_t *const base1 = cur1 + (uint32_t)lane * rt_lane_bytes(c1), *const base2 = cur2 + (uint32_t)lane * rt_lane_bytes(c2);
        uint32_t bad = 0;
        // the form of the expression: ONE uniform branch per tile, then 32 rows of straight-line code
#define MI355_ARITH_MODE(M) case M: arith_rows<CO, CHECKED, M>(a, base1, c1, vmask1, base2, c2, vmask2, res, bad); break
        switch (mode) {
            MI355_ARITH_MODE(kArithBZero);
            MI355_ARITH_MODE(kArithBPlus);
            MI355_ARITH_MODE(kArithBMinus);
            MI355_ARITH_MODE(kArithBAny);
            MI355_ARITH_MODE(kArithAAny + kArithBZero);
            MI355_ARITH_MODE(kArithAAny + kArithBPlus);
            MI355_ARITH_MODE(kArithAAny + kArithBMinus);
            MI355_ARITH_MODE(kArithAAny + kArithBAny);
            MI355_ARITH_MODE(kArithModeMul);
        default:
            arith_rows<CO, CHECKED, kArithModeMul + kArithAAny>(a, base1, c1, vmask1, base2, c2, vmask2, res, bad);
            break;
        }
#undef MI355_ARITH_MODE
        if (tile < nfull) {
            prev = tile;
        } else {
            // rows >= n hold stale LDS: they reach neither a stored byte nor the counter
            const int64_t left = (int64_t)(n - tile * kRtTileRows) - (int64_t)lane * VPL;
            const int valid = left >= VPL ? VPL : (left <= 0 ? 0 : (int)left);
            rt_store_tail<CO>(out_lane + tile * OUT_TILE, res, valid);
            bad &= tail_mask(valid, 0);
            prev = ~0ull;
        }
        if constexpr (CHECKED) outside += (uint32_t)__builtin_popcount(bad);
        uint8_t *t1 = cur1, *t2 = cur2;
        cur1 = nxt1, cur2 = nxt2;
        nxt1 = t1, nxt2 = t2;
        tile = next;
    }
    if (prev != ~0ull) store_prev();
    if constexpr (CHECKED) {
        if (a.out_of_range) {
            const unsigned long long total = wave_sum64(outside);
            if (lane == 0 && total) __hip_atomic_fetch_add(a.out_of_range, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <int CO> __global__ __launch_bounds__(kBlockThreads) void arith_exact_kernel(ArithArgs a) { arith_body<CO, false>(a); }

template <int CO> __global__ __launch_bounds__(kBlockThreads) void arith_checked_kernel(ArithArgs a) { arith_body<CO, true>(a); }

} // namespace mi355
