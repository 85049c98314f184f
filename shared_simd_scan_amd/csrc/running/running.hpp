// running/running.hpp -- the device code of mi355_running_sum_dev and mi355_delta_dev: the two calls whose rows depend on the rows
// before them, packed in and packed out,
//   running_sum  r_i = k + sum_{j <= i} t_j (exclusive: j < i),  t_j = (no mask || bit j of the mask) ? x_j + b : 0
//   delta        r_i = x_i - x_{i-1} + k,  x_{-1} = first
//   both         out_i = 0 <= r_i < 2^CO ? r_i : miss
// -- the decoder of delta-coded columns, the window sum in row order, a row's position among the selected rows (the bitmap as a 1-bit
// column), and the encoder / the descent counter.  gfx950 only; part of libmi355scan.so through running/running_sum.hip and
// running/delta.hip.
//
// Pipeline.  The run-time-width tile stream of kernels/rt_column.hpp in, packed out: a wave owns tiles of 64 x 32 consecutive rows,
// lane l rows [32 l, 32 l + 32); the emitting kernels are templates of the OUTPUT width CO only, a lane's 32 results are exactly CO
// dwords (rt_insert<CO, K>), full tiles leave one tile late (rt_store), the ragged tile writes exactly the bytes it owns
// (rt_store_tail).  The input width is a wave-uniform run-time number: the tile travels by LDS-DMA into one of the wave's two images
// and is decoded from there (columns_lds_value).
//
// running_sum is three launches over the chunk prefix of kernels/bitmap.hpp (a chunk = 16384 rows = 8 tiles, a wave per chunk):
//   1  running_sum_totals_kernel  the chunk's sum of terms as a 64-bit word (two's complement) into the caller's workspace
//   2  rowid_scan_kernel          as it stands: unsigned wrap-around over those words is the signed sum
//   3  running_sum_exact_kernel<CO> / running_sum_checked_kernel<CO>: chunk_span_wave(...).before + k is the chunk's carry; per tile
//      the lane's 32 terms are summed, the lanes' totals go through an exclusive wave scan, the running sum walks the 32 rows again
//      and the carry moves on by the tile's total.
// Rows >= n of the ragged tile hold stale LDS: their terms are masked to zero in BOTH kernels, so they reach neither a chunk total,
// nor the carry, nor a stored byte, nor the counter.
//
// Arithmetic, as in arith/arith.hpp.  The host has bounded every partial sum in 128 bits: [k + n min(0, b), k + n max(0, 2^c - 1 + b)].
//   exact    the interval lies within [0, 2^CO - 1]: no test, no counter; 32-bit wrap-around arithmetic with b, k and the carry
//            reduced mod 2^32 yields the true result, which lies in [0, 2^32).
//   checked  the interval lies within int64: 64-bit wrap-around arithmetic is exact, (uint64)r >> CO == 0 is the range test, `miss`
//            is selected without a branch, a wave adds its count of replaced rows with ONE atomic at its end.
// delta has one kernel per family: exact when k >= 2^c - 1 and k + 2^c - 1 < 2^CO.  Its checked form needs no range rule: a
// result beyond int64 wraps to a value of magnitude >= 2^63 - 2^32, which the test sends to `miss` like the true one.
// The kernels test no switch bit.
#pragma once

#include <type_traits>

#include "../kernels.hpp"
#include "../kernels/rt_column.hpp" // the tile stream of a column of run-time width, and the packed-out half

namespace mi355 {

constexpr uint32_t kRunningInclusive = 0, kRunningExclusive = 1; // MI355_RUNNING_INCLUSIVE, MI355_RUNNING_EXCLUSIVE
constexpr int kRunningChunkRows = kRowidChunk * 8;               // 16384: the chunk of the prefix over a bitmap of n rows
constexpr int kRunningChunkTiles = kRunningChunkRows / kRtTileRows;
static_assert(kRunningChunkTiles == 8 && kRunningChunkTiles * kRtTileRows == kRunningChunkRows, "a chunk is a whole number of tiles");

struct RunningArgs {
    const uint8_t *packed;            // n values of c bits, 16 B aligned
    const uint8_t *mask;              // nullable: a bitmap of n rows, 4 B aligned, ceil(n / 8) bytes
    uint64_t n;
    uint8_t *out;                     // n values of CO bits, 16 B aligned; exactly ceil(n CO / 8) bytes are written
    unsigned long long *chunk_totals; // the caller's workspace: rowid_prefix_words(nchunks) words (kernels/bitmap.hpp ChunkPrefix)
    uint64_t nchunks;
    unsigned long long *result;       // nullable: [0] k + the sum of all terms, [1] rows replaced by miss (zeroed in front of the launch)
    int64_t b, k;
    uint32_t c;
    uint32_t miss;      // < 2^CO
    uint32_t exclusive; // 0 | 1
    uint32_t nts;       // result stores: 0 plain, 1 non-temporal, 2 write-through
};

struct DeltaArgs {
    const uint8_t *packed;
    uint64_t n;
    uint8_t *out;
    unsigned long long *out_of_range; // checked kernel, nullable: zeroed in front of the launch, one add per wave
    int64_t k;
    uint32_t c;
    uint32_t first; // x_{-1}, < 2^c
    uint32_t miss;
    uint32_t nts;
};

// a wave's two images of the column; + 16: the dword behind the last lane's run is read (and not used)
constexpr uint32_t running_wave_lds(uint32_t c) { return 2u * rt_image(c); }
constexpr uint32_t running_block_lds(uint32_t c) { return kWavesPerBlock * running_wave_lds(c) + 16u; }
static_assert(running_block_lds(32) <= kCuLdsBytes, "LDS budget");

// f(integral_constant<int, K>) for the K = 0 .. 31 of a lane's run, straight-line
template <int K = 0, typename F> __device__ __forceinline__ void running_rows(F &&f)
{
    f(std::integral_constant<int, K>{});
    if constexpr (K + 1 < kRtVpl) running_rows<K + 1>(f);
}

// the tile a wave that walks its chunks tile by tile takes after tile t: the chunk's next one, else the first of the wave's next chunk
__device__ __forceinline__ uint64_t running_next_tile(uint64_t t, uint64_t ntiles, uint64_t nwaves)
{
    const uint64_t nx = t + 1;
    if ((nx % kRunningChunkTiles) != 0 && nx < ntiles) return nx;
    return (t / kRunningChunkTiles + nwaves) * kRunningChunkTiles;
}

// the lane's dword of the mask for tile t: its 32 rows are exactly one dword (all ones without a mask)
__device__ __forceinline__ uint32_t running_mask_word(const RunningArgs &a, uint64_t mask_bytes, uint64_t t, int lane)
{
    if (!a.mask) return 0xffffffffu;
    return bitmap_word_at(a.mask, mask_bytes, (t * 64 + (uint64_t)lane) * 4);
}

// ---- launch 1: a chunk's sum of terms -------------------------------------------------------------------------------------
static __global__ __launch_bounds__(kBlockThreads) void running_sum_totals_kernel(RunningArgs a)
{
    constexpr int AUX = 0; // the column is read again by the emitting kernel: default policy
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t c = a.c;
    const uint32_t tile_bytes = rt_tile_bytes(c);
    uint8_t *cur = mi355_dyn_lds + (uint32_t)wave * running_wave_lds(c);
    uint8_t *nxt = cur + rt_image(c);
    const uint32_t vmask = rt_vmask(c);
    const uint64_t n = a.n;
    const uint64_t ntiles = rt_ntiles(n);
    const uint64_t data_bytes = (n * c + 7) / 8, mask_bytes = (n + 7) / 8;
    const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
    uint64_t tile = ((uint64_t)blockIdx.x * kWavesPerBlock + wave) * kRunningChunkTiles;
    uint32_t mnext = 0;
    auto issue = [&](uint64_t t, uint8_t *dst) {
        rt_issue_tile<AUX>(a.packed, data_bytes, tile_bytes, t, dst, lane);
        mnext = running_mask_word(a, mask_bytes, t, lane);
    };
    if (tile < ntiles) issue(tile, cur);
    unsigned long long acc = 0; // the lane's terms of the chunk so far
    while (tile < ntiles) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the tile has landed
        // rows >= n hold stale LDS: their terms are masked away
        const uint32_t m = mnext & tail_mask(lane_valid_rows<kRtVpl>(n, tile, lane), 0);
        const uint64_t next = running_next_tile(tile, ntiles, nwaves);
        if (next < ntiles) issue(next, nxt);
        const uint8_t *const base = cur + (uint32_t)lane * rt_lane_bytes(c);
        unsigned long long sx = 0;
        running_rows([&](auto K) {
            const uint32_t x = columns_lds_value<decltype(K)::value>(base, c, vmask);
            sx += (m >> decltype(K)::value) & 1u ? x : 0u;
        });
        acc += sx + (unsigned long long)a.b * (unsigned long long)__builtin_popcount(m);
        if ((tile + 1) % kRunningChunkTiles == 0 || tile + 1 >= ntiles) { // the chunk ends: 64-bit wrap-around is the signed sum
            const unsigned long long total = wave_sum64(acc);
            if (lane == 0) a.chunk_totals[tile / kRunningChunkTiles] = total;
            acc = 0;
        }
        uint8_t *t = cur;
        cur = nxt;
        nxt = t;
        tile = next;
    }
}

// ---- launch 3: the running sum itself -------------------------------------------------------------------------------------
template <int CO, bool CHECKED> __device__ __forceinline__ void running_sum_body(const RunningArgs &a)
{
    using T = std::conditional_t<CHECKED, unsigned long long, uint32_t>; // the arithmetic: 64-bit, or 32-bit wrap-around
    constexpr int AUX = 2;                                               // the column's last read: non-temporal DMA
    constexpr uint32_t OUT_TILE = rt_tile_bytes(CO);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t c = a.c;
    const uint32_t tile_bytes = rt_tile_bytes(c);
    uint8_t *cur = mi355_dyn_lds + (uint32_t)wave * running_wave_lds(c);
    uint8_t *nxt = cur + rt_image(c);
    const uint32_t vmask = rt_vmask(c);
    const uint64_t n = a.n;
    const uint64_t ntiles = rt_ntiles(n), nfull = rt_nfull(n);
    const uint64_t data_bytes = (n * c + 7) / 8, mask_bytes = (n + 7) / 8;
    const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
    uint64_t tile = ((uint64_t)blockIdx.x * kWavesPerBlock + wave) * kRunningChunkTiles;
    const uint32_t nts = a.nts;
    const T b = (T)a.b;
    const T with_own = a.exclusive ? (T)0 : ~(T)0; // inclusive: a row's own term counts
    const ChunkPrefix prefix{a.chunk_totals, a.nchunks};
    uint32_t mnext = 0;
    auto issue = [&](uint64_t t, uint8_t *dst) {
        rt_issue_tile<AUX>(a.packed, data_bytes, tile_bytes, t, dst, lane);
        mnext = running_mask_word(a, mask_bytes, t, lane);
    };
    if (tile < ntiles) issue(tile, cur);

    uint32_t res[CO];
    uint64_t prev = ~0ull;
    unsigned long long outside = 0; // CHECKED: the lane's replaced rows so far
    T carry = 0;                    // k + every term in front of the tile
    uint8_t *const out_lane = a.out + (uint32_t)lane * (4u * CO);
    while (tile < ntiles) {
        // a chunk begins: what the prefix has in front of it (the loads travel beside the tile)
        if (tile % kRunningChunkTiles == 0) carry = (T)(chunk_span_wave(prefix, tile / kRunningChunkTiles, lane).before + (unsigned long long)a.k);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the tile has landed
        const int valid = lane_valid_rows<kRtVpl>(n, tile, lane);
        const uint32_t m = mnext & tail_mask(valid, 0); // rows >= n hold stale LDS: no term
        if (prev != ~0ull) store_words_by<CO>(out_lane + prev * OUT_TILE, res, nts);
        const uint64_t next = running_next_tile(tile, ntiles, nwaves);
        if (next < ntiles) issue(next, nxt);

        const uint8_t *const base = cur + (uint32_t)lane * rt_lane_bytes(c);
        uint32_t x[kRtVpl];
        T mine = 0;
        running_rows([&](auto K) {
            constexpr int k = decltype(K)::value;
            x[k] = columns_lds_value<k>(base, c, vmask);
            mine += (m >> k) & 1u ? (T)x[k] + b : (T)0;
        });
        // the lanes' totals: exclusive scan over the wave, and the tile's total
        T before, total;
        if constexpr (CHECKED) {
            unsigned long long incl = mine;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned long long t = __shfl_up(incl, d, 64);
                if (lane >= d) incl += t;
            }
            before = incl - mine;
            total = __shfl(incl, 63, 64);
        } else {
            const uint32_t incl = wave_inclusive_scan(mine);
            before = incl - mine;
            total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        }
        T r = carry + before;
        uint32_t bad = 0;
        running_rows([&](auto K) {
            constexpr int k = decltype(K)::value;
            const T t = (m >> k) & 1u ? (T)x[k] + b : (T)0;
            const T e = r + (t & with_own);
            r += t;
            if constexpr (CHECKED) {
                // 64-bit wrap-around is exact under the range rule; (uint64)e >> CO also sends a negative sum to `miss`
                const bool in = (e >> CO) == 0;
                rt_insert<CO, k>(res, in ? (uint32_t)e : a.miss);
                bad |= in ? 0u : (1u << k);
            } else {
                rt_insert<CO, k>(res, (uint32_t)e); // the true sum lies in [0, 2^CO): 32-bit wrap-around yields it
            }
        });
        if (tile < nfull) {
            prev = tile;
        } else {
            rt_store_tail<CO>(out_lane + tile * OUT_TILE, res, valid);
            bad &= tail_mask(valid, 0);
            prev = ~0ull;
        }
        if constexpr (CHECKED) outside += (uint32_t)__builtin_popcount(bad);
        carry += total;
        if (tile + 1 == ntiles && a.result && lane == 0) a.result[0] = (unsigned long long)carry; // exact: the total lies in [0, 2^32)
        uint8_t *t = cur;
        cur = nxt;
        nxt = t;
        tile = next;
    }
    if (prev != ~0ull) store_words_by<CO>(out_lane + prev * OUT_TILE, res, nts);
    if constexpr (CHECKED) {
        if (a.result) {
            const unsigned long long total = wave_sum64(outside);
            if (lane == 0 && total) __hip_atomic_fetch_add(a.result + 1, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <int CO> __global__ __launch_bounds__(kBlockThreads) void running_sum_exact_kernel(RunningArgs a) { running_sum_body<CO, false>(a); }

template <int CO> __global__ __launch_bounds__(kBlockThreads) void running_sum_checked_kernel(RunningArgs a) { running_sum_body<CO, true>(a); }

// ---- delta: tiles dealt out across the waves ------------------------------------------------------------------------------
// the last row of tile t - 1 (t >= 1), straight from global memory: it ends on the tile's first byte, so its c bits are the top c of
// the two dwords in front of that byte (the same address in every lane)
__device__ __forceinline__ uint32_t delta_row_before_tile(const uint8_t *packed, uint32_t c, uint64_t t)
{
    const uint32_t *const w = (const uint32_t *)packed + t * (uint64_t)(64u * c);
    const unsigned long long pair = ((unsigned long long)w[-1] << 32) | w[-2];
    return (uint32_t)(pair >> (64u - c));
}

template <int CO, bool CHECKED> __device__ __forceinline__ void delta_body(const DeltaArgs &a)
{
    using T = std::conditional_t<CHECKED, unsigned long long, uint32_t>;
    constexpr int AUX = 2; // the column is streamed once: non-temporal DMA
    constexpr uint32_t OUT_TILE = rt_tile_bytes(CO);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t c = a.c;
    const uint32_t tile_bytes = rt_tile_bytes(c);
    uint8_t *cur = mi355_dyn_lds + (uint32_t)wave * running_wave_lds(c);
    uint8_t *nxt = cur + rt_image(c);
    const uint32_t vmask = rt_vmask(c);
    const uint64_t n = a.n;
    const uint64_t ntiles = rt_ntiles(n), nfull = rt_nfull(n);
    const uint64_t data_bytes = (n * c + 7) / 8;
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock;
    uint64_t tile = (uint64_t)blockIdx.x * kWavesPerBlock + wave;
    const uint32_t nts = a.nts;
    const T k = (T)a.k;
    uint32_t edge = 0; // the row in front of the tile in flight: lane 0's x_{-1}
    auto issue = [&](uint64_t t, uint8_t *dst) {
        rt_issue_tile<AUX>(a.packed, data_bytes, tile_bytes, t, dst, lane);
        edge = t ? delta_row_before_tile(a.packed, c, t) : a.first; // beside the DMA, not behind the wait
    };
    if (tile < ntiles) issue(tile, cur);

    uint32_t res[CO];
    uint64_t prev = ~0ull;
    unsigned long long outside = 0;
    uint8_t *const out_lane = a.out + (uint32_t)lane * (4u * CO);
    // the row in front of the lane's run, row 32 lane - 1 of the same image: a lane-varying bit offset
    const uint32_t back_bit = (uint32_t)lane * (kRtVpl * c) - c; // (lane > 0)
    while (tile < ntiles) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the tile has landed
        uint32_t xp = edge;
        if (prev != ~0ull) store_words_by<CO>(out_lane + prev * OUT_TILE, res, nts);
        const uint64_t next = tile + stride;
        if (next < ntiles) issue(next, nxt);

        if (lane > 0) {
            const uint32_t *const p = (const uint32_t *)(cur + (back_bit >> 5) * 4);
            xp = __builtin_amdgcn_alignbit(p[1], p[0], back_bit & 31u) & vmask;
        }
        const uint8_t *const base = cur + (uint32_t)lane * rt_lane_bytes(c);
        uint32_t bad = 0;
        running_rows([&](auto K) {
            constexpr int kk = decltype(K)::value;
            const uint32_t x = columns_lds_value<kk>(base, c, vmask);
            const T e = (T)x - (T)xp + k;
            xp = x;
            if constexpr (CHECKED) {
                const bool in = (e >> CO) == 0;
                rt_insert<CO, kk>(res, in ? (uint32_t)e : a.miss);
                bad |= in ? 0u : (1u << kk);
            } else {
                rt_insert<CO, kk>(res, (uint32_t)e); // k - (2^c - 1) >= 0 and k + 2^c - 1 < 2^CO: stale rows included
            }
        });
        if (tile < nfull) {
            prev = tile;
        } else {
            // rows >= n hold stale LDS: they reach neither a stored byte nor the counter
            const int valid = lane_valid_rows<kRtVpl>(n, tile, lane);
            rt_store_tail<CO>(out_lane + tile * OUT_TILE, res, valid);
            bad &= tail_mask(valid, 0);
            prev = ~0ull;
        }
        if constexpr (CHECKED) outside += (uint32_t)__builtin_popcount(bad);
        uint8_t *t = cur;
        cur = nxt;
        nxt = t;
        tile = next;
    }
    if (prev != ~0ull) store_words_by<CO>(out_lane + prev * OUT_TILE, res, nts);
    if constexpr (CHECKED) {
        if (a.out_of_range) {
            const unsigned long long total = wave_sum64(outside);
            if (lane == 0 && total) __hip_atomic_fetch_add(a.out_of_range, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <int CO> __global__ __launch_bounds__(kBlockThreads) void delta_exact_kernel(DeltaArgs a) { delta_body<CO, false>(a); }

template <int CO> __global__ __launch_bounds__(kBlockThreads) void delta_checked_kernel(DeltaArgs a) { delta_body<CO, true>(a); }

} // namespace mi355
