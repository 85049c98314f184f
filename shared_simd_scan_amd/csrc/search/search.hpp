// search/search.hpp -- the device code of mi355_search_sorted_dev: for every row x_i of a packed column its position in a sorted
// packed table t, pos_i = #{j < R : t_j < x_i} (LEFT) or #{j < R : t_j <= x_i} (RIGHT), packed out, the bitmap of the rows that
// end beside an equal entry and their number.  gfx950 only; part of libmi355scan.so through search/search_sorted.hip.
//
// Pipeline.  lookup's (lookup/lookup.hpp), on the run-time-width tile stream of kernels/rt_column.hpp: a wave owns tiles of
// 64 x 32 consecutive rows, lane l rows [32 l, 32 l + 32).  The column travels by non-temporal LDS-DMA into two alternating
// images and is decoded from there (columns_lds_value); the lane's 32 positions are CO whole dwords (rt_insert<CO, K>) and leave
// one tile later (rt_store), the ragged tile writes exactly its bytes (rt_store_tail).  The lane's 32 found bits are one dword of
// the bitmap, at byte 4 lane of the tile's 256.  The kernels are templates of the OUTPUT width CO only; c and ct are wave-uniform
// run-time numbers.  Without out_dev the same instance runs and a uniform branch skips its position stores.
//
// One descent for both tiers.  pos = 0; for s = top, top / 2, ..., 1 (top: the largest power of two <= `rows`, a host number,
// so the step count is wave-uniform): cand = pos + s is accepted when cand <= R and t[min(cand, R) - 1] < x (RIGHT: <= x --
// never `< x + 1`, which wraps at x = 2^32 - 1).  Every index lies in [0, R): that is the bound on reads whatever the table
// holds, sorted or not, and pos <= R follows.  R == 0 skips the descent: the table is not read.  A lane's 32 descents are
// independent: each step issues its 32 reads before the first is consumed.  RIGHT: found = the last accepted entry equals x (no
// further read); LEFT: one clamped read of t[min(pos, R - 1)].
//
// Samples.  The block keeps sample[k] = t[(k + 1) S - 1], for (k + 1) S <= R, as uint32 in its dynamic LDS behind the waves'
// images, staged while its first tiles are in flight.  While s >= S, pos and cand are multiples of S, so the entry cand - 1 a
// probe with cand <= R reads is sample cand / S - 1: those steps are one ds_read_b32 each.  A probe with cand > R is discarded
// whatever it reads; its sample index is clamped into the staged ones (into the table's first LDS dword when none is staged).
//   search_lds_kernel    rows * 4 <= kSearchLdsMaxBytes: S = 1, every entry is a sample, no step reads global memory.
//   search_global_kernel everything larger: S = search_stride(rows), the smallest power of two whose samples fit.  The log2 S
//                        steps below S read the table where it lies, one or two dwords and v_alignbit_b32, with the DEFAULT cache
//                        policy: the table's hot levels live in L2 and the Infinity Cache while the column streams past them.
// Of the table only the dwords 0 .. last_word are ever read, last_word the dword that holds the last bit of entry R - 1; a
// value's second dword is min(w + 1, last_word), as runs/runs.hpp's run_entry reads it (SearchRead splits that read into issue
// and use, so that 32 of them are in flight).
//   LDS budget: all of a block's LDS is dynamic.  The waves' images take 4 x 2 x 8 KiB at c = 32; what is left of a CU's 160 KiB
//   minus kSearchLdsSlack is the samples' ceiling kSearchLdsMaxBytes.  The launcher sizes the dynamic LDS to c and `rows`, so a
//   narrow column and a short edge list leave room for several blocks per CU.
// The kernels test no switch bit.
#pragma once

#include "../kernels.hpp"
#include "../kernels/rt_column.hpp" // the tile stream of a column of run-time width, and the packed-out half

namespace mi355 {

struct SearchArgs {
    const uint8_t *packed;              // n values of c bits, 16 B aligned
    uint64_t n;
    const uint32_t *table;              // entries of ct bits, 4 B aligned; dwords 0 .. last_word are read and no more
    const unsigned long long *rows_dev; // nullable: R = min(rows, *rows_dev)
    uint8_t *out;                       // nullable: n values of CO bits, 16 B aligned
    uint8_t *found;                     // nullable: the bitmap of n rows, 4 B aligned
    unsigned long long *hits;           // nullable: zeroed in front of the kernel; one atomic per wave
    uint32_t rows;                      // the host's bound of R
    uint32_t top;                       // the largest power of two <= rows; 0: no step
    uint32_t lg;                        // log2 S
    uint32_t c, ct;
    uint32_t right;                     // MI355_SEARCH_RIGHT
    uint32_t exact;
    uint32_t miss;                      // < 2^CO
    uint32_t nts;                       // result stores: 0 plain, 1 non-temporal, 2 write-through (one uniform branch per tile)
};

constexpr uint32_t kSearchLdsSlack = 64; // the dword behind the last lane's run, rounding to 16

// the waves' images of a block, two per wave; + 16: the dword behind the last lane's run is read (and not used)
constexpr uint32_t search_images_lds(uint32_t c) { return kWavesPerBlock * 2u * rt_image(c) + 16u; }
// MI355_SEARCH_LDS_MAX_BYTES: what the widest images (c = 32) leave of a CU's LDS for the samples
constexpr uint32_t kSearchLdsMaxBytes = (kCuLdsBytes - kWavesPerBlock * 2u * rt_image(32) - kSearchLdsSlack) & ~15u;
static_assert(search_images_lds(32) + kSearchLdsMaxBytes <= kCuLdsBytes, "LDS budget");
constexpr bool search_in_lds(uint64_t rows) { return rows * 4u <= kSearchLdsMaxBytes; }
// S: the smallest power of two with floor(rows / S) samples inside the ceiling (rows <= 2^32 - 1)
constexpr uint64_t search_stride(uint64_t rows)
{
    uint64_t s = 1;
    while ((rows / s) * 4u > kSearchLdsMaxBytes) s <<= 1;
    return s;
}
// dynamic LDS of the samples: whole 16 bytes, and a dword for the clamped probe where none is staged
constexpr uint32_t search_samples_lds(uint64_t rows) { return (uint32_t)(((rows / search_stride(rows)) * 4u + 16u) & ~15ull); }
static_assert(search_stride(kSearchLdsMaxBytes / 4) == 1 && search_stride(kSearchLdsMaxBytes / 4 + 1) == 2, "the tier boundary");
static_assert(search_images_lds(32) + search_samples_lds(kSearchLdsMaxBytes / 4) <= kCuLdsBytes, "LDS budget");
static_assert(search_samples_lds(0xffffffffull) <= kSearchLdsMaxBytes + 16u, "the samples of the largest table fit");

// the table as the descent reads it: entries of run-time width w, never beyond dword last_word
struct SearchTable {
    const uint32_t *table;
    uint32_t w, vmask, last_word;
    bool one_dword; // w divides 32: no entry straddles a dword, the second load is skipped (wave-uniform)
};
// entry j (< R) where it lies, issue and use apart: one or two dwords, v_alignbit_b32, a mask
struct SearchRead {
    uint32_t lo, hi;
    template <bool ONE> __device__ __forceinline__ void load(const SearchTable &t, uint32_t j)
    {
        const uint32_t d = (uint32_t)(((uint64_t)j * t.w) >> 5); // j w needs 37 bits, the dword index 32
        lo = t.table[d];
        hi = lo;
        if constexpr (!ONE) hi = t.table[d < t.last_word ? d + 1u : t.last_word];
    }
    __device__ __forceinline__ uint32_t value(const SearchTable &t, uint32_t j) const
    {
        return __builtin_amdgcn_alignbit(hi, lo, (j * t.w) & 31u) & t.vmask;
    }
};

// the block's samples t[(k + 1) S - 1], k < R >> lg.  Every thread of the block calls it (barrier inside).
__device__ __forceinline__ void search_stage_samples(const SearchTable &t, uint32_t *samples, uint32_t R, uint32_t lg)
{
    const uint32_t ns = R >> lg;
    constexpr uint32_t kInFlight = 8; // entries a thread loads before it stores the first
    for (uint32_t k0 = threadIdx.x; k0 < ns; k0 += kInFlight * kBlockThreads) {
        SearchRead r[kInFlight];
#pragma unroll
        for (uint32_t q = 0; q < kInFlight; q++) {
            const uint32_t k = k0 + q * kBlockThreads;
            if (k < ns) r[q].template load<false>(t, ((k + 1u) << lg) - 1u);
        }
#pragma unroll
        for (uint32_t q = 0; q < kInFlight; q++) {
            const uint32_t k = k0 + q * kBlockThreads;
            if (k < ns) samples[k] = r[q].value(t, ((k + 1u) << lg) - 1u);
        }
    }
    __syncthreads();
}

// the lane's 32 input values out of the image (run-time width: scalar offsets)
template <int K = 0> __device__ __forceinline__ void search_decode(const uint8_t *base, uint32_t c, uint32_t vmask, uint32_t (&v)[kRtVpl])
{
    v[K] = columns_lds_value<K>(base, c, vmask);
    if constexpr (K + 1 < kRtVpl) search_decode<K + 1>(base, c, vmask, v);
}

// The descents of a lane's 32 rows, R >= 1 -> pos, and the rows that end beside an equal entry as a bit each.
// RIGHT: the comparison of the launch (wave-uniform; the caller branches once per tile).
template <bool GLOBAL, bool RIGHT>
__device__ __forceinline__ uint32_t search_descend(const SearchTable &t, const uint32_t *samples, uint32_t R, uint32_t top, uint32_t lg,
                                                   const uint32_t (&x)[kRtVpl], uint32_t (&pos)[kRtVpl])
{
    constexpr int VPL = kRtVpl;
    const uint32_t ns = R >> lg;
    uint32_t last[RIGHT ? VPL : 1]; // RIGHT: the entry of the last accepted step
#pragma unroll
    for (int k = 0; k < VPL; k++) pos[k] = 0;
    if constexpr (RIGHT) {
#pragma unroll
        for (int k = 0; k < VPL; k++) last[k] = 0;
    }
    for (uint32_t s = top; s; s >>= 1) {
        uint32_t e[VPL];
        if (!GLOBAL || (s >> lg)) {
            // s >= S: entry cand - 1 is sample cand / S - 1; beyond R the clamped one (discarded below)
#pragma unroll
            for (int k = 0; k < VPL; k++) {
                const uint32_t cs = (pos[k] + s) >> lg;
                const uint32_t kk = cs < ns ? cs : ns;
                e[k] = samples[kk ? kk - 1u : 0u];
            }
        } else {
            // s < S: the table where it lies, every load of the lane's step issued before the first is consumed
            SearchRead r[VPL];
            if (t.one_dword) { // one branch per step, not one per load
#pragma unroll
                for (int k = 0; k < VPL; k++) {
                    const uint32_t cand = pos[k] + s;
                    r[k].template load<true>(t, (cand < R ? cand : R) - 1u); // R >= 1, cand >= 1
                }
            } else {
#pragma unroll
                for (int k = 0; k < VPL; k++) {
                    const uint32_t cand = pos[k] + s;
                    r[k].template load<false>(t, (cand < R ? cand : R) - 1u);
                }
            }
            __builtin_amdgcn_sched_barrier(0); // (the scheduler would otherwise start on the first value after some of the loads)
#pragma unroll
            for (int k = 0; k < VPL; k++) {
                const uint32_t cand = pos[k] + s;
                e[k] = r[k].value(t, (cand < R ? cand : R) - 1u);
            }
        }
#pragma unroll
        for (int k = 0; k < VPL; k++) {
            const uint32_t cand = pos[k] + s; // <= 2 top - 1: no wrap
            const bool ok = cand <= R && (RIGHT ? e[k] <= x[k] : e[k] < x[k]);
            pos[k] = ok ? cand : pos[k];
            if constexpr (RIGHT) last[k] = ok ? e[k] : last[k];
        }
    }
    uint32_t fnd = 0;
    if constexpr (RIGHT) {
#pragma unroll
        for (int k = 0; k < VPL; k++) fnd |= (pos[k] != 0 && last[k] == x[k] ? 1u : 0u) << k;
    } else {
        // one clamped read of t[pos]
        uint32_t e[VPL];
        if constexpr (!GLOBAL) {
#pragma unroll
            for (int k = 0; k < VPL; k++) e[k] = samples[pos[k] < R ? pos[k] : R - 1u];
        } else {
            SearchRead r[VPL];
            if (t.one_dword) {
#pragma unroll
                for (int k = 0; k < VPL; k++) r[k].template load<true>(t, pos[k] < R ? pos[k] : R - 1u);
            } else {
#pragma unroll
                for (int k = 0; k < VPL; k++) r[k].template load<false>(t, pos[k] < R ? pos[k] : R - 1u);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < VPL; k++) e[k] = r[k].value(t, pos[k] < R ? pos[k] : R - 1u);
        }
#pragma unroll
        for (int k = 0; k < VPL; k++) fnd |= (pos[k] < R && e[k] == x[k] ? 1u : 0u) << k;
    }
    return fnd;
}

// both tiers.  GLOBAL: the steps below S read the table where it lies; else S = 1 and every step reads LDS.
template <int CO, bool GLOBAL> __device__ __forceinline__ void search_body(const SearchArgs &a)
{
    constexpr int VPL = kRtVpl;
    constexpr int AUX = 2; // the column is streamed once: non-temporal DMA
    constexpr uint32_t OUT_TILE = rt_tile_bytes(CO); // output bytes of a tile
    constexpr uint32_t BIT_TILE = kRtTileRows / 8;   // bitmap bytes of a tile
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t c = a.c;
    const uint32_t tile_bytes = rt_tile_bytes(c); // a multiple of 256
    const uint32_t image = rt_image(c);
    uint8_t *cur = mi355_dyn_lds + (uint32_t)wave * 2u * image; // the image being decoded ...
    uint8_t *nxt = cur + image;                                 // ... and where the next tile lands
    uint32_t *const samples = (uint32_t *)(mi355_dyn_lds + search_images_lds(c)); // the block's samples, behind the images
    const uint32_t vmask = rt_vmask(c);

    const uint64_t n = a.n;
    const uint64_t ntiles = rt_ntiles(n), nfull = rt_nfull(n);
    const uint64_t data_bytes = (n * c + 7) / 8;
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock;
    uint64_t tile = (uint64_t)blockIdx.x * kWavesPerBlock + wave;
    const uint32_t top = a.top, lg = GLOBAL ? a.lg : 0u, miss = a.miss, nts = a.nts;
    const bool right = a.right != 0, exact = a.exact != 0, with_out = a.out != nullptr, with_found = a.found != nullptr;

    auto issue = [&](uint64_t t, uint8_t *dst) { rt_issue_tile<AUX>(a.packed, data_bytes, tile_bytes, t, dst, lane); };
    if (tile < ntiles) issue(tile, cur);

    // R, read on the device; the samples, staged while the first tiles are in flight
    uint32_t R = a.rows;
    if (a.rows_dev) {
        const unsigned long long have = uniform64(*a.rows_dev);
        R = have < R ? (uint32_t)have : R;
    }
    const SearchTable t{a.table, a.ct, rt_vmask(a.ct), R ? (uint32_t)(((uint64_t)R * a.ct - 1) >> 5) : 0u, 32u % a.ct == 0u};
    search_stage_samples(t, samples, R, lg);

    uint32_t res[CO];
    uint32_t fprev = 0;
    unsigned long long hits = 0;
    uint64_t prev = ~0ull;
    uint8_t *const out_lane = a.out + (uint32_t)lane * (4u * CO);
    uint8_t *const found_lane = a.found + (uint32_t)lane * 4u;
    auto store_prev = [&]() {
        if (with_out) store_words_by<CO>(out_lane + prev * OUT_TILE, res, nts);
        if (with_found) {
            const uint32_t w[1] = {fprev};
            store_words_by<1>(found_lane + prev * BIT_TILE, w, nts);
        }
    };
    while (tile < ntiles) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the tile has landed
        if (prev != ~0ull) store_prev();
        const uint64_t next = tile + stride;
        if (next < ntiles) issue(next, nxt);

        uint32_t x[VPL], pos[VPL];
        search_decode(cur + (uint32_t)lane * rt_lane_bytes(c), c, vmask, x);
        uint32_t fnd = 0;
        if (R == 0) {
#pragma unroll
            for (int k = 0; k < VPL; k++) pos[k] = 0;
        } else if (right) {
            fnd = search_descend<GLOBAL, true>(t, samples, R, top, lg, x, pos);
        } else {
            fnd = search_descend<GLOBAL, false>(t, samples, R, top, lg, x, pos);
        }
        if (exact) {
#pragma unroll
            for (int k = 0; k < VPL; k++) pos[k] = (fnd >> k) & 1u ? pos[k] : miss;
        }
        rt_insert_all<CO>(res, pos);
        if (tile < nfull) {
            prev = tile;
            fprev = fnd;
        } else {
            const int valid = lane_valid_rows<VPL>(n, tile, lane);
            fnd &= tail_mask(valid, 0); // rows >= n reach neither a stored byte nor the counter
            if (with_out) rt_store_tail<CO>(out_lane + tile * OUT_TILE, res, valid);
            if (with_found) {
                uint8_t *const dst = found_lane + tile * BIT_TILE;
#pragma unroll
                for (int b = 0; b < 4; b++)
                    if (8 * b < valid) dst[b] = (uint8_t)(fnd >> (8 * b));
            }
            prev = ~0ull;
        }
        hits += (uint32_t)__builtin_popcount(fnd);
        uint8_t *const t2 = cur;
        cur = nxt;
        nxt = t2;
        tile = next;
    }
    if (prev != ~0ull) store_prev();
    if (a.hits) {
        const unsigned long long total = wave_sum64(hits);
        if (lane == 0 && total) __hip_atomic_fetch_add(a.hits, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <int CO> __global__ __launch_bounds__(kBlockThreads) void search_lds_kernel(SearchArgs a) { search_body<CO, false>(a); }

template <int CO> __global__ __launch_bounds__(kBlockThreads) void search_global_kernel(SearchArgs a) { search_body<CO, true>(a); }

} // namespace mi355
