// extras/histogram.hpp -- how often every value occurs in a packed column (SELECT v, count(*) ... GROUP BY v -- with the
// c-bit value a dictionary index, the usual aggregation over a dictionary-coded column), optionally only over the rows of a
// bitmap.  Widths up to 14 bits: the 2^c counters live in LDS, one LDS atomic per value, one global atomic per non-empty
// counter and block at the end.  Built from the scan's tile pipeline; included by extras.hip only.
#pragma once

#include "../launch_util.hpp"
#include "../kernels.hpp"
#include "../kernels/rt_column.hpp" // lane_valid_rows: the ragged last tile

namespace mi355 {

constexpr int kHistogramMaxBits = 14; // 2^14 counters = 64 KiB of LDS next to the block's tiles

struct HistArgs {
    const uint8_t *packed; // 16 B aligned
    uint64_t n;
    const uint8_t *mask;     // rows that count (ceil(n/8) bytes, 4 B aligned) or null = every row
    unsigned long long *out; // 2^C counters, zeroed in front of the launch
};

template <int C, int VPL>
__global__ __launch_bounds__(kBlockThreads) void histogram_kernel(HistArgs a)
{
    static_assert(C <= kHistogramMaxBits, "the counters must fit in LDS");
    using G = ScanGeom<C, VPL>;
    constexpr int WORDS = G::WORDS;
    constexpr int AUX = 2; // the column is streamed once: non-temporal DMA
    __shared__ __attribute__((aligned(16))) uint8_t lds[kWavesPerBlock][G::LDS_BYTES];
    __shared__ uint32_t hist[1 << C]; // a block sees at most n / gridDim.x values: 32 bits are plenty
    for (uint32_t k = threadIdx.x; k < (1u << C); k += kBlockThreads) hist[k] = 0;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint8_t *lds_wave = lds[wave];
    const TileCtx<C, VPL> tc(a.n);
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock;
    uint64_t tile = (uint64_t)blockIdx.x * kWavesPerBlock + wave;
    const uint64_t nbytes = (a.n + 7) / 8;

    auto load_mask = [&](uint64_t t, uint32_t (&m)[WORDS]) { // the lane's mask words of a tile; no mask: every row counts
#pragma unroll
        for (int j = 0; j < WORDS; j++) m[j] = 0xffffffffu;
        if (a.mask) tc.template load_bitmap_words<true>(a.mask, t, lane, m, nbytes);
    };

    uint32_t mnext[WORDS];
    if (tile < tc.ntiles) {
        tc.template issue<AUX>(a.packed, tile, lds_wave, lane);
        load_mask(tile, mnext);
    }
    __syncthreads(); // the counters are zero
    while (tile < tc.ntiles) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        uint32_t w[G::LANE_DWORDS];
        read_lane_data<C, VPL>(lds_wave, lane, w);
        uint32_t m[WORDS];
#pragma unroll
        for (int j = 0; j < WORDS; j++) m[j] = mnext[j];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const uint64_t next = tile + stride;
        if (next < tc.ntiles) {
            tc.template issue<AUX>(a.packed, next, lds_wave, lane);
            load_mask(next, mnext);
        }
        const bool full = tile < tc.nfull;
        if (!full) { // rows behind the column count for nothing
            const int valid = lane_valid_rows<VPL>(a.n, tile, lane);
#pragma unroll
            for (int j = 0; j < WORDS; j++) m[j] &= tail_mask(valid, j);
        }
        uint32_t xs[VPL];
        extract_all<C, VPL, 0, G::LANE_DWORDS>(w, xs);
        if (!a.mask && full) {
#pragma unroll
            for (int v = 0; v < VPL; v++) __hip_atomic_fetch_add(&hist[xs[v]], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
#pragma unroll
            for (int v = 0; v < VPL; v++)
                if ((m[v >> 5] >> (v & 31)) & 1u) __hip_atomic_fetch_add(&hist[xs[v]], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        tile = next;
    }
    __syncthreads(); // every wave's adds are done
    for (uint32_t k = threadIdx.x; k < (1u << C); k += kBlockThreads) {
        const uint32_t v = hist[k];
        if (v) __hip_atomic_fetch_add(a.out + k, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Env: LaunchEnv (ctx.hpp).  Option "max_blocks_per_cu" does not reach this grid.
template <int C, typename Env> inline void launch_histogram(const Env &env, const HistArgs &a)
{
    constexpr int VPL = 128;
    using G = ScanGeom<C, VPL>;
    const uint64_t ntiles = (a.n + G::TILE_VALUES - 1) / G::TILE_VALUES;
    const unsigned grid = grid_for(ntiles, counters_bpc(G::LDS_BYTES, 4u << C), env.num_cus);
    MI355_LAUNCH(env.record, 0, (histogram_kernel<C, VPL>), dim3(grid), dim3(kBlockThreads), 0, env.stream, a);
}

template <typename Env> inline hipError_t launch_histogram_width(unsigned c, const Env &env, const HistArgs &a)
{
    return launch_by_width<1, kHistogramMaxBits>(c, a, [&](auto w, const HistArgs &q) { return launch_histogram<decltype(w)::value>(env, q), hipSuccess; });
}

} // namespace mi355
