// extras/aggregate.hpp -- sum / min / max / count of a packed column, optionally only over the rows of a bitmap
// (SELECT sum(b), min(b), max(b), count(*) WHERE <bitmap>): the consumer that ends most predicate chains.  Built from the
// scan's pipeline (kernels/tile.hpp, kernels/scan.hpp: LDS-DMA tiles, lane owns a run, compile-time bit offsets) but not
// one of the profiled hot-path kernels; included by extras.hip only.
#pragma once

#include "../launch_util.hpp"
#include "../kernels.hpp"

namespace mi355 {

struct AggArgs {
    const uint8_t *packed; // 16 B aligned
    uint64_t n;
    const uint8_t *mask;   // bitmap of the rows that count (ceil(n/8) bytes, 4 B aligned) or null = every row
    unsigned long long *out; // [0] sum, [1] count, [2] min, [3] max -- initialised to 0, 0, ~0, 0 in front of the launch
};

static __global__ void aggregate_init_kernel(unsigned long long *out)
{
    out[0] = 0;
    out[1] = 0;
    out[2] = ~0ull;
    out[3] = 0;
}

// One pass over the column: per value an extraction, the row's bitmap bit spread over a word (v_bfe_i32), AND, add, max, and
// for the minimum a subtraction and a max (see the loop).  The lane's sum of a tile stays in 32 bits while 128 * 2^C fits
// (C <= 24), else 64.  ~7.5 VALU operations per value with a mask, ~4.5 without: at c = 9 about the time of the stream.
template <int C, int VPL>
__global__ __launch_bounds__(kBlockThreads) void aggregate_kernel(AggArgs a)
{
    using G = ScanGeom<C, VPL>;
    constexpr int WORDS = G::WORDS;
    constexpr int AUX = 2; // the column is streamed once: non-temporal DMA
    __shared__ __attribute__((aligned(16))) uint8_t lds[kWavesPerBlock][G::LDS_BYTES];
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

    unsigned long long sum = 0, cnt = 0;
    uint32_t nmn = 0, mx = 0; // nmn: maximum of ~value over the rows that count (the minimum, complemented)
    uint32_t mnext[WORDS];
    if (tile < tc.ntiles) {
        tc.template issue<AUX>(a.packed, tile, lds_wave, lane);
        load_mask(tile, mnext);
    }
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
        if (tile >= tc.nfull) { // rows behind the column count for nothing
            const int64_t left = (int64_t)(a.n - tile * G::TILE_VALUES) - (int64_t)lane * VPL; // (lane_valid_rows compiles to another stream)
            const int valid = left >= VPL ? VPL : (left <= 0 ? 0 : (int)left);
#pragma unroll
            for (int j = 0; j < WORDS; j++) m[j] &= tail_mask(valid, j);
        }
        uint32_t xs[VPL];
        extract_all<C, VPL, 0, G::LANE_DWORDS>(w, xs);
        uint32_t s32 = 0;
        unsigned long long s64 = 0;
        if (!a.mask && tile < tc.nfull) {
            // every row counts: add, max, min per value
#pragma unroll
            for (int v = 0; v < VPL; v++) {
                const uint32_t x = xs[v];
                if constexpr (C <= 24)
                    s32 += x;
                else
                    s64 += x;
                mx = x > mx ? x : mx;
                nmn = ~x > nmn ? ~x : nmn;
            }
        } else {
            // sel = the row's bitmap bit spread over the word (one v_bfe_i32); excluded rows contribute 0 to the sum and the
            // maximum; the minimum is kept as the maximum of sel - x (= ~x for a row that counts, 0 for one that does not)
#pragma unroll
            for (int v = 0; v < VPL; v++) {
                const uint32_t sel = (uint32_t)__builtin_amdgcn_sbfe((int)m[v >> 5], v & 31, 1);
                const uint32_t x = xs[v] & sel;
                if constexpr (C <= 24)
                    s32 += x;
                else
                    s64 += x;
                mx = x > mx ? x : mx;
                const uint32_t z = sel - x;
                nmn = z > nmn ? z : nmn;
            }
        }
        sum += C <= 24 ? (unsigned long long)s32 : s64;
#pragma unroll
        for (int j = 0; j < WORDS; j++) cnt += __builtin_popcount(m[j]);
        tile = next;
    }
    // wave totals (once per wave): 64-bit sums by 24-bit limbs through the DPP scan, min / max by a butterfly
    const unsigned long long lo = wave_sum((uint32_t)(sum & 0xffffffull)), mid = wave_sum((uint32_t)((sum >> 24) & 0xffffffull)),
                             hi = wave_sum((uint32_t)((sum >> 48) & 0xffffull));
    // (a lane's sum is below 2^58 -- 2^32 values x 2^26 lanes' worth is far beyond any column -- so 16 bits of hi suffice)
    const unsigned long long wsum = lo + (mid << 24) + (hi << 48);
    const unsigned long long wcnt = (unsigned long long)wave_sum((uint32_t)(cnt & 0xffffffull)) + ((unsigned long long)wave_sum((uint32_t)(cnt >> 24)) << 24);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t omn = (uint32_t)__shfl_xor((int)nmn, o, 64), omx = (uint32_t)__shfl_xor((int)mx, o, 64);
        nmn = omn > nmn ? omn : nmn;
        mx = omx > mx ? omx : mx;
    }
    const uint32_t mn = ~nmn;
    if (lane == 0 && wcnt) {
        __hip_atomic_fetch_add(a.out + 0, wsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(a.out + 1, wcnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_min(a.out + 2, (unsigned long long)mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(a.out + 3, (unsigned long long)mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Env: LaunchEnv (ctx.hpp).  Option "max_blocks_per_cu" does not reach these grids.
template <int C, typename Env> inline void launch_aggregate(const Env &env, const AggArgs &a)
{
    constexpr int VPL = scan_vpl(C, kModeEq);
    using G = ScanGeom<C, VPL>;
    const uint64_t ntiles = (a.n + G::TILE_VALUES - 1) / G::TILE_VALUES;
    // one 4-wave block per CU keeps ~36-48 KiB of DMA in flight at c = 9, as the scans do; small tiles take two
    const unsigned grid = grid_for(ntiles, G::TILE_BYTES < 6144 ? 2 : 1, env.num_cus);
    MI355_LAUNCH(env.record, 0, aggregate_init_kernel, dim3(1), dim3(1), 0, env.stream, a.out);
    MI355_LAUNCH(env.record, 0, (aggregate_kernel<C, VPL>), dim3(grid), dim3(kBlockThreads), 0, env.stream, a);
}

template <typename Env> inline hipError_t launch_aggregate_width(unsigned c, const Env &env, const AggArgs &a)
{
    return launch_by_width<1, 32>(c, a, [&](auto w, const AggArgs &q) { return launch_aggregate<decltype(w)::value>(env, q), hipSuccess; });
}

} // namespace mi355
