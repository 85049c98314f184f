// distinct/value_set.hpp -- the device code of mi355_value_set_dev: bit v of a set in device memory is set for every row a mask
// selects whose value v is below set_bits -- the set of values that occur in a column, in the bitmap format mi355_semijoin_dev
// reads.  gfx950 only; part of libmi355scan.so through distinct/value_set.hip.
//
// Both kernels are histogram_kernel's pipeline (extras/histogram.hpp) at every width: a wave owns tiles of 64 x VPL rows
// (VPL = scan_vpl(C, kModeEq)), the tile travels by non-temporal LDS-DMA (AUX = 2) while the tile before it is decoded at
// compile-time bit offsets, the lane's mask words come by load_bitmap_words (the ragged tile reads only the bytes the mask is
// guaranteed to hold), rows behind the column are cut by lane_valid_rows.
//
// Bound.  reach = min(set_bits, 2^C) is what a value can address; a selected row whose value is >= reach is exactly a row whose
// value is >= set_bits (no C-bit value is >= 2^C): it sets nothing and is counted per lane, summed per wave (wave_sum64) and added
// to out[1] with one atomic per wave.  An unselected row, or one beyond reach, looks up word 0 and needs nothing: no lane ever forms
// an address outside the reach / 32 words of the set or of its LDS image (reach == 0: the LDS tier, whose image always holds a word).
//
// value_set_lds_kernel (reach <= kValueSetLdsMaxBits).  The block keeps ceil(reach / 32) words of bitset in its dynamic LDS, zeroed
// at its start.  Per 32 values the lane first reads the 32 words it would touch, then issues ds_or_b32 only where its bit is
// missing: after the first tiles nearly every bit is there, a read of one address by many lanes is a broadcast and an atomic on one
// address by many lanes is serialised (a column over few values: every lane of a wave hits one of a handful of words).  A stale
// read costs a redundant OR, never a wrong bit.  At its end the block merges its non-zero words into the set in device memory: a
// word whose bits are all present (tested with a load that bypasses L1) needs no atomic; the others take one device-scope atomicOr
// whose returned old word gives the bits this call turned on, popcount(mine & ~old) -- every 0 -> 1 transition is seen by exactly
// one atomic, whatever the grid is.
//   LDS budget: the tiles (4 waves x ScanGeom::LDS_BYTES, 64 KiB at C = 16 and C = 32) are static; the bitset is dynamic, sized to
//   the reach passed, so a narrow column runs several blocks per CU (table_bpc).  kValueSetLdsMaxBits = 2^19: 64 KiB, what
//   histogram_kernel keeps of counters; with the widest tiles a block then takes 128 KiB of the CU's 160.
//
// value_set_global_kernel (everything larger, up to 2^32 bits; C >= 20 by construction).  The set stays where it is.  Per 32
// values the lane loads the 32 words (relaxed, agent scope: served by L2, never by a CU's L1, which no atomic refreshes -- a hot
// word would read "missing" for as long as it stays there) and issues atomicOr where the bit is missing.  Within the call bits only
// go 0 -> 1 and the clear was complete before the kernel began, so a stale read can only say "missing" and cost a redundant atomic;
// the atomic drops the line from the issuing XCD's L2, so the next test of that word reads what the memory side holds.  The old
// words are consumed after all 32 atomics are issued.  A value equal to its predecessor's in the lane's run looks nothing up: its
// predecessor does (the runs of a sorted or an all-equal column, where every lane of every wave would otherwise ask one L2 channel
// for one word).
// In both tiers the 32 tests are folded into one mask and the atomics sit behind ONE branch per 32 values: with a branch per value the
// LDS tier ran 3.1 x histogram_kernel's time on the same 1e9 x 9 bit column (profiles/r19_value_set.txt names what is left).
// The kernels test no switch bit.
#pragma once

#include "../kernels.hpp"
#include "../kernels/rt_column.hpp" // lane_valid_rows, wave_sum64

namespace mi355 {

struct ValueSetArgs {
    const uint8_t *packed;   // 16 B aligned
    uint64_t n;
    const uint8_t *mask;     // rows that count (ceil(n/8) bytes, 4 B aligned) or null = every row
    uint32_t *set;           // bitmap format, 4 B aligned, whole dwords
    unsigned long long *out; // {bits turned on, selected rows beyond the set}, zeroed in front of the launch
    uint32_t bound;          // LDS tier: reach (a value is inside when v < bound); global tier: reach - 1 (inside when v <= bound)
    uint32_t words;          // LDS tier: ceil(reach / 32), the words of the block's bitset
};

constexpr uint64_t kValueSetLdsMaxBits = 1ull << 19; // MI355_VALUE_SET_LDS_MAX_BITS
constexpr int kValueSetGlobalMinBits = 20;           // the global tier exists from this width on (2^19 is the LDS ceiling)
static_assert(kValueSetLdsMaxBits < (1ull << kValueSetGlobalMinBits), "widths below kValueSetGlobalMinBits never reach the global tier");

constexpr bool value_set_in_lds(unsigned c, uint64_t set_bits) { return value_reach(c, set_bits) <= kValueSetLdsMaxBits; }
// static LDS of a block at width C: the waves' tiles
template <int C> constexpr uint32_t value_set_static_lds() { return (uint32_t)kWavesPerBlock * (uint32_t)ScanGeom<C, scan_vpl(C, kModeEq)>::LDS_BYTES; }
// dynamic LDS of value_set_lds_kernel for a bitset of `words` words: at least one word (reach == 0 looks word 0 up), whole 16 bytes
constexpr uint32_t value_set_dyn_lds(uint32_t words) { return words ? (4u * words + 15u) & ~15u : 16u; }
static_assert(value_set_static_lds<32>() + value_set_dyn_lds((uint32_t)(kValueSetLdsMaxBits / 32)) + 64u <= (uint32_t)kCuLdsBytes, "LDS budget");
static_assert(value_set_static_lds<16>() + value_set_dyn_lds((uint32_t)(kValueSetLdsMaxBits / 32)) + 64u <= (uint32_t)kCuLdsBytes, "LDS budget");

// the 32 values of a lane's bitmap word j: `sel` = the rows that count.  ALL: every row counts (no mask, a full tile).
// LDS_SET: `set` is the block's bitset in LDS, else the set in device memory.  -> `fresh` (global tier: bits turned on), `outside`
template <bool LDS_SET, bool ALL>
__device__ __forceinline__ void value_set_word(const uint32_t *xs, uint32_t sel, uint32_t bound, uint32_t *set, uint32_t &fresh, uint32_t &outside)
{
    uint32_t t[32];
    uint32_t inside = 0; // bit k: row k counts and its value is within reach
    uint32_t probe = 0;  // bit k: ... and its word is looked up
#pragma unroll
    for (int k = 0; k < 32; k++) {
        const uint32_t v = xs[k];
        const bool in = (ALL || ((sel >> k) & 1u)) && (LDS_SET ? v < bound : v <= bound);
        inside |= (in ? 1u : 0u) << k;
        bool ask = in;
        if constexpr (!LDS_SET) { // global tier: a value equal to its predecessor's rides on that row's lookup (runs of a sorted column)
            if (k > 0) ask = in && !(((inside >> (k - 1)) & 1u) && v == xs[k - 1]);
        }
        probe |= (ask ? 1u : 0u) << k;
        const uint32_t at = ask ? v >> 5 : 0u;
        if constexpr (LDS_SET)
            t[k] = set[at];
        else
            t[k] = __hip_atomic_load(set + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    outside += __builtin_popcount((ALL ? 0xffffffffu : sel) & ~inside);
    __builtin_amdgcn_sched_barrier(0); // every word is asked for before the first is tested
    uint32_t need = 0; // bit k: the bit of row k is missing
#pragma unroll
    for (int k = 0; k < 32; k++) need |= (~(t[k] >> (xs[k] & 31u)) & 1u) << k;
    need &= probe;
    if (need == 0) return; // the steady state: every bit is there, one branch per 32 values
#pragma unroll
    for (int k = 0; k < 32; k++) {
        const uint32_t v = xs[k];
        const uint32_t bit = 1u << (v & 31u);
        const bool mine = (need >> k) & 1u;
        if constexpr (LDS_SET) {
            if (mine) __hip_atomic_fetch_or(set + (v >> 5), bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
            t[k] = bit; // no atomic: nothing turned on
            if (mine) t[k] = __hip_atomic_fetch_or(set + (v >> 5), bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if constexpr (!LDS_SET) { // the old words are consumed after every atomic of the 32 is issued
#pragma unroll
        for (int k = 0; k < 32; k++) fresh += (t[k] >> (xs[k] & 31u)) & 1u ? 0u : 1u;
    }
}

// the tile loop of both tiers; every thread of the block calls it
template <int C, bool LDS_SET>
__device__ __forceinline__ void value_set_tiles(const ValueSetArgs &a, uint32_t *set, uint8_t *lds_wave, uint32_t &fresh, unsigned long long &outside)
{
    constexpr int VPL = scan_vpl(C, kModeEq);
    using G = ScanGeom<C, VPL>;
    constexpr int WORDS = G::WORDS;
    constexpr int AUX = 2; // the column is streamed once: non-temporal DMA
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const TileCtx<C, VPL> tc(a.n);
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock;
    uint64_t tile = (uint64_t)blockIdx.x * kWavesPerBlock + wave;
    const uint64_t nbytes = (a.n + 7) / 8;
    const uint32_t bound = a.bound;

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
    if constexpr (LDS_SET) __syncthreads(); // the bitset is zero
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
        uint32_t out_tile = 0;
        if (LDS_SET && !a.mask && full) {
#pragma unroll
            for (int j = 0; j < WORDS; j++) value_set_word<LDS_SET, true>(xs + 32 * j, 0xffffffffu, bound, set, fresh, out_tile);
        } else {
#pragma unroll
            for (int j = 0; j < WORDS; j++) value_set_word<LDS_SET, false>(xs + 32 * j, m[j], bound, set, fresh, out_tile);
        }
        outside += out_tile;
        tile = next;
    }
}

// the wave's two counts: one atomic each, and only where there is something to add
__device__ __forceinline__ void value_set_counts(const ValueSetArgs &a, uint32_t fresh, unsigned long long outside)
{
    const int lane = threadIdx.x & 63;
    const uint32_t f = wave_sum(fresh); // a wave turns on at most 2^32 / 64 bits per lane: the sum may wrap only beyond 2^32 bits
    const unsigned long long o = wave_sum64(outside);
    if (lane == 0 && f) __hip_atomic_fetch_add(a.out, (unsigned long long)f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lane == 0 && o) __hip_atomic_fetch_add(a.out + 1, o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int C> __global__ __launch_bounds__(kBlockThreads) void value_set_lds_kernel(ValueSetArgs a)
{
    using G = ScanGeom<C, scan_vpl(C, kModeEq)>;
    __shared__ __attribute__((aligned(16))) uint8_t lds[kWavesPerBlock][G::LDS_BYTES];
    uint32_t *const bits = (uint32_t *)mi355_dyn_lds;
    const uint32_t words = a.words;
    for (uint32_t k = threadIdx.x; k < (words ? words : 1u); k += kBlockThreads) bits[k] = 0;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t fresh = 0;
    unsigned long long outside = 0;
    value_set_tiles<C, true>(a, bits, lds[wave], fresh, outside);
    __syncthreads(); // every wave's bits are in
    for (uint32_t k = threadIdx.x; k < words; k += kBlockThreads) {
        const uint32_t mine = bits[k];
        if (!mine) continue;
        const uint32_t there = __hip_atomic_load(a.set + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!(mine & ~there)) continue; // all present: no atomic
        const uint32_t old = __hip_atomic_fetch_or(a.set + k, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        fresh += __builtin_popcount(mine & ~old);
    }
    value_set_counts(a, fresh, outside);
}

template <int C> __global__ __launch_bounds__(kBlockThreads) void value_set_global_kernel(ValueSetArgs a)
{
    static_assert(C >= kValueSetGlobalMinBits, "narrower columns reach no set beyond the LDS tier");
    using G = ScanGeom<C, scan_vpl(C, kModeEq)>;
    __shared__ __attribute__((aligned(16))) uint8_t lds[kWavesPerBlock][G::LDS_BYTES];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t fresh = 0;
    unsigned long long outside = 0;
    value_set_tiles<C, false>(a, a.set, lds[wave], fresh, outside);
    value_set_counts(a, fresh, outside);
}

} // namespace mi355
