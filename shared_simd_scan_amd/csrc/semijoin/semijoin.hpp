// semijoin/semijoin.hpp -- the device code of mi355_semijoin_dev: bitmap[i] = (v_i < set_bits && bit v_i of a set that lives in
// device memory) -- `fact.fk IN (SELECT pk FROM dim WHERE ...)` with dense keys, the set being the result bitmap of a scan
// over the dimension table.  gfx950 only; part of libmi355scan.so through semijoin/semijoin.hip.
//
// Both kernels are in_kernel's pipeline (kernels/in_list.hpp) with another lookup: a wave owns tiles of 64 x VPL rows
// (VPL = scan_vpl(C, kModeEq)), the tile and the tile's AND-mask bytes travel by LDS-DMA, the lane's run is read into
// registers and decoded at compile-time bit offsets, the result words of a full tile leave one tile later (in front of the next
// DMA, so no wait for a tile ever waits for a younger store), the ragged tile writes exactly the bytes it owns.  a.s.out == null:
// count only, no store is issued.  Hit counts go through hits_add / hits_finalize.
//
// Bound.  m = min(set_bits, 2^C) is what a value can reach; set_bytes = ceil(m / 8) is all that is ever read of the set.  The index
// is clamped without a branch, and a value >= m finds a zero:
//   LDS tier     the byte looked up is min(v >> 3, set_bytes), the bit v & 7 (both straight out of the packed word by v_bfe_u32).
//                The block's image holds a zero wherever a value >= m lands: the bits >= m of its last byte are cleared and byte
//                set_bytes, behind the image, is zero.  The clamped lookup IS the comparison -- one v_min_u32 per value (and the
//                add of the image's base: dynamic LDS has no immediate address) on top of in_kernel's bitset lookup.  (Clamping the
//                bit index and ANDing the looked-up bit with v < m as well costs a shift, a v_cmp and a v_cndmask more per value;
//                the kernel is bound by its VALU work at narrow widths: profiles/r08_semijoin_with_compare.txt.)
//   global tier  the set cannot be given a zero bit, so x = min(v, m - 1) is looked up and the bit found is ANDed with (v <= m - 1).
// No lane ever forms an address outside [set, set + set_bytes) or outside the image.
//
// semijoin_lds_kernel (m <= kSemiLdsMaxBits).  The block copies the set's set_bytes bytes into its dynamic LDS once, while
// its waves' first tiles are in flight: 16-byte loads over the 16-byte-aligned middle of [set, set + set_bytes), 4-byte and
// single-byte loads over what is left at both ends (the set is 4-byte aligned), no byte behind the set is read.  The LDS
// image starts at the base of the dynamic LDS whatever the set's address is (a 16-byte load is stored as four dwords).  Then the
// bits >= m of the last byte are cleared and the byte behind the image is zeroed (m == 0: no byte is copied and every lookup
// reads that zero byte).
// Per value one ds_read_u8 and a bit extract; byte lookups of a wave spread over the 64 banks as the values do.
//   LDS budget: the tiles (4 waves x ScanGeom::LDS_BYTES, at most 16 KiB each: C = 16 and C = 32) and the mask images (4 x 1 KiB)
//   are static; what is left of a CU's 160 KiB at the widest width, minus kSemiLdsSlack for the last-block flag of
//   hits_finalize and the image's zero byte, is the ceiling of the set: semijoin_lds_max_bits().  The launcher sizes
//   the dynamic LDS to the set passed, so a small set leaves room for several blocks per CU.
//
// semijoin_global_kernel (everything larger, up to 2^32 bits = 512 MiB; C >= 20 by construction).  The set stays where it is:
// one global_load_ubyte per value with the DEFAULT cache policy, so the set's hot part lives in L2 and the Infinity Cache, while
// the column keeps streaming through with the non-temporal LDS-DMA policy.  A lane forms the 64 byte offsets of its tile and
// issues the 64 loads (scalar base + 32-bit offset, independent addresses) before it assembles the two result words.
// The kernels test no switch bit.
#pragma once

#include "../kernels.hpp"

namespace mi355 {

struct SemiArgs {
    ScanArgs s;          // packed, n, out (null: count only), hits, scratch, and_mask, invert; everything else unused
    const uint8_t *set;  // bitmap format, 4 B aligned; set_bytes bytes are read and no more
    uint32_t set_bytes;  // ceil(min(set_bits, 2^C) / 8); LDS tier: also the index of the image's zero byte
    uint32_t limit;      // global tier: m - 1, the last bit a lookup may address (m = min(set_bits, 2^C) > 0 there)
    uint32_t last_keep;  // mask of the valid bits of byte set_bytes - 1 (0xff: all eight)
};

constexpr uint32_t kSemiMaskLds = 1024; // a tile's AND-mask bytes per wave: one LDS-DMA instruction
constexpr uint32_t kSemiLdsSlack = 64;  // hits_finalize's flag, the image's zero byte, rounding to 16
constexpr int kSemiGlobalMinBits = 20;  // the global tier exists from this width on (2^19 < the LDS ceiling)

// static LDS of a block at width C: the waves' tiles and mask images
template <int C> constexpr uint32_t semijoin_static_lds()
{
    return (uint32_t)kWavesPerBlock * ((uint32_t)ScanGeom<C, scan_vpl(C, kModeEq)>::LDS_BYTES + kSemiMaskLds);
}
// MI355_SEMIJOIN_LDS_MAX_BITS: the largest set the LDS tier holds -- what the widest tiles (C = 32; C = 16 ties) leave of a CU's LDS
constexpr uint64_t semijoin_lds_max_bits()
{
    constexpr uint32_t widest = semijoin_static_lds<32>() > semijoin_static_lds<16>() ? semijoin_static_lds<32>() : semijoin_static_lds<16>();
    return 8ull * ((kCuLdsBytes - widest - kSemiLdsSlack) & ~15u);
}
static_assert(semijoin_lds_max_bits() >= (1ull << 19), "the LDS tier serves at least what histogram keeps next to its tiles");
static_assert(semijoin_lds_max_bits() < (1ull << kSemiGlobalMinBits), "widths below kSemiGlobalMinBits never reach the global tier");
constexpr bool semijoin_in_lds(unsigned c, uint64_t set_bits) { return value_reach(c, set_bits) <= semijoin_lds_max_bits(); }
// dynamic LDS of semijoin_lds_kernel for a set of set_bytes bytes: the image, its zero byte, whole 16 bytes
constexpr uint32_t semijoin_dyn_lds(uint32_t set_bytes) { return (set_bytes + 1u + 15u) & ~15u; }
static_assert(semijoin_static_lds<32>() + 16u + semijoin_dyn_lds((uint32_t)(semijoin_lds_max_bits() / 8)) <= kCuLdsBytes, "LDS budget");
static_assert(semijoin_static_lds<16>() + 16u + semijoin_dyn_lds((uint32_t)(semijoin_lds_max_bits() / 8)) <= kCuLdsBytes, "LDS budget");

// [from, to) of the set -> LDS with 4-byte loads, then single bytes; `from` is a multiple of 4
__device__ __forceinline__ void semijoin_copy_narrow(const uint8_t *set, uint8_t *image, uint32_t from, uint32_t to)
{
    const uint32_t words = (to - from) / 4u;
    for (uint32_t i = threadIdx.x; i < words; i += kBlockThreads) *(uint32_t *)(image + from + 4u * i) = *(const uint32_t *)(set + from + 4u * i);
    for (uint32_t o = from + 4u * words + threadIdx.x; o < to; o += kBlockThreads) image[o] = set[o];
}

// the block's copy of the set: returns where byte 0 of the set is in LDS.  Every thread of the block calls it (barriers inside).
__device__ __forceinline__ const uint8_t *semijoin_stage_set(const SemiArgs &a)
{
    const uint32_t nbytes = a.set_bytes;
    uint8_t *const image = mi355_dyn_lds;
    const uint32_t to16 = (16u - (uint32_t)((uintptr_t)a.set & 15u)) & 15u; // 0, 12, 8, 4
    const uint32_t head = to16 < nbytes ? to16 : nbytes;       // [0, head): in front of the set's first 16-byte boundary
    const uint32_t chunks = (nbytes - head) / 16u;             // [head, head + 16 chunks): whole aligned 16-byte chunks of the set
    const uint32_t body_end = head + 16u * chunks;
    constexpr uint32_t kInFlight = 8; // 16-byte loads a thread issues before it stores the first: a 92 KiB set is three round trips
    for (uint32_t i0 = threadIdx.x; i0 < chunks; i0 += kInFlight * kBlockThreads) {
        u32x4 t[kInFlight];
#pragma unroll
        for (uint32_t q = 0; q < kInFlight; q++)
            if (i0 + q * kBlockThreads < chunks) t[q] = *(const u32x4 *)(a.set + head + 16u * (i0 + q * kBlockThreads));
#pragma unroll
        for (uint32_t q = 0; q < kInFlight; q++)
            if (i0 + q * kBlockThreads < chunks) { // the image is 4-byte aligned where the set is 16-byte aligned: four dword stores
                uint32_t *const dst = (uint32_t *)(image + head + 16u * (i0 + q * kBlockThreads));
                dst[0] = t[q].x, dst[1] = t[q].y, dst[2] = t[q].z, dst[3] = t[q].w;
            }
    }
    semijoin_copy_narrow(a.set, image, 0, head);
    semijoin_copy_narrow(a.set, image, body_end, nbytes); // body_end is a multiple of 4 (or nbytes itself)
    __syncthreads();
    if (threadIdx.x == 0) {
        if (nbytes) image[nbytes - 1] &= (uint8_t)a.last_keep; // bits >= set_bits of the last byte never reach a result
        image[nbytes] = 0;                                      // the zero byte every value beyond the set is clamped to
    }
    __syncthreads();
    return image;
}

// the tile loop of both tiers.  LDS_SET: `set` is the block's LDS image, else the set in global memory.
template <int C, int AUX_, bool LDS_SET> __device__ __forceinline__ void semijoin_tiles(const SemiArgs &a, const uint8_t *set, uint8_t *lds_wave, uint8_t *mlds_wave)
{
    constexpr int VPL = scan_vpl(C, kModeEq);
    using G = ScanGeom<C, VPL>;
    constexpr int WORDS = G::WORDS;
    constexpr int AUX = AUX_ & 15;
    constexpr int NTS = store_policy_of(AUX_);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const TileCtx<C, VPL> tc(a.s.n);
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock;
    uint64_t tile = (uint64_t)blockIdx.x * kWavesPerBlock + wave;
    const uint8_t *const mask = a.s.and_mask;
    const bool store = a.s.out != nullptr;
    const uint32_t limit = a.limit, zero_byte = a.set_bytes, inv = a.s.invert;

    uint32_t hits = 0;
    uint32_t res[WORDS];
    uint64_t prev = ~0ull;
    uint8_t *const out_lane = a.s.out + lane * (WORDS * 4);
    while (tile < tc.ntiles) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the tile (and its mask bytes) have landed
        uint32_t w[G::LANE_DWORDS];
        read_lane_data<C, VPL>(lds_wave, lane, w);
        uint32_t mcur[WORDS];
        if (mask && tile < tc.nfull) {
#pragma unroll
            for (int j = 0; j < WORDS; j++) mcur[j] = ((const uint32_t *)(mlds_wave + lane * (WORDS * 4)))[j];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (prev != ~0ull && store) store_words<WORDS, NTS>(out_lane + prev * G::BITMAP_BYTES, res);
        const uint64_t next = tile + stride;
        if (next < tc.ntiles) {
            if (mask && next < tc.nfull && lane * 16 < G::BITMAP_BYTES)
                __builtin_amdgcn_global_load_lds(MI355_GPTR(mask + next * G::BITMAP_BYTES + lane * 16), MI355_LPTR(mlds_wave), 16, 0, 0);
            tc.template issue<AUX>(a.s.packed, next, lds_wave, lane);
        }

        uint32_t xs[VPL];
        extract_all<C, VPL, 0, G::LANE_DWORDS>(w, xs);
        if constexpr (LDS_SET) {
#pragma unroll
            for (int j = 0; j < WORDS; j++) {
                uint32_t acc = 0;
#pragma unroll
                for (int k = 31; k >= 0; k--) { // value 32j+0 ends in bit 0
                    const uint32_t v = xs[32 * j + k];
                    const uint32_t at = (v >> 3) < zero_byte ? (v >> 3) : zero_byte; // a value beyond the set looks up a zero
                    const uint32_t bit = (set[at] >> (v & 7)) & 1u;
                    acc = (acc << 1) | bit;
                }
                res[j] = acc;
            }
        } else {
            // every load of the lane's tile is issued before the first is consumed: 64 independent addresses in flight
            uint32_t b[VPL];
#pragma unroll
            for (int k = 0; k < VPL; k++) {
                const uint32_t v = xs[k];
                const uint32_t x = v < limit ? v : limit;
                b[k] = set[x >> 3]; // default cache policy: the set's hot bytes stay in L2 / the Infinity Cache
            }
            __builtin_amdgcn_sched_barrier(0); // (the scheduler would otherwise start on the first word after half of the loads)
#pragma unroll
            for (int j = 0; j < WORDS; j++) {
                uint32_t acc = 0;
#pragma unroll
                for (int k = 31; k >= 0; k--) {
                    const uint32_t v = xs[32 * j + k];
                    const uint32_t x = v < limit ? v : limit;
                    const uint32_t bit = (b[32 * j + k] >> (x & 7)) & (v <= limit ? 1u : 0u);
                    acc = (acc << 1) | bit;
                }
                res[j] = acc;
            }
        }
#pragma unroll
        for (int j = 0; j < WORDS; j++) res[j] ^= inv;
        if (tile < tc.nfull) {
            if (mask) {
#pragma unroll
                for (int j = 0; j < WORDS; j++) res[j] &= mcur[j];
            }
#pragma unroll
            for (int j = 0; j < WORDS; j++) hits += __builtin_popcount(res[j]);
            prev = tile;
        } else {
            if (mask) { // the ragged tile reads only the bytes the mask is guaranteed to hold (ceil(n/8))
                const int64_t left = (int64_t)(tc.n - tile * G::TILE_VALUES) - (int64_t)lane * VPL;
                const int nbytes = left <= 0 ? 0 : (int)((left >= VPL ? VPL : left) + 7) / 8;
                const uint8_t *mp = mask + tile * G::BITMAP_BYTES + lane * (WORDS * 4);
#pragma unroll
                for (int j = 0; j < WORDS; j++) {
                    uint32_t mm = 0;
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        if (4 * j + q < nbytes) mm |= (uint32_t)mp[4 * j + q] << (8 * q);
                    res[j] &= mm;
                }
            }
            hits += tc.finish_tail(tile, res, out_lane + tile * G::BITMAP_BYTES, 1, lane, store);
            prev = ~0ull;
        }
        tile = next;
    }
    if (prev != ~0ull && store) store_words<WORDS, NTS>(out_lane + prev * G::BITMAP_BYTES, res);
    if (a.s.hits) hits_add(a.s, 0, wave_sum(hits), lane);
    hits_finalize(a.s, 1, lane);
}

// the wave's first tile and its mask bytes: in flight while the block stages the set
template <int C, int AUX_> __device__ __forceinline__ void semijoin_first_tile(const SemiArgs &a, uint8_t *lds_wave, uint8_t *mlds_wave)
{
    constexpr int VPL = scan_vpl(C, kModeEq);
    using G = ScanGeom<C, VPL>;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const TileCtx<C, VPL> tc(a.s.n);
    const uint64_t tile = (uint64_t)blockIdx.x * kWavesPerBlock + wave;
    if (tile >= tc.ntiles) return;
    if (a.s.and_mask && tile < tc.nfull && lane * 16 < G::BITMAP_BYTES)
        __builtin_amdgcn_global_load_lds(MI355_GPTR(a.s.and_mask + tile * G::BITMAP_BYTES + lane * 16), MI355_LPTR(mlds_wave), 16, 0, 0);
    tc.template issue<AUX_ & 15>(a.s.packed, tile, lds_wave, lane);
}

template <int C, int AUX_> __global__ __launch_bounds__(kBlockThreads) void semijoin_lds_kernel(SemiArgs a)
{
    using G = ScanGeom<C, scan_vpl(C, kModeEq)>;
    __shared__ __attribute__((aligned(16))) uint8_t lds[kWavesPerBlock][G::LDS_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t mlds[kWavesPerBlock][kSemiMaskLds];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    semijoin_first_tile<C, AUX_>(a, lds[wave], mlds[wave]);
    const uint8_t *const set_lds = semijoin_stage_set(a);
    semijoin_tiles<C, AUX_, true>(a, set_lds, lds[wave], mlds[wave]);
}

template <int C, int AUX_> __global__ __launch_bounds__(kBlockThreads) void semijoin_global_kernel(SemiArgs a)
{
    static_assert(C >= kSemiGlobalMinBits, "narrower columns reach no set beyond the LDS tier");
    using G = ScanGeom<C, scan_vpl(C, kModeEq)>;
    __shared__ __attribute__((aligned(16))) uint8_t lds[kWavesPerBlock][G::LDS_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t mlds[kWavesPerBlock][kSemiMaskLds];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    semijoin_first_tile<C, AUX_>(a, lds[wave], mlds[wave]);
    semijoin_tiles<C, AUX_, false>(a, a.set, lds[wave], mlds[wave]);
}

} // namespace mi355
