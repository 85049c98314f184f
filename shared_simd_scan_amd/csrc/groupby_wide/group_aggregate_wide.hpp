// groupby_wide/group_aggregate_wide.hpp -- the device code of mi355_group_aggregate_wide_dev: sum / count / min / max of one
// packed column per value of another for a dense key domain of up to 2^26 groups, whose result table lives in device memory
// (group_aggregate_kernel, groupby/group_aggregate.hpp, keeps it in LDS and stops at 2^12).  gfx950 only; part of
// libmi355scan.so through groupby_wide/group_aggregate_wide.hip.
//
// Pipeline.  The run-time-width tile stream of kernels/rt_column.hpp, twice: a wave owns tiles of 64 x 32 consecutive rows, lane l
// rows [32 l, 32 l + 32) of BOTH columns.  ONE kernel, no template of a width: both widths are wave-uniform run-time numbers, both
// tiles travel by non-temporal LDS-DMA (rt_issue_tile), stay in LDS and are decoded from there (columns_lds_value), so a wave has two
// alternating images of EACH column -- the next tiles land in one pair while the other is decoded.  The mask word of a lane's
// 32 rows is loaded one tile ahead and the ragged tile handled as in group_aggregate_kernel: only the ceil(n / 8) bytes a
// bitmap is guaranteed to hold are read, rows >= n are masked off, so what lies behind the columns never reaches a result.
//
// Why not one global atomic per row.  Agent-scope atomics execute at the memory side; a wave-instruction whose 64 lanes
// scatter runs an order of magnitude below the contiguous rate, and one hot address saturates near 1e8 updates per second: a
// key that holds a tenth of 1e9 rows would take on the order of a second.  So each block keeps a FIRST-COME FRONT in LDS.
//   Slots.  S slots (a power of two, chosen by the launcher: group_wide_front_slots), slot = key & (S - 1), 24 bytes each, as
//   four arrays in front of the tiles: sum (uint64, 0), {min, max} pair (2 x uint32: ~0, 0), tag (uint32, EMPTY = 0xffffffff --
//   no valid key, a valid key is < groups <= 2^26), count (uint32, 0).  Initialised before the first tile is decoded.
//   Per counted row, in this order: key >= groups -> the lane's dropped count.  Else tag[slot]: EMPTY -> ONE LDS
//   compare-and-swap EMPTY -> key; the winner and whoever finds tag == key own the slot.  A tag never changes once set: no
//   eviction, hence no eviction race.
//     hit   exactly group_aggregate_kernel's row: ds_add_u64 (sum), ds_add_u32 (count), one 8-byte read of the pair and a
//           ds_min_u32 / ds_max_u32 only when the row tightens it.
//     miss  (the slot belongs to another key) the row goes to out_dev: agent-scope fetch_add on sum and count; for min / max a
//           relaxed agent-scope load of the group's pair first and an atomic only when the row tightens what was read.  The pair
//           only ever tightens, so a stale read can cost an atomic that was not needed, never skip one that was.
//   The tags and the pairs of eight rows are read together, in front of those rows' updates.
//   A block's counts stay in 32 bits: the launcher sizes the grid so that a block sees fewer than 2^32 rows.
// Flush: behind a block barrier thread s (+ 256, ...) adds every claimed slot with count > 0 to out_dev[4 tag ...] with four
// agent-scope atomics; each wave adds its dropped total with ONE vector atomic.  out_dev was set to (0, 0, ~0, 0) per group and
// *dropped to 0 by group_aggregate_wide_init_kernel in front of the launch.  out_dev is addressed in 64 bits throughout: 32 g
// reaches 2^31 bytes.  Unsigned throughout; no switch bits.
#pragma once

#include "../kernels.hpp"
#include "../kernels/rt_column.hpp" // the tile stream of a column of run-time width: geometry, DMA, decode

namespace mi355 {

constexpr uint64_t kGroupWideMaxGroups = 1ull << 26; // MI355_GROUP_WIDE_MAX_GROUPS
constexpr uint32_t kGroupWideSlotBytes = 24;         // sum 8, min 4, max 4, tag 4, count 4
constexpr uint32_t kGroupWideEmpty = 0xffffffffu;    // the tag of a slot nobody has claimed
#ifndef MI355_GROUP_WIDE_MAX_SLOTS
#define MI355_GROUP_WIDE_MAX_SLOTS 4096 // (a rebuild with EXTRA_FLAGS=-DMI355_GROUP_WIDE_MAX_SLOTS=1024 trades slots for blocks per CU)
#endif
constexpr uint32_t kGroupWideMaxSlots = MI355_GROUP_WIDE_MAX_SLOTS, kGroupWideMinSlots = 1024;
static_assert(kGroupWideMaxSlots >= kGroupWideMinSlots && (kGroupWideMaxSlots & (kGroupWideMaxSlots - 1)) == 0, "a power of two, at least 1024");

struct GroupWideArgs {
    const uint8_t *keys;         // ck bits per row, 16 B aligned
    const uint8_t *values;       // cv bits per row, 16 B aligned (may be `keys` when cv == ck)
    uint64_t n;
    const uint8_t *mask;         // rows that count (ceil(n/8) bytes, 4 B aligned) or null = every row
    unsigned long long *out;     // [4 g + 0] sum, [1] count, [2] min, [3] max -- the empty result in front of the launch
    unsigned long long *dropped; // nullable: counted rows with key >= groups -- 0 in front of the launch, one add per wave
    uint32_t groups;             // 1 .. 2^26
    uint32_t ck, cv;
    uint32_t slots;              // S = group_wide_front_slots(ck, cv)
};

// a wave's images: two of each column
constexpr uint32_t group_wide_wave_lds(uint32_t ck, uint32_t cv) { return 2u * rt_image(ck) + 2u * rt_image(cv); }
// + 16: the dword behind the last lane's run is read (and not used)
constexpr uint32_t group_wide_block_lds(uint32_t slots, uint32_t ck, uint32_t cv)
{
    return kGroupWideSlotBytes * slots + kWavesPerBlock * group_wide_wave_lds(ck, cv) + 16u;
}
// THE rule for S: the largest of 4096 / 2048 / 1024 whose front fits a CU's LDS next to one block's tiles.  (Whether fewer
// slots and a second block per CU serve the miss path better has not been measured: MI355_GROUP_WIDE_MAX_SLOTS above.)
constexpr uint32_t group_wide_front_slots(uint32_t ck, uint32_t cv)
{
    uint32_t s = kGroupWideMaxSlots;
    while (s > kGroupWideMinSlots && group_wide_block_lds(s, ck, cv) > (uint32_t)kCuLdsBytes) s >>= 1;
    return s;
}
static_assert(group_wide_block_lds(group_wide_front_slots(32, 32), 32, 32) <= (uint32_t)kCuLdsBytes, "a front exists at every pair of widths");

static __global__ void group_aggregate_wide_init_kernel(unsigned long long *out, uint32_t groups, unsigned long long *dropped)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g == 0 && dropped) *dropped = 0;
    if (g >= groups) return;
    unsigned long long *const o = out + 4ull * g;
    o[0] = 0;
    o[1] = 0;
    o[2] = ~0ull;
    o[3] = 0;
}

// the block's front: four arrays of S entries in its dynamic LDS
struct GroupWideFront {
    unsigned long long *sum;
    uint32_t *mm; // [2 slot] min, [2 slot + 1] max: one 8-byte aligned pair
    uint32_t *tag, *cnt;
    uint32_t smask; // S - 1
    __device__ __forceinline__ GroupWideFront(uint8_t *lds, uint32_t slots)
        : sum((unsigned long long *)lds), mm((uint32_t *)(lds + 8u * slots)), tag((uint32_t *)(lds + 16u * slots)), cnt((uint32_t *)(lds + 20u * slots)),
          smask(slots - 1u)
    {
    }
};

// rows V0 + Q .. V0 + 7 of the lane's run: key and value out of the two images (scalar offsets)
template <int V0, int Q = 0>
__device__ __forceinline__ void group_wide_decode(const uint8_t *kbase, uint32_t ck, uint32_t kmask, const uint8_t *vbase, uint32_t cv, uint32_t vmask,
                                                  uint32_t (&key)[8], uint32_t (&x)[8])
{
    key[Q] = columns_lds_value<V0 + Q>(kbase, ck, kmask);
    x[Q] = columns_lds_value<V0 + Q>(vbase, cv, vmask);
    if constexpr (Q + 1 < 8) group_wide_decode<V0, Q + 1>(kbase, ck, kmask, vbase, cv, vmask, key, x);
}

// eight rows of a lane.  m: bit q = row V0 + q counts (mask and tail applied).  Returns the rows that were dropped.
template <int V0>
__device__ __forceinline__ uint32_t group_wide_rows(const GroupWideFront &f, unsigned long long *out, uint32_t groups, const uint8_t *kbase, uint32_t ck,
                                                    uint32_t kmask, const uint8_t *vbase, uint32_t cv, uint32_t vmask, uint32_t m)
{
    uint32_t key[8], x[8], tg[8];
    group_wide_decode<V0>(kbase, ck, kmask, vbase, cv, vmask, key, x);
    uint32_t oob = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        oob |= (key[q] >= groups ? 1u : 0u) << q;
        tg[q] = __hip_atomic_load(f.tag + (key[q] & f.smask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); // (any key: the slot index is < S)
    }
    const uint32_t live = m & ~oob; // from here on every row that counts has key < groups: the only keys that address out[]
    // an EMPTY slot: one compare-and-swap; on failure it returns the tag that is there for good
    uint32_t own = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        if (((live >> q) & 1u) && tg[q] == kGroupWideEmpty) {
            uint32_t seen = kGroupWideEmpty;
            const bool won = __hip_atomic_compare_exchange_strong(f.tag + (key[q] & f.smask), &seen, key[q], __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                                  __HIP_MEMORY_SCOPE_WORKGROUP);
            tg[q] = won ? key[q] : seen;
        }
        own |= (tg[q] == key[q] ? 1u : 0u) << q;
    }
    const uint32_t hit = live & own, miss = live & ~own;
    // the pairs of the eight rows, in front of their updates: bit q of lo / hi = row q tightens the minimum / maximum read
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        // one ds_read_b64: the pair is 8-byte aligned, min in the low word
        const unsigned long long mm = __hip_atomic_load((const unsigned long long *)(f.mm + 2u * (key[q] & f.smask)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        lo |= (x[q] < (uint32_t)mm ? 1u : 0u) << q;
        hi |= (x[q] > (uint32_t)(mm >> 32) ? 1u : 0u) << q;
    }
    lo &= hit, hi &= hit;
    if (miss) {
        // the group's pair in out_dev, all eight rows' loads in flight together (a row that does not miss reads group 0's).  The
        // pair only ever tightens: a stale read can cost an atomic that was not needed, never skip one that was.
        unsigned long long gmn[8], gmx[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const unsigned long long *const o = out + 4ull * (((miss >> q) & 1u) ? key[q] : 0u);
            gmn[q] = __hip_atomic_load(o + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            gmx[q] = __hip_atomic_load(o + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        uint32_t glo = 0, ghi = 0;
#pragma unroll
        for (int q = 0; q < 8; q++) {
            glo |= ((unsigned long long)x[q] < gmn[q] ? 1u : 0u) << q;
            ghi |= ((unsigned long long)x[q] > gmx[q] ? 1u : 0u) << q;
        }
        lo |= glo & miss, hi |= ghi & miss;
    }
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const uint32_t bit = 1u << q;
        if (hit & bit) {
            const uint32_t slot = key[q] & f.smask;
            __hip_atomic_fetch_add(f.sum + slot, (unsigned long long)x[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(f.cnt + slot, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (lo & bit) __hip_atomic_fetch_min(f.mm + 2u * slot, x[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (hi & bit) __hip_atomic_fetch_max(f.mm + 2u * slot + 1u, x[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else if (miss & bit) {
            unsigned long long *const o = out + 4ull * key[q];
            __hip_atomic_fetch_add(o + 0, (unsigned long long)x[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(o + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (lo & bit) __hip_atomic_fetch_min(o + 2, (unsigned long long)x[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (hi & bit) __hip_atomic_fetch_max(o + 3, (unsigned long long)x[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    return m & oob;
}

static __global__ __launch_bounds__(kBlockThreads) void group_aggregate_wide_kernel(GroupWideArgs a)
{
    constexpr int VPL = kRtVpl;
    constexpr int AUX = 2; // both columns are streamed once: non-temporal DMA
    constexpr uint32_t MASK_TILE = kRtTileRows / 8; // mask bytes of a tile
    const uint32_t slots = a.slots;
    const GroupWideFront f(mi355_dyn_lds, slots);
    for (uint32_t k = threadIdx.x; k < slots; k += kBlockThreads) {
        f.sum[k] = 0;
        f.mm[2 * k] = 0xffffffffu;
        f.mm[2 * k + 1] = 0;
        f.tag[k] = kGroupWideEmpty;
        f.cnt[k] = 0;
    }

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t ck = a.ck, cv = a.cv, groups = a.groups;
    const uint32_t tile_bytes1 = rt_tile_bytes(ck), tile_bytes2 = rt_tile_bytes(cv); // multiples of 256
    const uint32_t image1 = rt_image(ck), image2 = rt_image(cv);
    uint8_t *cur1 = mi355_dyn_lds + kGroupWideSlotBytes * slots + (uint32_t)wave * group_wide_wave_lds(ck, cv); // the images being decoded ...
    uint8_t *nxt1 = cur1 + image1;                                                                              // ... and where the next tiles land
    uint8_t *cur2 = cur1 + 2u * image1;
    uint8_t *nxt2 = cur2 + image2;
    const uint32_t kmask = rt_vmask(ck), vmask = rt_vmask(cv);

    const uint64_t n = a.n;
    const uint64_t ntiles = rt_ntiles(n), nfull = rt_nfull(n);
    const uint64_t data_bytes1 = (n * ck + 7) / 8, data_bytes2 = (n * cv + 7) / 8;
    const uint64_t mask_bytes = (n + 7) / 8;
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock;
    uint64_t tile = (uint64_t)blockIdx.x * kWavesPerBlock + wave;

    auto issue = [&](uint64_t t, uint8_t *dst1, uint8_t *dst2) {
        rt_issue_tile<AUX>(a.keys, data_bytes1, tile_bytes1, t, dst1, lane);
        rt_issue_tile<AUX>(a.values, data_bytes2, tile_bytes2, t, dst2, lane);
    };
    // the lane's mask word of tile t (ragged end: only the bytes the bitmap is guaranteed to hold)
    auto load_mask = [&](uint64_t t) -> uint32_t {
        // (the kernel's own copy of bitmap_word_at's rule: the shared form compiles to another stream)
        if (!a.mask) return 0xffffffffu;
        const uint64_t at = t * MASK_TILE + (uint64_t)lane * 4;
        if (t < nfull) return *(const uint32_t *)(a.mask + at);
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; b++)
            if (at + b < mask_bytes) v |= (uint32_t)a.mask[at + b] << (8 * b);
        return v;
    };

    uint32_t mnext = 0;
    if (tile < ntiles) {
        issue(tile, cur1, cur2);
        mnext = load_mask(tile);
    }
    unsigned long long dropped = 0; // the lane's counted rows with key >= groups so far
    __syncthreads();                // the front is initialised
    while (tile < ntiles) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // both tiles and the mask word have landed
        uint32_t m = mnext;
        const uint64_t next = tile + stride;
        if (next < ntiles) {
            issue(next, nxt1, nxt2);
            mnext = load_mask(next);
        }
        if (tile >= nfull) { // rows behind the column count for nothing
            const int64_t left = (int64_t)(n - tile * kRtTileRows) - (int64_t)lane * VPL; // (lane_valid_rows compiles to another schedule)
            const int valid = left >= VPL ? VPL : (left <= 0 ? 0 : (int)left);
            m &= tail_mask(valid, 0);
        }
        const uint8_t *const kbase = cur1 + (uint32_t)lane * rt_lane_bytes(ck), *const vbase = cur2 + (uint32_t)lane * rt_lane_bytes(cv);
        uint32_t bad = group_wide_rows<0>(f, a.out, groups, kbase, ck, kmask, vbase, cv, vmask, m & 0xffu);
        bad |= group_wide_rows<8>(f, a.out, groups, kbase, ck, kmask, vbase, cv, vmask, (m >> 8) & 0xffu) << 8;
        bad |= group_wide_rows<16>(f, a.out, groups, kbase, ck, kmask, vbase, cv, vmask, (m >> 16) & 0xffu) << 16;
        bad |= group_wide_rows<24>(f, a.out, groups, kbase, ck, kmask, vbase, cv, vmask, m >> 24) << 24;
        dropped += (uint32_t)__builtin_popcount(bad);
        uint8_t *const t1 = cur1, *const t2 = cur2;
        cur1 = nxt1, cur2 = nxt2;
        nxt1 = t1, nxt2 = t2;
        tile = next;
    }
    __syncthreads(); // every wave's updates of the front are done
    for (uint32_t s = threadIdx.x; s < slots; s += kBlockThreads) {
        const uint32_t tag = f.tag[s], cnt = f.cnt[s];
        if (tag != kGroupWideEmpty && cnt) {
            unsigned long long *const o = a.out + 4ull * tag;
            __hip_atomic_fetch_add(o + 0, f.sum[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(o + 1, (unsigned long long)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_min(o + 2, (unsigned long long)f.mm[2 * s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(o + 3, (unsigned long long)f.mm[2 * s + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (a.dropped) {
        const unsigned long long total = wave_sum64(dropped);
        if (lane == 0 && total) __hip_atomic_fetch_add(a.dropped, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

} // namespace mi355
