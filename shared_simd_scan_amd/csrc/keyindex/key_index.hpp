// keyindex/key_index.hpp -- the device code of mi355_key_index_dev: table[j] = the first or the last row a mask selects whose key
// is j, packed at CT bits -- the inverse of a key column, the table mi355_lookup_dev takes.  gfx950 only; part of libmi355scan.so
// through keyindex/key_index.hip.
//
// Two phases over reach = min(table_rows, 2^C) 32-bit slots in the context's selection workspace, zeroed on the stream in front of
// every call.  A slot holds 0 for "no row", else an encoding of the winning row i (the row's index within the call) that ONE
// unsigned maximum resolves: ~i for FIRST (the lowest row has the largest code), i + 1 for LAST.  Both are >= 1 because
// n <= 2^32 - 1.  The maximum is monotone: within a call a slot only grows, and the clear was complete before the kernel began, so a
// stale read of a slot can only show too small a code and cost a redundant atomic, never lose a winner -- the argument of
// distinct/value_set.hpp, with "maximum" in the place of "or".  The result is therefore the same whatever the grid is.
//
// Phase 1 is value_set's pipeline (distinct/value_set.hpp) at every width: a wave owns tiles of 64 x VPL rows
// (VPL = scan_vpl(C, kModeEq)), the tile travels by non-temporal LDS-DMA (AUX = 2) while the tile before it is decoded at
// compile-time bit offsets, the lane's mask words come by load_bitmap_words (the ragged tile reads only the bytes the mask is
// guaranteed to hold), rows behind the column are cut by lane_valid_rows.
//
// Bound.  A selected row whose key is >= reach is exactly a row whose key is >= table_rows (no C-bit key is >= 2^C): it enters
// nothing and is counted "outside"; the others are counted "inside" -- per lane, summed per wave (wave_sum64), one atomic per wave
// and counter.  An unselected row, one beyond reach or one that cannot win looks slot 0 up and needs nothing: no lane ever forms an
// address outside the reach slots or their LDS image (reach == 0: the LDS tier, whose image always holds a slot).
//
// Runs.  Within the 32 rows of a lane's bitmap word, of a run of equal keys only the first (FIRST) or the last (LAST) selected row
// can win: the others look nothing up.  An all-equal or a sorted column then asks for one slot per lane and word, not 32 times.
//
// key_index_lds_kernel (reach <= kKeyIndexLdsMaxRows).  The block keeps reach slots in its dynamic LDS, zeroed at its start.  A row
// reads its slot and issues ds_max_u32 only where it would raise it: a read of one address by many lanes is a broadcast, an atomic
// on one address by many lanes is serialised.  At its end the block merges every non-zero slot into the workspace: a load that
// bypasses L1 (relaxed, agent scope) shows whether the slot would be raised, and only then one device-scope atomic maximum follows.
//   LDS budget: the tiles (4 waves x ScanGeom::LDS_BYTES, 64 KiB at C = 16 and C = 32) are static; the slots are dynamic, sized to
//   the reach passed, so a narrow key runs several blocks per CU (table_bpc).  kKeyIndexLdsMaxRows = 2^14: 64 KiB; with the widest
//   tiles a block then takes 128 KiB of the CU's 160.
//
// key_index_global_kernel (everything larger, up to 2^32 slots; C >= 15 by construction).  The slots stay in the workspace.  Per
// row the lane loads its slot (relaxed, agent scope: served by L2, never by a CU's L1, which no atomic refreshes) and issues
// the atomic maximum only where the row wins.
// In both tiers the 32 tests are folded into one mask and the atomics sit behind ONE branch per 32 rows.
//
// Phase 2, key_index_pack_kernel<CT>, streams the slots and writes the table.  A lane owns 32 consecutive entries, a wave 2048: the
// lane's 32 slots are 128 contiguous, 16-byte aligned bytes of the workspace and come by eight straight 16-byte loads (the last,
// ragged lane of the reach: slot by slot).  No LDS stage: a wave reads its 8 KiB of slots exactly once, the eight loads of a lane
// fill whole 128-byte lines between them, and without LDS the kernel runs at the occupancy its registers admit.  A slot decodes to
// 0 -> miss, else first_row + i in 64 bits, and to miss plus an "unfit" count where that is >= 2^CT.  Entries >= reach are miss and
// read no slot.  The 32 entries are exactly CT whole dwords (rt_insert_all), stored whole (store_words_by) or, for the lane that
// holds entry table_rows - 1, as the bytes its valid entries fill (rt_store_tail: trailing bits zero).  Members and unfit are
// summed per wave, one atomic each.
// The kernels test no switch bit.
#pragma once

#include "../kernels.hpp"
#include "../kernels/rt_column.hpp" // lane_valid_rows, wave_sum64, rt_insert_all, store_words_by, rt_store_tail

namespace mi355 {

struct KeyIndexArgs {
    const uint8_t *packed;   // the keys, 16 B aligned
    uint64_t n;              // <= 2^32 - 1
    const uint8_t *mask;     // rows that count (ceil(n/8) bytes, 4 B aligned) or null = every row
    uint32_t *slots;         // reach slots of the selection workspace, zeroed in front of the launch
    unsigned long long *out; // the four output words, zeroed in front of the launch; phase 1 adds to [1] (outside) and [2] (inside)
    uint32_t bound;          // LDS tier: reach (a key is inside when k < bound); global tier: reach - 1 (inside when k <= bound)
    uint32_t nslots;         // LDS tier: reach, the slots of the block's image
    uint32_t last;           // 0: the first row of a key wins (code ~i), 1: the last (code i + 1)
};

struct KeyIndexPackArgs {
    const uint32_t *slots;   // as phase 1 left them
    uint64_t reach;          // slots that exist; entries at and above it are miss (0 when n == 0: nothing is read)
    uint64_t table_rows;     // >= 1
    uint64_t first_row;      // < 2^32
    uint8_t *table;          // 16 B aligned
    unsigned long long *out; // the pack kernel adds to [0] (members) and [3] (unfit)
    uint32_t miss;
    uint32_t last;
    uint32_t nts;            // store policy of the whole lanes (one_pass_store_policy)
};

constexpr uint64_t kKeyIndexLdsMaxRows = 1ull << 14; // MI355_KEY_INDEX_LDS_MAX_ROWS
constexpr int kKeyIndexGlobalMinBits = 15;           // the global tier exists from this width on (2^14 is the LDS ceiling)
static_assert(kKeyIndexLdsMaxRows < (1ull << kKeyIndexGlobalMinBits), "widths below kKeyIndexGlobalMinBits never reach the global tier");

constexpr bool key_index_in_lds(unsigned c, uint64_t table_rows) { return value_reach(c, table_rows) <= kKeyIndexLdsMaxRows; }
// static LDS of a block at width C: the waves' tiles
template <int C> constexpr uint32_t key_index_static_lds() { return (uint32_t)kWavesPerBlock * (uint32_t)ScanGeom<C, scan_vpl(C, kModeEq)>::LDS_BYTES; }
// dynamic LDS of key_index_lds_kernel for `nslots` slots: at least one (reach == 0 looks slot 0 up), whole 16 bytes
constexpr uint32_t key_index_dyn_lds(uint32_t nslots) { return nslots ? (4u * nslots + 15u) & ~15u : 16u; }
static_assert(key_index_dyn_lds((uint32_t)kKeyIndexLdsMaxRows) == 64u * 1024u, "64 KiB of slots");
static_assert(key_index_static_lds<32>() + key_index_dyn_lds((uint32_t)kKeyIndexLdsMaxRows) + 64u <= (uint32_t)kCuLdsBytes, "LDS budget");
static_assert(key_index_static_lds<16>() + key_index_dyn_lds((uint32_t)kKeyIndexLdsMaxRows) + 64u <= (uint32_t)kCuLdsBytes, "LDS budget");

// the code of row i in a slot
__device__ __forceinline__ uint32_t key_index_code(uint32_t i, uint32_t last) { return last ? i + 1u : ~i; }

// the 32 rows of a lane's bitmap word: `sel` = the rows that count, row0 = the index of row 0 of the word.  ALL: every row counts
// (no mask, a full tile).  LDS_SLOTS: `slots` is the block's image in LDS, else the workspace.  -> `inside`, `outside`
template <bool LDS_SLOTS, bool ALL>
__device__ __forceinline__ void key_index_word(const uint32_t *xs, uint32_t sel, uint32_t bound, uint32_t *slots, uint32_t row0, uint32_t last,
                                               uint32_t &inside_rows, uint32_t &outside_rows)
{
    uint32_t t[32];
    uint32_t inside = 0; // bit k: row k counts and its key is within reach
    uint32_t same = 0;   // bit k: row k carries the key of row k - 1
#pragma unroll
    for (int k = 0; k < 32; k++) {
        const uint32_t v = xs[k];
        const bool in = (ALL || ((sel >> k) & 1u)) && (LDS_SLOTS ? v < bound : v <= bound);
        inside |= (in ? 1u : 0u) << k;
        if (k > 0) same |= (v == xs[k - 1] ? 1u : 0u) << k;
    }
    inside_rows += __builtin_popcount(inside);
    outside_rows += __builtin_popcount((ALL ? 0xffffffffu : sel) & ~inside);
    // a row rides on its neighbour in a run of equal keys: FIRST on the row before it, LAST on the row behind it
    const uint32_t ride = last ? (inside & same) >> 1 : (inside << 1) & same;
    const uint32_t probe = inside & ~ride; // bit k: the slot of row k is looked up
#pragma unroll
    for (int k = 0; k < 32; k++) {
        const uint32_t at = (probe >> k) & 1u ? xs[k] : 0u;
        if constexpr (LDS_SLOTS)
            t[k] = slots[at];
        else
            t[k] = __hip_atomic_load(slots + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_sched_barrier(0); // every slot is asked for before the first is tested
    uint32_t need = 0; // bit k: row k would raise its slot
#pragma unroll
    for (int k = 0; k < 32; k++) need |= (key_index_code(row0 + (uint32_t)k, last) > t[k] ? 1u : 0u) << k;
    need &= probe;
    if (need == 0) return; // the steady state of a column with few keys: one branch per 32 rows
#pragma unroll
    for (int k = 0; k < 32; k++) {
        if ((need >> k) & 1u) {
            if constexpr (LDS_SLOTS)
                __hip_atomic_fetch_max(slots + xs[k], key_index_code(row0 + (uint32_t)k, last), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else
                __hip_atomic_fetch_max(slots + xs[k], key_index_code(row0 + (uint32_t)k, last), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// the tile loop of both tiers; every thread of the block calls it
template <int C, bool LDS_SLOTS>
__device__ __forceinline__ void key_index_tiles(const KeyIndexArgs &a, uint32_t *slots, uint8_t *lds_wave, unsigned long long &inside, unsigned long long &outside)
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
    const uint32_t bound = a.bound, last = a.last;

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
    if constexpr (LDS_SLOTS) __syncthreads(); // the image is zero
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
        // the lane's first row of the tile: below 2^32 for every row inside the column (rows behind it are cut above)
        const uint32_t row0 = (uint32_t)(tile * (uint64_t)G::TILE_VALUES) + (uint32_t)lane * (uint32_t)VPL;
        uint32_t in_tile = 0, out_tile = 0;
        if (LDS_SLOTS && !a.mask && full) {
#pragma unroll
            for (int j = 0; j < WORDS; j++) key_index_word<LDS_SLOTS, true>(xs + 32 * j, 0xffffffffu, bound, slots, row0 + 32u * j, last, in_tile, out_tile);
        } else {
#pragma unroll
            for (int j = 0; j < WORDS; j++) key_index_word<LDS_SLOTS, false>(xs + 32 * j, m[j], bound, slots, row0 + 32u * j, last, in_tile, out_tile);
        }
        inside += in_tile;
        outside += out_tile;
        tile = next;
    }
}

// the wave's two counts: one atomic each, and only where there is something to add
__device__ __forceinline__ void key_index_counts(const KeyIndexArgs &a, unsigned long long inside, unsigned long long outside)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long o = wave_sum64(outside), i = wave_sum64(inside);
    if (lane == 0 && o) __hip_atomic_fetch_add(a.out + 1, o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lane == 0 && i) __hip_atomic_fetch_add(a.out + 2, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int C> __global__ __launch_bounds__(kBlockThreads) void key_index_lds_kernel(KeyIndexArgs a)
{
    using G = ScanGeom<C, scan_vpl(C, kModeEq)>;
    __shared__ __attribute__((aligned(16))) uint8_t lds[kWavesPerBlock][G::LDS_BYTES];
    uint32_t *const image = (uint32_t *)mi355_dyn_lds;
    const uint32_t nslots = a.nslots;
    for (uint32_t k = threadIdx.x; k < (nslots ? nslots : 1u); k += kBlockThreads) image[k] = 0;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned long long inside = 0, outside = 0;
    key_index_tiles<C, true>(a, image, lds[wave], inside, outside);
    __syncthreads(); // every wave's rows are in
    for (uint32_t k = threadIdx.x; k < nslots; k += kBlockThreads) {
        const uint32_t mine = image[k];
        if (!mine) continue;
        const uint32_t there = __hip_atomic_load(a.slots + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (mine <= there) continue; // another block's row wins: no atomic
        __hip_atomic_fetch_max(a.slots + k, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    key_index_counts(a, inside, outside);
}

template <int C> __global__ __launch_bounds__(kBlockThreads) void key_index_global_kernel(KeyIndexArgs a)
{
    static_assert(C >= kKeyIndexGlobalMinBits, "narrower keys reach no table beyond the LDS tier");
    using G = ScanGeom<C, scan_vpl(C, kModeEq)>;
    __shared__ __attribute__((aligned(16))) uint8_t lds[kWavesPerBlock][G::LDS_BYTES];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned long long inside = 0, outside = 0;
    key_index_tiles<C, false>(a, a.slots, lds[wave], inside, outside);
    key_index_counts(a, inside, outside);
}

constexpr int kKeyIndexPackRows = 64 * kRtVpl; // entries of a wave's step: 2048, a lane's 32 at CT whole dwords

template <int CT> __global__ __launch_bounds__(kBlockThreads) void key_index_pack_kernel(KeyIndexPackArgs g)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t nsteps = (g.table_rows + kKeyIndexPackRows - 1) / kKeyIndexPackRows;
    constexpr unsigned long long kIds = CT >= 32 ? (1ull << 32) : (1ull << (CT & 31)); // the row ids CT bits hold
    const uint32_t miss = g.miss, last = g.last;
    uint32_t members = 0, unfit = 0; // a lane sees at most 2^32 / 64 entries
    for (uint64_t step = wave; step < nsteps; step += nwaves) {
        const uint64_t word = step * 64 + (uint64_t)lane; // the lane's run of 32 entries
        const uint64_t first = word * kRtVpl;             // its entry 0
        if (first >= g.table_rows) continue;
        const int valid = g.table_rows - first >= kRtVpl ? kRtVpl : (int)(g.table_rows - first);
        uint32_t s[kRtVpl];
        if (first + kRtVpl <= g.reach) { // 128 contiguous bytes at a multiple of 128
#pragma unroll
            for (int q = 0; q < kRtVpl / 4; q++) {
                const u32x4 v = ((const u32x4 *)(g.slots + first))[q];
                s[4 * q] = v[0], s[4 * q + 1] = v[1], s[4 * q + 2] = v[2], s[4 * q + 3] = v[3];
            }
        } else {
#pragma unroll
            for (int b = 0; b < kRtVpl; b++) s[b] = first + (uint64_t)b < g.reach ? g.slots[first + (uint64_t)b] : 0u;
        }
        uint32_t x[kRtVpl];
#pragma unroll
        for (int b = 0; b < kRtVpl; b++) {
            const uint32_t i = last ? s[b] - 1u : ~s[b];
            const unsigned long long id = g.first_row + i;
            const bool member = s[b] != 0, fits = id < kIds;
            members += member ? 1u : 0u;
            unfit += member && !fits ? 1u : 0u;
            x[b] = member && fits ? (uint32_t)id : miss;
        }
        uint32_t r[CT];
        rt_insert_all<CT>(r, x);
        uint8_t *const dst = g.table + word * (4ull * CT);
        if (valid == kRtVpl)
            store_words_by<CT>(dst, r, g.nts);
        else
            rt_store_tail<CT>(dst, r, valid);
    }
    const unsigned long long m = wave_sum64(members), u = wave_sum64(unfit);
    if (lane == 0 && m) __hip_atomic_fetch_add(g.out, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lane == 0 && u) __hip_atomic_fetch_add(g.out + 3, u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

} // namespace mi355
