// groupby/group_aggregate.hpp -- the device code of mi355_group_aggregate_dev: sum / count / min / max of one packed column
// per value of another (SELECT g, sum(v), count(*), min(v), max(v) ... WHERE <bitmap> GROUP BY g), both columns read once,
// neither decompressed.  gfx950 only; part of libmi355scan.so through groupby/group_aggregate.hip.
//
// Pipeline.  scan_columns_kernel's run-time-width form (predicates/columns.hpp, SAME = false): a wave owns tiles of
// 64 x 32 consecutive rows, lane l rows [32 l, 32 l + 32) of BOTH columns.  The kernel is a template of the KEY width only
// (12 instantiations): the keys' tile travels by LDS-DMA into one image per wave, is read into registers and decoded at
// compile-time bit offsets (extract<CK, K>).  The value width cv is a wave-uniform run-time number: the values' tile is the
// run-time-width stream of kernels/rt_column.hpp (its geometry and decode; the DMA loop is the kernel's own copy), stays
// in LDS and is decoded from there (columns_lds_value), so a wave has two images of it and alternates -- the next tile
// lands in one while the other is decoded.  The mask word of a lane's 32 rows is loaded one tile ahead like
// aggregate_kernel's (extras/aggregate.hpp); the ragged tile reads only the ceil(n / 8) bytes a bitmap is guaranteed to
// hold, and rows >= n are masked off, so whatever lies behind the columns never reaches a result.
//
// Per-group state, in the block's dynamic LDS in front of the tiles: a 64-bit sum, a 32-bit count, a 32-bit min and a 32-bit
// max -- 20 bytes per group and copy, as three arrays (sums, counts, {min, max} pairs) indexed by  slot = key * R + copy.
//   Replication.  With few groups all 64 lanes of a wave hit the same handful of slots, and same-address LDS atomics
//   serialise.  The table is therefore held R times, R the largest power of two <= 64 for which 20 * 2^CK * R stays within
//   kGroupTableBudget (10 KiB): 64 copies up to 8 groups, 32 / 16 / 8 / 4 / 2 at 16 .. 256 groups, one from 512 on.  A lane
//   uses copy lane & (R - 1).  The copy index is the minor one, so at R = 64 every lane of an LDS atomic has its own bank
//   (count: dword lane of 64; sum: dwords 2 lane, 2 lane + 1 of its half wave) whatever the keys are; at smaller R the keys
//   of a wave spread over 2^CK * R >= 512 slots.  The copies are summed when the block flushes.
//   Per row: ds_add_u64 (sum), ds_add_u32 (count), and for min / max one plain 8-byte read of the slot's pair: only a value
//   below the minimum or above the maximum read issues a ds_min_u32 / ds_max_u32.  The pair only ever tightens, so a stale
//   read can cost an atomic that was not needed, never skip one that was; after the first rows of a group nearly no row
//   issues either.  The pairs of eight rows are read together, in front of those rows' atomics.
//   A block's counts stay in 32 bits: the launcher sizes the grid so that a block sees fewer than 2^32 rows.
// Flush: thread g (+ 256, ...) sums the R copies of group g and adds a non-empty group to out_dev with four agent-scope
// atomics; out_dev was set to (0, 0, ~0, 0) per group by group_aggregate_init_kernel in front of the launch.
// Unsigned throughout; no switch bits.
#pragma once

#include "../kernels.hpp"
#include "../kernels/rt_column.hpp" // the values: the tile stream of a column of run-time width

namespace mi355 {

constexpr int kGroupMaxBits = 12;                 // MI355_GROUP_MAX_KEY_BITS: 2^12 x 20 B = 80 KiB next to the tiles
constexpr uint32_t kGroupEntryBytes = 20;         // sum 8, count 4, min 4, max 4
constexpr uint32_t kGroupTableBudget = 10 * 1024; // bytes of LDS the replicated table may take (one copy may take more)

struct GroupArgs {
    const uint8_t *keys;     // ck bits per row, 16 B aligned
    const uint8_t *values;   // cv bits per row, 16 B aligned (may be `keys` when cv == ck)
    uint64_t n;
    const uint8_t *mask;     // rows that count (ceil(n/8) bytes, 4 B aligned) or null = every row
    unsigned long long *out; // [4 g + 0] sum, [1] count, [2] min, [3] max -- the empty result in front of the launch
    uint32_t cv;
};

// copies of the table: see "Replication" above
constexpr uint32_t group_copies(int ck)
{
    uint32_t r = 64;
    while (r > 1 && (kGroupEntryBytes << ck) * r > kGroupTableBudget) r >>= 1;
    return r;
}
constexpr uint32_t group_table_bytes(int ck) { return (kGroupEntryBytes << ck) * group_copies(ck); } // a multiple of 16
// a wave's images: the keys' tile and two of the values'
template <int CK> constexpr uint32_t group_wave_lds(uint32_t cv) { return (uint32_t)ScanGeom<CK, kRtVpl>::LDS_BYTES + 2u * rt_image(cv); }
// + 16: the dword behind the last lane's run of values is read (and not used), as in scan_columns_kernel
template <int CK> constexpr uint32_t group_block_lds(uint32_t cv) { return group_table_bytes(CK) + kWavesPerBlock * group_wave_lds<CK>(cv) + 16u; }

static __global__ void group_aggregate_init_kernel(unsigned long long *out, uint32_t groups)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= groups) return;
    out[4 * g + 0] = 0;
    out[4 * g + 1] = 0;
    out[4 * g + 2] = ~0ull;
    out[4 * g + 3] = 0;
}

// the lane's 32 keys (registers, compile-time offsets) and values (LDS, scalar offsets)
template <int CK, int K> __device__ __forceinline__ void group_decode(const uint32_t (&w)[CK], const uint8_t *base, uint32_t cv, uint32_t vmask,
                                                                      uint32_t (&key)[kRtVpl], uint32_t (&x)[kRtVpl])
{
    key[K] = extract<CK, K, CK>(w);
    x[K] = columns_lds_value<K>(base, cv, vmask);
    if constexpr (K + 1 < kRtVpl) group_decode<CK, K + 1>(w, base, cv, vmask, key, x);
}

template <int CK> __global__ __launch_bounds__(kBlockThreads, 2) void group_aggregate_kernel(GroupArgs a)
{
    static_assert(CK >= 1 && CK <= kGroupMaxBits, "the groups' state must fit in LDS");
    constexpr int VPL = kRtVpl;
    using G = ScanGeom<CK, VPL>;
    static_assert(G::WORDS == 1 && G::LANE_DWORDS == CK, "32 rows per lane: one mask word, CK key dwords");
    constexpr int AUX = 2; // both columns are streamed once: non-temporal DMA
    constexpr uint32_t GROUPS = 1u << CK, R = group_copies(CK), SLOTS = GROUPS * R;

    unsigned long long *const t_sum = (unsigned long long *)mi355_dyn_lds;
    uint32_t *const t_cnt = (uint32_t *)(t_sum + SLOTS);
    uint32_t *const t_mm = t_cnt + SLOTS; // [2 slot] min, [2 slot + 1] max
    for (uint32_t k = threadIdx.x; k < SLOTS; k += kBlockThreads) {
        t_sum[k] = 0;
        t_cnt[k] = 0;
        t_mm[2 * k] = 0xffffffffu;
        t_mm[2 * k + 1] = 0;
    }

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t cv = a.cv;
    const uint32_t tile_bytes2 = rt_tile_bytes(cv); // a multiple of 256
    const uint32_t image2 = rt_image(cv);
    uint8_t *const lds1 = mi355_dyn_lds + group_table_bytes(CK) + (uint32_t)wave * ((uint32_t)G::LDS_BYTES + 2u * image2);
    uint8_t *lds2 = lds1 + G::LDS_BYTES;   // the values' image being decoded ...
    uint8_t *lds2_next = lds2 + image2;     // ... and where their next tile lands
    const uint32_t vmask = rt_vmask(cv);
    const uint32_t copy = (uint32_t)lane & (R - 1u);

    const TileCtx<CK, VPL> tc(a.n);
    const uint64_t data_bytes2 = (a.n * cv + 7) / 8;
    const uint64_t mask_bytes = (a.n + 7) / 8;
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock;
    uint64_t tile = (uint64_t)blockIdx.x * kWavesPerBlock + wave;

    // tile t of both columns: LDS-DMA into the wave's images (the values': into `dst2`)
    auto issue = [&](uint64_t t, uint8_t *dst2) {
        tc.template issue<AUX>(a.keys, t, lds1, lane);
        // (the kernel's own copy of rt_issue_tile's loop: behind tc.issue in one lambda the shared form compiles to another schedule)
        const uint64_t first = t * tile_bytes2;
        const uint8_t *src = a.values + first;
        const uint64_t left = data_bytes2 - first; // t < ntiles: at least one byte
        const uint32_t lim = left < tile_bytes2 ? (uint32_t)left : tile_bytes2;
#pragma unroll
        for (int j = 0; j < kRtDmaInstrs; j++) {
            const uint32_t o = j * 1024 + lane * 16;
            if ((uint32_t)j * 1024u < tile_bytes2 && o < lim) __builtin_amdgcn_global_load_lds(MI355_GPTR(src + o), MI355_LPTR(dst2 + j * 1024), 16, 0, AUX);
        }
    };
    // the lane's mask word of tile t (ragged end: only the bytes the bitmap is guaranteed to hold)
    auto load_mask = [&](uint64_t t) -> uint32_t {
        // (the kernel's own copy of bitmap_word_at's rule: with the shared form all twelve widths compile to another stream, c = 1 to 122 VGPRs for 116)
        if (!a.mask) return 0xffffffffu;
        const uint64_t at = t * G::BITMAP_BYTES + (uint64_t)lane * 4;
        if (t < tc.nfull) return *(const uint32_t *)(a.mask + at);
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; b++)
            if (at + b < mask_bytes) v |= (uint32_t)a.mask[at + b] << (8 * b);
        return v;
    };
    auto add_row = [&](uint32_t slot, uint32_t x, uint32_t mn, uint32_t mx) {
        __hip_atomic_fetch_add(t_sum + slot, (unsigned long long)x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(t_cnt + slot, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (x < mn) __hip_atomic_fetch_min(t_mm + 2 * slot, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (x > mx) __hip_atomic_fetch_max(t_mm + 2 * slot + 1, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };

    uint32_t mnext = 0;
    if (tile < tc.ntiles) {
        issue(tile, lds2);
        mnext = load_mask(tile);
    }
    __syncthreads(); // the table is initialised
    while (tile < tc.ntiles) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the tile's images and mask word have landed
        uint32_t w[CK];
        read_lane_data<CK, VPL>(lds1, lane, w);
        uint32_t m = mnext;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // the keys are in registers: the next tile flies during the decode -- the values' into the image that is not being decoded
        const uint64_t next = tile + stride;
        if (next < tc.ntiles) {
            issue(next, lds2_next);
            mnext = load_mask(next);
        }
        const bool full = tile < tc.nfull;
        if (!full) { // rows behind the column count for nothing
            const int64_t left = (int64_t)(a.n - tile * G::TILE_VALUES) - (int64_t)lane * VPL; // (lane_valid_rows compiles to another schedule)
            const int valid = left >= VPL ? VPL : (left <= 0 ? 0 : (int)left);
            m &= tail_mask(valid, 0);
        }
        uint32_t key[VPL], x[VPL];
        group_decode<CK, 0>(w, lds2 + (uint32_t)lane * rt_lane_bytes(cv), cv, vmask, key, x);
        const bool all = !a.mask && full; // wave-uniform
#pragma unroll
        for (int v0 = 0; v0 < VPL; v0 += 8) {
            uint32_t mn[8], mx[8];
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const uint32_t slot = key[v0 + q] * R + copy;
                // one ds_read_b64: the pair is 8-byte aligned, min in the low word
                const unsigned long long mm = __hip_atomic_load((const unsigned long long *)(t_mm + 2 * slot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                mn[q] = (uint32_t)mm;
                mx[q] = (uint32_t)(mm >> 32);
            }
            if (all) {
#pragma unroll
                for (int q = 0; q < 8; q++) add_row(key[v0 + q] * R + copy, x[v0 + q], mn[q], mx[q]);
            } else {
#pragma unroll
                for (int q = 0; q < 8; q++)
                    if ((m >> (v0 + q)) & 1u) add_row(key[v0 + q] * R + copy, x[v0 + q], mn[q], mx[q]);
            }
        }
        uint8_t *const t2 = lds2;
        lds2 = lds2_next;
        lds2_next = t2;
        tile = next;
    }
    __syncthreads(); // every wave's updates are done
    for (uint32_t g = threadIdx.x; g < GROUPS; g += kBlockThreads) {
        unsigned long long sum = 0, cnt = 0;
        uint32_t mn = 0xffffffffu, mx = 0;
#pragma unroll 4
        for (uint32_t r = 0; r < R; r++) {
            const uint32_t slot = g * R + r;
            sum += t_sum[slot];
            cnt += t_cnt[slot];
            const uint32_t smn = t_mm[2 * slot], smx = t_mm[2 * slot + 1];
            mn = smn < mn ? smn : mn;
            mx = smx > mx ? smx : mx;
        }
        if (cnt) {
            unsigned long long *const o = a.out + 4ull * g;
            __hip_atomic_fetch_add(o + 0, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(o + 1, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_min(o + 2, (unsigned long long)mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(o + 3, (unsigned long long)mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

} // namespace mi355
