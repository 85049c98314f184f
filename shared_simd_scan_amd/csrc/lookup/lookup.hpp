// lookup/lookup.hpp -- the device code of mi355_lookup_dev: out_i = v_i < table_rows ? table[v_i] : miss, packed in and packed out --
// for each fact row the attribute of the dimension row its foreign key points at (GROUP BY d.attr), or a dictionary re-code.
// gfx950 only; part of libmi355scan.so through lookup/lookup.hip.
//
// Pipeline.  The run-time-width tile stream of kernels/rt_column.hpp, packed in and packed out: a wave owns tiles of 64 x 32
// consecutive rows, lane l rows [32 l, 32 l + 32).  The kernels are templates of the OUTPUT width CT only (32 instantiations
// each): the lane's 32 results are 32 CT bits = exactly CT whole dwords, assembled at compile-time bit offsets (rt_insert<CT, K>,
// the mirror of extract<C, K>) and stored at byte 4 CT lane of the tile's 256 CT output bytes -- no two lanes share a dword.
// The input width c is a wave-uniform run-time number: the tile travels by LDS-DMA (non-temporal: the column is
// read once; the kernel's own copy of rt_issue_tile's loop), stays in LDS and is decoded from there (columns_lds_value), so a wave has two images of it and alternates -- the
// next tile lands in one while the other is decoded.  The result dwords of a full tile leave one tile later, in front of the next
// DMA (so no wait for a tile ever waits for a younger store), with the widest stores the lane's alignment admits (rt_store): 16
// bytes when CT is a multiple of 4, 8 when it is even, else 4.  The ragged tile writes exactly the bytes it owns, the bits behind
// value n - 1 of the last byte zero (rt_store_tail).
//
// Bound.  reach = min(table_rows, 2^c) is what a value can address; values >= reach get `miss`.  The index is clamped
// without a branch, so rows >= n of the ragged tile (stale LDS) form clamped addresses only:
//   LDS tier     the entry looked up is min(v, reach); entry `reach`, behind the image, holds `miss`: the clamp IS the
//                comparison (the semi-join's zero byte, semijoin/semijoin.hpp).
//   global tier  x = min(v, reach - 1) is looked up and `miss` selected when v > reach - 1 (reach >= 1 there).
// Of the table only the dwords 0 .. last_word are ever read, last_word the dword that holds the last bit of value
// reach - 1: a value's two dwords are w = x CT >> 5 and min(w + 1, last_word) (when w + 1 is beyond, the value does not
// straddle and the second dword is not used; widths that divide 32 never straddle and load one dword).
//
// lookup_lds_kernel ((reach + 1) entries of 1 / 2 / 4 bytes for CT <= 8 / <= 16 / above fit kLookupLdsMaxBytes).  The block
// decodes the reachable table once into its dynamic LDS, behind the waves' images, while its waves' first tiles are in
// flight: thread t entries t, t + 256, ..., eight loads issued before the first is stored.  Per value: ds_read2_b32 (the
// input's two dwords), v_add (their address), v_alignbit, v_and, v_min, an address v_add / v_lshl_add, ONE ds_read_u8 / u16 /
// b32 and one v_lshl_or_b32 (a shift more where the value straddles an output dword): 6-7 VALU, 2 LDS operations.
//   LDS budget: all of a block's LDS is dynamic.  The waves' images take 4 x 2 x 8 KiB at c = 32; what is left of a CU's
//   160 KiB, minus kLookupLdsSlack for the dword read behind the last lane's run and rounding, is the table's ceiling
//   kLookupLdsMaxBytes.  The launcher sizes the dynamic LDS to the width and the table passed, so a narrow column and a
//   small table leave room for several blocks per CU.
//
// lookup_global_kernel (everything larger, up to 2^32 rows).  The packed table stays where it is: per value the address
// arithmetic in 64 bits (x CT needs 37), one or two global_load_dword with the DEFAULT cache policy -- the table's hot part
// lives in L2 and the Infinity Cache while the column streams through non-temporally --, all of a lane's loads issued before
// the first is consumed, then v_alignbit, v_and and the select of `miss`.
// The kernels test no switch bit.
#pragma once

#include "../kernels.hpp"
#include "../kernels/rt_column.hpp" // the tile stream of a column of run-time width, and the packed-out half

namespace mi355 {

struct LookupArgs {
    const uint8_t *packed; // n values of c bits, 16 B aligned
    uint64_t n;
    const uint32_t *table; // values of CT bits, 4 B aligned; dwords 0 .. last_word are read and no more
    uint8_t *out;          // n values of CT bits, 16 B aligned; exactly ceil(n CT / 8) bytes are written
    uint32_t c;
    uint32_t reach;        // LDS tier: min(table_rows, 2^c), the index of the entry that holds `miss`
    uint32_t limit;        // global tier: reach - 1, the last row a lookup may address
    uint32_t last_word;    // the dword of the table that holds the last bit of value reach - 1
    uint32_t miss;         // < 2^CT
    uint32_t nts;          // result stores: 0 plain, 1 non-temporal, 2 write-through (one uniform branch per tile)
};

constexpr uint32_t kLookupLdsSlack = 64;                  // the dword behind the last lane's run, rounding to 16

// the waves' images of a block, two per wave; + 16: the dword behind the last lane's run is read (and not used)
constexpr uint32_t lookup_images_lds(uint32_t c) { return kWavesPerBlock * 2u * rt_image(c) + 16u; }
// MI355_LOOKUP_LDS_MAX_BYTES: what the widest images (c = 32) leave of a CU's LDS for the table and its `miss` entry
constexpr uint32_t kLookupLdsMaxBytes = (kCuLdsBytes - kWavesPerBlock * 2u * rt_image(32) - kLookupLdsSlack) & ~15u;
constexpr uint32_t lookup_entry_bytes(unsigned ct) { return ct <= 8 ? 1u : (ct <= 16 ? 2u : 4u); }
constexpr bool lookup_in_lds(unsigned c, uint64_t table_rows, unsigned ct)
{
    return (value_reach(c, table_rows) + 1) * lookup_entry_bytes(ct) <= kLookupLdsMaxBytes;
}
// dynamic LDS of lookup_lds_kernel's table: reach + 1 entries, whole 16 bytes
constexpr uint32_t lookup_table_lds(uint32_t reach, unsigned ct) { return ((reach + 1u) * lookup_entry_bytes(ct) + 15u) & ~15u; }
static_assert(lookup_images_lds(32) + kLookupLdsMaxBytes <= kCuLdsBytes, "LDS budget");
static_assert(kLookupLdsMaxBytes >= (4096u + 1u) * 4u, "a 12-bit key column's whole table fits at any output width");

// the lane's 32 input values out of the image (run-time width: scalar offsets)
template <int K = 0> __device__ __forceinline__ void lookup_decode(const uint8_t *base, uint32_t c, uint32_t vmask, uint32_t (&v)[kRtVpl])
{
    v[K] = columns_lds_value<K>(base, c, vmask);
    if constexpr (K + 1 < kRtVpl) lookup_decode<K + 1>(base, c, vmask, v);
}

// ---- a value of the packed table: gather's two-dword read (extras/gather.hpp), never beyond dword last_word ----
template <int CT> constexpr bool lookup_one_dword() { return 32 % CT == 0; } // such a value never straddles a dword
template <int CT> struct TableRead {
    uint32_t lo, hi;
    // issue the loads of row x
    __device__ __forceinline__ void load(const uint32_t *table, uint32_t x, uint32_t last_word)
    {
        const uint32_t w = (uint32_t)(((uint64_t)x * CT) >> 5); // x CT needs 37 bits, the dword index 32
        lo = table[w];
        if constexpr (!lookup_one_dword<CT>()) hi = table[w < last_word ? w + 1u : last_word];
    }
    __device__ __forceinline__ uint32_t value(uint32_t x) const
    {
        const uint32_t s = (x * CT) & 31u;
        if constexpr (CT == 32) return lo;
        else if constexpr (lookup_one_dword<CT>()) return (lo >> s) & ((1u << CT) - 1u);
        else return __builtin_amdgcn_alignbit(hi, lo, s) & ((1u << CT) - 1u);
    }
};

// the block's decoded copy of the reachable table, entry `reach` = miss.  Every thread of the block calls it (barrier inside).
template <int CT> __device__ __forceinline__ void lookup_stage_table(const LookupArgs &a, uint8_t *image)
{
    constexpr uint32_t EB = lookup_entry_bytes(CT);
    auto put = [image](uint32_t j, uint32_t x) {
        if constexpr (EB == 1) image[j] = (uint8_t)x;
        else if constexpr (EB == 2) ((uint16_t *)image)[j] = (uint16_t)x;
        else ((uint32_t *)image)[j] = x;
    };
    const uint32_t reach = a.reach;
    constexpr uint32_t kInFlight = 8; // rows a thread loads before it stores the first
    for (uint32_t j0 = threadIdx.x; j0 < reach; j0 += kInFlight * kBlockThreads) {
        TableRead<CT> t[kInFlight];
#pragma unroll
        for (uint32_t q = 0; q < kInFlight; q++)
            if (j0 + q * kBlockThreads < reach) t[q].load(a.table, j0 + q * kBlockThreads, a.last_word);
#pragma unroll
        for (uint32_t q = 0; q < kInFlight; q++)
            if (j0 + q * kBlockThreads < reach) put(j0 + q * kBlockThreads, t[q].value(j0 + q * kBlockThreads));
    }
    if (threadIdx.x == 0) put(reach, a.miss); // what every value beyond the table is clamped to
    __syncthreads();
}

// both tiers.  LDS_TABLE: the table is staged into the block's LDS, else read where it lies.
template <int CT, bool LDS_TABLE> __device__ __forceinline__ void lookup_body(const LookupArgs &a)
{
    constexpr int VPL = kRtVpl;
    constexpr int AUX = 2; // the column is streamed once: non-temporal DMA
    constexpr uint32_t EB = lookup_entry_bytes(CT);
    constexpr uint32_t OUT_TILE = rt_tile_bytes(CT); // output bytes of a tile
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t c = a.c;
    const uint32_t tile_bytes = rt_tile_bytes(c); // a multiple of 256
    const uint32_t image = rt_image(c);
    uint8_t *cur = mi355_dyn_lds + (uint32_t)wave * 2u * image; // the image being decoded ...
    uint8_t *nxt = cur + image;                                 // ... and where the next tile lands
    uint8_t *const table_lds = mi355_dyn_lds + lookup_images_lds(c); // LDS tier: the block's decoded table, behind the images
    const uint32_t vmask = rt_vmask(c);

    const uint64_t n = a.n;
    const uint64_t ntiles = rt_ntiles(n), nfull = rt_nfull(n);
    const uint64_t data_bytes = (n * c + 7) / 8;
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock;
    uint64_t tile = (uint64_t)blockIdx.x * kWavesPerBlock + wave;
    const uint32_t reach = a.reach, limit = a.limit, last_word = a.last_word, miss = a.miss, nts = a.nts;

    // tile t of the column: LDS-DMA into `dst` (the last tile: only 16-byte chunks that start inside the payload).  The kernel's own
    // copy of rt_issue_tile's loop, as its store dispatch is of store_words_by and `left` of lane_valid_rows (kernels/rt_column.hpp):
    // with the shared forms all 64 instantiations compile to another schedule, five to other register counts
    auto issue = [&](uint64_t t, uint8_t *dst) {
        const uint64_t first = t * tile_bytes;
        const uint8_t *src = a.packed + first;
        const uint64_t left = data_bytes - first; // t < ntiles: at least one byte
        const uint32_t lim = left < tile_bytes ? (uint32_t)left : tile_bytes;
#pragma unroll
        for (int j = 0; j < kRtDmaInstrs; j++) {
            const uint32_t o = j * 1024 + lane * 16;
            if ((uint32_t)j * 1024u < tile_bytes && o < lim) __builtin_amdgcn_global_load_lds(MI355_GPTR(src + o), MI355_LPTR(dst + j * 1024), 16, 0, AUX);
        }
    };

    if (tile < ntiles) issue(tile, cur);
    if constexpr (LDS_TABLE) lookup_stage_table<CT>(a, table_lds); // the first tiles are in flight

    uint32_t res[CT];
    uint64_t prev = ~0ull;
    uint8_t *const out_lane = a.out + (uint32_t)lane * (4u * CT);
    auto store_prev = [&]() {
        uint8_t *dst = out_lane + prev * OUT_TILE;
        if (nts == 2)
            rt_store<CT, 2>(dst, res);
        else if (nts == 1)
            rt_store<CT, 1>(dst, res);
        else
            rt_store<CT, 0>(dst, res);
    };
    while (tile < ntiles) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the tile has landed
        if (prev != ~0ull) store_prev();
        const uint64_t next = tile + stride;
        if (next < ntiles) issue(next, nxt);

        uint32_t v[VPL], x[VPL];
        lookup_decode(cur + (uint32_t)lane * rt_lane_bytes(c), c, vmask, v);
        if constexpr (LDS_TABLE) {
#pragma unroll
            for (int k = 0; k < VPL; k++) {
                const uint32_t at = v[k] < reach ? v[k] : reach; // a value beyond the table looks up `miss`
                if constexpr (EB == 1) x[k] = table_lds[at];
                else if constexpr (EB == 2) x[k] = ((const uint16_t *)table_lds)[at];
                else x[k] = ((const uint32_t *)table_lds)[at];
            }
        } else {
            // every load of the lane's tile is issued before the first is consumed: 32 (or 64) independent addresses in flight
            TableRead<CT> t[VPL];
#pragma unroll
            for (int k = 0; k < VPL; k++) t[k].load(a.table, v[k] < limit ? v[k] : limit, last_word); // default policy: L2 / Infinity Cache
            __builtin_amdgcn_sched_barrier(0); // (the scheduler would otherwise start on the first value after some of the loads)
#pragma unroll
            for (int k = 0; k < VPL; k++) x[k] = v[k] > limit ? miss : t[k].value(v[k] < limit ? v[k] : limit);
        }
        rt_insert_all<CT>(res, x);
        if (tile < nfull) {
            prev = tile;
        } else {
            const int64_t left = (int64_t)(n - tile * kRtTileRows) - (int64_t)lane * VPL;
            rt_store_tail<CT>(out_lane + tile * OUT_TILE, res, left >= VPL ? VPL : (left <= 0 ? 0 : (int)left));
            prev = ~0ull;
        }
        uint8_t *const t2 = cur;
        cur = nxt;
        nxt = t2;
        tile = next;
    }
    if (prev != ~0ull) store_prev();
}

template <int CT> __global__ __launch_bounds__(kBlockThreads) void lookup_lds_kernel(LookupArgs a) { lookup_body<CT, true>(a); }

template <int CT> __global__ __launch_bounds__(kBlockThreads) void lookup_global_kernel(LookupArgs a) { lookup_body<CT, false>(a); }

} // namespace mi355
