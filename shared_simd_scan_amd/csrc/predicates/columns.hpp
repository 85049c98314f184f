// predicates/columns.hpp -- the device code of scan_columns_kernel: a predicate over the row-wise DIFFERENCE of two packed columns,
//   p[i] = lo <= v1_i - v2_i <= hi   (possibly negated, possibly combined with an earlier bitmap),
// the comparison of two columns row by row (col1 < col2, col1 >= col2 + 30, |col1 - col2| <= 3, col1 == col2) without
// either column being decompressed.  gfx950 only; part of libmi355scan.so through predicates/columns_group.hip.
//
// The pipeline is scan2_kernel's (kernels/scan.hpp): a wave owns tiles of 64 x VPL consecutive rows, lane l rows
// [l * VPL, (l + 1) * VPL) of BOTH columns; VPL is a multiple of 32, so a lane's run starts on a dword boundary at any width.
// Both columns' tiles travel by LDS-DMA, the result words of a tile are stored while the next tile is being waited for,
// hit counts go through hits_add / hits_finalize, TileCtx carries the 64-bit tile indices and the ragged tail.
//
// Width pairs.  The kernel is a template of column 1's width only (its values leave registers at compile-time bit
// offsets: extract<C1, K>); 1024 pair instantiations would double the library.  Two forms:
//   SAME  = true   c2 == C1: column 2 is decoded from registers like column 1.  Both next tiles are in flight during the
//                  whole decode, as in scan2_kernel.
//   SAME  = false  c2 is a wave-uniform run-time value.  Row K of a lane starts at bit K * c2 of the lane's run -- K is a
//                  compile-time constant, so the position is scalar arithmetic: the value is the two dwords at the scalar
//                  offset (K * c2 >> 5) * 4 from the lane's base in LDS (ds_read2_b32), a funnel shift by the scalar
//                  K * c2 & 31 and a mask.  Column 2's tile therefore stays in LDS during the decode, so a wave has two
//                  images of it and alternates: the next tile lands in one while the other is decoded.  32 rows per lane
//                  keep a wave's four LDS images at 25 KiB or less at any width pair.
//
// Exactness.  d = v1 - v2 lies in [-(2^c2 - 1), 2^C1 - 1].  The host clamps the predicate's bounds to that domain, so
// lo <= hi are values of d (an empty range arrives as the full one with the negation word flipped).
//   WIDE = false   max(C1, c2) <= 30: d fits an int32 and hi - lo < 2^31, so (uint32)(d - lo) <= hi - lo is exact: the
//                  range push of kernels/tile.hpp on v1 - v2.
//   WIDE = true    a width of 31 or 32: d - lo spans up to 2^33 - 2 and would alias modulo 2^32; the same test in 64 bits,
//                  plain C++.  Chosen at compile time (by the launcher for a run-time c2), so narrower pairs never pay.
//
// Mask (AND / OR / XOR / ANDNOT with an earlier bitmap, which may be the output itself): a full tile's mask bytes are a
// third LDS-DMA stream issued with the tile's columns, one tile ahead, and read into registers with column 1 -- before the
// tile's result is stored, by the only wave that stores it, so the combination may be made in place.  The ragged tile
// reads only the ceil(n / 8) bytes a bitmap is guaranteed to hold.
#pragma once

#include "../kernels.hpp"
#include "../kernels/rt_column.hpp" // columns_lds_value: column 2's decode when SAME = false

namespace mi355 {

struct ColumnsArgs {
    ScanArgs s;          // packed, packed2, n, out (null: count only), hits, scratch, and_mask, mask_op, invert
    uint32_t c2;         // width of column 2 (SAME: == C1)
    uint32_t nts;        // bitmap stores: 0 plain, 1 non-temporal, 2 write-through (one uniform branch per tile)
    uint32_t lo, span;   // WIDE = false: (uint32)(int32)lo and hi - lo
    int64_t lo64;        // WIDE = true
    uint64_t span64;
};

constexpr int kColumnsMaskLds = 1024; // per wave: one LDS-DMA instruction's worth (a tile's mask is 8 * VPL <= 1024 bytes)

// rows per lane and tile: the plain scans' geometry when both columns sit in registers, 32 when column 2 is read from LDS
constexpr int columns_vpl(int C, bool same) { return same ? scan_vpl(C, kModeRange) : 32; }
// per-wave LDS: column 1's tile, column 2's tile (two of them when it is decoded out of LDS), the mask image
template <int C1, int VPL, bool SAME> constexpr uint32_t columns_wave_lds(uint32_t c2)
{
    return (uint32_t)ScanGeom<C1, VPL>::LDS_BYTES + (SAME ? 1u : 2u) * ((64u * VPL * c2 / 8 + 1023u) / 1024u * 1024u) + (uint32_t)kColumnsMaskLds;
}
// + 16: the dword behind the last lane's run of column 2 is read (and not used) when c2 is a multiple of 4
template <int C1, int VPL, bool SAME> constexpr uint32_t columns_block_lds(uint32_t c2)
{
    return kWavesPerBlock * columns_wave_lds<C1, VPL, SAME>(c2) + 16u;
}

// ---- one bitmap word: 32 rows as four independent chains of 8 (see push4 in kernels/tile.hpp), highest row first ----
template <bool WIDE> struct ColumnsPred {
    uint32_t lo, span;
    int64_t lo64;
    uint64_t span64;
    __device__ __forceinline__ void push(uint32_t (&acc)[4], const uint32_t (&v1)[4], const uint32_t (&v2)[4]) const
    {
        if constexpr (WIDE) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int64_t d = (int64_t)v1[q] - (int64_t)v2[q];
                acc[q] = (acc[q] << 1) | ((uint64_t)(d - lo64) <= span64 ? 1u : 0u);
            }
        } else {
            push4<kModeRange>(acc[0], acc[1], acc[2], acc[3], v1[0] - v2[0], v1[1] - v2[1], v1[2] - v2[2], v1[3] - v2[3], lo, span);
        }
    }
};

template <int C1, int VPL, bool SAME, bool WIDE, int J, int K, int NW>
__device__ __forceinline__ void columns_step(const uint32_t (&w1)[NW], const uint32_t (&w2)[SAME ? NW : 1], const uint8_t *base2, uint32_t c2,
                                             uint32_t vmask2, const ColumnsPred<WIDE> &pred, uint32_t (&acc)[4])
{
    constexpr int R = 32 * J + K; // rows R, R + 8, R + 16, R + 24: one per chain
    const uint32_t v1[4] = {extract<C1, R, NW>(w1), extract<C1, R + 8, NW>(w1), extract<C1, R + 16, NW>(w1), extract<C1, R + 24, NW>(w1)};
    uint32_t v2[4];
    if constexpr (SAME) {
        v2[0] = extract<C1, R, NW>(w2), v2[1] = extract<C1, R + 8, NW>(w2), v2[2] = extract<C1, R + 16, NW>(w2), v2[3] = extract<C1, R + 24, NW>(w2);
    } else {
        v2[0] = columns_lds_value<R>(base2, c2, vmask2), v2[1] = columns_lds_value<R + 8>(base2, c2, vmask2);
        v2[2] = columns_lds_value<R + 16>(base2, c2, vmask2), v2[3] = columns_lds_value<R + 24>(base2, c2, vmask2);
    }
    pred.push(acc, v1, v2);
    if constexpr (K > 0) columns_step<C1, VPL, SAME, WIDE, J, K - 1, NW>(w1, w2, base2, c2, vmask2, pred, acc);
}

template <int C1, int VPL, bool SAME, bool WIDE, int J, int NW>
__device__ __forceinline__ void columns_words(const uint32_t (&w1)[NW], const uint32_t (&w2)[SAME ? NW : 1], const uint8_t *base2, uint32_t c2,
                                              uint32_t vmask2, const ColumnsPred<WIDE> &pred, uint32_t (&res)[VPL / 32])
{
    uint32_t acc[4] = {0, 0, 0, 0};
    columns_step<C1, VPL, SAME, WIDE, J, 7, NW>(w1, w2, base2, c2, vmask2, pred, acc);
    res[J] = acc[0] | (acc[1] << 8) | (acc[2] << 16) | (acc[3] << 24);
    if constexpr (J + 1 < VPL / 32) columns_words<C1, VPL, SAME, WIDE, J + 1, NW>(w1, w2, base2, c2, vmask2, pred, res);
}

// waves per SIMD handed to the register allocator: scan2_kernel's when both columns are held in registers
template <int C1, int VPL, bool SAME> constexpr int columns_occ()
{
    if (SAME) return burst_occ<C1, VPL, 1>() > 1 ? burst_occ<C1, VPL, 1>() / 2 : 1;
    return 2;
}

// the whole kernel; its entry point scan_columns_kernel is defined by the translation unit that instantiates it
// (columns_group.hip), with __launch_bounds__(kBlockThreads, columns_occ())
template <int C1, int VPL, bool SAME, bool WIDE> __device__ __forceinline__ void scan_columns_body(const ColumnsArgs &a)
{
    using G = ScanGeom<C1, VPL>;
    static_assert(!SAME || WIDE == (C1 > 30), "the same-width form knows its comparison width");
    constexpr int WORDS = G::WORDS;
    constexpr int AUX = 2; // non-temporal DMA loads: both columns are read once
    constexpr uint32_t MASK_TILE = G::BITMAP_BYTES;
    static_assert(MASK_TILE <= (uint32_t)kColumnsMaskLds, "a tile's mask is one LDS-DMA instruction");

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t c2 = SAME ? (uint32_t)C1 : a.c2;
    const uint32_t tile_bytes2 = 64u * VPL / 8u * c2; // a multiple of 256
    const uint32_t lds2_bytes = (tile_bytes2 + 1023u) / 1024u * 1024u;
    uint8_t *const lds1 = mi355_dyn_lds + (uint32_t)wave * ((uint32_t)G::LDS_BYTES + (SAME ? 1u : 2u) * lds2_bytes + (uint32_t)kColumnsMaskLds);
    uint8_t *const mlds = lds1 + G::LDS_BYTES + (SAME ? 1u : 2u) * lds2_bytes;
    uint8_t *lds2 = lds1 + G::LDS_BYTES;                     // column 2's image of the tile being decoded ...
    uint8_t *lds2_next = SAME ? lds2 : lds2 + lds2_bytes;    // ... and where its next tile lands

    const ScanArgs &s = a.s;
    const TileCtx<C1, VPL> tc(s.n);
    const uint64_t data_bytes2 = (s.n * c2 + 7) / 8;
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock;
    uint64_t tile = (uint64_t)blockIdx.x * kWavesPerBlock + wave;
    const ColumnsPred<WIDE> pred{a.lo, a.span, a.lo64, a.span64};
    const uint32_t vmask2 = c2 >= 32 ? 0xffffffffu : ((1u << c2) - 1u);
    const uint32_t inv = s.invert, mop = s.mask_op, nts = a.nts;
    const uint8_t *const mask = s.and_mask;
    auto combine = [mop](uint32_t r, uint32_t m) -> uint32_t {
        return mop == 0 ? (r & m) : mop == 1 ? (r | m) : mop == 2 ? (r ^ m) : (m & ~r);
    };
    uint32_t hits = 0;
    uint8_t *const out_lane = s.out + lane * (WORDS * 4);
    const bool store = s.out != nullptr;
    uint32_t res[WORDS];
    uint64_t prev = ~0ull;
    auto store_prev = [&]() {
        uint8_t *dst = out_lane + prev * G::BITMAP_BYTES;
        if (nts == 2)
            store_words<WORDS, 2>(dst, res);
        else if (nts == 1)
            store_words<WORDS, 1>(dst, res);
        else
            store_words<WORDS, 0>(dst, res);
    };

    // tile t of both columns, and of the mask when the tile is full: LDS-DMA into the wave's images (column 2: into `dst2`).
    // Kept in its own form -- the DMA loop is rt_issue_tile's, the store dispatch store_words_by's, `left` lane_valid_rows' (all
    // kernels/rt_column.hpp): with them nine instantiations took more registers (c = 19, SAME: 128 -> 139), DESIGN.md 3.1.
    auto issue = [&](uint64_t t, uint8_t *dst2) {
        tc.template issue<AUX>(s.packed, t, lds1, lane);
        if constexpr (SAME) {
            tc.template issue<AUX>(s.packed2, t, dst2, lane);
        } else {
            const uint64_t first = t * tile_bytes2;
            const uint8_t *src = s.packed2 + first;
            const uint64_t left = data_bytes2 - first; // t < ntiles: at least one byte
            const uint32_t lim = left < tile_bytes2 ? (uint32_t)left : tile_bytes2;
#pragma unroll
            for (int j = 0; j < 8; j++) { // VPL = 32: a tile of column 2 is at most 8 KiB
                const uint32_t o = j * 1024 + lane * 16;
                if ((uint32_t)j * 1024u < tile_bytes2 && o < lim) __builtin_amdgcn_global_load_lds(MI355_GPTR(src + o), MI355_LPTR(dst2 + j * 1024), 16, 0, AUX);
            }
        }
        if (mask && t < tc.nfull && (uint32_t)lane * 16u < MASK_TILE)
            __builtin_amdgcn_global_load_lds(MI355_GPTR(mask + t * MASK_TILE + lane * 16), MI355_LPTR(mlds), 16, 0, 0);
    };
    static_assert(SAME || VPL == 32, "run-time widths: the DMA loop above covers 8 KiB");

    if (tile < tc.ntiles) issue(tile, lds2);
    while (tile < tc.ntiles) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the tile's images have landed
        uint32_t w1[G::LANE_DWORDS], w2[SAME ? G::LANE_DWORDS : 1], mw[WORDS] = {};
        read_lane_data<C1, VPL>(lds1, lane, w1);
        if constexpr (SAME) read_lane_data<C1, VPL>(lds2, lane, w2);
        const bool full = tile < tc.nfull;
        if (mask && full) {
#pragma unroll
            for (int j = 0; j < WORDS; j++) mw[j] = ((const uint32_t *)(mlds + lane * (WORDS * 4)))[j];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // column 1, the mask and (SAME) column 2 are in registers: earlier results leave, then the next tile flies during
        // the decode -- column 2's into the image that is not being decoded
        if (prev != ~0ull && store) store_prev();
        const uint64_t next = tile + stride;
        if (next < tc.ntiles) issue(next, lds2_next);
        columns_words<C1, VPL, SAME, WIDE, 0, G::LANE_DWORDS>(w1, w2, lds2 + (uint32_t)lane * (VPL / 8u * c2), c2, vmask2, pred, res);
        if constexpr (!SAME) {
            uint8_t *const t2 = lds2;
            lds2 = lds2_next;
            lds2_next = t2;
        }
#pragma unroll
        for (int j = 0; j < WORDS; j++) res[j] ^= inv;
        if (full) {
            if (mask) {
#pragma unroll
                for (int j = 0; j < WORDS; j++) res[j] = combine(res[j], mw[j]);
            }
#pragma unroll
            for (int j = 0; j < WORDS; j++) hits += __builtin_popcount(res[j]);
            prev = tile;
        } else {
            if (mask) { // the ragged tile (the column's last): only the bytes the mask is guaranteed to hold
                const uint8_t *mp = mask + tile * MASK_TILE + lane * (WORDS * 4);
                const int64_t left = (int64_t)(tc.n - tile * G::TILE_VALUES) - (int64_t)lane * VPL;
                const int nbytes = left <= 0 ? 0 : (int)((left >= VPL ? VPL : left) + 7) / 8;
#pragma unroll
                for (int j = 0; j < WORDS; j++) {
                    uint32_t m = 0;
#pragma unroll
                    for (int b = 0; b < 4; b++)
                        if (4 * j + b < nbytes) m |= (uint32_t)mp[4 * j + b] << (8 * b);
                    res[j] = combine(res[j], m);
                }
            }
            hits += tc.finish_tail(tile, res, out_lane + tile * G::BITMAP_BYTES, 1, lane, store);
            prev = ~0ull;
        }
        tile = next;
    }
    if (prev != ~0ull && store) store_prev();
    if (s.hits) hits_add(s, 0, wave_sum(hits), lane);
    hits_finalize(s, 1, lane);
}

} // namespace mi355
