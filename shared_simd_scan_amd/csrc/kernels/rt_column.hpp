// kernels/rt_column.hpp -- a packed column whose width is known only at run time, streamed through LDS: the tile geometry, the
// tile's LDS-DMA, the decode out of LDS, the ragged last tile, and the packed-out half (results assembled into whole dwords and
// stored).  The geometry, the decode and the packed-out helpers are what scan_columns_kernel's SAME = false form, group_aggregate,
// group_aggregate_wide, lookup, arith and compact share.  rt_issue_tile, lane_valid_rows and store_words_by are the one definition
// of their rule, used where the kernel compiles to the same registers with them (group_aggregate_wide; extras/histogram.hpp, topk/,
// compact/); the other kernels keep a copy in their own lambda, marked as such, because the shared form moved their register counts
// (profiles/r14_feature_kernels_asm.txt).  Device and constexpr code only; not part of kernels.hpp: whoever streams
// such a column includes it.  gfx950 only.
#pragma once

#include "tile.hpp"

namespace mi355 {

// ---- geometry: a wave owns tiles of 64 x 32 consecutive rows, lane l rows [32 l, 32 l + 32) -- 32 c bits = c whole dwords, so a
// lane's run starts on a dword boundary at any width ----
constexpr int kRtVpl = 32;                // rows per lane and tile
constexpr int kRtTileRows = 64 * kRtVpl;  // 2048
constexpr uint32_t rt_tile_bytes(uint32_t c) { return 64u * kRtVpl / 8u * c; }                    // 256 c
constexpr uint32_t rt_lane_bytes(uint32_t c) { return kRtVpl / 8u * c; }                          // the lane's run: at lane * this
// a tile in whole LDS-DMA instructions (the expression every kernel had: 256 c spelled otherwise compiles to other scalar code)
constexpr uint32_t rt_image(uint32_t c) { return (64u * kRtVpl * c / 8 + 1023u) / 1024u * 1024u; }
constexpr uint32_t rt_vmask(uint32_t c) { return c >= 32 ? 0xffffffffu : ((1u << c) - 1u); }
constexpr uint64_t rt_ntiles(uint64_t n) { return (n + kRtTileRows - 1) / kRtTileRows; }
constexpr uint64_t rt_nfull(uint64_t n) { return n / kRtTileRows; }

// tile t (< rt_ntiles) of a column of data_bytes = ceil(n c / 8) bytes: LDS-DMA into `dst` (the last tile: only 16-byte chunks
// that start inside the payload; they end inside the pad every packed buffer carries)
constexpr int kRtDmaInstrs = 8; // a tile is at most 8 KiB
static_assert(rt_image(32) == kRtDmaInstrs * 1024u, "the DMA loop covers the widest tile");
template <int AUX>
__device__ __forceinline__ void rt_issue_tile(const uint8_t *packed, uint64_t data_bytes, uint32_t tile_bytes, uint64_t t, uint8_t *dst, int lane)
{
    const uint64_t first = t * tile_bytes;
    const uint8_t *src = packed + first;
    const uint64_t left = data_bytes - first; // t < ntiles: at least one byte
    const uint32_t lim = left < tile_bytes ? (uint32_t)left : tile_bytes;
#pragma unroll
    for (int j = 0; j < kRtDmaInstrs; j++) {
        const uint32_t o = j * 1024 + lane * 16;
        if ((uint32_t)j * 1024u < tile_bytes && o < lim) __builtin_amdgcn_global_load_lds(MI355_GPTR(src + o), MI355_LPTR(dst + j * 1024), 16, 0, AUX);
    }
}

// value `ROW` of a lane's run of run-time width c, out of LDS: base = the lane's first byte.  ROW is a compile-time constant, so
// the position is scalar arithmetic: two dwords at a scalar offset (ds_read2_b32), a funnel shift by a scalar, a mask.  When c is a
// multiple of 4 the dword behind the last lane's run is read (and not used): the images' owners leave 16 bytes for it.
template <int ROW> __device__ __forceinline__ uint32_t columns_lds_value(const uint8_t *base, uint32_t c, uint32_t vmask)
{
    const uint32_t bit = (uint32_t)ROW * c; // wave-uniform
    const uint32_t *p = (const uint32_t *)(base + (bit >> 5) * 4);
    return __builtin_amdgcn_alignbit(p[1], p[0], bit & 31u) & vmask;
}

// ---- the ragged last tile: rows of the lane that lie inside a column of n rows (0 .. VPL), in a tile of 64 x VPL rows.
// Its bitmap bytes: (valid + 7) / 8. ----
template <int VPL> __device__ __forceinline__ int lane_valid_rows(uint64_t n, uint64_t tile, int lane)
{
    const int64_t left = (int64_t)(n - tile * (64 * VPL)) - (int64_t)lane * VPL;
    return left >= VPL ? VPL : (left <= 0 ? 0 : (int)left);
}

// ---- packed out: a lane's 32 results of CT bits are exactly CT whole dwords, at byte 4 CT lane of the tile's 256 CT bytes ----
// rt_insert: value K of the lane's run into its CT output dwords, the mirror of extract<C, K>.  Called for K = 0, 1, ..., 31 in
// this order: the first value that touches a dword assigns it (bit offset 0, or the upper part of a straddling value), so the
// dwords need no clearing.  x < 2^CT.
template <int CT, int K> __device__ __forceinline__ void rt_insert(uint32_t (&w)[CT], uint32_t x)
{
    constexpr int bit = K * CT;
    constexpr int d = bit >> 5;
    constexpr int s = bit & 31;
    if constexpr (s == 0) {
        w[d] = x;
    } else {
        w[d] |= x << s; // v_lshl_or_b32
        if constexpr (s + CT > 32) w[d + 1] = x >> (32 - s);
    }
}
template <int CT, int K = 0> __device__ __forceinline__ void rt_insert_all(uint32_t (&w)[CT], const uint32_t (&x)[kRtVpl])
{
    rt_insert<CT, K>(w, x[K]);
    if constexpr (K + 1 < kRtVpl) rt_insert_all<CT, K + 1>(w, x);
}

// N dwords of a lane at 4 N lane bytes of alignment: the widest stores that admits (store_words itself for N = 1, 2, 4)
template <int N, int NT> __device__ __forceinline__ void rt_store(uint8_t *dst, const uint32_t (&r)[N])
{
    constexpr int W = N % 4 == 0 ? 4 : (N % 2 == 0 ? 2 : 1);
#pragma unroll
    for (int j = 0; j < N; j += W) {
        uint32_t part[W];
#pragma unroll
        for (int q = 0; q < W; q++) part[q] = r[j + q];
        store_words<W, NT>(dst + 4 * j, part);
    }
}
// ... by the launch's store policy (0 plain, 1 non-temporal, 2 write-through): one wave-uniform branch
template <int N> __device__ __forceinline__ void store_words_by(uint8_t *dst, const uint32_t (&v)[N], uint32_t nts)
{
    if (nts == 2)
        rt_store<N, 2>(dst, v);
    else if (nts == 1)
        rt_store<N, 1>(dst, v);
    else
        rt_store<N, 0>(dst, v);
}

// the ragged tile: the lane's `valid` (0 .. 32) rows -- ceil(valid CT / 8) bytes, trailing bits of the last one zero
template <int CT> __device__ __forceinline__ void rt_store_tail(uint8_t *dst, const uint32_t (&r)[CT], int valid)
{
    const int bits = valid * CT;
    const int nbytes = (bits + 7) / 8;
    const int whole = nbytes / 4; // dwords written whole; dword `whole` gives the 0 .. 3 bytes left
    uint32_t part = 0;
#pragma unroll
    for (int j = 0; j < CT; j++) {
        const uint32_t v = r[j] & tail_mask(bits, j);
        if (j < whole) ((uint32_t *)dst)[j] = v;
        if (j == whole) part = v;
    }
#pragma unroll
    for (int b = 0; b < 3; b++)
        if (4 * whole + b < nbytes) dst[4 * whole + b] = (uint8_t)(part >> (8 * b));
}

// ---- a lane's 64-bit counter summed over the wave (the same total in every lane): 64 lanes x 2^24 stays inside 32 bits, so three
// 24-bit limbs go through the 32-bit wave_sum ----
__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long x)
{
    const unsigned long long lo = wave_sum((uint32_t)(x & 0xffffffull)), mid = wave_sum((uint32_t)((x >> 24) & 0xffffffull)),
                             hi = wave_sum((uint32_t)(x >> 48));
    return lo + (mid << 24) + (hi << 48);
}

} // namespace mi355
