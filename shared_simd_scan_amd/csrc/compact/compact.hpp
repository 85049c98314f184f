// compact/compact.hpp -- the device code of mi355_compact_dev: the values of the rows a bitmap selects, in row order, as a packed
// column of the same width.  gfx950 only; part of libmi355scan.so through compact/compact.hip.
//
// No block ever waits for another block: where a chunk's values go is known before compact_kernel starts, from the separate
// launches in front of it (kernels/bitmap.hpp: rowid_count_kernel counts the set bits of every chunk of kRowidChunk bitmap bytes
// = 16384 rows, rowid_scan_kernel turns the counts into exclusive prefixes inside scan groups of 1024 chunks plus one
// total per group).  A chunk's first output index and its count come from that prefix (chunk_span_wave, and chunk_span_serial in
// compact_edges_kernel: kernels/bitmap.hpp), as rowid_write_kernel's do.
//
// Edge dwords.  Chunk k owns the bit range [before_k c, end_k c) of the output, clipped at m c (m = min(total, capacity)).  The
// whole dwords inside it are its own and get plain stores.  The dword a range starts in (when it does not start on a dword
// boundary) and the dword it ends in (likewise) are shared with neighbours -- at low selectivity many chunks share one dword.
// compact_edges_kernel, one thread per chunk, zeroes those dwords first; compact_kernel then ORs its bits into them with
// global_atomic_or: OR is commutative, so the bytes do not depend on the order.  The output's very last dword is zeroed only
// up to byte ceil(m c / 8) and receives zero bits behind that, so the bytes behind the payload keep their values.
// compact_edges_kernel also leaves the grand total behind the chunk counts for the caller's count.
//
// compact_kernel<C>: persistent grid, a wave per chunk, chunks dealt out by stride.  A chunk whose count is zero (or whose
// first index is beyond the capacity) is not touched: no bitmap byte, no column byte.  Otherwise the chunk is 8 tiles of 64
// lanes x 32 consecutive rows (the geometry of kernels/rt_column.hpp), and lane l's mask of tile t is bitmap dword 64 t + l
// of the chunk: the lane reads its 8 words up front (bitmap_word_at: words beyond ceil(n/8) bytes bytewise).  A
// tile without a set bit (one ballot) moves nothing.  The others travel by LDS-DMA (non-temporal: the column is read once)
// into one of the wave's two images; the next such tile of the chunk is on its way while the current one is decoded.
//   decode      the lane's C dwords out of the image into registers, 32 unrolled steps of extract<C, K> under the mask bit:
//               no register array is indexed at run time, so nothing spills.
//   stage       a wave-private image of the OUTPUT: 64 C + 4 dwords, all zero between tiles.  Value p of the tile (p = the
//               wave's exclusive prefix of the lanes' popcounts + the lane's own earlier bits) is ORed into bit
//               carry + p C of it with ds_or_b32, a second one where it straddles a dword (never when C divides 32).  Lanes
//               address the stage by their values' positions, which differ by the lanes' popcounts: there is no fixed
//               stride for the banks to trip over, which the alternative -- a stage of values, gathered per output dword at
//               stride 32 / C -- would have needed padding for.
//   store       the whole dwords of the stage leave with consecutive lanes writing consecutive dwords (256 bytes per store
//               instruction, one_pass_store_policy on the output's bytes) and are zeroed again; the < 32 bits behind them
//               move to the stage's dword 0 and `carry` says how many they are.  They leave with the next tile, or with an
//               atomic OR when the chunk ends.  The chunk's first dword, when shared, leaves with an atomic OR too.
//   capacity    a value whose index in the chunk is not below the chunk's room (capacity - before) is not staged.
// Rows >= n have zero mask bits (the bitmap is canonical); the bytes behind row n - 1 may hold anything and select nothing.
// Dynamic LDS per wave: two images of 256 C bytes in whole KiB and the stage -- 2.3 KiB at C = 1, 24.0 KiB at C = 32.
// The kernels test no switch bit.
#pragma once

#include "../kernels.hpp"
#include "../kernels/rt_column.hpp" // the image of a tile; store_words_by

namespace mi355 {

struct CompactArgs {
    const uint8_t *packed;   // n values of c bits, 16 B aligned
    uint64_t n;
    const uint8_t *bitmap;   // canonical, 4 B aligned, nbytes = ceil(n / 8) are read
    uint64_t nbytes;
    unsigned long long *chunk_counts; // the workspace of RowidArgs: nchunks in-group prefixes, [nchunks] = the total
                                      // (written by compact_edges_kernel), then one total per scan group
    uint64_t nchunks;
    uint32_t *out;           // 16 B aligned; may be null when capacity == 0
    uint64_t capacity;       // values
    uint32_t c;
    uint32_t nts;            // result stores: 0 plain, 1 non-temporal, 2 write-through
};

constexpr int kCompactTiles = kRowidChunk * 8 / kRtTileRows;               // 8 tiles per chunk: a lane's mask of a tile is one bitmap dword
// the output stage: 64 C whole dwords, the carry's, the straddle's; a wave's LDS: two images of the input tile and the stage
constexpr uint32_t compact_stage_dwords(uint32_t c) { return 64u * c + 4u; }
constexpr uint32_t compact_wave_lds(uint32_t c) { return 2u * rt_image(c) + 4u * compact_stage_dwords(c); }
constexpr uint32_t compact_lds(uint32_t c) { return kWavesPerBlock * compact_wave_lds(c); }
static_assert(compact_lds(32) <= kCuLdsBytes, "LDS budget");

// Zeroes the dwords of the output that chunks share, one thread per chunk; thread 0 leaves the total at chunk_counts[nchunks].
static __global__ __launch_bounds__(256) void compact_edges_kernel(CompactArgs a)
{
    const uint64_t ch = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= a.nchunks) return;
    const ChunkPrefix prefix{a.chunk_counts, a.nchunks};
    unsigned long long total;
    const ChunkSpan s = chunk_span_serial(prefix, ch, total);
    if (ch == 0) *prefix.total() = total;
    if (s.count == 0 || s.before >= a.capacity) return;
    const unsigned long long m = total < a.capacity ? total : a.capacity;
    const unsigned long long end = s.before + s.count < a.capacity ? s.before + s.count : a.capacity;
    const unsigned long long last_bits = m * a.c;
    auto zero = [&](unsigned long long d) {
        if (d == (last_bits >> 5) && (last_bits & 31)) { // the output's last dword: only the payload's bytes
            const uint32_t nb = ((uint32_t)(last_bits & 31) + 7u) / 8u;
            for (uint32_t b = 0; b < nb; b++) ((uint8_t *)(a.out + d))[b] = 0;
        } else {
            a.out[d] = 0;
        }
    };
    const unsigned long long B = s.before * a.c, E = end * a.c;
    if (B & 31) zero(B >> 5);
    if (E & 31) zero(E >> 5);
}

// one of the lane's mask words by a wave-uniform index, without indexing the register array
__device__ __forceinline__ uint32_t compact_pick(const uint32_t (&m)[kCompactTiles], int t)
{
    uint32_t r = 0;
#pragma unroll
    for (int q = 0; q < kCompactTiles; q++) r = t == q ? m[q] : r;
    return r;
}

// value x of the tile at position p into the stage (bit `carry + p C`)
template <int C> __device__ __forceinline__ void compact_put(uint32_t *stage, uint32_t carry, uint32_t p, uint32_t x)
{
    const uint32_t bit = carry + p * C;
    const uint32_t d = bit >> 5, s = bit & 31u;
    __hip_atomic_fetch_or(stage + d, x << s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    if constexpr (32 % C != 0) { // a width that divides 32 never straddles: carry and p C are multiples of it
        if (s + C > 32) __hip_atomic_fetch_or(stage + d + 1, x >> (32u - s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
}

template <int C, int K = 0>
__device__ __forceinline__ void compact_decode(const uint32_t (&w)[C], uint32_t mask, uint32_t *stage, uint32_t carry, uint32_t &pos, uint32_t room)
{
    if ((mask >> K) & 1u) {
        if (pos < room) compact_put<C>(stage, carry, pos, extract<C, K, C>(w));
        pos++;
    }
    if constexpr (K + 1 < kRtVpl) compact_decode<C, K + 1>(w, mask, stage, carry, pos, room);
}

template <int C> __global__ __launch_bounds__(kBlockThreads) void compact_kernel(CompactArgs a)
{
    constexpr int AUX = 2; // the column is streamed once: non-temporal DMA
    constexpr uint32_t TILE_BYTES = rt_tile_bytes(C);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint8_t *const images = mi355_dyn_lds + (uint32_t)wave * compact_wave_lds(C);
    uint32_t *const stage = (uint32_t *)(images + 2u * rt_image(C));
    for (uint32_t j = lane; j < compact_stage_dwords(C); j += 64) stage[j] = 0;

    const uint64_t data_bytes = (a.n * C + 7) / 8;
    const ChunkPrefix prefix{a.chunk_counts, a.nchunks};
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock;
    const uint32_t nts = a.nts;

    // tile t of the chunk's column rows: LDS-DMA into `dst` (the column's last tile: only 16-byte pieces that start inside the payload)
    auto issue = [&](uint64_t tile, uint8_t *dst) {
        const uint64_t first = tile * TILE_BYTES; // a tile with a set bit holds a row < n: first < data_bytes
        if (data_bytes - first >= TILE_BYTES)
            dma_tile_full<(int)TILE_BYTES, AUX>(a.packed + first, dst, lane);
        else
            dma_tile_partial<(int)TILE_BYTES, AUX>(a.packed + first, data_bytes - first, dst, lane);
    };

    for (uint64_t ch = (uint64_t)blockIdx.x * kWavesPerBlock + wave; ch < a.nchunks; ch += stride) {
        const ChunkSpan span = chunk_span_wave(prefix, ch, lane); // the values in front of this chunk, and its own
        const unsigned long long before = span.before, count = span.count;
        if (count == 0 || before >= a.capacity) continue; // nothing of this chunk is read
        const uint32_t room = (uint32_t)(a.capacity - before < count ? a.capacity - before : count); // <= 16384

        // the lane's mask word of each of the 8 tiles, and which tiles select anything
        uint32_t m[kCompactTiles];
        uint32_t live = 0;
#pragma unroll
        for (int t = 0; t < kCompactTiles; t++) {
            const uint32_t w = bitmap_word_at(a.bitmap, a.nbytes, ch * kRowidChunk + (uint64_t)(t * 64 + lane) * 4);
            m[t] = w;
            if (__ballot(w != 0)) live |= 1u << t;
        }
        live = __builtin_amdgcn_readfirstlane(live);
        if (live == 0) continue; // (a bitmap that changed behind the count pass: nothing to address a tile with)

        const unsigned long long first_bit = before * C;
        uint32_t *dst = a.out + (first_bit >> 5);               // the output dword of the stage's dword 0
        uint32_t carry = (uint32_t)(first_bit & 31);            // bits of it that are not this tile's: a neighbour's, or carried over
        bool shared_first = carry != 0;                         // the chunk's first dword is a neighbour's too
        uint32_t done = 0;                                      // values of this chunk staged so far
        int cur = __builtin_ctz(live), buf = 0;
        issue(ch * kCompactTiles + cur, images);
        while (true) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the tile has landed
            live &= live - 1;
            const int next = live ? __builtin_ctz(live) : -1;
            if (next >= 0) issue(ch * kCompactTiles + next, images + (uint32_t)(buf ^ 1) * rt_image(C));

            const uint32_t mask = compact_pick(m, cur);
            uint32_t w[C];
            read_lane_data<C, kRtVpl>(images + (uint32_t)buf * rt_image(C), lane, w);
            const uint32_t mine = __builtin_popcount(mask);
            const uint32_t incl = wave_inclusive_scan(mine);
            uint32_t in_tile = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            uint32_t pos = incl - mine;
            const uint32_t left = room - done;
            compact_decode<C>(w, mask, stage, carry, pos, left);
            if (in_tile > left) in_tile = left;
            done += in_tile;

            const uint32_t bits = carry + in_tile * C;
            const uint32_t whole = bits >> 5;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the wave's ORs are in the stage (LDS is in order per wave)
            for (uint32_t j = lane; j < whole; j += 64) {
                const uint32_t v = stage[j];
                stage[j] = 0;
                const uint32_t one[1] = {v};
                if (shared_first && j == 0)
                    atomicOr(dst, v);
                else
                    store_words_by<1>((uint8_t *)(dst + j), one, nts);
            }
            if (whole) {
                // the bits behind the last whole dword move to the front of the stage
                const uint32_t rest = stage[whole];
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (lane == 0) {
                    stage[whole] = 0;
                    stage[0] = rest;
                }
                dst += whole;
                shared_first = false;
            }
            carry = bits & 31u;
            if (next < 0 || done >= room) break;
            cur = next;
            buf ^= 1;
        }
        // (the capacity may end a chunk with its next tile still on its way: it must have landed before the image is used again,
        // or the wave ends)
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        // what is left is less than a dword: the chunk's last dword, shared with the next chunk (or the output's last)
        if (carry) {
            const uint32_t v = stage[0];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (lane == 0) {
                atomicOr(dst, v);
                stage[0] = 0;
            }
        }
    }
}

} // namespace mi355
