// kernels/bitmap.hpp -- bitmap consumers: combine / count / row ids, and the chunk prefix over a bitmap that the row ids, compact/
// and topk/ share (ChunkPrefix, chunk_span_wave / chunk_span_serial, bitmap_word_at).  Part of kernels.hpp (gfx950 only).
#pragma once

#include "tile.hpp"

namespace mi355 {

// ---- bitmap consumers (the step after the path) ----------------------------------------
// combine: out = a OP b over ceil(n/8) bytes (16 B per lane), popcount of the result in the same pass.
// The bitmaps are canonical (bits >= n are zero), so AND / OR / XOR / ANDNOT keep them canonical.
enum BitmapOp { kBitAnd = 0, kBitOr = 1, kBitXor = 2, kBitAndNot = 3, kBitCount = 4 };

struct BitmapArgs {
    const uint8_t *a, *b;
    uint8_t *out;
    uint64_t nbytes;             // ceil(n/8)
    unsigned long long *count;   // device counter, pre-zeroed, may be null
};

template <int OP> __global__ __launch_bounds__(256) void bitmap_kernel(BitmapArgs g)
{
    const uint64_t nvec = g.nbytes / 16;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t cnt = 0;
    auto combine = [](uint32_t x, uint32_t y) -> uint32_t {
        return OP == kBitAnd ? (x & y) : OP == kBitOr ? (x | y) : OP == kBitXor ? (x ^ y) : OP == kBitAndNot ? (x & ~y) : x;
    };
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
        u32x4 x = ((const u32x4 *)g.a)[i];
        u32x4 r;
        if constexpr (OP != kBitCount) {
            u32x4 y = ((const u32x4 *)g.b)[i];
            r = u32x4{combine(x.x, y.x), combine(x.y, y.y), combine(x.z, y.z), combine(x.w, y.w)};
            ((u32x4 *)g.out)[i] = r;
        } else {
            r = x;
        }
        cnt += __builtin_popcount(r.x) + __builtin_popcount(r.y) + __builtin_popcount(r.z) + __builtin_popcount(r.w);
    }
    // the < 16 trailing bytes
    if (blockIdx.x == 0 && threadIdx.x < (g.nbytes & 15)) {
        const uint64_t i = nvec * 16 + threadIdx.x;
        uint32_t r = g.a[i];
        if constexpr (OP != kBitCount) {
            r = combine(r, g.b[i]) & 0xffu;
            g.out[i] = (uint8_t)r;
        }
        cnt += __builtin_popcount(r);
    }
    if (g.count) {
        cnt = wave_sum(cnt);
        if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(g.count + (blockIdx.x % kHitSlots), (unsigned long long)cnt);
    }
}

// moves the kHitSlots partial counts of bitmap_kernel into *out and re-zeroes them
static __global__ __launch_bounds__(64) void sum_slots_kernel(unsigned long long *slots, unsigned long long *out)
{
    unsigned long long v = slots[threadIdx.x];
    slots[threadIdx.x] = 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (threadIdx.x == 0) *out = v;
}

// selection vector: row ids (first_row + i for every set bit i) in ascending order.
// Pass 1 (rowid_count_kernel): popcount per chunk of kRowidChunk bytes.  Pass 2 (rowid_scan_kernel): exclusive scan of
// the chunk counts, in groups.  Pass 3 (rowid_write_kernel): each wave expands its chunk.
constexpr int kRowidChunk = 2048; // bytes of bitmap per wave = 16384 rows

// the bitmap's dword at byte `o`, safe at the ragged end: the whole dword if it lies inside the nbytes = ceil(n / 8) a bitmap is
// guaranteed to hold, else the bytes below nbytes
__device__ __forceinline__ uint32_t bitmap_word_at(const uint8_t *bitmap, uint64_t nbytes, uint64_t o)
{
    if (o + 4 <= nbytes) return *(const uint32_t *)(bitmap + o);
    uint32_t w = 0;
    for (int b = 0; b < 4; b++)
        if (o + b < nbytes) w |= (uint32_t)bitmap[o + b] << (8 * b);
    return w;
}

struct RowidArgs {
    const uint8_t *bitmap;
    uint64_t nbytes;
    uint64_t first_row;
    unsigned long long *chunk_counts; // nchunks + 1 entries (exclusive scan inside each group of kRowidScanGroup, in place;
                                      // [nchunks] = total), followed by one total per group
    uint64_t nchunks;
    uint64_t *rowids;
    uint64_t capacity;
};

static __global__ __launch_bounds__(256) void rowid_count_kernel(RowidArgs g)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t ch = wave; ch < g.nchunks; ch += nwaves) {
        const uint64_t base = ch * kRowidChunk;
        uint32_t cnt = 0;
#pragma unroll
        for (int k = 0; k < kRowidChunk / (64 * 4); k++)
            cnt += __builtin_popcount(bitmap_word_at(g.bitmap, g.nbytes, base + (uint64_t)(k * 64 + lane) * 4));
        cnt = wave_sum(cnt);
        if (lane == 0) g.chunk_counts[ch] = cnt;
    }
}

// Pass 2: exclusive scan of the chunk counts in groups of kRowidScanGroup (one block per group: coalesced loads of
// four counts per thread, wave shuffles, four wave totals through LDS); each group's total goes to group_totals[],
// and pass 3 adds the (few) totals of the groups before its own.  The first version scanned all counts in ONE block
// with every thread walking a private strip: 115 us for the 61 k chunks of 1e9 rows, more than passes 1 and 3 together
// at low selectivity.
constexpr int kRowidScanGroup = 1024;

// The prefix part of the selection workspace as pass 2 leaves it: nchunks prefixes (exclusive inside each scan group), the slot
// of the grand total, one total per scan group.  rowid_prefix_words() is its size; the kernels that consume it (pass 3 below,
// compact/, topk/) ask chunk_span_wave / chunk_span_serial where a chunk's items go.
constexpr uint64_t rowid_scan_groups(uint64_t nchunks) { return (nchunks + kRowidScanGroup - 1) / kRowidScanGroup; }
constexpr uint64_t rowid_prefix_words(uint64_t nchunks) { return nchunks + 1 + rowid_scan_groups(nchunks); }
struct ChunkPrefix {
    unsigned long long *counts;
    uint64_t nchunks;
    __device__ __forceinline__ unsigned long long *total() const { return counts + nchunks; }
    __device__ __forceinline__ unsigned long long *group_totals() const { return counts + nchunks + 1; }
    __device__ __forceinline__ uint64_t ngroups() const { return rowid_scan_groups(nchunks); }
};
// where a chunk's items go: `before` of them precede it, `count` are its own
struct ChunkSpan {
    unsigned long long before, count;
};

__device__ __forceinline__ unsigned long long uniform64(unsigned long long v)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
// the sum of the first `groups` group totals, by the 64 lanes of a wave (the same in every lane)
__device__ __forceinline__ unsigned long long chunk_groups_sum(const ChunkPrefix &p, uint64_t groups, int lane)
{
    const unsigned long long *const totals = p.group_totals();
    unsigned long long s = 0;
    for (uint64_t i = lane; i < groups; i += 64) s += totals[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}
// A wave's view of chunk ch, wave-uniform: before = the totals of the earlier scan groups + the chunk's prefix inside its group;
// count = the next prefix, or its group's total, minus its own prefix.
__device__ __forceinline__ ChunkSpan chunk_span_wave(const ChunkPrefix &p, uint64_t ch, int lane)
{
    const uint64_t g = ch / kRowidScanGroup;
    const unsigned long long before = chunk_groups_sum(p, g, lane);
    const unsigned long long prefix = p.counts[ch];
    const bool last_of_group = (ch + 1) % kRowidScanGroup == 0 || ch + 1 == p.nchunks;
    const unsigned long long count = uniform64((last_of_group ? p.group_totals()[g] : p.counts[ch + 1]) - prefix);
    return {uniform64(before + prefix), count};
}
// One thread's view of chunk ch (a kernel with a thread per chunk); `total` gets the grand total.
__device__ __forceinline__ ChunkSpan chunk_span_serial(const ChunkPrefix &p, uint64_t ch, unsigned long long &total)
{
    const unsigned long long *const totals = p.group_totals();
    const uint64_t ngroups = p.ngroups(), g = ch / kRowidScanGroup;
    unsigned long long before = 0;
    total = 0;
    for (uint64_t i = 0; i < ngroups; i++) {
        const unsigned long long t = totals[i];
        total += t;
        if (i < g) before += t;
    }
    const unsigned long long prefix = p.counts[ch];
    const bool last_of_group = (ch + 1) % kRowidScanGroup == 0 || ch + 1 == p.nchunks;
    const unsigned long long next = last_of_group ? totals[g] : p.counts[ch + 1];
    return {before + prefix, next - prefix};
}

static __global__ __launch_bounds__(256) void rowid_scan_kernel(RowidArgs g)
{
    __shared__ unsigned long long wave_tot[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t i0 = (uint64_t)blockIdx.x * kRowidScanGroup + (uint64_t)threadIdx.x * 4;
    unsigned long long v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = i0 + j < g.nchunks ? g.chunk_counts[i0 + j] : 0ull;
    const unsigned long long mine = v[0] + v[1] + v[2] + v[3];
    unsigned long long incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        unsigned long long t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    unsigned long long run = incl - mine;
    for (int w = 0; w < wave; w++) run += wave_tot[w];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (i0 + j < g.nchunks) g.chunk_counts[i0 + j] = run;
        run += v[j];
    }
    if (threadIdx.x == 255) ChunkPrefix{g.chunk_counts, g.nchunks}.group_totals()[blockIdx.x] = run;
}

// Pass 3.  A step covers 64 lanes x 32 bits = 2048 rows.  Each lane expands its word into a wave-private LDS buffer
// (16-bit offsets inside the step, at the position given by the wave prefix of the popcounts), then the wave copies
// the buffer out with consecutive lanes writing consecutive ids (512 B per store instruction).  Expanding straight
// into global memory made every store instruction touch up to 64 lines: 2.7 ms for 5e8 ids against 4 GB / 6 TB/s.
static __global__ __launch_bounds__(256) void rowid_write_kernel(RowidArgs g)
{
    __shared__ uint16_t stage[4][2048];
    const int lane = threadIdx.x & 63;
    uint16_t *const st = stage[threadIdx.x >> 6];
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const ChunkPrefix prefix{g.chunk_counts, g.nchunks};
    if (wave == 0) { // the grand total, for the caller's count
        const unsigned long long s = chunk_groups_sum(prefix, prefix.ngroups(), lane);
        if (lane == 0) *prefix.total() = s;
    }
    for (uint64_t ch = wave; ch < g.nchunks; ch += nwaves) {
        const uint64_t base = ch * kRowidChunk;
        uint64_t out = chunk_span_wave(prefix, ch, lane).before; // ids before this chunk
#pragma unroll 1
        for (int k = 0; k < kRowidChunk / (64 * 4); k++) {
            uint32_t w = bitmap_word_at(g.bitmap, g.nbytes, base + (uint64_t)(k * 64 + lane) * 4);
            // exclusive prefix of the lanes' popcounts inside the wave
            const uint32_t c = __builtin_popcount(w);
            uint32_t incl = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                uint32_t t = __shfl_up(incl, d, 64);
                if (lane >= d) incl += t;
            }
            const uint32_t total = __shfl(incl, 63, 64);
            uint32_t pos = incl - c;
            const uint32_t off0 = lane * 32; // row offset of the lane's bit 0 inside the step
            while (w) {
                const int bit = __builtin_ctz(w);
                w &= w - 1;
                st[pos++] = (uint16_t)(off0 + bit);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the wave's LDS writes are done (LDS is in order per wave)
            const uint64_t row0 = g.first_row + (base + (uint64_t)k * 256) * 8;
            for (uint32_t i = lane; i < total; i += 64) {
                const uint64_t p = out + i;
                if (p < g.capacity) g.rowids[p] = row0 + st[i];
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // reads done before the next step overwrites the buffer
            out += total;
        }
    }
}

} // namespace mi355
