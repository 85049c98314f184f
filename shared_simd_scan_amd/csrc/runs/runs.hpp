// runs/runs.hpp -- the device code of mi355_run_encode_dev and mi355_run_decode_dev: a packed column's runs as two packed columns
// (the runs' values, the runs' ends = the row behind a run's last row), and the expansion of such a pair back onto the rows.
// gfx950 only; part of libmi355scan.so through runs/run_encode.hip and runs/run_decode.hip.
//
// run_encode.  Row i is a TAIL when i == n - 1 or x_i != x_{i+1}; run j ends at the j-th tail.  The tail form makes chunk k (16384
// rows, a wave per chunk) own the slots [before_k, before_k + count_k) of BOTH outputs, which is compact's geometry unchanged
// (compact/compact.hpp): no block ever waits for another, where a chunk's runs go is known from the launches in front.
//   1  run_count_kernel     run-time width; a chunk's tails into the chunk's word of the caller's workspace, the wave's chunks
//                           together into the call's count with one atomic add per wave
//   2  rowid_scan_kernel    as it stands (kernels/bitmap.hpp)
//   3  compact_edges_kernel as it stands, once per output given with that output's width: zeroes the dwords chunks share
//   4  run_emit_kernel<C>   C = the column's width, the ends' width at run time.  chunk_span_wave gives the chunk's first slot and
//                           count; a chunk without a tail touches nothing.  Per tile a lane forms the tail word of its 32 rows, the
//                           lanes' popcounts go through the exclusive wave scan, tail number p of the tile puts its value into a
//                           wave-private stage at C bits and its end (first row of the lane + bit + 1) into a second stage at ce
//                           bits: compact_put's scheme -- ds_or_b32 into a zeroed stage, whole dwords leave with consecutive lanes
//                           writing consecutive dwords, the carry stays in dword 0, atomic ORs go to the chunk's first and last
//                           shared dword.  A slot at or beyond the capacity is not staged.
// The row behind a lane's 32 rows is the first row of the next lane's run, which starts on a dword boundary of the same image; for
// lane 63 it is the first row of the next tile, the low c bits of that tile's first dword in global memory, read beside the DMA and
// only when the row exists.  Rows >= n are masked out of the tail word and row n - 1 is forced in, so what lies behind the column
// reaches nothing.
//
// run_decode_kernel<CV>: tiles of 64 x 32 rows dealt out across the waves; j(i) = the number of j < R with end_j <= i.  Per tile
// the wave finds j(first row) by a 64-way search over the ends (each lane probes one of 64 evenly spaced entries, a ballot narrows
// the range: at most six rounds for 2^32 runs), and j(last row) the same way unless the run of the first row also covers the last.
// One run: the tile is one value, or `miss`, with no further read.  Several: a lane binary-searches [j_lo, j_hi] for its own first
// row and walks its 32 rows, advancing while end_j <= i -- bounded by R, exact for any number of zero-length runs.  Every index is
// clamped to [0, R): unsorted ends yield some value of the table or `miss`, never a read beyond the tables.
// The kernels test no switch bit.
#pragma once

#include <type_traits>

#include "../compact/compact.hpp"   // compact_edges_kernel, compact_put, the stage's size
#include "../kernels.hpp"
#include "../kernels/rt_column.hpp" // the tile stream of a column of run-time width, and the packed-out half

namespace mi355 {

constexpr int kRunsChunkRows = kRowidChunk * 8; // 16384: the chunk of the prefix over n rows
constexpr int kRunsChunkTiles = kRunsChunkRows / kRtTileRows;
static_assert(kRunsChunkTiles == 8 && kRunsChunkTiles * kRtTileRows == kRunsChunkRows, "a chunk is a whole number of tiles");

struct RunEncodeArgs {
    const uint8_t *packed;            // n values of c bits, 16 B aligned
    uint64_t n;
    unsigned long long *chunk_counts; // the caller's workspace: rowid_prefix_words(nchunks) words
    uint64_t nchunks;
    uint32_t *values;                 // nullable: min(r, capacity) values of c bits
    uint32_t *ends;                   // nullable: as many ends of ce bits
    uint64_t capacity;
    unsigned long long *count;        // zeroed in front of run_count_kernel, whose waves add to it
    uint32_t c, ce;
    uint32_t nts;                     // result stores: 0 plain, 1 non-temporal, 2 write-through
};

struct RunDecodeArgs {
    const uint32_t *values; // R entries of CV bits, 4 B aligned
    const uint32_t *ends;   // R entries of ce bits, 4 B aligned, non-decreasing
    const unsigned long long *runs_dev; // nullable: R = min(runs, *runs_dev)
    uint64_t runs;          // <= 2^32 - 1
    uint64_t n;
    uint8_t *out;           // n values of CV bits, 16 B aligned; exactly ceil(n CV / 8) bytes are written
    unsigned long long *uncovered; // nullable: zeroed in front of the launch, one add per wave
    uint32_t ce;
    uint32_t miss;          // < 2^CV
    uint32_t nts;
};

// run_count_kernel: a wave's two images; + 16: the dword behind the last lane's run is read (and not used)
constexpr uint32_t run_count_wave_lds(uint32_t c) { return 2u * rt_image(c); }
constexpr uint32_t run_count_block_lds(uint32_t c) { return kWavesPerBlock * run_count_wave_lds(c) + 16u; }
// run_emit_kernel: two images and the two output stages
constexpr uint32_t run_emit_wave_lds(uint32_t c, uint32_t ce) { return 2u * rt_image(c) + 4u * compact_stage_dwords(c) + 4u * compact_stage_dwords(ce); }
constexpr uint32_t run_emit_block_lds(uint32_t c, uint32_t ce) { return kWavesPerBlock * run_emit_wave_lds(c, ce); }
static_assert(run_count_block_lds(32) <= kCuLdsBytes && run_emit_block_lds(32, 32) <= kCuLdsBytes, "LDS budget");

// f(integral_constant<int, K>) for the K = 0 .. 31 of a lane's run, straight-line
template <int K = 0, typename F> __device__ __forceinline__ void run_rows(F &&f)
{
    f(std::integral_constant<int, K>{});
    if constexpr (K + 1 < kRtVpl) run_rows<K + 1>(f);
}

// the tile a wave that walks its chunks tile by tile takes after tile t: the chunk's next one, else the first of the wave's next chunk
__device__ __forceinline__ uint64_t run_next_tile(uint64_t t, uint64_t ntiles, uint64_t nwaves)
{
    const uint64_t nx = t + 1;
    if ((nx % kRunsChunkTiles) != 0 && nx < ntiles) return nx;
    return (t / kRunsChunkTiles + nwaves) * kRunsChunkTiles;
}

// the first row of tile t + 1, straight from global memory (the same address in every lane), 0 when the column ends in tile t
__device__ __forceinline__ uint32_t run_row_behind_tile(const uint8_t *packed, uint32_t tile_bytes, uint32_t vmask, uint64_t n, uint64_t t)
{
    if ((t + 1) * kRtTileRows >= n) return 0;
    return *(const uint32_t *)(packed + (t + 1) * tile_bytes) & vmask;
}

// the tail word of a lane's 32 rows from their "differs from the next row" word: rows >= n leave it, row n - 1 enters it
__device__ __forceinline__ uint32_t run_clip_tails(uint32_t differs, uint64_t n, uint64_t tile, int lane)
{
    const int64_t left = (int64_t)(n - tile * kRtTileRows) - (int64_t)lane * kRtVpl; // rows from the lane's first to the column's end
    if (left > kRtVpl) return differs;
    if (left <= 0) return 0;
    return (differs & tail_mask((int)left, 0)) | (1u << (left - 1));
}

// ---- launch 1: a chunk's number of tails ------------------------------------------------------------------------------------
static __global__ __launch_bounds__(kBlockThreads) void run_count_kernel(RunEncodeArgs a)
{
    constexpr int AUX = 0; // the column is read again by the emitting kernel: default policy
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t c = a.c;
    const uint32_t tile_bytes = rt_tile_bytes(c);
    uint8_t *cur = mi355_dyn_lds + (uint32_t)wave * run_count_wave_lds(c);
    uint8_t *nxt = cur + rt_image(c);
    const uint32_t vmask = rt_vmask(c);
    const uint64_t n = a.n;
    const uint64_t ntiles = rt_ntiles(n);
    const uint64_t data_bytes = (n * c + 7) / 8;
    const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
    uint64_t tile = ((uint64_t)blockIdx.x * kWavesPerBlock + wave) * kRunsChunkTiles;
    uint32_t edge_next = 0;
    auto issue = [&](uint64_t t, uint8_t *dst) {
        rt_issue_tile<AUX>(a.packed, data_bytes, tile_bytes, t, dst, lane);
        edge_next = run_row_behind_tile(a.packed, tile_bytes, vmask, n, t); // beside the DMA, not behind the wait
    };
    if (tile < ntiles) issue(tile, cur);
    uint32_t acc = 0;                 // the lane's tails of the chunk so far (<= 16384)
    unsigned long long mine = 0;      // the wave's chunks together
    while (tile < ntiles) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the tile has landed
        const uint32_t edge = edge_next;
        const uint64_t next = run_next_tile(tile, ntiles, nwaves);
        if (next < ntiles) issue(next, nxt);
        const uint8_t *const base = cur + (uint32_t)lane * rt_lane_bytes(c);
        // the row behind the lane's run: the next lane's first row, on a dword boundary of the image; lane 63: the next tile's
        const uint32_t behind = lane < 63 ? (*(const uint32_t *)(base + rt_lane_bytes(c)) & vmask) : edge;
        uint32_t differs = 0;
        uint32_t x = columns_lds_value<0>(base, c, vmask);
        run_rows([&](auto K) {
            constexpr int k = decltype(K)::value;
            uint32_t y = behind;
            if constexpr (k + 1 < kRtVpl) y = columns_lds_value<(k + 1) % kRtVpl>(base, c, vmask);
            differs |= (x != y ? 1u : 0u) << k;
            x = y;
        });
        acc += (uint32_t)__builtin_popcount(run_clip_tails(differs, n, tile, lane));
        if ((tile + 1) % kRunsChunkTiles == 0 || tile + 1 >= ntiles) { // the chunk ends
            const uint32_t total = wave_sum(acc);
            if (lane == 0) a.chunk_counts[tile / kRunsChunkTiles] = total;
            mine += total;
            acc = 0;
        }
        uint8_t *t = cur;
        cur = nxt;
        nxt = t;
        tile = next;
    }
    if (lane == 0 && mine) __hip_atomic_fetch_add(a.count, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- launch 4: the runs themselves --------------------------------------------------------------------------------------------
// value x at position p of the tile into a stage of run-time width w (bit `carry + p w`): compact_put with the width in a register
__device__ __forceinline__ void run_put(uint32_t *stage, uint32_t carry, uint32_t p, uint32_t w, uint32_t x)
{
    const uint32_t bit = carry + p * w;
    const uint32_t d = bit >> 5, s = bit & 31u;
    __hip_atomic_fetch_or(stage + d, x << s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    if (s + w > 32) __hip_atomic_fetch_or(stage + d + 1, x >> (32u - s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// where a chunk's part of one output stands: the output dword of the stage's dword 0, the bits of it that are not this tile's, and
// whether the chunk's first dword is a neighbour's too
struct RunOut {
    uint32_t *dst;
    uint32_t carry;
    bool shared_first;
};
__device__ __forceinline__ RunOut run_out_at(uint32_t *out, unsigned long long before, uint32_t w)
{
    const unsigned long long first_bit = before * w;
    const uint32_t carry = (uint32_t)(first_bit & 31);
    return {out + (first_bit >> 5), carry, carry != 0};
}
// the whole dwords of a stage that holds `staged` more values of w bits leave, consecutive lanes writing consecutive dwords, and are
// zeroed again; the < 32 bits behind them move to the stage's dword 0 (compact_kernel's store step)
__device__ __forceinline__ void run_flush(uint32_t *stage, RunOut &o, uint32_t staged, uint32_t w, int lane, uint32_t nts)
{
    const uint32_t bits = o.carry + staged * w;
    const uint32_t whole = bits >> 5;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the wave's ORs are in the stage (LDS is in order per wave)
    for (uint32_t j = lane; j < whole; j += 64) {
        const uint32_t v = stage[j];
        stage[j] = 0;
        const uint32_t one[1] = {v};
        if (o.shared_first && j == 0)
            atomicOr(o.dst, v);
        else
            store_words_by<1>((uint8_t *)(o.dst + j), one, nts);
    }
    if (whole) {
        const uint32_t rest = stage[whole];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane == 0) {
            stage[whole] = 0;
            stage[0] = rest;
        }
        o.dst += whole;
        o.shared_first = false;
    }
    o.carry = bits & 31u;
}
// what is left when the chunk ends is less than a dword: the chunk's last dword, shared with the next chunk (or the output's last)
__device__ __forceinline__ void run_flush_last(uint32_t *stage, RunOut &o, int lane)
{
    if (!o.carry) return;
    const uint32_t v = stage[0];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (lane == 0) {
        atomicOr(o.dst, v);
        stage[0] = 0;
    }
}

// "row K differs from the row behind it" for the lane's 32 rows out of its C dwords
template <int C, int K = 0> __device__ __forceinline__ uint32_t run_differs(const uint32_t (&w)[C], uint32_t behind)
{
    const uint32_t x = extract<C, K, C>(w);
    if constexpr (K + 1 < kRtVpl) {
        return ((x != extract<C, K + 1, C>(w) ? 1u : 0u) << K) | run_differs<C, K + 1>(w, behind);
    } else {
        return (x != behind ? 1u : 0u) << K;
    }
}

template <int C> __global__ __launch_bounds__(kBlockThreads) void run_emit_kernel(RunEncodeArgs a)
{
    constexpr int AUX = 2; // the column's last read: non-temporal DMA
    constexpr uint32_t TILE_BYTES = rt_tile_bytes(C);
    constexpr uint32_t VMASK = rt_vmask(C);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t ce = a.ce;
    uint8_t *const images = mi355_dyn_lds + (uint32_t)wave * run_emit_wave_lds(C, ce);
    uint32_t *const vstage = (uint32_t *)(images + 2u * rt_image(C));
    uint32_t *const estage = vstage + compact_stage_dwords(C);
    for (uint32_t j = lane; j < compact_stage_dwords(C) + compact_stage_dwords(ce); j += 64) vstage[j] = 0;

    const uint64_t n = a.n;
    const uint64_t ntiles = rt_ntiles(n);
    const uint64_t data_bytes = (n * C + 7) / 8;
    const ChunkPrefix prefix{a.chunk_counts, a.nchunks};
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock;
    const uint32_t nts = a.nts;
    const bool with_values = a.values != nullptr, with_ends = a.ends != nullptr;
    uint32_t edge_next = 0;
    auto issue = [&](uint64_t t, uint8_t *dst) {
        rt_issue_tile<AUX>(a.packed, data_bytes, TILE_BYTES, t, dst, lane);
        edge_next = run_row_behind_tile(a.packed, TILE_BYTES, VMASK, n, t);
    };

    for (uint64_t ch = (uint64_t)blockIdx.x * kWavesPerBlock + wave; ch < a.nchunks; ch += stride) {
        const ChunkSpan span = chunk_span_wave(prefix, ch, lane); // the runs that end in front of this chunk, and in it
        const unsigned long long before = span.before, count = span.count;
        if (count == 0 || before >= a.capacity) continue; // nothing of this chunk is read
        const uint32_t room = (uint32_t)(a.capacity - before < count ? a.capacity - before : count); // <= 16384
        RunOut vo = run_out_at(a.values, before, C), eo = run_out_at(a.ends, before, ce);
        uint32_t done = 0; // runs of this chunk staged so far
        uint64_t tile = ch * kRunsChunkTiles;
        const uint64_t tend = tile + kRunsChunkTiles < ntiles ? tile + kRunsChunkTiles : ntiles;
        int buf = 0;
        issue(tile, images);
        while (true) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the tile has landed
            const uint32_t edge = edge_next;
            const bool more = tile + 1 < tend;
            if (more) issue(tile + 1, images + (uint32_t)(buf ^ 1) * rt_image(C));

            const uint8_t *const image = images + (uint32_t)buf * rt_image(C);
            uint32_t w[C];
            read_lane_data<C, kRtVpl>(image, lane, w);
            const uint32_t *const mine_lds = (const uint32_t *)(image + (uint32_t)lane * rt_lane_bytes(C));
            const uint32_t behind = lane < 63 ? (mine_lds[C] & VMASK) : edge; // the next lane's first row; lane 63: the next tile's
            uint32_t tails = run_clip_tails(run_differs<C>(w, behind), n, tile, lane);
            const uint32_t mine = (uint32_t)__builtin_popcount(tails);
            const uint32_t incl = wave_inclusive_scan(mine);
            uint32_t in_tile = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            if (in_tile) {
                uint32_t pos = incl - mine;
                const uint32_t left = room - done;
                const uint32_t row0 = (uint32_t)(tile * kRtTileRows) + (uint32_t)lane * kRtVpl; // n <= 2^32 - 1
                while (tails && pos < left) { // the lane's tails in row order; a slot at or beyond the capacity is not staged
                    const uint32_t k = (uint32_t)__builtin_ctz(tails);
                    tails &= tails - 1;
                    if (with_values) {
                        // row k of the lane's run out of the image (a run-time row: the registers are not indexed)
                        const uint32_t bit = k * C, d = bit >> 5;
                        const uint32_t lo = mine_lds[d], hi = mine_lds[d + 1 < (uint32_t)C ? d + 1 : (uint32_t)C - 1];
                        compact_put<C>(vstage, vo.carry, pos, __builtin_amdgcn_alignbit(hi, lo, bit & 31u) & VMASK);
                    }
                    if (with_ends) run_put(estage, eo.carry, pos, ce, row0 + k + 1u);
                    pos++;
                }
                if (in_tile > left) in_tile = left;
                done += in_tile;
                if (with_values) run_flush(vstage, vo, in_tile, C, lane, nts);
                if (with_ends) run_flush(estage, eo, in_tile, ce, lane, nts);
            }
            if (!more || done >= room) break;
            tile++;
            buf ^= 1;
        }
        // (the capacity may end a chunk with its next tile still on its way: it must have landed before the image is used again)
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        if (with_values) run_flush_last(vstage, vo, lane);
        if (with_ends) run_flush_last(estage, eo, lane);
    }
}

// ---- run_decode ---------------------------------------------------------------------------------------------------------------
// entry j (< R) of a packed table of run-time width w, read where it lies: two dwords, never beyond dword last_word
__device__ __forceinline__ uint32_t run_entry(const uint32_t *table, uint32_t j, uint32_t w, uint32_t vmask, uint32_t last_word)
{
    const uint64_t bit = (uint64_t)j * w; // 37 bits, the dword index 32
    const uint32_t d = (uint32_t)(bit >> 5);
    const uint32_t lo = table[d], hi = table[d < last_word ? d + 1u : last_word];
    return __builtin_amdgcn_alignbit(hi, lo, (uint32_t)bit & 31u) & vmask;
}
template <int CV> __device__ __forceinline__ uint32_t run_value(const uint32_t *table, uint32_t j, uint32_t last_word)
{
    return run_entry(table, j, CV, rt_vmask(CV), last_word);
}

// the dword that holds the last bit of entry R - 1 (R >= 1)
__device__ __forceinline__ uint32_t run_last_word(uint64_t R, uint32_t w) { return (uint32_t)((R * w - 1) >> 5); }

struct RunEnds {
    const uint32_t *table;
    uint32_t w, vmask, last_word;
    __device__ __forceinline__ uint64_t at(uint32_t j) const { return run_entry(table, j, w, vmask, last_word); }
};

// j(i) within [lo, hi] (lo <= hi <= R), the whole wave together: each lane probes one of 64 evenly spaced entries, the ballot of
// "end <= i" narrows [lo, hi] to what lies between two probes.  Wave-uniform in, wave-uniform out.  Ends that are not sorted still
// leave the range inside [lo, hi], smaller every round.
__device__ __forceinline__ uint64_t run_search_wave(const RunEnds &e, uint64_t i, uint64_t lo, uint64_t hi, int lane)
{
    while (lo < hi) {
        const uint64_t len = hi - lo, step = (len + 63) / 64;
        const uint64_t at = lo + (uint64_t)lane * step;
        const bool below = at < hi && e.at((uint32_t)at) <= i;
        const uint64_t k = (uint64_t)__builtin_popcountll(__ballot(below)); // probes 0 .. k - 1 end at or in front of row i
        if (k == 0) {
            hi = lo;
        } else {
            const uint64_t cut = lo + k * step;
            lo = lo + (k - 1) * step + 1;
            hi = cut < hi ? cut : hi;
        }
    }
    return lo;
}

template <int CV> __global__ __launch_bounds__(kBlockThreads) void run_decode_kernel(RunDecodeArgs a)
{
    constexpr uint32_t OUT_TILE = rt_tile_bytes(CV);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t n = a.n;
    const uint64_t ntiles = rt_ntiles(n), nfull = rt_nfull(n);
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock;
    const uint32_t nts = a.nts, miss = a.miss;
    uint64_t R = a.runs;
    if (a.runs_dev) {
        const uint64_t have = uniform64(*a.runs_dev);
        R = have < R ? have : R;
    }
    const uint32_t vlast = R ? run_last_word(R, CV) : 0u;
    const RunEnds ends{a.ends, a.ce, rt_vmask(a.ce), R ? run_last_word(R, a.ce) : 0u};

    uint32_t res[CV];
    unsigned long long outside = 0; // the lane's rows behind the last run so far
    uint8_t *const out_lane = a.out + (uint32_t)lane * (4u * CV);
    uint64_t j_from = 0; // the wave's tiles ascend: j(first row) of the tile before bounds the next search from below
    for (uint64_t tile = (uint64_t)blockIdx.x * kWavesPerBlock + wave; tile < ntiles; tile += stride) {
        const uint64_t row0 = tile * kRtTileRows;
        const uint64_t last = row0 + kRtTileRows - 1 < n - 1 ? row0 + kRtTileRows - 1 : n - 1;
        const int valid = lane_valid_rows<kRtVpl>(n, tile, lane);
        const uint64_t j_lo = run_search_wave(ends, row0, j_from, R, lane);
        j_from = j_lo;
        // one run covers the tile when the run of the first row ends behind the last row (or no run is left)
        uint64_t j_hi = j_lo;
        if (j_lo < R && ends.at((uint32_t)j_lo) <= last) j_hi = run_search_wave(ends, last, j_lo, R, lane);
        uint32_t bad = 0;
        if (j_lo == j_hi) {
            const uint32_t v = j_lo < R ? run_value<CV>(a.values, (uint32_t)j_lo, vlast) : miss;
            run_rows([&](auto K) { rt_insert<CV, decltype(K)::value>(res, v); });
            bad = j_lo < R ? 0u : 0xffffffffu;
        } else {
            // the lane's own first row: binary search inside [j_lo, j_hi]
            const uint64_t i0 = row0 + (uint64_t)lane * kRtVpl;
            uint64_t lo = j_lo, hi = j_hi;
            while (lo < hi) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if (ends.at((uint32_t)mid) <= i0)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            uint64_t j = lo, loaded = ~0ull;
            uint64_t e = j < R ? ends.at((uint32_t)j) : ~0ull;
            uint32_t v = miss;
            run_rows([&](auto K) {
                constexpr int k = decltype(K)::value;
                const uint64_t i = i0 + k;
                while (j < R && e <= i) { // zero-length runs and runs that end here: bounded by R
                    j++;
                    e = j < R ? ends.at((uint32_t)j) : ~0ull;
                }
                if (j < R && loaded != j) {
                    v = run_value<CV>(a.values, (uint32_t)j, vlast);
                    loaded = j;
                }
                rt_insert<CV, k>(res, j < R ? v : miss);
                bad |= j < R ? 0u : (1u << k);
            });
        }
        if (tile < nfull) {
            store_words_by<CV>(out_lane + tile * OUT_TILE, res, nts);
        } else {
            rt_store_tail<CV>(out_lane + tile * OUT_TILE, res, valid); // rows >= n reach neither a stored byte nor the counter
            bad &= tail_mask(valid, 0);
        }
        outside += (uint32_t)__builtin_popcount(bad);
    }
    if (a.uncovered) {
        const unsigned long long total = wave_sum64(outside);
        if (lane == 0 && total) __hip_atomic_fetch_add(a.uncovered, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

} // namespace mi355
