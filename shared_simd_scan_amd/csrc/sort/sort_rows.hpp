// sort/sort_rows.hpp -- the device code of mi355_sort_rows_dev: the row ids of a packed column's qualifying rows in value order
// (ascending or descending, then by row id: a stable sort), optionally with the values in that order.  gfx950 only; part of
// libmi355scan.so through sort/sort_rows.hip.
//
// Keys.  A row's key is its value (ascending) or the value's complement within c bits (descending: top_k's `flip`), sorted
// ascending by a stable least-significant-digit radix sort.  D = ceil(c / 8) digits of 8 bits, the top one takes c - 8 (D - 1) bits
// and has only 2^that many buckets (the second pass of a 9-bit column has two).
//
// Spans.  The input of a pass is cut into spans of kSortSpan = 16384 rows (8 tiles of kRtTileRows), whatever the grid: a wave owns
// a span at a time, blocks stride over the spans.  Pass 0 reads the packed column and the mask, the later passes the items the
// pass before wrote -- 64 bits each, the key above the row's 32-bit index inside the view.
//
// Launches of a pass, in stream order (no block ever waits for another):
//   sort_count_kernel / sort_item_count_kernel      the wave counts the span's qualifying rows per digit value in 256 LDS words of
//                              its own and leaves them at counts[digit * nspans + span]: every counter of the pass is written, so
//                              nothing needs zeroing, and no atomic reaches memory.
//   rowid_scan_kernel          (kernels/bitmap.hpp) the exclusive prefix of the nb * nspans counters, digit-major, inside groups of
//                              1024, and one total per group.
//   sort_offsets_kernel        one block: the group totals become their own exclusive prefix, so that a counter's rank is
//                              group_prefix[i / 1024] + counts[i] -- two loads, not a sum over the groups in front (a 2.5e8-row
//                              column has 3815 of them in front of its last counter); the grand total of pass 0 is q and goes to
//                              count_dev and to the state word the later kernels test.
//   sort_scatter_kernel / sort_item_scatter_kernel   the same walk.  A row's place is the rank of (its digit, its span) + the rows of
//                              the same digit in front of it in the span (through an LDS stage: below).  The last pass writes first_row + row to rowids (and
//                              the value to values), the others write items.  With q > capacity every scatter and every later
//                              count returns at once: nothing is written.
//
// Order inside a span.  The tile is decoded TRANSPOSED: in step j = 0 .. 31 lane l takes row 64 j + l of the tile, at bit
// (64 j + l) c of the LDS image (two dwords at a per-lane offset and v_alignbit: columns_lds_value with a vector offset), so the
// 64 rows of a step are consecutive, their mask bits are one 64-bit word (two v_readlane of the tile's mask dwords), and lane
// order is row order.  sort_rank: one ballot per digit bit gives every lane the set of lanes with its digit; rank = the digit's
// running offset (256 LDS words per wave) + the lanes of the set below this one; the set's highest lane adds the set's size to
// the offset.  LDS operations of a wave execute in order, so the next step reads what this one wrote.  The item passes take item
// 64 j + l of the span in step j (coalesced as it lies) and share sort_rank.
//
// The stage.  Ranked straight into the pass's output, the 64 rows of a step leave for up to 64 places per store instruction, and a
// pass costs what its buckets cost, not what its bytes cost (measured: profiles/r16_sort_rows.txt and DESIGN.md 3.14).  So a
// scatter ranks kSortStageRows = 2048 rows at a time inside LDS first: one sweep counts the rows per digit (the count kernels'
// loop), sort_stage_prefix turns the counts into every digit's first place in the stage, a second sweep ranks the rows into the
// stage with sort_rank -- 16-bit row indices in the column kernel, which decodes the key again on the way out, whole items in the
// item kernel --, and the copy-out writes entry i of the stage to offset[digit] + (i - first place of the digit): a digit's rows
// of the stage leave side by side.  Where that cannot pay -- a pass of at most 8 buckets, a tile with fewer than 1024 qualifying
// rows (sort_stage_pays) -- the rows go straight to their places as described above.  Either way a row's place is the same.
//
// LDS: a wave of the two column kernels has two images of rt_image(c) bytes (the next tile is on its way while this one is
// ranked) and 16 bytes behind them for the dword the last row's funnel shift reads; then 256 counters (count: 7.0 KiB per wave at
// c = 9, 17.0 KiB at c = 32) or the stage's 768 words and 2048 16-bit entries (scatter: 13.0 KiB / 23.0 KiB); dynamic, sized to the
// width.  sort_item_count_kernel has its counters only (1 KiB per wave, static), sort_item_scatter_kernel the stage's words and
// 2048 items (19 KiB per wave, dynamic).  The kernels test no switch bit.
#pragma once

#include "../kernels.hpp"
#include "../kernels/rt_column.hpp" // rt_issue_tile, lane_valid_rows, the tile geometry

namespace mi355 {

constexpr int kSortDigitBits = 8;
constexpr int kSortBuckets = 1 << kSortDigitBits;
constexpr int kSortSpan = 16384;                          // rows (pass 0) or items (later passes) a wave ranks at a time
constexpr int kSortSpanTiles = kSortSpan / kRtTileRows;   // 8
constexpr int kSortStateWords = 8;                        // [0] = q, the number of qualifying rows
static_assert(kSortSpan % kRtTileRows == 0, "a span is whole tiles");
constexpr unsigned sort_passes(unsigned c) { return c >= 1 && c <= 32 ? (c + kSortDigitBits - 1) / kSortDigitBits : 0; }
// buckets of the pass that needs the most: 2^c at a one-pass width, else 256
constexpr uint32_t sort_max_buckets(unsigned c) { return c < (unsigned)kSortDigitBits ? 1u << c : (uint32_t)kSortBuckets; }
constexpr uint64_t sort_spans(uint64_t rows) { return (rows + kSortSpan - 1) / kSortSpan; }
// a scatter's stage: a wave ranks kSortStageRows rows at a time inside LDS and copies them out in digit order
constexpr int kSortStageRows = kRtTileRows;
// the words of a wave in front of a stage: the digits' offsets in the pass's output, their first places in the stage, their cursors
constexpr uint32_t kSortStageWords = 3u * kSortBuckets;
// a wave's LDS in the column kernels: two images, the funnel shift's last dword, then the counters (count) or the stage's words and
// a stage of 16-bit row indices (scatter)
constexpr uint32_t sort_wave_lds(uint32_t c, bool scatter)
{
    return 2u * rt_image(c) + 16u + (scatter ? 4u * kSortStageWords + 2u * kSortStageRows : 4u * kSortBuckets);
}
constexpr uint32_t sort_lds(uint32_t c, bool scatter) { return kWavesPerBlock * sort_wave_lds(c, scatter); }
// ... and in sort_item_scatter_kernel: the stage's words and a stage of 64-bit items
constexpr uint32_t kSortItemWaveLds = 4u * kSortStageWords + 8u * kSortStageRows;
constexpr uint32_t kSortItemLds = kWavesPerBlock * kSortItemWaveLds;
static_assert(sort_lds(32, true) <= kCuLdsBytes && kSortItemLds <= kCuLdsBytes, "LDS budget");

struct SortArgs {
    const uint8_t *packed;  // n values of c bits, 16 B aligned (pass 0)
    uint64_t n;
    const uint8_t *mask;    // 4 B aligned, ceil(n / 8) bytes are read; null = every row (pass 0)
    const unsigned long long *items_in; // later passes: q items
    unsigned long long *items_out;      // every pass but the last
    unsigned long long *counts;         // the pass's nb * nspans counters, RowidArgs' layout behind them
    uint64_t nspans;
    unsigned long long *state;          // kSortStateWords words
    uint64_t capacity;
    uint64_t first_row;
    uint64_t *rowids;       // the last pass
    uint32_t *values;       // the last pass; may be null
    uint64_t *count_out;    // sort_offsets_kernel of pass 0: the caller's count word
    uint32_t c, flip;       // flip: 0 ascending, 2^c - 1 descending
    uint32_t shift, dbits;  // the pass's digit is (key >> shift), dbits wide: nb = 2^dbits buckets
    uint32_t last;          // the call's last pass
};

// where counter i's rows begin: the prefix of its scan group (sort_offsets_kernel) + its prefix inside the group
__device__ __forceinline__ uint32_t sort_rank_of(const unsigned long long *counts, uint64_t ncounters, uint64_t i)
{
    return (uint32_t)(counts[ncounters + 1 + i / kRowidScanGroup] + counts[i]); // a rank is below q <= 2^32; an empty bucket's may wrap
}

// the wave's 256 offsets of a span: the ranks of (digit, span), lane l those of digits l, l + 64, ...
__device__ __forceinline__ void sort_load_offsets(const SortArgs &a, uint32_t *off, uint64_t span, int lane)
{
    const uint32_t nb = 1u << a.dbits;
    const uint64_t ncounters = (uint64_t)nb * a.nspans;
#pragma unroll
    for (int k = 0; k < kSortBuckets / 64; k++) {
        const uint32_t d = (uint32_t)lane + 64u * k;
        if (d < nb) off[d] = sort_rank_of(a.counts, ncounters, (uint64_t)d * a.nspans + span);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// the wave's 256 counters of a span go to the pass's and are zero again
__device__ __forceinline__ void sort_store_counts(const SortArgs &a, uint32_t *hist, uint64_t span, int lane)
{
    const uint32_t nb = 1u << a.dbits;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the wave's LDS atomics are done (LDS is in order per wave)
#pragma unroll
    for (int k = 0; k < kSortBuckets / 64; k++) {
        const uint32_t d = (uint32_t)lane + 64u * k;
        if (d < nb) {
            a.counts[(uint64_t)d * a.nspans + span] = hist[d];
            hist[d] = 0;
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// One step of 64 consecutive rows, lane order = row order: the place of the lane's row (digit d, `take`: it qualifies) among
// the pass's output.  Wave-uniform control flow; every lane calls it.
__device__ __forceinline__ uint32_t sort_rank(uint32_t *off, uint32_t d, bool take, uint32_t dbits, int lane)
{
    unsigned long long peers = __builtin_amdgcn_ballot_w64(take);
    for (uint32_t b = 0; b < dbits; b++) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long has = __builtin_amdgcn_ballot_w64(bit);
        peers &= bit ? has : ~has;
    }
    const uint32_t below = (uint32_t)__builtin_popcountll(peers & ((1ull << lane) - 1ull));
    uint32_t pos = 0;
    if (take) pos = off[d] + below;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // every lane has read its digit's offset before the set's highest lane moves it
    if (take && (peers >> lane) == 1ull) off[d] = pos + 1u;
    asm volatile("" ::: "memory");
    return pos;
}

// Does a stage pay?  (wave-uniform)  A pass of few buckets scatters into few places as it is -- the second pass of a 9-bit column
// has two --, and a stage of few rows holds runs of one: below 2^4 buckets, or below half a stage of rows (4 rows per digit of 256
// on uniform values), every row goes straight to its place.  Both thresholds are set by that reasoning, not by a sweep.
constexpr uint32_t kSortDirectBits = 3;
constexpr uint32_t kSortStageMinRows = kSortStageRows / 2;
__device__ __forceinline__ bool sort_stage_pays(uint32_t dbits, uint32_t rows) { return dbits > kSortDirectBits && rows >= kSortStageMinRows; }

// The stage's words of a wave.  Between two stages every cursor is zero; a stage's first sweep counts its rows per digit into them.
struct SortStage {
    uint32_t *off, *start, *cursor; // 256 words each
    __device__ __forceinline__ explicit SortStage(uint32_t *words) : off(words), start(words + kSortBuckets), cursor(words + 2 * kSortBuckets) {}
};

// The cursors hold the stage's rows per digit: their exclusive prefix becomes every digit's first place in the stage (start, and
// the cursor sort_rank moves); -> the stage's rows.  Lane l has digits 4 l .. 4 l + 3.
__device__ __forceinline__ uint32_t sort_stage_prefix(const SortStage &st, int lane)
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the wave's LDS atomics are done (LDS is in order per wave)
    uint32_t h[4];
#pragma unroll
    for (int k = 0; k < 4; k++) h[k] = st.cursor[4 * lane + k];
    const uint32_t mine = h[0] + h[1] + h[2] + h[3];
    const uint32_t incl = wave_inclusive_scan(mine);
    uint32_t run = incl - mine;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        st.start[4 * lane + k] = run;
        st.cursor[4 * lane + k] = run;
        run += h[k];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    return (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
}

// the stage has left: every digit's offset moves on by its rows, the cursors are zero again
__device__ __forceinline__ void sort_stage_done(const SortStage &st, int lane)
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the copy-out has read its offsets
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int d = 4 * lane + k;
        st.off[d] += st.cursor[d] - st.start[d];
        st.cursor[d] = 0;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

__device__ __forceinline__ void sort_emit(const SortArgs &a, uint32_t pos, uint32_t key, uint32_t row)
{
    if (a.last) {
        a.rowids[pos] = a.first_row + row;
        if (a.values) a.values[pos] = key ^ a.flip;
    } else {
        a.items_out[pos] = ((unsigned long long)key << 32) | row;
    }
}

// ---- pass 0: the packed column and the mask ----
template <bool SCATTER> __device__ __forceinline__ void sort_column_pass(const SortArgs &a)
{
    constexpr int AUX = 2; // the column is streamed: non-temporal DMA
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t c = a.c, image = rt_image(c), tile_bytes = rt_tile_bytes(c), vmask = rt_vmask(c);
    uint8_t *cur = mi355_dyn_lds + (uint32_t)wave * sort_wave_lds(c, SCATTER);
    uint8_t *nxt = cur + image;
    uint32_t *const words = (uint32_t *)(cur + 2u * image + 16u); // the wave's counters (count), or the stage's words and the stage
    const SortStage st(words);
    uint16_t *const stage = (uint16_t *)(words + kSortStageWords);
    const uint64_t n = a.n, ntiles = rt_ntiles(n), data_bytes = (n * c + 7) / 8, mask_bytes = (n + 7) / 8;
    const uint64_t nspans = a.nspans, stride = (uint64_t)gridDim.x * kWavesPerBlock;
    const uint32_t shift = a.shift, dbits = a.dbits, dmask = (1u << dbits) - 1u, flip = a.flip;
    uint32_t *const tally = SCATTER ? st.cursor : words; // where a sweep counts its rows per digit
    if constexpr (SCATTER) {
        if (uniform64(a.state[0]) > a.capacity) return; // all or nothing
    }
#pragma unroll
    for (int k = 0; k < kSortBuckets / 64; k++) tally[lane + 64 * k] = 0;
    uint64_t span = (uint64_t)blockIdx.x * kWavesPerBlock + wave;
    if (span >= nspans) return;
    uint64_t tile = span * kSortSpanTiles; // (< ntiles: a span holds a row)

    // the lane's mask dword of tile t: rows 32 lane .. 32 lane + 31 of it (ragged end: only the bytes the bitmap is guaranteed to hold)
    auto load_mask = [&](uint64_t t) -> uint32_t {
        return a.mask ? bitmap_word_at(a.mask, mask_bytes, t * (kRtTileRows / 8) + (uint64_t)lane * 4) : 0xffffffffu;
    };
    // the key of row r of the tile in `cur`: two dwords at a per-lane offset and a funnel shift
    auto key_of = [&](uint32_t r) -> uint32_t {
        const uint32_t bit = r * c;
        const uint32_t *p = (const uint32_t *)(cur + (bit >> 5) * 4);
        return (__builtin_amdgcn_alignbit(p[1], p[0], bit & 31u) & vmask) ^ flip;
    };
    rt_issue_tile<AUX>(a.packed, data_bytes, tile_bytes, tile, cur, lane);
    uint32_t mnext = load_mask(tile);
    while (true) {
        // what follows this tile in the wave's walk: the span's next tile, or the first one of the wave's next span
        uint64_t nspan = span, ntile = tile + 1;
        if (ntile == (span + 1) * kSortSpanTiles || ntile >= ntiles) {
            nspan = span + stride;
            ntile = nspan * kSortSpanTiles;
        }
        const bool more = nspan < nspans;
        if constexpr (SCATTER) {
            if (tile == span * kSortSpanTiles) sort_load_offsets(a, st.off, span, lane);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the tile has landed, and the lane's mask dword of it
        const uint32_t m = mnext;
        if (more) {
            rt_issue_tile<AUX>(a.packed, data_bytes, tile_bytes, ntile, nxt, lane);
            mnext = load_mask(ntile);
        }
        // one sweep over the tile's 32 steps: f(row in the tile, its key's digit, whether it qualifies), wave-uniform control flow
        auto sweep = [&](auto f) {
#pragma unroll 2
            for (int j = 0; j < kRtVpl; j++) {
                const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)m, 2 * j), hi = (uint32_t)__builtin_amdgcn_readlane((int)m, 2 * j + 1);
                if ((lo | hi) == 0) continue; // (wave-uniform) no row of the step qualifies
                const uint32_t in_tile = 64u * j + lane;
                const uint32_t d = (key_of(in_tile) >> shift) & dmask;
                const uint32_t word = lane < 32 ? lo : hi;
                // rows behind the column count for nothing: lane_valid_rows over steps of 64 x 1 rows
                const bool take = ((word >> (lane & 31)) & 1u) && lane_valid_rows<1>(n, tile * kRtVpl + j, lane) != 0;
                f(in_tile, d, take);
            }
        };
        bool staged = false;
        if constexpr (SCATTER) staged = sort_stage_pays(dbits, wave_sum((uint32_t)__builtin_popcount(m)));
        if (__builtin_amdgcn_ballot_w64(m != 0) == 0) {
            // no row of the tile qualifies
        } else if (SCATTER && !staged) {
            // few buckets or few rows: every row straight to its place
            sweep([&](uint32_t in_tile, uint32_t d, bool take) {
                const uint32_t pos = sort_rank(st.off, d, take, dbits, lane);
                if (take) sort_emit(a, pos, key_of(in_tile), (uint32_t)(tile * kRtTileRows) + in_tile);
            });
        } else {
            sweep([&](uint32_t, uint32_t d, bool take) {
                if (take) __hip_atomic_fetch_add(&tally[d], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            });
            if constexpr (SCATTER) {
                // the tile's rows into the stage in digit order, then out: a digit's rows of the tile leave side by side
                const uint32_t total = sort_stage_prefix(st, lane);
                sweep([&](uint32_t in_tile, uint32_t d, bool take) {
                    const uint32_t at = sort_rank(st.cursor, d, take, dbits, lane);
                    if (take) stage[at] = (uint16_t)in_tile;
                });
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                for (uint32_t i = lane; i < total; i += 64) {
                    const uint32_t r = stage[i];
                    const uint32_t key = key_of(r);
                    const uint32_t d = (key >> shift) & dmask;
                    sort_emit(a, st.off[d] + (i - st.start[d]), key, (uint32_t)(tile * kRtTileRows) + r);
                }
                sort_stage_done(st, lane);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the image is read before a later tile's DMA overwrites it
        if constexpr (!SCATTER) {
            if (nspan != span) sort_store_counts(a, tally, span, lane);
        }
        if (!more) break;
        uint8_t *const t = cur;
        cur = nxt, nxt = t;
        tile = ntile, span = nspan;
    }
}

static __global__ __launch_bounds__(kBlockThreads) void sort_count_kernel(SortArgs a) { sort_column_pass<false>(a); }
static __global__ __launch_bounds__(kBlockThreads) void sort_scatter_kernel(SortArgs a) { sort_column_pass<true>(a); }

// ---- later passes: the items of the pass before ----
constexpr int kSortItemBatch = 8; // steps whose loads are in flight together

// steps [j0, j0 + steps) of the span that begins at item `first`: f(the lane's item, whether it exists)
template <typename F>
__device__ __forceinline__ void sort_item_sweep(const SortArgs &a, unsigned long long q, uint64_t first, uint32_t j0, uint32_t steps, int lane, F f)
{
    for (uint32_t j1 = j0; j1 < j0 + steps && first + 64ull * j1 < q; j1 += kSortItemBatch) {
        unsigned long long it[kSortItemBatch];
#pragma unroll
        for (int j = 0; j < kSortItemBatch; j++) {
            const uint64_t i = first + 64ull * (j1 + j) + lane;
            it[j] = i < q ? a.items_in[i] : 0ull;
        }
#pragma unroll
        for (int j = 0; j < kSortItemBatch; j++) f(it[j], first + 64ull * (j1 + j) + lane < q);
    }
}

static __global__ __launch_bounds__(kBlockThreads) void sort_item_count_kernel(SortArgs a)
{
    __shared__ uint32_t tallies[kWavesPerBlock][kSortBuckets];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t *const tally = tallies[wave];
    const unsigned long long q = uniform64(a.state[0]);
    if (q > a.capacity) return; // all or nothing: the scatter in front wrote no item
    const uint64_t nspans = a.nspans, stride = (uint64_t)gridDim.x * kWavesPerBlock;
    const uint32_t shift = a.shift, dmask = (1u << a.dbits) - 1u;
#pragma unroll
    for (int k = 0; k < kSortBuckets / 64; k++) tally[lane + 64 * k] = 0;
    for (uint64_t span = (uint64_t)blockIdx.x * kWavesPerBlock + wave; span < nspans; span += stride) {
        sort_item_sweep(a, q, span * kSortSpan, 0, kSortSpan / 64, lane, [&](unsigned long long item, bool take) {
            if (take) __hip_atomic_fetch_add(&tally[((uint32_t)(item >> 32) >> shift) & dmask], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        });
        sort_store_counts(a, tally, span, lane); // (an empty span: zeros)
    }
}

static __global__ __launch_bounds__(kBlockThreads) void sort_item_scatter_kernel(SortArgs a)
{
    constexpr uint32_t STEPS = kSortStageRows / 64; // steps of a stage
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t *const words = (uint32_t *)(mi355_dyn_lds + (uint32_t)wave * kSortItemWaveLds);
    const SortStage st(words);
    unsigned long long *const stage = (unsigned long long *)(words + kSortStageWords);
    const unsigned long long q = uniform64(a.state[0]);
    if (q > a.capacity) return;
    const uint64_t nspans = a.nspans, stride = (uint64_t)gridDim.x * kWavesPerBlock;
    const uint32_t shift = a.shift, dbits = a.dbits, dmask = (1u << dbits) - 1u;
#pragma unroll
    for (int k = 0; k < kSortBuckets / 64; k++) st.cursor[lane + 64 * k] = 0;
    for (uint64_t span = (uint64_t)blockIdx.x * kWavesPerBlock + wave; span < nspans; span += stride) {
        const uint64_t first = span * kSortSpan;
        if (first >= q) break; // (the spans behind are empty too)
        sort_load_offsets(a, st.off, span, lane);
        for (uint32_t j0 = 0; j0 < kSortSpan / 64 && first + 64ull * j0 < q; j0 += STEPS) {
            const unsigned long long left = q - (first + 64ull * j0);
            if (!sort_stage_pays(dbits, left < kSortStageRows ? (uint32_t)left : (uint32_t)kSortStageRows)) {
                // few buckets or few items: every item straight to its place
                sort_item_sweep(a, q, first, j0, STEPS, lane, [&](unsigned long long item, bool take) {
                    const uint32_t key = (uint32_t)(item >> 32);
                    const uint32_t pos = sort_rank(st.off, (key >> shift) & dmask, take, dbits, lane);
                    if (take) sort_emit(a, pos, key, (uint32_t)item);
                });
                continue;
            }
            sort_item_sweep(a, q, first, j0, STEPS, lane, [&](unsigned long long item, bool take) {
                if (take) __hip_atomic_fetch_add(&st.cursor[((uint32_t)(item >> 32) >> shift) & dmask], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            });
            // the items into the stage in digit order (read a second time: they are in the cache), then out
            const uint32_t total = sort_stage_prefix(st, lane);
            sort_item_sweep(a, q, first, j0, STEPS, lane, [&](unsigned long long item, bool take) {
                const uint32_t at = sort_rank(st.cursor, ((uint32_t)(item >> 32) >> shift) & dmask, take, dbits, lane);
                if (take) stage[at] = item;
            });
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            for (uint32_t i = lane; i < total; i += 64) {
                const unsigned long long item = stage[i];
                const uint32_t key = (uint32_t)(item >> 32);
                const uint32_t d = (key >> shift) & dmask;
                sort_emit(a, st.off[d] + (i - st.start[d]), key, (uint32_t)item);
            }
            sort_stage_done(st, lane);
        }
    }
}

// One block of 256 threads behind rowid_scan_kernel: the scan groups' totals become their exclusive prefix in place, the grand total
// goes behind the counters (ChunkPrefix::total) and, in pass 0 (count_out set), to the caller's count word and the state.
static __global__ __launch_bounds__(256) void sort_offsets_kernel(SortArgs a)
{
    __shared__ unsigned long long part[256];
    const uint64_t ncounters = (uint64_t)(1u << a.dbits) * a.nspans;
    const ChunkPrefix prefix{a.counts, ncounters};
    unsigned long long *const totals = prefix.group_totals();
    const uint64_t ngroups = prefix.ngroups(), per = (ngroups + 255) / 256;
    const uint64_t lo = threadIdx.x * per < ngroups ? threadIdx.x * per : ngroups, hi = lo + per < ngroups ? lo + per : ngroups;
    unsigned long long sum = 0;
    for (uint64_t i = lo; i < hi; i++) sum += totals[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    unsigned long long run = 0;
    for (uint32_t t = 0; t < threadIdx.x; t++) run += part[t];
    for (uint64_t i = lo; i < hi; i++) {
        const unsigned long long v = totals[i];
        totals[i] = run;
        run += v;
    }
    if (threadIdx.x == 255) { // run: everything
        *prefix.total() = run;
        if (a.count_out) {
            a.count_out[0] = run;
            a.state[0] = run;
        }
    }
}

} // namespace mi355
