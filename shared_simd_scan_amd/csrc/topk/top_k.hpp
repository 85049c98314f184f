// topk/top_k.hpp -- the device code of mi355_top_k_dev: the k largest (or smallest) rows of a packed column as a bitmap, by a
// radix select over the packed values.  gfx950 only; part of libmi355scan.so through topk/top_k.hip.
//
// Keys.  A row's key is its value (largest) or the value's complement within C bits (smallest): the call always selects the
// LARGEST keys, one code path for both directions.  The key is split, most significant first, into D = ceil(C / 12) digits: the
// top digit takes C - 12 (D - 1) bits, every other one 12.
//
// Launches of a call, in stream order (no block ever waits for another):
//   D x  topk_hist_kernel<C>   the tile pipeline of histogram_kernel (extras/histogram.hpp), same mask handling and ragged tail:
//                              every qualifying row whose higher digits equal the prefix found so far adds 1 to one of <= 4096
//                              32-bit LDS counters; the block flushes its non-empty counters with agent-scope atomics into the
//                              pass's 64-bit counters in the workspace.  The block's loop is uniform over its four waves, so it
//                              can also flush every kTopkFlushRounds rounds: 2^31 rows at the most between two flushes, no
//                              LDS counter can overflow whatever n and the grid are.
//        topk_pick_kernel      one block: walks the pass's counters from the top, finds the bucket in which the running count
//                              reaches what is left of k, appends the digit to the prefix and subtracts what lay beyond it.  The
//                              first pick also takes q = the sum of the counters and m = min(k, q) (m == 0 raises `none`); the
//                              last one writes result_dev and leaves r = m - beyond, the number of ties to keep.
//   topk_emit_kernel<C>        one more pass over the column: the compare chains of the range / equality scans (decode_words),
//                              one for `key >= T` and one for `key == T`, with the bitmap store policy of the one-pass kernels;
//                              the qualifying rows equal to T (the ties) are counted per chunk of 16384 rows into chunk_counts
//                              (RowidArgs' layout, zeroed in front), one atomic per tile that holds any.  Which bits it writes
//                              is decided on the device (topk_ties_in): with at least half of the ties to keep, or in place,
//                              bit = mask AND (key >= T) and the trim takes the surplus ties away; with fewer, bit = mask AND
//                              (key > T) and the trim adds the r it keeps.  Either way the trim reads the column again only
//                              on the smaller side of the cut: a dictionary column has ties in every chunk, and k = 1 on it
//                              must not cost a second pass.  A lane reads its mask words before it stores the same words:
//                              bitmap == mask works in place (then the ties are always written first: taking them away needs
//                              no mask, adding them would need the one just overwritten).
//   rowid_scan_kernel          (kernels/bitmap.hpp) the counts' exclusive prefix inside groups of 1024 chunks, one total per group.
//   topk_trim_kernel<C>        a wave per chunk; `before` = the ties in front of the chunk, `count` its own.  Taking away: before +
//                              count <= r: done, nothing is read -- every chunk when the cut does not go through ties.  Adding:
//                              before >= r: done.  Otherwise the chunk's tiles are read again in row order; a tie is "v == T AND
//                              output bit" (taking away) or "v == T AND mask bit" (adding); its rank is before + the ties of the
//                              chunk's earlier tiles + the wave's exclusive prefix over the lanes' counts + its place in the
//                              lane; ties of rank >= r lose their bit, or those of rank < r get theirs.
// Workspace (the context's selection workspace, 64-bit words): nchunks chunk counts, the total's slot, one total per scan group
// (RowidArgs), kTopkStateWords of state, then D x 4096 counters.  All of it is zeroed by one memset in front of the first launch.
// LDS: the waves' tiles (4 x <= 16 KiB) and, in topk_hist_kernel, 16 KiB of counters.  The kernels test no switch bit.
#pragma once

#include "../kernels.hpp"
#include "../kernels/rt_column.hpp" // lane_valid_rows, store_words_by

namespace mi355 {

constexpr int kTopkDigitBits = 12;
constexpr int kTopkBuckets = 1 << kTopkDigitBits;
constexpr unsigned topk_passes(unsigned c) { return c >= 1 && c <= 32 ? (c + kTopkDigitBits - 1) / kTopkDigitBits : 0; }
// rounds of a block (4 tiles of <= 8192 rows each) between two flushes of its LDS counters: 2^31 rows at the most
constexpr uint32_t kTopkFlushRounds = 1u << 16;

// the state words behind the scan groups' totals
enum TopkState {
    kTopkPrefix = 0,    // the key's digits found so far, in place (after the last pick: the threshold's key)
    kTopkRemaining = 1, // what is left of k inside the prefix (after the last pick: r, the ties to keep)
    kTopkM = 2,         // min(k, q)
    kTopkBeyond = 3,    // qualifying rows whose key lies beyond the prefix
    kTopkNone = 4,      // m == 0
    kTopkTies = 5,      // qualifying rows equal to the threshold (after the last pick)
    kTopkStateWords = 8
};

struct TopkArgs {
    const uint8_t *packed; // n values of C bits, 16 B aligned
    uint64_t n;
    const uint8_t *mask;   // canonical, 4 B aligned, ceil(n / 8) bytes are read; null = every row
    uint8_t *bitmap;       // 4 B aligned; may be the mask
    unsigned long long *chunk_counts; // RowidArgs' layout
    uint64_t nchunks;
    unsigned long long *state; // kTopkStateWords words
    unsigned long long *hist;  // topk_hist_kernel: this pass's counters
    uint32_t flip;             // 0: largest; 2^C - 1: smallest
    uint32_t shift, dmask, himask; // topk_hist_kernel: the pass's digit is (key >> shift) & dmask; himask: the digits above it (pass 0: 0)
    uint32_t nts;              // bitmap stores: 0 plain, 1 non-temporal, 2 write-through
    uint32_t in_place;         // bitmap == mask
};

// Does topk_emit_kernel write the ties' bits (the trim then clears those of rank >= r), or leave them out (the trim then sets those
// of rank < r)?  The side on which the trim has less to read again; in place only the first works.  Both kernels ask the same state.
__device__ __forceinline__ bool topk_ties_in(const TopkArgs &a)
{
    const unsigned long long r = a.state[kTopkRemaining], ties = a.state[kTopkTies];
    return a.in_place || 2 * r >= ties;
}

struct TopkPickArgs {
    unsigned long long *hist;  // the pass's counters
    unsigned long long *state;
    uint64_t k;
    uint64_t *result;          // the caller's four words (written by the last pick)
    uint32_t nb, shift;        // counters of the pass; where its digit sits in the key
    uint32_t first, last;      // the call's first / last pick
    uint32_t flip;
};

template <int C> constexpr int topk_vpl() { return scan_vpl(C, kModeEq); }

// value K of the lane: one LDS atomic when its row qualifies and its higher digits are the prefix's
template <int C, int VPL, bool MASKED, int K = 0>
__device__ __forceinline__ void topk_count(const uint32_t (&w)[VPL * C / 32], const uint32_t (&m)[VPL / 32], uint32_t *hist, uint32_t flip,
                                           uint32_t shift, uint32_t dmask, uint32_t himask, uint32_t hival)
{
    const uint32_t key = extract<C, K, VPL * C / 32>(w) ^ flip;
    bool take = (key & himask) == hival;
    if constexpr (MASKED) take = take && ((m[K >> 5] >> (K & 31)) & 1u);
    if (take) __hip_atomic_fetch_add(&hist[(key >> shift) & dmask], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if constexpr (K + 1 < VPL) topk_count<C, VPL, MASKED, K + 1>(w, m, hist, flip, shift, dmask, himask, hival);
}

template <int C> __global__ __launch_bounds__(kBlockThreads) void topk_hist_kernel(TopkArgs a)
{
    constexpr int VPL = topk_vpl<C>();
    using G = ScanGeom<C, VPL>;
    constexpr int WORDS = G::WORDS;
    constexpr int AUX = 2; // the column is streamed: non-temporal DMA
    __shared__ __attribute__((aligned(16))) uint8_t lds[kWavesPerBlock][G::LDS_BYTES];
    __shared__ uint32_t hist[kTopkBuckets];
    const uint32_t nb = a.dmask + 1u;
    for (uint32_t k = threadIdx.x; k < nb; k += kBlockThreads) hist[k] = 0;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint8_t *lds_wave = lds[wave];
    const TileCtx<C, VPL> tc(a.n);
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock;
    const uint32_t flip = a.flip, shift = a.shift, dmask = a.dmask, himask = a.himask;
    const uint32_t hival = himask ? __builtin_amdgcn_readfirstlane((uint32_t)a.state[kTopkPrefix]) : 0u;

    // every thread of the block: the non-empty counters go to the pass's totals and are zero again
    auto flush = [&]() {
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < nb; k += kBlockThreads) {
            const uint32_t v = hist[k];
            if (v) {
                __hip_atomic_fetch_add(a.hist + k, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                hist[k] = 0;
            }
        }
        __syncthreads();
    };

    uint32_t mnext[WORDS];
#pragma unroll
    for (int j = 0; j < WORDS; j++) mnext[j] = 0xffffffffu;
    uint64_t base = (uint64_t)blockIdx.x * kWavesPerBlock; // the block's first tile of this round: the same in all four waves
    if (base + wave < tc.ntiles) {
        tc.template issue<AUX>(a.packed, base + wave, lds_wave, lane);
        if (a.mask) tc.load_bitmap_words(a.mask, base + wave, lane, mnext);
    }
    __syncthreads(); // the counters are zero
    uint32_t rounds = 0;
    for (; base < tc.ntiles; base += stride) {
        const uint64_t tile = base + wave;
        if (tile < tc.ntiles) {
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
                if (a.mask) tc.load_bitmap_words(a.mask, next, lane, mnext);
            }
            const bool full = tile < tc.nfull;
            if (!full) { // rows behind the column count for nothing
                const int valid = lane_valid_rows<VPL>(tc.n, tile, lane);
#pragma unroll
                for (int j = 0; j < WORDS; j++) m[j] &= tail_mask(valid, j);
            }
            if (!a.mask && full)
                topk_count<C, VPL, false>(w, m, hist, flip, shift, dmask, himask, hival);
            else
                topk_count<C, VPL, true>(w, m, hist, flip, shift, dmask, himask, hival);
        }
        if (++rounds == kTopkFlushRounds && base + stride < tc.ntiles) { // (block-uniform)
            flush();
            rounds = 0;
        }
    }
    flush();
}

// One block of 256 threads.  Thread t sums the `per` counters of rank [t per, (t + 1) per) from the top; thread 0 then walks the
// 256 sums and the counters of the one thread that holds the cut.
static __global__ __launch_bounds__(256) void topk_pick_kernel(TopkPickArgs a)
{
    __shared__ unsigned long long part[256];
    const uint32_t nb = a.nb, per = (nb + 255u) / 256u;
    unsigned long long sum = 0;
    for (uint32_t i = 0; i < per; i++) {
        const uint32_t j = threadIdx.x * per + i;
        if (j < nb) sum += a.hist[nb - 1u - j];
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned long long *const s = a.state;
    unsigned long long remaining = s[kTopkRemaining];
    bool none = s[kTopkNone] != 0;
    if (a.first) {
        unsigned long long q = 0;
        for (int t = 0; t < 256; t++) q += part[t];
        const unsigned long long m = a.k < q ? a.k : q;
        s[kTopkM] = m;
        remaining = m;
        none = m == 0;
        s[kTopkNone] = none ? 1ull : 0ull;
    }
    if (none) {
        s[kTopkRemaining] = 0;
        if (a.last) a.result[0] = a.result[1] = a.result[2] = a.result[3] = 0;
        return;
    }
    // the bucket of rank j from the top in which the running count reaches `remaining`
    unsigned long long cum = 0;
    uint32_t t = 0;
    while (t < 255u && cum + part[t] < remaining) cum += part[t++];
    uint32_t j = t * per < nb ? t * per : nb - 1u; // (inside the counters whatever they hold)
    unsigned long long cnt = a.hist[nb - 1u - j];
    while (cum + cnt < remaining && j + 1u < nb) {
        cum += cnt;
        cnt = a.hist[nb - 1u - ++j];
    }
    const unsigned long long prefix = s[kTopkPrefix] | ((unsigned long long)(nb - 1u - j) << a.shift);
    const unsigned long long beyond = s[kTopkBeyond] + cum;
    remaining -= cum;
    s[kTopkPrefix] = prefix;
    s[kTopkBeyond] = beyond;
    s[kTopkRemaining] = remaining;
    if (a.last) {
        s[kTopkTies] = cnt;
        a.result[0] = s[kTopkM];
        a.result[1] = (uint32_t)prefix ^ a.flip;
        a.result[2] = beyond;
        a.result[3] = cnt;
    }
}

// the ragged tile: only the lane's first `nbytes` bytes
template <int WORDS> __device__ __forceinline__ void topk_store_bytes(uint8_t *dst, const uint32_t (&v)[WORDS], int nbytes)
{
#pragma unroll
    for (int j = 0; j < WORDS; j++)
#pragma unroll
        for (int b = 0; b < 4; b++)
            if (4 * j + b < nbytes) dst[4 * j + b] = (uint8_t)(v[j] >> (8 * b));
}

template <int C> __global__ __launch_bounds__(kBlockThreads) void topk_emit_kernel(TopkArgs a)
{
    constexpr int VPL = topk_vpl<C>();
    using G = ScanGeom<C, VPL>;
    constexpr int WORDS = G::WORDS;
    constexpr int AUX = 2;
    constexpr uint32_t VMAX = C == 32 ? 0xffffffffu : ((1u << (C & 31)) - 1u);
    __shared__ __attribute__((aligned(16))) uint8_t lds[kWavesPerBlock][G::LDS_BYTES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint8_t *lds_wave = lds[wave];
    const TileCtx<C, VPL> tc(a.n);
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock;
    uint64_t tile = (uint64_t)blockIdx.x * kWavesPerBlock + wave;
    // the threshold as a value; beyond-or-equal as an inclusive range of values: [T, 2^C - 1] (largest) or [0, T] (smallest)
    const uint32_t T = __builtin_amdgcn_readfirstlane((uint32_t)a.state[kTopkPrefix] ^ a.flip);
    const uint32_t keep = __builtin_amdgcn_readfirstlane((uint32_t)a.state[kTopkNone]) ? 0u : 0xffffffffu;
    const uint32_t tie_bits = __builtin_amdgcn_readfirstlane(topk_ties_in(a) ? 0xffffffffu : 0u);
    const uint32_t lo = a.flip ? 0u : T, span = a.flip ? T : VMAX - T;
    const uint32_t range_key[kMaxKeysPerPass] = {lo, span, 0, 0, 0, 0, 0, 0}, eq_key[kMaxKeysPerPass] = {T, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t nts = a.nts;

    uint32_t mnext[WORDS];
#pragma unroll
    for (int j = 0; j < WORDS; j++) mnext[j] = 0xffffffffu;
    if (tile < tc.ntiles) {
        tc.template issue<AUX>(a.packed, tile, lds_wave, lane);
        if (a.mask) tc.load_bitmap_words(a.mask, tile, lane, mnext);
    }
    while (tile < tc.ntiles) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the tile has landed, and the lane's mask words of it
        uint32_t w[G::LANE_DWORDS];
        read_lane_data<C, VPL>(lds_wave, lane, w);
        uint32_t m[WORDS];
#pragma unroll
        for (int j = 0; j < WORDS; j++) m[j] = mnext[j];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const uint64_t next = tile + stride;
        if (next < tc.ntiles) {
            tc.template issue<AUX>(a.packed, next, lds_wave, lane);
            if (a.mask) tc.load_bitmap_words(a.mask, next, lane, mnext);
        }
        uint32_t ge[1][WORDS], eq[1][WORDS];
        decode_words<C, VPL, 0, 1, kModeRange, G::LANE_DWORDS>(w, ge, range_key);
        decode_words<C, VPL, 0, 1, kModeEq, G::LANE_DWORDS>(w, eq, eq_key);
        const bool full = tile < tc.nfull;
        const int valid = full ? VPL : lane_valid_rows<VPL>(tc.n, tile, lane);
        uint32_t out[WORDS];
        uint32_t ties = 0;
#pragma unroll
        for (int j = 0; j < WORDS; j++) {
            uint32_t q = m[j] & keep; // the qualifying rows
            if (!full) q &= tail_mask(valid, j);
            out[j] = ge[0][j] & (~eq[0][j] | tie_bits) & q;
            ties += __builtin_popcount(eq[0][j] & q);
        }
        uint8_t *const dst = a.bitmap + tile * G::BITMAP_BYTES + (uint64_t)lane * (WORDS * 4);
        if (full) {
            store_words_by<WORDS>(dst, out, nts);
        } else {
            topk_store_bytes<WORDS>(dst, out, (valid + 7) / 8);
        }
        ties = wave_sum(ties);
        if (lane == 0 && ties)
            __hip_atomic_fetch_add(a.chunk_counts + tile * G::TILE_VALUES / (kRowidChunk * 8), (unsigned long long)ties, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        tile = next;
    }
}

template <int C> __global__ __launch_bounds__(kBlockThreads) void topk_trim_kernel(TopkArgs a)
{
    constexpr int VPL = topk_vpl<C>();
    using G = ScanGeom<C, VPL>;
    constexpr int WORDS = G::WORDS;
    constexpr int TILES = kRowidChunk * 8 / G::TILE_VALUES; // tiles per chunk
    __shared__ __attribute__((aligned(16))) uint8_t lds[kWavesPerBlock][G::LDS_BYTES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint8_t *lds_wave = lds[wave];
    const TileCtx<C, VPL> tc(a.n);
    const unsigned long long r = uniform64(a.state[kTopkRemaining]);
    const bool add = __builtin_amdgcn_readfirstlane(topk_ties_in(a) ? 0 : 1) != 0; // the ties' bits are not there yet
    const uint32_t T = __builtin_amdgcn_readfirstlane((uint32_t)a.state[kTopkPrefix] ^ a.flip);
    const uint32_t eq_key[kMaxKeysPerPass] = {T, 0, 0, 0, 0, 0, 0, 0};
    const ChunkPrefix ties{a.chunk_counts, a.nchunks};
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock;

    for (uint64_t ch = (uint64_t)blockIdx.x * kWavesPerBlock + wave; ch < a.nchunks; ch += stride) {
        const auto [before, count] = chunk_span_wave(ties, ch, lane); // the ties in front of this chunk, and its own
        // every tie of the chunk has the bit it should have: nothing of it is read
        if (count == 0 || (add ? before >= r : before + count <= r)) continue;

        uint32_t base = 0; // ties in the chunk's earlier tiles
        for (int t = 0; t < TILES; t++) {
            const uint64_t tile = ch * TILES + t;
            if (tile >= tc.ntiles) break;
            tc.template issue<0>(a.packed, tile, lds_wave, lane);
            uint32_t o[WORDS], q[WORDS]; // the output's words; where a tie may be: in the output, or (adding) among the qualifying rows
            tc.load_bitmap_words(a.bitmap, tile, lane, o);
            if (add) {
                const int valid = lane_valid_rows<VPL>(tc.n, tile, lane);
#pragma unroll
                for (int j = 0; j < WORDS; j++) q[j] = 0xffffffffu;
                if (a.mask) tc.load_bitmap_words(a.mask, tile, lane, q);
#pragma unroll
                for (int j = 0; j < WORDS; j++) q[j] &= tail_mask(valid, j);
            } else {
#pragma unroll
                for (int j = 0; j < WORDS; j++) q[j] = o[j];
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            uint32_t w[G::LANE_DWORDS];
            read_lane_data<C, VPL>(lds_wave, lane, w);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // read before the next tile's DMA overwrites it
            uint32_t eq[1][WORDS];
            decode_words<C, VPL, 0, 1, kModeEq, G::LANE_DWORDS>(w, eq, eq_key);
            uint32_t e[WORDS];
            uint32_t cnt = 0;
#pragma unroll
            for (int j = 0; j < WORDS; j++) {
                e[j] = eq[0][j] & q[j];
                cnt += __builtin_popcount(e[j]);
            }
            const uint32_t incl = wave_inclusive_scan(cnt);
            const uint32_t in_tile = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            const unsigned long long rank0 = before + base + (incl - cnt); // rank of the lane's first tie
            uint32_t allowed = rank0 >= r ? 0u : (r - rank0 < cnt ? (uint32_t)(r - rank0) : cnt);
            if (add ? allowed > 0 : allowed < cnt) {
                const bool full = tile < tc.nfull;
                const int nbytes = (lane_valid_rows<VPL>(tc.n, tile, lane) + 7) / 8;
                uint8_t *const dst = a.bitmap + tile * G::BITMAP_BYTES + (uint64_t)lane * (WORDS * 4);
#pragma unroll
                for (int j = 0; j < WORDS; j++) {
                    const uint32_t pc = __builtin_popcount(e[j]);
                    const uint32_t take = allowed < pc ? allowed : pc; // the word's lowest `take` ties are kept
                    allowed -= take;
                    uint32_t x = take == pc ? 0u : e[j];                // ... and x, the others, are not
                    if (x)
                        for (uint32_t i = take; i; i--) x &= x - 1u;
                    const uint32_t v = add ? (o[j] | (e[j] & ~x)) : (o[j] & ~x);
                    if (v == o[j]) continue;
                    if (full) {
                        ((uint32_t *)dst)[j] = v;
                    } else {
#pragma unroll
                        for (int b = 0; b < 4; b++)
                            if (4 * j + b < nbytes) dst[4 * j + b] = (uint8_t)(v >> (8 * b));
                    }
                }
            }
            base += in_tile;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
}

} // namespace mi355
