// runagg/run_aggregate.hpp -- the device code of mi355_run_aggregate_dev: sum / count / min / max of a packed column per RUN of a
// table of run ends (the row behind a run's last row, as mi355_run_encode_dev leaves them): the aggregates of a sort-based GROUP BY
// and of run-length-coded data.  gfx950 only; part of libmi355scan.so through runagg/run_aggregate.hip.
//
// j(i) = the number of j < R with end_j <= i, as in run_decode_kernel (runs/runs.hpp), whose table machinery this uses unchanged:
// RunEnds, run_entry, run_search_wave.  Groups are contiguous, so a wave needs no hash front and almost no atomics.
//
// Tile stream.  The run-time-width stream of kernels/rt_column.hpp: a wave owns a chunk of 8 consecutive tiles of 64 x 32 rows
// (16384 rows, run_count_kernel's geometry) and then the chunk `waves` further on; two LDS images alternate, the mask dword of a
// lane's 32 rows is loaded one tile ahead; rows >= n are masked off, so what lies behind the column reaches nothing.
//
// Which runs a tile touches.  j_lo = j(first row): the 64-way search, started from the tile before -- and skipped while the end
// read for that tile's run still lies behind this tile's first row.  j_hi = j(last row) is searched only when run j_lo ends inside
// the tile.
//   one run (j_lo == j_hi)   lanes reduce their rows in registers, one wave reduction (DPP), the result joins the CARRY: the open
//                            run's partial, kept by the wave from tile to tile.  No table read.
//   span tier                j_hi - j_lo + 1 <= S (run_agg_span_slots): a lane binary-searches [j_lo, j_hi] for its first row and
//                            walks its 32 rows as the decoder does, accumulating per run in registers; a (lane, run) PIECE costs one
//                            set of LDS atomics on slot j - j_lo of the wave's span table -- never one per row.  Then the first slot
//                            joins the carry, the last becomes the new carry, and the slots strictly between -- runs that begin and
//                            end inside the tile, which no other tile touches -- leave by plain stores, consecutive lanes writing
//                            consecutive 32-byte entries.
//   dense                    more runs than slots: a lane's piece that lies strictly between its first and its last belongs to a
//                            run inside the lane's rows and is stored plainly; the first and the last go to memory with agent-scope
//                            atomics.  The carry is flushed in front.
// The carry is flushed with four agent-scope atomics when the run changes and when the chunk ends: a run costs global atomics per
// chunk it crosses, not per tile or row.  out_dev holds the empty result and *uncovered 0 in front of the launch
// (run_aggregate_init_kernel), so plain stores and atomics both land on initialised words.
// Index safety: a run index that addresses out_dev or the table is < R, a slot index < the slots the tile uses <= S, whatever the
// ends hold.  Unsigned throughout.  The kernels test no switch bit.
#pragma once

#include "../runs/runs.hpp" // RunEnds, run_entry, run_search_wave, run_next_tile, run_rows, the chunk of 8 tiles

namespace mi355 {

struct RunAggArgs {
    const uint8_t *values;              // n values of cv bits, 16 B aligned
    uint64_t n;
    const uint8_t *mask;                // rows that count (ceil(n/8) bytes, 4 B aligned) or null = every row
    const uint32_t *ends;               // R entries of ce bits, 4 B aligned, non-decreasing
    const unsigned long long *runs_dev; // nullable: R = min(runs, *runs_dev)
    uint64_t runs;                      // <= 2^32 - 1
    unsigned long long *out;            // [4 j + 0] sum, [1] count, [2] min, [3] max -- the empty result in front of the launch
    unsigned long long *uncovered;      // nullable: counted rows with j(i) == R -- 0 in front of the launch, one add per wave
    uint32_t cv, ce;
    uint32_t slots;                     // S = run_agg_span_slots(cv)
};

// a slot of a wave's span table: sum u64, count u32, min u32, max u32, as four arrays behind the wave's two images
constexpr uint32_t kRunAggSlotBytes = 20;
constexpr uint32_t kRunAggMaxSlots = 1024, kRunAggMinSlots = 128;
// the blocks of a CU the rule below leaves room for: the tile search and the walk wait on dependent table reads, which further
// waves per SIMD hide.  Measured (profiles/r24_run_aggregate.txt against r24_run_aggregate_two_blocks.txt): four blocks with 128
// slots beat two with 512 at every gated shape, 1.30-1.56 x, and lose on runs of fewer than 16 rows
#ifndef MI355_RUN_AGG_RESIDENT_BLOCKS
#define MI355_RUN_AGG_RESIDENT_BLOCKS 4 // (a rebuild with EXTRA_FLAGS=-DMI355_RUN_AGG_RESIDENT_BLOCKS=2 trades blocks per CU for slots)
#endif
constexpr uint32_t kRunAggResidentBlocks = MI355_RUN_AGG_RESIDENT_BLOCKS;
constexpr uint32_t run_agg_wave_lds(uint32_t cv, uint32_t slots) { return 2u * rt_image(cv) + kRunAggSlotBytes * slots; }
constexpr uint32_t run_agg_block_lds(uint32_t cv, uint32_t slots) { return kWavesPerBlock * run_agg_wave_lds(cv, slots); }
// THE rule for S: the largest power of two with which the images and span tables of the four waves of four blocks fit a CU's LDS,
// and never below 128, which two blocks hold at every width (three up to 20 bits): 256 up to 8 bits, 128 beyond.
constexpr uint32_t run_agg_span_slots(uint32_t cv)
{
    uint32_t s = kRunAggMaxSlots;
    while (s > kRunAggMinSlots && kRunAggResidentBlocks * run_agg_block_lds(cv, s) > (uint32_t)kCuLdsBytes) s >>= 1;
    return s;
}
static_assert(2u * run_agg_block_lds(32, kRunAggMinSlots) <= (uint32_t)kCuLdsBytes, "LDS budget at the widest column");
static_assert(run_agg_span_slots(32) <= 256 && run_agg_span_slots(32) % 4 == 0, "a span table keeps the images 16 bytes aligned");

static __global__ void run_aggregate_init_kernel(unsigned long long *out, uint64_t runs, unsigned long long *uncovered)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j == 0 && uncovered) *uncovered = 0;
    if (j >= runs) return;
    unsigned long long *const o = out + 4ull * j;
    o[0] = 0;
    o[1] = 0;
    o[2] = ~0ull;
    o[3] = 0;
}

// minimum / maximum over the 64 lanes, wave-uniform: wave_inclusive_scan's DPP steps (kernels/tile.hpp) with the operation's
// neutral element where a step has no source lane, then lane 63's total
__device__ __forceinline__ uint32_t run_agg_wave_min(uint32_t x)
{
    constexpr int I = -1; // 0xffffffff
    uint32_t r = x;
    r = min(r, (uint32_t)__builtin_amdgcn_update_dpp(I, (int)x, 0x111, 0xf, 0xf, false)); // row_shr:1
    r = min(r, (uint32_t)__builtin_amdgcn_update_dpp(I, (int)x, 0x112, 0xf, 0xf, false)); // row_shr:2
    r = min(r, (uint32_t)__builtin_amdgcn_update_dpp(I, (int)x, 0x113, 0xf, 0xf, false)); // row_shr:3
    r = min(r, (uint32_t)__builtin_amdgcn_update_dpp(I, (int)r, 0x114, 0xf, 0xe, false)); // row_shr:4, banks 1-3
    r = min(r, (uint32_t)__builtin_amdgcn_update_dpp(I, (int)r, 0x118, 0xf, 0xc, false)); // row_shr:8, banks 2-3
    r = min(r, (uint32_t)__builtin_amdgcn_update_dpp(I, (int)r, 0x142, 0xa, 0xf, false)); // row_bcast:15 into rows 1, 3
    r = min(r, (uint32_t)__builtin_amdgcn_update_dpp(I, (int)r, 0x143, 0xc, 0xf, false)); // row_bcast:31 into rows 2, 3
    return (uint32_t)__builtin_amdgcn_readlane((int)r, 63);
}
__device__ __forceinline__ uint32_t run_agg_wave_max(uint32_t x)
{
    uint32_t r = x;
    r = max(r, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false));
    r = max(r, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false));
    r = max(r, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x113, 0xf, 0xf, false));
    r = max(r, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)r, 0x114, 0xf, 0xe, false));
    r = max(r, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)r, 0x118, 0xf, 0xc, false));
    r = max(r, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)r, 0x142, 0xa, 0xf, false));
    r = max(r, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)r, 0x143, 0xc, 0xf, false));
    return (uint32_t)__builtin_amdgcn_readlane((int)r, 63);
}
// a lane's sum of 32 values of at most 32 bits (< 2^37) over the wave: two limbs of 24 and 13 bits through the 32-bit wave_sum
__device__ __forceinline__ unsigned long long run_agg_wave_sum(unsigned long long x)
{
    const unsigned long long lo = wave_sum((uint32_t)(x & 0xffffffull)), hi = wave_sum((uint32_t)(x >> 24));
    return lo + (hi << 24);
}

// one set of agent-scope atomics on entry j (< R) of the result
__device__ __forceinline__ void run_agg_to_memory(unsigned long long *out, uint32_t j, unsigned long long sum, uint32_t cnt, uint32_t mn, uint32_t mx)
{
    unsigned long long *const o = out + 4ull * j;
    __hip_atomic_fetch_add(o + 0, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(o + 1, (unsigned long long)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_min(o + 2, (unsigned long long)mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(o + 3, (unsigned long long)mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a wave's span table: four arrays of S entries behind its two images
struct RunAggSpan {
    unsigned long long *sum;
    uint32_t *cnt, *mn, *mx;
    __device__ __forceinline__ RunAggSpan(uint8_t *lds, uint32_t slots)
        : sum((unsigned long long *)lds), cnt((uint32_t *)(lds + 8u * slots)), mn((uint32_t *)(lds + 12u * slots)), mx((uint32_t *)(lds + 16u * slots))
    {
    }
    __device__ __forceinline__ void reset(uint32_t s) const
    {
        sum[s] = 0;
        cnt[s] = 0;
        mn[s] = 0xffffffffu;
        mx[s] = 0;
    }
};

static __global__ __launch_bounds__(kBlockThreads) void run_aggregate_kernel(RunAggArgs a)
{
    constexpr uint32_t MASK_TILE = kRtTileRows / 8; // mask bytes of a tile
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t cv = a.cv, S = a.slots;
    const uint32_t tile_bytes = rt_tile_bytes(cv), image = rt_image(cv), vmask = rt_vmask(cv);
    uint8_t *cur = mi355_dyn_lds + (uint32_t)wave * run_agg_wave_lds(cv, S); // the image being decoded ...
    uint8_t *nxt = cur + image;                                              // ... and where the next tile lands
    const RunAggSpan span(cur + 2u * image, S);
    for (uint32_t s = lane; s < S; s += 64) span.reset(s);

    const uint64_t n = a.n;
    const uint64_t ntiles = rt_ntiles(n), nfull = rt_nfull(n);
    const uint64_t data_bytes = (n * cv + 7) / 8, mask_bytes = (n + 7) / 8;
    const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
    uint64_t R = a.runs;
    if (a.runs_dev) {
        const uint64_t have = uniform64(*a.runs_dev);
        R = have < R ? have : R;
    }
    const RunEnds ends{a.ends, a.ce, rt_vmask(a.ce), R ? run_last_word(R, a.ce) : 0u};
    unsigned long long *const out = a.out;

    // the lane's mask word of tile t (ragged end: only the bytes the bitmap is guaranteed to hold)
    auto load_mask = [&](uint64_t t) -> uint32_t {
        if (!a.mask) return 0xffffffffu;
        const uint64_t at = t * MASK_TILE + (uint64_t)lane * 4;
        if (t < nfull) return *(const uint32_t *)(a.mask + at);
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; b++)
            if (at + b < mask_bytes) v |= (uint32_t)a.mask[at + b] << (8 * b);
        return v;
    };

    // the carry: the partial of run cj, wave-uniform; nothing is carried while ccnt == 0
    uint32_t cj = 0, ccnt = 0, cmn = 0xffffffffu, cmx = 0;
    unsigned long long csum = 0;
    auto flush = [&]() {
        if (ccnt && lane == 0) run_agg_to_memory(out, cj, csum, ccnt, cmn, cmx);
        csum = 0, ccnt = 0, cmn = 0xffffffffu, cmx = 0;
    };
    // the carry becomes run j's: what it holds of another run leaves first
    auto carry_run = [&](uint32_t j) {
        if (cj != j) flush();
        cj = j;
    };

    uint64_t tile = ((uint64_t)blockIdx.x * kWavesPerBlock + wave) * kRunsChunkTiles;
    uint32_t mnext = 0;
    if (tile < ntiles) {
        rt_issue_tile<2>(a.values, data_bytes, tile_bytes, tile, cur, lane); // the column is streamed once: non-temporal DMA
        mnext = load_mask(tile);
    }
    unsigned long long outside = 0; // the lane's counted rows behind the last run so far
    uint64_t j_from = 0;            // the wave's tiles ascend: j(first row) is at least the last tile's
    uint64_t e_from = 0;            // the end of run j_from, ~0 for j_from == R; 0: not read yet
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the span table is initialised
    while (tile < ntiles) {
        const uint64_t row0 = tile * kRtTileRows;
        const uint64_t last = row0 + kRtTileRows - 1 < n - 1 ? row0 + kRtTileRows - 1 : n - 1;
        // the runs of the tile's first and last row, in front of the next tile's DMA: a table read behind it would wait for it
        if (e_from <= row0) {
            j_from = run_search_wave(ends, row0, j_from, R, lane);
            e_from = j_from < R ? ends.at((uint32_t)j_from) : ~0ull;
        }
        const uint32_t j_lo = (uint32_t)j_from;
        uint64_t j_top = j_from;
        if (e_from <= last) j_top = run_search_wave(ends, last, j_from, R, lane);
        const uint32_t j_hi = (uint32_t)j_top;

        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the tile and its mask word have landed
        uint32_t m = mnext;
        const uint64_t next = run_next_tile(tile, ntiles, nwaves);
        if (next < ntiles) {
            rt_issue_tile<2>(a.values, data_bytes, tile_bytes, next, nxt, lane);
            mnext = load_mask(next);
        }
        const int valid = lane_valid_rows<kRtVpl>(n, tile, lane);
        if (tile >= nfull) m &= tail_mask(valid, 0); // rows behind the column count for nothing
        const uint8_t *const base = cur + (uint32_t)lane * rt_lane_bytes(cv);

        if (j_lo == j_hi) {
            if (j_lo >= R) {
                outside += (uint32_t)__builtin_popcount(m);
            } else {
                // one run covers the tile
                unsigned long long ls = 0;
                uint32_t lmn = 0xffffffffu, lmx = 0;
                run_rows([&](auto K) {
                    constexpr int k = decltype(K)::value;
                    const uint32_t x = columns_lds_value<k>(base, cv, vmask);
                    const bool on = (m >> k) & 1u;
                    ls += on ? x : 0u;
                    lmn = min(lmn, on ? x : 0xffffffffu);
                    lmx = max(lmx, on ? x : 0u);
                });
                const uint32_t c = wave_sum((uint32_t)__builtin_popcount(m));
                if (c) {
                    carry_run(j_lo);
                    csum += run_agg_wave_sum(ls);
                    ccnt += c;
                    cmn = min(cmn, run_agg_wave_min(lmn));
                    cmx = max(cmx, run_agg_wave_max(lmx));
                }
            }
        } else {
            // several runs: j_lo < j_hi <= R.  The runs the tile addresses are j_lo .. j_last (< R); rows of run R are uncovered
            const uint32_t j_last = j_hi < R ? j_hi : (uint32_t)R - 1u;
            const uint32_t nslots = j_last - j_lo + 1u;
            const bool tier = nslots <= S;
            if (tier)
                carry_run(j_lo);
            else
                flush();
            if (valid > 0) {
                const uint64_t i0 = row0 + (uint64_t)lane * kRtVpl;
                uint32_t lo = j_lo, hi = j_hi; // the lane's own first row: binary search inside [j_lo, j_hi]
                while (lo < hi) {
                    const uint32_t mid = lo + (hi - lo) / 2;
                    if (ends.at(mid) <= i0)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                uint32_t j = lo;
                uint64_t e = j < R ? ends.at(j) : ~0ull;
                unsigned long long ps = 0;
                uint32_t pc = 0, pmn = 0xffffffffu, pmx = 0, beyond = 0;
                bool first = true;
                // the piece of run j (< R) leaves the lane.  edge: the lane's first or last piece, which other lanes may share
                auto emit = [&](bool edge) {
                    if (pc) {
                        const uint32_t s = j - j_lo;
                        if (tier && s < nslots) {
                            __hip_atomic_fetch_add(span.sum + s, ps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            __hip_atomic_fetch_add(span.cnt + s, pc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            __hip_atomic_fetch_min(span.mn + s, pmn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            __hip_atomic_fetch_max(span.mx + s, pmx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        } else if (edge || tier) {
                            run_agg_to_memory(out, j, ps, pc, pmn, pmx);
                        } else {
                            unsigned long long *const o = out + 4ull * j;
                            o[0] = ps;
                            o[1] = pc;
                            o[2] = pmn;
                            o[3] = pmx;
                        }
                    }
                    ps = 0, pc = 0, pmn = 0xffffffffu, pmx = 0;
                };
#pragma unroll 1
                for (int k = 0; k < kRtVpl; k++) {
                    if (k < valid) {
                        const uint64_t i = i0 + (uint32_t)k;
                        if (e <= i) { // run j (< R: its end is no ~0) ends here; zero-length runs behind it are skipped, bounded by R
                            emit(first);
                            first = false;
                            do {
                                j++;
                                e = j < R ? ends.at(j) : ~0ull;
                            } while (e <= i);
                        }
                        if ((m >> k) & 1u) {
                            const uint32_t bit = (uint32_t)k * cv; // wave-uniform
                            const uint32_t *const p = (const uint32_t *)(base + (bit >> 5) * 4);
                            const uint32_t x = __builtin_amdgcn_alignbit(p[1], p[0], bit & 31u) & vmask;
                            if (j < R) {
                                ps += x;
                                pc++;
                                pmn = min(pmn, x);
                                pmx = max(pmx, x);
                            } else {
                                beyond++;
                            }
                        }
                    }
                }
                if (j < R) emit(true);
                outside += beyond;
            }
            if (tier) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the wave's updates are in the table (LDS is in order per wave)
                {
                    // the first slot is run j_lo's: it joins the carry
                    const unsigned long long s0 = uniform64(span.sum[0]);
                    const uint32_t c0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)span.cnt[0]);
                    const uint32_t n0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)span.mn[0]);
                    const uint32_t x0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)span.mx[0]);
                    csum += s0;
                    ccnt += c0;
                    cmn = min(cmn, n0);
                    cmx = max(cmx, x0);
                }
                if (nslots > 1) {
                    flush(); // run j_lo ends inside the tile
                    // the slots strictly between belong to this tile alone: consecutive lanes, consecutive 32-byte entries
                    for (uint32_t s = 1u + (uint32_t)lane; s + 1u < nslots; s += 64) {
                        const unsigned long long ss = span.sum[s];
                        const uint32_t sc = span.cnt[s], sn = span.mn[s], sx = span.mx[s];
                        span.reset(s);
                        if (sc) {
                            unsigned long long *const o = out + 4ull * (j_lo + s);
                            o[0] = ss;
                            o[1] = sc;
                            o[2] = sn;
                            o[3] = sx;
                        }
                    }
                    // the last slot is the run that may go on in the next tile: the new carry
                    const uint32_t t = nslots - 1u;
                    csum = uniform64(span.sum[t]);
                    ccnt = (uint32_t)__builtin_amdgcn_readfirstlane((int)span.cnt[t]);
                    cmn = (uint32_t)__builtin_amdgcn_readfirstlane((int)span.mn[t]);
                    cmx = (uint32_t)__builtin_amdgcn_readfirstlane((int)span.mx[t]);
                    cj = j_last;
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (lane == 0) {
                    span.reset(0);
                    span.reset(nslots - 1u);
                }
            }
            // the next tile's first row lies in run j_hi or behind it; that run's end is not known to the whole wave
            j_from = j_top;
            e_from = 0;
        }
        if (next != tile + 1) flush(); // the chunk ends
        uint8_t *const t = cur;
        cur = nxt;
        nxt = t;
        tile = next;
    }
    if (a.uncovered) {
        const unsigned long long total = wave_sum64(outside);
        if (lane == 0 && total) __hip_atomic_fetch_add(a.uncovered, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

} // namespace mi355
