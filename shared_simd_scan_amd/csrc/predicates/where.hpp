// predicates/where.hpp -- shared scans over range and comparison predicates (gfx950 only): up to 1024 predicates
// `v OP a [, b]` (== != < <= > >= BETWEEN NOT BETWEEN) answered in one pass over a packed column.
//
// Every predicate arrives normalised as (lo, span, neg): it holds for x iff ((x - lo) <= span) != (neg != 0), in unsigned
// 32-bit arithmetic -- the inclusive range [lo, lo + span] clamped to the column's domain plus a negation word, the form
// capi.hip's fill_predicate gives the single-predicate scan.  An empty range is lo = 0xffffffff, span = 0 below c = 32 and
// the full range with the negation flipped at c = 32.
//
//   shared_where_lut_kernel    c <= 16: the organisation of shared_lut_kernel -- one LDS byte lookup per value and pass of
//                              8 predicates, entry[v] bit q = predicate q holds for v -- with FULL tables of 2^c entries in
//                              every pass (a range does not decompose into digit tables the way equality does) and a
//                              prologue that builds them in O(table / threads + P) per block
//   shared_where_chain_kernel  everything else: the organisation of shared_general_kernel, the compare of the range scan
//                              (v_sub + v_cmp + v_addc per value and predicate) against 8 predicates per pass
// Neither reads ScanArgs::flags.
#pragma once

#include "../kernels.hpp"

namespace mi355 {

struct WhereArgs {
    ScanArgs s;                // packed, n, out, out_stride, hits, scratch, nkeys, layout: as for the equality shared scans
                               // (key[], keys_dev and flags are not read)
    uint32_t lo[kMaxKeysPerPass], span[kMaxKeysPerPass], neg[kMaxKeysPerPass]; // P <= 8: the predicates
    const uint32_t *preds_dev; // P > 8: (lo, span, neg) of predicate k at [3k, 3k + 3), padded to a multiple of 8 predicates
};

// ---- lookup tables --------------------------------------------------------------------------------------------------
template <int C> struct WhereLutGeom {
    static_assert(C >= 1 && C <= 16, "full tables: c <= 16");
    static constexpr int ENTRIES = 1 << C;
    static constexpr int TABLE_BYTES = ENTRIES < 4 ? 4 : ENTRIES; // per pass of 8 predicates; c = 1: padded to a whole dword
    static constexpr int TABLE_DWORDS = TABLE_BYTES / 4;
    // prefix pass: a thread owns CH consecutive dwords (one ds_read_b128 / ds_write_b128 where the table has them: lanes
    // at consecutive 16-byte addresses, no bank conflicts), T threads cover a table
    static constexpr int CH = TABLE_DWORDS >= 4 ? 4 : 1;
    static constexpr int T = TABLE_DWORDS / CH;
};

// Builds the npass tables at `lut` (npass * TABLE_BYTES bytes, 16-byte aligned): bit (k % 8) of entry v of table k / 8 =
// predicate k holds for v.  Not by walking every range (O(table x P)) but by its derivative: zero the tables, toggle bit
// q where predicate q's value changes -- at lo, behind lo + span when that is still inside the table, and at entry 0 for
// a negated predicate (LDS atomic XOR on the containing dword: several predicates may meet in one dword; an empty range,
// lo beyond the table, toggles nothing of its own) -- and take the inclusive prefix XOR over the bytes of each table:
// inside a dword x ^= x << 8, x ^= x << 16; a thread's dwords in sequence; the threads of a table by a segmented wave
// scan, the wave totals through LDS, and a running byte for tables of more than 256 threads' worth.  O(table / 256 + P)
// per block.  Every thread of the block calls this; s_carry: 2 x kWavesPerBlock dwords of LDS.
template <int C, bool MULTI>
__device__ __forceinline__ void where_build_tables(const WhereArgs &a, uint8_t *lut, uint32_t P, uint32_t npass, uint32_t *s_carry)
{
    using W = WhereLutGeom<C>;
    uint32_t *const lut32 = (uint32_t *)lut;
    const uint32_t ndw = npass * W::TABLE_DWORDS;
    for (uint32_t i = threadIdx.x; i < ndw; i += kBlockThreads) lut32[i] = 0;
    __syncthreads();
    auto toggle = [&](uint32_t k, uint32_t lo, uint32_t span, uint32_t neg) {
        const uint32_t base = (k >> 3) * W::TABLE_BYTES;
        const uint32_t bit = 1u << (k & 7);
        auto flip = [&](uint32_t e) {
            const uint32_t idx = base + e;
            __hip_atomic_fetch_xor(lut32 + (idx >> 2), bit << (8 * (idx & 3)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        };
        if (lo < (uint32_t)W::ENTRIES) {
            flip(lo);
            const uint64_t end = (uint64_t)lo + span + 1;
            if (end < (uint64_t)W::ENTRIES) flip((uint32_t)end);
        }
        if (neg) flip(0);
    };
    if constexpr (MULTI) {
        for (uint32_t k = threadIdx.x; k < P; k += kBlockThreads) toggle(k, a.preds_dev[3 * k], a.preds_dev[3 * k + 1], a.preds_dev[3 * k + 2]);
    } else {
        if (threadIdx.x < (uint32_t)kMaxKeysPerPass && threadIdx.x < P) toggle(threadIdx.x, a.lo[threadIdx.x], a.span[threadIdx.x], a.neg[threadIdx.x]);
    }
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const uint32_t units = npass * W::T; // a unit: the CH dwords of one thread
    uint32_t carry = 0;                  // T > 256: prefix byte of the table in progress, the same in every thread
    for (uint32_t u0 = 0, round = 0; u0 < units; u0 += kBlockThreads, round++) {
        const uint32_t u = u0 + threadIdx.x;
        const bool on = u < units;
        uint32_t d[W::CH];
        if constexpr (W::CH == 4) {
            const u32x4 v = on ? ((const u32x4 *)lut32)[u] : u32x4{0, 0, 0, 0};
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        } else {
            d[0] = on ? lut32[u] : 0u;
        }
        uint32_t run = 0; // prefix byte at the end of the dwords so far
#pragma unroll
        for (int j = 0; j < W::CH; j++) {
            uint32_t x = d[j];
            x ^= x << 8;
            x ^= x << 16;
            x ^= run * 0x01010101u;
            d[j] = x;
            run = x >> 24;
        }
        // threads of one table are neighbours: inclusive XOR scan of `run` over segments of min(T, 64) lanes ...
        constexpr int SEGW = W::T < 64 ? W::T : 64;
        uint32_t inc = run;
#pragma unroll
        for (int s = 1; s < SEGW; s <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)inc, s);
            if ((lane & (SEGW - 1)) >= s) inc ^= up;
        }
        uint32_t before = inc ^ run; // prefix byte in front of this thread's dwords
        if constexpr (W::T > 64) {
            // ... and over the waves of the table (one barrier per round: the totals alternate between two rows)
            constexpr int SEGB = (W::T < kBlockThreads ? W::T : kBlockThreads) / 64;
            uint32_t *const row = s_carry + (round & 1) * kWavesPerBlock;
            if (lane == 63) row[wave] = inc;
            __syncthreads();
            uint32_t total = 0;
#pragma unroll
            for (int w = 0; w < kWavesPerBlock; w++) {
                const uint32_t t = row[w];
                if (w / SEGB == wave / SEGB) {
                    if (w < wave) before ^= t;
                    total ^= t;
                }
            }
            if constexpr (W::T > kBlockThreads) {
                if (u0 % (uint32_t)W::T == 0) carry = 0; // a new table starts with this round
                before ^= carry;
                carry ^= total;
            }
        }
        const uint32_t pre = before * 0x01010101u;
        if (on) {
            if constexpr (W::CH == 4) {
                ((u32x4 *)lut32)[u] = u32x4{d[0] ^ pre, d[1] ^ pre, d[2] ^ pre, d[3] ^ pre};
            } else {
                lut32[u] = d[0] ^ pre;
            }
        }
    }
    __syncthreads();
}

// ---- table kernel ---------------------------------------------------------------------------------------------------
// The tile loop of shared_lut_kernel (kernels/shared.hpp) over the tables above: LAYOUT 0 per-predicate bitmaps at
// out + k * out_stride, 1 linear (byte of 8-value group g and predicate k at g * P + k).  MULTI false: P <= 8, one pass, the
// table in static LDS, stores deferred by one tile; true: ceil(P / 8) passes per tile over tables in dynamic LDS (the
// launcher checks that they fit), stored pass by pass, per-block hit counters.
template <int C, int AUX_, int VPL, int LAYOUT, bool MULTI>
__global__ __launch_bounds__(kBlockThreads) void shared_where_lut_kernel(WhereArgs a)
{
    using G = ScanGeom<C, VPL>;
    using W = WhereLutGeom<C>;
    constexpr int WORDS = G::WORDS;
    constexpr int GROUPS = VPL / 8;
    constexpr int AUX = AUX_ & 15;
    constexpr int NTS = store_policy_of(AUX_); // result stores: 1 non-temporal, 2 write-through (sc1)
    constexpr int NRES = LAYOUT == 0 ? 8 * WORDS : GROUPS * 2;   // result dwords per lane, tile and pass
    __shared__ __attribute__((aligned(16))) uint8_t lds[kWavesPerBlock][G::LDS_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t lut_static[(MULTI || W::TABLE_BYTES < 16) ? 16 : W::TABLE_BYTES];
    uint8_t *const lut = MULTI ? mi355_dyn_lds : lut_static; // MULTI: npass * TABLE_BYTES dynamic bytes
    __shared__ uint32_t s_hits[MULTI ? kMaxKeys : 1];          // MULTI: per-block hit counters (block_hits_add8)
    __shared__ uint32_t s_carry[2 * kWavesPerBlock];
    __shared__ __attribute__((aligned(16))) uint8_t stage[(LAYOUT == 1 && !MULTI) ? kWavesPerBlock : 1][(LAYOUT == 1 && !MULTI) ? GROUPS * 8 * 64 : 16];
    if constexpr (MULTI) block_hits_clear(s_hits);

    const ScanArgs &s = a.s;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint8_t *lds_wave = lds[wave];
    const TileCtx<C, VPL> tc(s.n);
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock;
    uint64_t tile = (uint64_t)blockIdx.x * kWavesPerBlock + wave;
    const uint32_t P = s.nkeys;
    const uint32_t npass = MULTI ? (P + 7) / 8 : 1;

    // the tile's DMA does not depend on the tables: get it going first
    if (tile < tc.ntiles) tc.template issue<AUX>(s.packed, tile, lds_wave, lane);

    where_build_tables<C, MULTI>(a, lut, P, npass, s_carry);

    uint32_t hits[8];
#pragma unroll
    for (int q = 0; q < 8; q++) hits[q] = 0;

    // full-tile store of one pass: LAYOUT 0: res = out[q][j] (q-major); LAYOUT 1: res = Y[g][0..1]
    auto store_full = [&](uint64_t t, uint32_t pass, const uint32_t (&res)[NRES]) {
        if constexpr (LAYOUT == 0) {
            uint8_t *dst = s.out + (uint64_t)(pass * 8) * s.out_stride + t * G::BITMAP_BYTES + lane * (WORDS * 4);
#pragma unroll
            for (int q = 0; q < 8; q++) {
                if (pass * 8 + q < P) {
                    uint32_t v[WORDS];
#pragma unroll
                    for (int j = 0; j < WORDS; j++) v[j] = res[q * WORDS + j];
                    store_words<WORDS, NTS>(dst, v);
                }
                dst += s.out_stride;
            }
        } else {
            const uint64_t g0 = t * G::BITMAP_BYTES + (uint64_t)lane * GROUPS;
            if (!MULTI && P == 4) { // a group's row is the dword of predicates 0..3; the lane's GROUPS rows are contiguous
                u32x4 *dst = (u32x4 *)(s.out + g0 * 4);
#pragma unroll
                for (int g = 0; g < GROUPS; g += 4) {
                    u32x4 v = {res[2 * g], res[2 * g + 2], res[2 * g + 4], res[2 * g + 6]};
                    dst[g / 4] = v;
                }
            } else if (!MULTI && P == 2) { // a row is 2 bytes; rows of two groups share a dword
                u32x4 *dst = (u32x4 *)(s.out + g0 * 2);
#pragma unroll
                for (int g = 0; g < GROUPS; g += 8) {
                    u32x4 v = {__builtin_amdgcn_perm(res[2 * g + 2], res[2 * g], 0x05040100u),
                               __builtin_amdgcn_perm(res[2 * g + 6], res[2 * g + 4], 0x05040100u),
                               __builtin_amdgcn_perm(res[2 * g + 10], res[2 * g + 8], 0x05040100u),
                               __builtin_amdgcn_perm(res[2 * g + 14], res[2 * g + 12], 0x05040100u)};
                    dst[g / 8] = v;
                }
            } else if (!MULTI && P == 3) {
                store_linear_rows_packed<3, GROUPS, NRES>(s.out + g0 * 3, res);
            } else if (!MULTI && P == 5) {
                store_linear_rows_packed<5, GROUPS, NRES>(s.out + g0 * 5, res);
            } else if (!MULTI && P == 6) {
                store_linear_rows_packed<6, GROUPS, NRES>(s.out + g0 * 6, res);
            } else if (!MULTI && P == 7) {
                store_linear_rows_packed<7, GROUPS, NRES>(s.out + g0 * 7, res);
            } else {
                const uint32_t nk = (P - pass * 8) < 8 ? (P - pass * 8) : 8;
#pragma unroll
                for (int g = 0; g < GROUPS; g++) {
                    uint8_t *dst = s.out + (g0 + g) * P + pass * 8;
                    if (nk == 8) {
                        store8_unaligned(dst, res[2 * g], res[2 * g + 1]);
                    } else {
#pragma unroll
                        for (int q = 0; q < 8; q++)
                            if ((uint32_t)q < nk) dst[q] = (uint8_t)(res[2 * g + (q >> 2)] >> (8 * (q & 3)));
                    }
                }
            }
        }
    };

    // Linear layout, 8 predicates: the wave's tile is 64 x GROUPS x 8 contiguous output bytes; they pass through a per-wave
    // LDS stage so that every store instruction writes 1 KiB contiguous (see shared_lut_kernel)
    const bool lin8 = LAYOUT == 1 && !MULTI && P == 8;
    auto stage_put = [&](const uint32_t (&res)[NRES]) {
        u32x4 *st = (u32x4 *)stage[wave];
#pragma unroll
        for (int g = 0; g < GROUPS; g += 2) {
            u32x4 v = {res[2 * g], res[2 * g + 1], res[2 * g + 2], res[2 * g + 3]};
            st[lane * (GROUPS / 2) + g / 2] = v;
        }
    };
    auto stage_get = [&](u32x4 (&r)[GROUPS / 2]) {
        const u32x4 *st = (const u32x4 *)stage[wave];
#pragma unroll
        for (int j = 0; j < GROUPS / 2; j++) r[j] = st[j * 64 + lane];
    };
    auto stage_store = [&](uint64_t t, const u32x4 (&r)[GROUPS / 2]) {
        u32x4 *dst = (u32x4 *)(s.out + (t * G::BITMAP_BYTES) * 8);
#pragma unroll
        for (int j = 0; j < GROUPS / 2; j++) {
            if constexpr (NTS == 2)
                asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(dst + j * 64 + lane), "v"(r[j]) : "memory");
            else if constexpr (NTS == 1)
                __builtin_nontemporal_store(r[j], dst + j * 64 + lane);
            else
                dst[j * 64 + lane] = r[j];
        }
    };

    uint32_t resp[NRES]; // !MULTI: results of the previous tile, not yet stored (lin8: they wait in the LDS stage)
    uint64_t prev = ~0ull;

    while (tile < tc.ntiles) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        uint32_t w[G::LANE_DWORDS];
        read_lane_data<C, VPL>(lds_wave, lane, w);
        u32x4 staged[GROUPS / 2];
        if (lin8 && prev != ~0ull) stage_get(staged);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if constexpr (!MULTI) {
            if (prev != ~0ull) {
                if (lin8)
                    stage_store(prev, staged);
                else
                    store_full(prev, 0, resp);
            }
            prev = ~0ull;
        }
        const uint64_t next = tile + stride;
        if (next < tc.ntiles) tc.template issue<AUX>(s.packed, next, lds_wave, lane);
        const bool full = tile < tc.nfull;
        uint32_t xs[VPL];
        extract_all<C, VPL, 0, G::LANE_DWORDS>(w, xs);

        if constexpr (MULTI && LAYOUT == 1) {
            // Linear layout, many predicates: walk the lane's rows in order and, inside a row, the passes in order, so that
            // every row of P bytes is written start to end in one go
            if (full) {
                const uint64_t g0 = tile * G::BITMAP_BYTES + (uint64_t)lane * GROUPS;
#pragma unroll
                for (int g = 0; g < GROUPS; g++) {
                    uint8_t *row = s.out + (g0 + g) * P;
                    uint32_t xg[8];
#pragma unroll
                    for (int i = 0; i < 8; i++) xg[i] = xs[8 * g + i];
                    auto pass8 = [&](uint32_t pass, uint32_t &lo, uint32_t &hi) {
                        const uint8_t *table = lut + pass * W::TABLE_BYTES;
                        lo = 0;
                        hi = 0;
#pragma unroll
                        for (int i = 0; i < 8; i++) {
                            const uint32_t m = table[xg[i]];
                            if (i < 4)
                                lo |= m << (8 * i);
                            else
                                hi |= m << (8 * (i - 4));
                        }
                        transpose8x8(lo, hi);
                    };
                    uint32_t pass = 0;
                    for (; pass + 2 <= P / 8; pass += 2) { // two passes = 16 predicates = one 16-byte store
                        uint32_t l0, h0, l1, h1;
                        pass8(pass, l0, h0);
                        pass8(pass + 1, l1, h1);
                        Unaligned128 v;
                        v.w[0] = l0; v.w[1] = h0; v.w[2] = l1; v.w[3] = h1;
                        *(Unaligned128 *)(row + pass * 8) = v;
                    }
                    for (; pass < npass; pass++) {
                        uint32_t lo, hi;
                        pass8(pass, lo, hi);
                        const uint32_t nk = (P - pass * 8) < 8 ? (P - pass * 8) : 8;
                        if (nk == 8) {
                            store8_unaligned(row + pass * 8, lo, hi);
                        } else {
#pragma unroll
                            for (int q = 0; q < 8; q++)
                                if ((uint32_t)q < nk) row[pass * 8 + q] = (uint8_t)((q < 4 ? lo : hi) >> (8 * (q & 3)));
                        }
                    }
                }
            }
        }

        // pass-major loop: per-predicate stores, hit counts, tail tiles (and everything for one-pass scans)
        for (uint32_t pass = 0; pass < npass && (!(MULTI && LAYOUT == 1) || !full || s.hits); pass++) {
            const uint8_t *table = lut + pass * W::TABLE_BYTES;
            uint32_t Y[GROUPS][2];
            uint32_t out[8][WORDS];
            if (full) {
                lut_words<C, VPL, false, false>(xs, table, VPL, out);
                if constexpr (LAYOUT == 1) words_to_groups<VPL>(out, Y);
                if (s.hits) {
#pragma unroll
                    for (int q = 0; q < 8; q++)
#pragma unroll
                        for (int j = 0; j < WORDS; j++) hits[q] += __builtin_popcount(out[q][j]);
                }
                uint32_t res[NRES];
                if constexpr (LAYOUT == 0) {
#pragma unroll
                    for (int q = 0; q < 8; q++)
#pragma unroll
                        for (int j = 0; j < WORDS; j++) res[q * WORDS + j] = out[q][j];
                } else {
#pragma unroll
                    for (int g = 0; g < GROUPS; g++) { res[2 * g] = Y[g][0]; res[2 * g + 1] = Y[g][1]; }
                }
                if constexpr (!MULTI) {
                    if (lin8) {
                        stage_put(res);
                    } else {
#pragma unroll
                        for (int i = 0; i < NRES; i++) resp[i] = res[i];
                    }
                    prev = tile;
                } else {
                    if (s.hits) {
                        block_hits_add8(s_hits, pass * 8, P, hits, lane);
#pragma unroll
                        for (int q = 0; q < 8; q++) hits[q] = 0;
                    }
                    // LAYOUT 1: the rows are written group by group above (each row's P bytes back to back)
                    if constexpr (LAYOUT == 0) store_full(tile, pass, res);
                }
            } else {
                // tail tile: lookups of values >= n are zeroed; the bitmap is written byte-exact
                const int64_t left = (int64_t)(tc.n - tile * G::TILE_VALUES) - (int64_t)lane * VPL;
                const int valid = left >= VPL ? VPL : (left <= 0 ? 0 : (int)left);
                const int nbytes = (valid + 7) / 8;
                if constexpr (LAYOUT == 0) { // (the per-group form, as in shared_lut_kernel's cold branch)
                    lut_groups_x<C, VPL, true, false>(xs, table, valid, Y);
                    lut_gather_keys<VPL>(Y, out);
                } else {
                    lut_words<C, VPL, true, false>(xs, table, valid, out);
                }
                uint32_t tcnt[8];
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    const uint32_t k = pass * 8 + q;
                    tcnt[q] = 0;
                    if (k < P) {
                        uint32_t cnt = 0;
#pragma unroll
                        for (int j = 0; j < WORDS; j++) cnt += __builtin_popcount(out[q][j]);
                        if constexpr (!MULTI)
                            hits[q] += cnt;
                        else
                            tcnt[q] = cnt;
                        uint8_t *dst = LAYOUT == 0
                                           ? s.out + (uint64_t)k * s.out_stride + tile * G::BITMAP_BYTES + lane * (WORDS * 4)
                                           : s.out + (tile * G::BITMAP_BYTES + (uint64_t)lane * GROUPS) * P + k;
                        const uint64_t bstride = LAYOUT == 0 ? 1 : P;
#pragma unroll
                        for (int b = 0; b < WORDS * 4; b++)
                            if (b < nbytes) dst[(uint64_t)b * bstride] = (uint8_t)(out[q][b >> 2] >> (8 * (b & 3)));
                    }
                }
                if constexpr (MULTI) {
                    if (s.hits) block_hits_add8(s_hits, pass * 8, P, tcnt, lane);
                }
            }
        }
        tile = next;
    }
    if constexpr (MULTI) {
        if (s.hits) block_hits_flush(s, s_hits, P);
    }
    if constexpr (!MULTI) {
        if (prev != ~0ull) {
            if (lin8) {
                u32x4 staged[GROUPS / 2];
                stage_get(staged);
                stage_store(prev, staged);
            } else {
                store_full(prev, 0, resp);
            }
        }
        if (s.hits) {
#pragma unroll
            for (int q = 0; q < 8; q++) {
                uint32_t t = wave_sum(hits[q]);
                if ((uint32_t)q < P) hits_add(s, q, t, lane);
            }
        }
    }
    hits_finalize(s, P, lane);
}

// ---- compare chain --------------------------------------------------------------------------------------------------
// one value against four ranges: t = x - lo, span >= t appended to the accumulator (acc = 2 * acc + match) -- push4's
// range form (kernels/tile.hpp) with four predicates instead of four values: four independent chains, so every mask
// register is written four instructions before the v_addc that reads it
__device__ __forceinline__ void push_range4(uint32_t &a0, uint32_t &a1, uint32_t &a2, uint32_t &a3, uint32_t x, uint32_t l0, uint32_t l1,
                                            uint32_t l2, uint32_t l3, uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3)
{
    unsigned long long m0, m1, m2, m3;
    uint32_t t0, t1, t2, t3;
    asm("v_subrev_u32_e32 %8, %13, %12\n\t"
        "v_subrev_u32_e32 %9, %14, %12\n\t"
        "v_subrev_u32_e32 %10, %15, %12\n\t"
        "v_subrev_u32_e32 %11, %16, %12\n\t"
        "v_cmp_ge_u32_e64 %4, %17, %8\n\t"
        "v_cmp_ge_u32_e64 %5, %18, %9\n\t"
        "v_cmp_ge_u32_e64 %6, %19, %10\n\t"
        "v_cmp_ge_u32_e64 %7, %20, %11\n\t"
        "v_addc_co_u32_e64 %0, %4, %0, %0, %4\n\t"
        "v_addc_co_u32_e64 %1, %5, %1, %1, %5\n\t"
        "v_addc_co_u32_e64 %2, %6, %2, %2, %6\n\t"
        "v_addc_co_u32_e64 %3, %7, %3, %3, %7"
        : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "=&s"(m0), "=&s"(m1), "=&s"(m2), "=&s"(m3), "=&v"(t0), "=&v"(t1), "=&v"(t2),
          "=&v"(t3)
        : "v"(x), "s"(l0), "s"(l1), "s"(l2), "s"(l3), "s"(s0), "s"(s1), "s"(s2), "s"(s3));
}

// values 32J + K down to 32J of the lane against 8 ranges (the highest first, so that value 32J lands in bit 0)
template <int C, int J, int K, int NW>
__device__ __forceinline__ void where_step8(const uint32_t (&w)[NW], uint32_t (&acc)[8], const uint32_t (&lo)[8], const uint32_t (&span)[8])
{
    const uint32_t x = extract<C, 32 * J + K, NW>(w);
    push_range4(acc[0], acc[1], acc[2], acc[3], x, lo[0], lo[1], lo[2], lo[3], span[0], span[1], span[2], span[3]);
    push_range4(acc[4], acc[5], acc[6], acc[7], x, lo[4], lo[5], lo[6], lo[7], span[4], span[5], span[6], span[7]);
    if constexpr (K > 0) where_step8<C, J, K - 1, NW>(w, acc, lo, span);
}

template <int C, int VPL, int J, int NW>
__device__ __forceinline__ void where_words8(const uint32_t (&w)[NW], uint32_t (&res)[8][VPL / 32], const uint32_t (&lo)[8],
                                             const uint32_t (&span)[8], const uint32_t (&neg)[8])
{
    uint32_t acc[8];
#pragma unroll
    for (int q = 0; q < 8; q++) acc[q] = 0;
    where_step8<C, J, 31, NW>(w, acc, lo, span);
#pragma unroll
    for (int q = 0; q < 8; q++) res[q][J] = acc[q] ^ neg[q]; // the negation word: 0 or 0xffffffff (bits >= n are masked by the tail store)
    if constexpr (J + 1 < VPL / 32) where_words8<C, VPL, J + 1, NW>(w, res, lo, span, neg);
}

// any P <= 1024 at any width: ceil(P / 8) passes of 8 predicates over the lane's registers per tile, both layouts,
// per-block hit counters; the (lo, span, neg) triples of a pass are wave-uniform (kernel arguments for P <= 8, else read
// from the device array into scalar registers).  Right at c = 32: nothing here needs a value above the domain.
template <int C, int AUX_, int VPL>
__global__ __launch_bounds__(kBlockThreads) void shared_where_chain_kernel(WhereArgs a)
{
    using G = ScanGeom<C, VPL>;
    constexpr int NK = kMaxKeysPerPass;
    constexpr int WORDS = G::WORDS;
    constexpr int AUX = AUX_ & 15;
    __shared__ __attribute__((aligned(16))) uint8_t lds[kWavesPerBlock][G::LDS_BYTES];
    __shared__ uint32_t s_hits[kMaxKeys];
    block_hits_clear(s_hits);
    __syncthreads();

    const ScanArgs &s = a.s;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint8_t *lds_wave = lds[wave];
    const TileCtx<C, VPL> tc(s.n);
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock;
    uint64_t tile = (uint64_t)blockIdx.x * kWavesPerBlock + wave;
    const uint32_t P = s.nkeys;
    const bool preds_in_args = P <= (uint32_t)kMaxKeysPerPass;
    const uint32_t npass = (P + kMaxKeysPerPass - 1) / kMaxKeysPerPass;

    if (tile < tc.ntiles) tc.template issue<AUX>(s.packed, tile, lds_wave, lane);
    while (tile < tc.ntiles) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        uint32_t w[G::LANE_DWORDS];
        read_lane_data<C, VPL>(lds_wave, lane, w);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const uint64_t next = tile + stride;
        if (next < tc.ntiles) tc.template issue<AUX>(s.packed, next, lds_wave, lane);
        const bool full = tile < tc.nfull;

        for (uint32_t pass = 0; pass < npass; pass++) {
            uint32_t lo[NK], span[NK], neg[NK];
            if (preds_in_args) {
#pragma unroll
                for (int q = 0; q < NK; q++) {
                    lo[q] = a.lo[q];
                    span[q] = a.span[q];
                    neg[q] = a.neg[q];
                }
            } else {
                const uint32_t *p = a.preds_dev + (size_t)pass * (3 * NK);
#pragma unroll
                for (int q = 0; q < NK; q++) {
                    lo[q] = __builtin_amdgcn_readfirstlane(p[3 * q]);
                    span[q] = __builtin_amdgcn_readfirstlane(p[3 * q + 1]);
                    neg[q] = __builtin_amdgcn_readfirstlane(p[3 * q + 2]);
                }
            }
            uint32_t res[NK][WORDS];
            where_words8<C, VPL, 0, G::LANE_DWORDS>(w, res, lo, span, neg);
            uint32_t cnts[8];
#pragma unroll
            for (int q = 0; q < NK; q++) {
                const uint32_t k = pass * NK + q;
                cnts[q] = 0;
                if (k < P) {
                    uint32_t cnt = 0;
                    if (s.layout == 0) {
                        uint8_t *dst = s.out + (uint64_t)k * s.out_stride + tile * G::BITMAP_BYTES + lane * (WORDS * 4);
                        if (full) {
#pragma unroll
                            for (int j = 0; j < WORDS; j++) cnt += __builtin_popcount(res[q][j]);
                            store_words<WORDS>(dst, res[q]);
                        } else {
                            cnt = tc.finish_tail(tile, res[q], dst, 1, lane);
                        }
                    } else if (!full) {
                        uint8_t *dst = s.out + (tile * G::BITMAP_BYTES + (uint64_t)lane * (WORDS * 4)) * P + k;
                        cnt = tc.finish_tail(tile, res[q], dst, P, lane);
                    } else {
#pragma unroll
                        for (int j = 0; j < WORDS; j++) cnt += __builtin_popcount(res[q][j]);
                    }
                    cnts[q] = cnt;
                }
            }
            if (s.hits) block_hits_add8(s_hits, pass * NK, P, cnts, lane);
            if (s.layout != 0 && full) {
                // linear: the 8 predicates of this pass are 8 consecutive bytes of every 8-value group: gather them with
                // 4x4 byte transposes (predicate-major words -> group-major bytes) and store 8 bytes per group
                const uint32_t nk = (P - pass * 8) < 8 ? (P - pass * 8) : 8;
                const uint64_t g0 = tile * G::BITMAP_BYTES + (uint64_t)lane * (WORDS * 4);
#pragma unroll
                for (int j = 0; j < WORDS; j++) {
                    const uint32_t r0[4] = {res[0][j], res[1][j], res[2][j], res[3][j]};
                    const uint32_t r1[4] = {res[4][j], res[5][j], res[6][j], res[7][j]};
                    uint32_t c0[4], c1[4];
                    transpose4x4_bytes(r0, c0);
                    transpose4x4_bytes(r1, c1);
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        uint8_t *dst = s.out + (g0 + 4 * j + b) * P + pass * 8;
                        if (nk == 8) {
                            store8_unaligned(dst, c0[b], c1[b]);
                        } else {
#pragma unroll
                            for (int q = 0; q < 8; q++)
                                if ((uint32_t)q < nk) dst[q] = (uint8_t)((q < 4 ? c0[b] : c1[b]) >> (8 * (q & 3)));
                        }
                    }
                }
            }
        }
        tile = next;
    }
    if (s.hits) block_hits_flush(s, s_hits, P);
    hits_finalize(s, P, lane);
}

} // namespace mi355
