// distinct/set_ranks.hpp -- the device code of mi355_set_ranks_dev: table[j] = the number of set bits below j where bit j of a
// bitmap set is set, else `miss`, packed at CT bits -- the table mi355_lookup_dev takes, so that value_set -> set_ranks -> lookup
// re-codes a column to dense codes.  gfx950 only; part of libmi355scan.so through distinct/set_ranks.hip.
//
// The chunk prefix over the set is the row ids' (kernels/bitmap.hpp: rowid_count_kernel, rowid_scan_kernel); set_ranks_kernel<CT>
// then deals a wave per chunk of kRowidChunk bytes = 16384 bits, in eight steps of 64 lanes x 32 bits.  A lane's word gets its base
// rank from the chunk's `before` (chunk_span_wave) plus the wave prefix of the popcounts; its 32 entries -- base + the popcount of
// the word's lower bits for a member, `miss` for a clear bit or a rank beyond CT bits -- are exactly CT whole dwords
// (rt_insert_all), stored whole (store_words_by) or, for the word that holds bit set_bits - 1, as the bytes its valid entries fill
// (rt_store_tail: trailing bits zero).  The set is read by bitmap_word_at's rule -- nothing behind byte ceil(set_bits / 8) - 1 -- and
// the bits >= set_bits of the last word are cut before anything is counted.  rowid_count_kernel does count those bits: they sit in
// the last chunk and move only its count and the total, which nothing here reads -- no chunk's `before`.
// The two output words are the kernel's own sums: members below set_bits, and members whose rank did not fit -- per lane over the
// wave's chunks, then one atomic per wave.
#pragma once

#include "../kernels.hpp"
#include "../kernels/rt_column.hpp"

namespace mi355 {

struct SetRanksArgs {
    const uint8_t *set;                 // bitmap format, 4 B aligned; nbytes = ceil(set_bits / 8) bytes are read and no more
    uint64_t set_bits, nbytes;
    unsigned long long *chunk_counts;   // the chunk prefix as rowid_scan_kernel leaves it
    uint64_t nchunks;
    uint8_t *table;                     // 16 B aligned
    unsigned long long *out;            // {members, members whose rank did not fit}, zeroed in front of the launch
    uint32_t miss;
    uint32_t nts;                       // store policy of the whole tiles (one_pass_store_policy)
};

template <int CT> __global__ __launch_bounds__(kBlockThreads) void set_ranks_kernel(SetRanksArgs g)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const ChunkPrefix prefix{g.chunk_counts, g.nchunks};
    constexpr unsigned long long kRanks = CT >= 32 ? (1ull << 32) : (1ull << (CT & 31)); // the ranks CT bits hold
    const uint32_t miss = g.miss;
    unsigned long long members = 0, unfit = 0;
    for (uint64_t ch = wave; ch < g.nchunks; ch += nwaves) {
        unsigned long long run = chunk_span_wave(prefix, ch, lane).before; // members before this chunk
#pragma unroll 1
        for (int k = 0; k < kRowidChunk / (64 * 4); k++) {
            const uint64_t word = ch * (kRowidChunk / 4) + (uint64_t)(k * 64 + lane); // the lane's word of the set
            const uint64_t first = word * 32;                                         // its bit 0
            const int valid = first >= g.set_bits ? 0 : (g.set_bits - first >= 32 ? 32 : (int)(g.set_bits - first));
            const uint32_t w = valid ? bitmap_word_at(g.set, g.nbytes, word * 4) & tail_mask(valid, 0) : 0u;
            const uint32_t cnt = __builtin_popcount(w);
            const uint32_t incl = wave_inclusive_scan(cnt);
            const unsigned long long base = run + (incl - cnt); // rank of the word's first member
            run += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            members += cnt;
            // ranks ascend inside the word: the members at base + i >= kRanks are the last ones
            const unsigned long long over = base + cnt > kRanks ? base + cnt - kRanks : 0ull;
            unfit += over < cnt ? over : cnt;
            if (valid) {
                uint32_t x[kRtVpl];
#pragma unroll
                for (int b = 0; b < kRtVpl; b++) {
                    const unsigned long long rank = base + (uint32_t)__builtin_popcount(w & ((1u << b) - 1u));
                    x[b] = ((w >> b) & 1u) && rank < kRanks ? (uint32_t)rank : miss;
                }
                uint32_t r[CT];
                rt_insert_all<CT>(r, x);
                uint8_t *const dst = g.table + word * (4ull * CT);
                if (valid == 32)
                    store_words_by<CT>(dst, r, g.nts);
                else
                    rt_store_tail<CT>(dst, r, valid);
            }
        }
    }
    const unsigned long long m = wave_sum64(members), u = wave_sum64(unfit);
    if (lane == 0 && m) __hip_atomic_fetch_add(g.out, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lane == 0 && u) __hip_atomic_fetch_add(g.out + 1, u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

} // namespace mi355
