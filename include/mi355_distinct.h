/* mi355_distinct.h -- the set of values that occur in a packed column, as a bitmap over the value domain, and the rank of every
 * member among the members, as a packed table (part of the C ABI of libmi355scan.so).
 *
 * The producer the set consumers lacked: mi355_semijoin_dev takes a bitmap set, and until now only a scan over a dimension table
 * whose row number is the key wrote one.  mi355_value_set_dev writes it from any column -- `a IN (SELECT b FROM other WHERE ...)`
 * is value_set(b, mask) -> semijoin(a), INTERSECT / EXCEPT of two columns' values is mi355_bitmap_combine_dev on two sets,
 * count(DISTINCT v) is the first output word, SELECT DISTINCT v is mi355_bitmap_to_rowids_dev over the set (ascending).
 * mi355_set_ranks_dev turns the set into the table mi355_lookup_dev takes: value_set -> set_ranks -> lookup re-codes a column to
 * dense codes 0 .. d - 1 at the narrowest width (a sparse key for mi355_group_aggregate_wide_dev), and the row ids of the set decode
 * them.  Plain C99, like mi355_scan.h; the context and the status codes are that header's.
 */
#ifndef MI355_DISTINCT_H
#define MI355_DISTINCT_H

#include "mi355_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* largest reach min(set_bits, 2^c), in bits, that a block of mi355_value_set_dev keeps as a bitset in the LDS of its CU: 64 KiB,
 * what mi355_histogram_dev keeps of counters next to its tiles.  Every column of up to 19 bits stays below it with its full domain. */
#define MI355_VALUE_SET_LDS_MAX_BITS 524288

/* set bit v of set_dev for every row i < n that mask_dev selects (every row when NULL) whose unsigned value v_i < set_bits.
 *
 *   set         set_dev is in the bitmap format mi355_semijoin_dev reads: bit j is byte j / 8, bit j % 8.  set_bits is 0 .. 2^32; it
 *               may be smaller or larger than 2^c (bits at 2^c and above are unreachable and stay clear).  set_dev: 4 bytes
 *               aligned, NULL only when set_bits == 0; the memory must be writable in whole dwords, through byte
 *               4 * ceil(set_bits / 32) - 1.
 *               accumulate == 0: exactly ceil(set_bits / 8) bytes are overwritten; bits >= set_bits of the last byte become zero,
 *               so mi355_bitmap_count_dev over the result is right.  Bytes beyond ceil(set_bits / 8) keep their contents (those of
 *               the last dword may be the target of an atomic OR of zero).
 *               accumulate != 0: the call only ORs into what is there -- the union over several columns, shards or calls; bits
 *               >= set_bits are left as they were.
 *   rows        packed_dev: 16 bytes aligned, with the pad of mi355_compressed_buffer_size.  mask_dev: nullable, a bitmap over the
 *               n rows, 4 bytes aligned, read up to ceil(n / 8) bytes and no further; bits >= n of its last byte may hold anything
 *               (the rules of mi355_top_k_dev).  What lies behind row n - 1 never reaches the set, neither pad bytes nor mask bits
 *               >= n, so row-range views work.  n == 0 reads nothing; with accumulate == 0 it still clears the set, and it writes
 *               {0, 0}.  set_bits == 0 writes no set byte and counts every selected row as outside.
 *   outputs     out_dev: required, 8 bytes aligned, two words.  out_dev[0] = the number of bits this call turned from 0 to 1 --
 *               with accumulate == 0 the number of distinct qualifying values below set_bits.  out_dev[1] = the number of selected
 *               rows whose value is >= set_bits; they set nothing (the "outside" of mi355_group_aggregate_wide_dev).  Both are
 *               exact and independent of the grid: every 0 -> 1 transition is seen by exactly one atomic OR, in the old word it
 *               returns.
 *   kernels     min(set_bits, 2^c) <= MI355_VALUE_SET_LDS_MAX_BITS: value_set_lds_kernel -- every block keeps the reachable part of
 *               the set as a bitset in LDS and merges its non-zero words into set_dev at its end.  Larger: value_set_global_kernel
 *               -- per value a test of the set's word where it lies, an atomic OR only where the bit is missing; gather-bound.
 *   errors      MI355_E_INVALID, nothing launched, nothing written: c outside 1..32; set_bits > 2^32; packed_dev NULL (n > 0);
 *               set_dev NULL with set_bits > 0; out_dev NULL; a misaligned pointer; the set's bytes [set_dev, set_dev +
 *               ceil(set_bits / 8)) overlapping the column, the mask or out_dev.
 *   stream      asynchronous on the context's stream; the call holds the context's lock like every other.
 *   record      mi355_ctx_last_launch names the kernel the call launched.
 *   graph capture: capturable -- whatever its arguments: the clear is a memset node, the counts are zeroed on the stream, then
 *   the one kernel; no workspace of the context is used and nothing synchronises.  Column and mask are read at every replay. */
MI355_API int mi355_value_set_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const void *mask_dev, void *set_dev,
                                  uint64_t set_bits, int accumulate, uint64_t *out_dev);

/* kernel family the call above would launch: "value_set_lds_kernel" | "value_set_global_kernel"; NULL for c outside 1..32 or
 * set_bits > 2^32.  Pure arithmetic: needs no device and no context. */
MI355_API const char *mi355_value_set_kernel(unsigned c, uint64_t set_bits);

/* table[j] = the number of set bits below j if bit j of the set is set, else miss, for every j < set_bits, packed at ct bits.
 *
 *   set         set_dev as above, read only: 4 bytes aligned, NULL only when set_bits == 0, set_bits 0 .. 2^32.  Bits >= set_bits
 *               of the last byte and everything behind byte ceil(set_bits / 8) - 1 may hold anything: they never reach a result
 *               and the bytes behind are never read.
 *   outputs     table_dev: 16 bytes aligned; exactly ceil(set_bits * ct / 8) bytes are written, the trailing bits of the last
 *               byte zero.  It is a packed buffer of mi355_compressed_buffer_size(ct, set_bits) bytes: what mi355_lookup_dev takes
 *               as table_dev with table_rows = set_bits.  ct is 1..32 and miss < 2^ct; a member whose rank does not fit ct bits
 *               gets miss.  out_dev: required, 8 bytes aligned, two words: out_dev[0] = the number of set bits below set_bits,
 *               out_dev[1] = the number of members whose rank did not fit.  set_bits == 0 writes no table byte and gives {0, 0}.
 *   kernels     the chunk counts and their prefix are those of mi355_bitmap_to_rowids_dev (rowid_count_kernel, rowid_scan_kernel);
 *               set_ranks_kernel then writes the table, a wave per 16384 bits of the set.
 *   errors      MI355_E_INVALID, nothing launched, nothing written: ct outside 1..32; miss >= 2^ct; set_bits > 2^32; set_dev or
 *               table_dev NULL with set_bits > 0; out_dev NULL; a misaligned pointer; the set's bytes overlapping the table's, or
 *               out_dev overlapping either.
 *   stores      option "scan_nt_stores" (mi355_scan.h) governs set_ranks_kernel's stores to table_dev: -1 (the default) write-through
 *               up to 768 MiB of table, non-temporal beyond; 0 plain.  1 non-temporal, 2 write-through.  The bytes never depend on it.
 *   stream     asynchronous on the context's stream; the call holds the context's lock like every other.
 *   record      mi355_ctx_last_launch names the three kernels the call launched.
 *   graph capture: capturable after a warm-up call of at least the same set_bits -- the call takes the context's selection
 *   workspace, like mi355_compact_dev: (ceil(set_bits / 16384) + 1 + ceil(set_bits / 16777216)) words, grown outside capture
 *   only.  Under capture a call that would have to grow it is refused with MI355_E_INVALID, the message names graph capture and the
 *   capture stays intact.  The set is read at every replay: a graph of `value_set, set_ranks, lookup` follows the column's
 *   contents. */
MI355_API int mi355_set_ranks_dev(mi355_ctx *ctx, const void *set_dev, uint64_t set_bits, unsigned ct, uint32_t miss, void *table_dev,
                                  uint64_t *out_dev);

#ifdef __cplusplus
}
#endif

#endif /* MI355_DISTINCT_H */
