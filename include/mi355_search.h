/* mi355_search.h -- the positions of a packed column's rows in a sorted packed table (part of the C ABI of libmi355scan.so).
 *
 * Every other join and grouping call addresses its table by the key itself and so needs a dense key domain.  This call addresses
 * a table by ORDER: for every row of a packed column its position in a sorted packed table (numpy.searchsorted), as a packed
 * column, plus a bitmap of the rows whose value occurs in the table.  That is the join on sparse keys (mi355_sort_rows_dev on the
 * dimension's keys, this call with `exact`, then mi355_lookup_dev), binning by arbitrary edges (positions under
 * MI355_SEARCH_RIGHT, then mi355_group_aggregate_dev), `fk IN (sparse set)` (the bitmap alone), a percentile rank, and the probe
 * step of a sort-merge join.  Packed in, packed out: nothing is decompressed.  Plain C99, like mi355_scan.h; the context and the
 * status codes are that header's.
 */
#ifndef MI355_SEARCH_H
#define MI355_SEARCH_H

#include "mi355_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI355_SEARCH_LEFT  0   /* pos_i = number of j < R with t_j <  x_i  (lower bound) */
#define MI355_SEARCH_RIGHT 1   /* pos_i = number of j < R with t_j <= x_i  (upper bound) */

/* bytes of LDS a block's copy of the table (one uint32 per entry) or of its samples may take: 160 KiB minus the block's input
 * images at the widest width (4 waves x 2 x 8 KiB at c = 32) minus 64 bytes of bookkeeping, in whole 16 bytes. */
#define MI355_SEARCH_LDS_MAX_BYTES 98240

/* x_i: row i of packed_dev (n rows of c bits); t_j: entry j of table_dev, a packed column of ct bits, non-decreasing over
 * [0, R).  Values compare as unsigned 32-bit integers for any pair of widths, c < ct and c > ct included.
 *
 *   R           `rows`, or min(rows, *rows_dev) when rows_dev (a nullable device uint64, naturally aligned) is given: it is read
 *               on the device, as mi355_run_decode_dev reads its run count, so mi355_sort_rows_dev, mi355_run_encode_dev or
 *               mi355_value_set_dev -> this call never touches the host.  rows <= 2^32 - 1.  R == 0: pos_i = 0 for every row,
 *               nothing is found, and the table is not read; with rows == 0 table_dev may be NULL.
 *   found_i     true exactly when the search ends beside an equal entry: under MI355_SEARCH_LEFT pos_i < R and
 *               t[pos_i] == x_i, under MI355_SEARCH_RIGHT pos_i > 0 and t[pos_i - 1] == x_i.  On a sorted table: x_i occurs
 *               in t.
 *   outputs     out_dev (nullable): a packed column of n values of co bits, out_i = pos_i, or with exact != 0
 *               out_i = found_i ? pos_i : miss.  It requires rows <= 2^co - 1, and miss < 2^co when co < 32.
 *               found_dev (nullable): the bitmap of found_i over the n rows.
 *               hits_dev (nullable): a device uint64, naturally aligned, overwritten with the number of found rows.  It is zeroed
 *               on the stream in front of the kernel, whose waves add to it, one integer atomic each: the count is
 *               deterministic.
 *               At least one of the three must be given (n > 0).  Without out_dev, co must still be a width and names the instance.
 *   widths      c, ct and co are 1..32, in any combination.
 *   bytes       exactly ceil(n co / 8) bytes of out_dev are written, the bits behind value n - 1 in the last byte zero; exactly
 *               ceil(n / 8) bytes of found_dev, the bits >= n of the last byte zero.  Nothing behind either is touched.
 *   packed_dev  as everywhere: 16 bytes aligned, with the pad of mi355_compressed_buffer_size.  What lies behind row n - 1
 *               reaches nothing, so row-range views work.
 *   tables      table_dev is read where it lies, as mi355_lookup.h's global tier reads its table: 4 bytes aligned, dwords 0 up
 *               to the one that holds the last bit of entry R - 1 and no more.  The bits of that dword behind entry R - 1, and
 *               everything after, may hold anything.  The table is read, never written.
 *   unsorted    a table that is not sorted: every pos_i still lies in [0, R], found_i is set only where the named entry really
 *               equals x_i, and nothing outside entries [0, R) is read.
 *   alignment   out_dev 16 bytes, found_dev 4 bytes, rows_dev and hits_dev 8 bytes.
 *   aliasing    none: none of out_dev, found_dev and the 8 bytes of hits_dev may overlap the column (its ceil(n c / 8) bytes),
 *               the table (the whole dwords of its `rows` entries), the 8 bytes of rows_dev, or one another.
 *   kernels     rows * 4 <= MI355_SEARCH_LDS_MAX_BYTES: search_lds_kernel -- every block decodes entries [0, R) once into LDS
 *               as uint32, then a branchless descent in power-of-two steps, one LDS read per step and row.  Larger tables:
 *               search_global_kernel -- every block stages the samples t[(k + 1) S - 1], S = mi355_search_sorted_stride(rows),
 *               the steps >= S of the same descent read those, the log2 S steps below S read the table where it lies (L2 /
 *               Infinity Cache).
 *   n == 0      nothing is launched; *hits_dev = 0; packed_dev, out_dev and found_dev are not touched and may be NULL, all three
 *               results together included: an empty column has an empty answer.
 *   errors      MI355_E_INVALID, nothing launched, outputs untouched: c, ct or co outside 1..32; side neither
 *               MI355_SEARCH_LEFT nor MI355_SEARCH_RIGHT; rows > 2^32 - 1; with out_dev rows > 2^co - 1, or miss >= 2^co when
 *               co < 32; with n > 0 out_dev, found_dev and hits_dev all NULL; a misaligned pointer; with n > 0 packed_dev NULL; with
 *               rows > 0 table_dev NULL; any overlap named above.
 *   stores      option "scan_nt_stores" (mi355_scan.h) governs the stores to out_dev and found_dev alike: -1 (the default)
 *               write-through up to 768 MiB of positions and bitmap together, non-temporal beyond; 0 plain.  1 non-temporal,
 *               2 write-through.  The bytes never depend on it.
 *   stream     asynchronous on the context's stream; the call holds the context's lock like every other.
 *   record      mi355_ctx_last_launch names the kernel the call launched.
 *   graph capture: capturable -- the call enqueues its one kernel on the context's stream and, when a counter is given, the
 *   8-byte zeroing of hits_dev in front of it; it uploads nothing, takes no buffer of the context's pool, no scratch of the
 *   context's and never synchronises, whatever its arguments, and needs no warm-up call.  Column, table and *rows_dev are read at
 *   every replay. */
MI355_API int mi355_search_sorted_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const void *table_dev, unsigned ct,
                                      uint64_t rows, const uint64_t *rows_dev, int side, int exact, uint32_t miss, void *out_dev, unsigned co,
                                      void *found_dev, uint64_t *hits_dev);

/* kernel family the call above would launch: "search_lds_kernel" | "search_global_kernel"; NULL for what the call would refuse
 * whatever its buffers (a width outside 1..32, rows > 2^32 - 1).  Pure arithmetic: needs no device and no context. */
MI355_API const char *mi355_search_sorted_kernel(unsigned c, unsigned ct, unsigned co, uint64_t rows);

/* S, the distance of the samples a block keeps in LDS: the smallest power of two with floor(rows / S) * 4 <=
 * MI355_SEARCH_LDS_MAX_BYTES; 1 in the LDS tier (every entry is a sample).  Pure arithmetic. */
MI355_API uint64_t mi355_search_sorted_stride(uint64_t rows);

#ifdef __cplusplus
}
#endif

#endif /* MI355_SEARCH_H */
