/* mi355_sort.h -- the row ids of a packed column in value order (part of the C ABI of libmi355scan.so).
 *
 * ORDER BY v [DESC], the first step of a sort-based GROUP BY or a sort-merge join, and -- behind mi355_top_k_dev -- the order of
 * the k survivors of ORDER BY v LIMIT k, without decompressing anything: a stable radix sort over the packed values whose passes
 * follow the column's width, not a 32-bit key.  The result is what mi355_gather_dev takes (row ids and a device count), so it
 * composes with mi355_top_k_dev, mi355_bitmap_to_rowids_dev, mi355_gather_dev and mi355_compact_dev without a host round trip.
 * Plain C99, like mi355_scan.h; the context and the status codes are that header's.
 */
#ifndef MI355_SORT_H
#define MI355_SORT_H

#include "mi355_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Over the qualifying rows Q -- the i < n whose bit is set in mask_dev, every row when mask_dev is NULL --, q = |Q|: the call
 * orders Q by "value ascending (descending == 0) or descending, then row id ascending" -- a stable sort, top_k's order -- into
 * i_0, i_1, ..., i_(q-1).
 *
 *   count_dev   one word, 8 bytes aligned: count_dev[0] = q, always.
 *   rowids_dev  `capacity` entries, 8 bytes aligned.  ALL OR NOTHING: when q <= capacity, rowids_dev[j] = first_row + i_j for
 *               j < q and the entries at index >= q keep their bytes; when q > capacity NOTHING is written to rowids_dev or
 *               values_dev, and the caller sees count_dev[0] > capacity.  (mi355_bitmap_to_rowids_dev truncates instead; a
 *               truncated sort would still need workspace for all q rows.)  ORDER BY ... LIMIT k is mi355_top_k_dev, then this
 *               call under its bitmap with capacity = k.  May be NULL when capacity == 0: the call then only counts.
 *   values_dev  NULL, or `capacity` entries, 4 bytes aligned: values_dev[j] = the value of row i_j, under the same rule.
 *   first_row   any uint64_t: added to every row id (the view's first row in a longer column).
 *   size        n <= 2^32 rows -- a row index inside the view fits 32 bits, so an item in flight is 64 bits; c is 1..32.
 *   packed_dev  as everywhere: 16 bytes aligned, with the pad of mi355_compressed_buffer_size.  What lies behind row n - 1 never
 *               reaches a result, so row-range views work.
 *   mask_dev    NULL, or a bitmap of n rows, 4 bytes aligned, read up to ceil(n / 8) bytes and no further; the bits >= n of its
 *               last byte, and whatever bytes lie behind it, never reach a result.
 *   n == 0      count_dev[0] = 0, nothing is read; packed_dev, mask_dev, rowids_dev and values_dev may be NULL.
 *   result      every output byte is a function of the inputs only: the same call gives the same bytes, whatever the grid
 *               (options "grid_cus", "max_blocks_per_cu").
 *   kernels     a stable least-significant-digit radix sort with 8-bit digits; the top digit takes what is left, so a call makes
 *               mi355_sort_rows_passes(c) = ceil(c / 8) passes.  The input of a pass is cut into spans of 16384 rows, whatever
 *               the grid.  A pass is: sort_count_kernel (pass 0: the packed column and the mask) or sort_item_count_kernel (the
 *               64-bit items of the pass before) counts every span's qualifying rows per digit value; rowid_scan_kernel and
 *               sort_offsets_kernel turn the counters, digit-major, into ranks -- the total of pass 0 is q --; sort_scatter_kernel
 *               or sort_item_scatter_kernel walks the spans again and puts every row at the rank of (its digit, its span) + the
 *               rows of the same digit in front of it in the span -- 2048 rows at a time through a stage in LDS, so that a digit's
 *               rows leave side by side, or straight to their places where a pass has at most 8 buckets or a tile fewer than 1024
 *               qualifying rows; the bytes are the same either way.  The last pass writes rowids_dev and values_dev, the others
 *               64-bit items (key, row index) into the workspace.  That is 2 reads of the column and 2 (passes - 1) of the
 *               items from memory (a staged scatter reads its 2048 items a second time, from the cache).  A descending sort
 *               orders the value's complement within c bits.  No block ever waits for another: the steps are separate launches
 *               in stream order.
 *   errors      MI355_E_INVALID, nothing launched, outputs untouched: c outside 1..32; n > 2^32; rowids_dev NULL with
 *               capacity > 0 and n > 0; count_dev NULL; packed_dev NULL (n > 0); a misaligned pointer; any overlap of
 *               rowids_dev, values_dev or count_dev with the column, the mask or each other.
 *   stream      asynchronous on the context's stream, without a host round trip: q and every decision stay on the device.  The
 *               call holds the context's lock like every other.
 *   record      mi355_ctx_last_launch names the kernels the call launched.
 *   graph capture: capturable after a warm-up call of at least this size -- the call takes the context's selection
 *   workspace, like mi355_compact_dev: mi355_sort_rows_workspace_words(n, capacity, c) words, grown outside capture only.  Under
 *   capture a call that would have to grow it is refused with MI355_E_INVALID, the message names graph capture and the capture
 *   stays intact.  Column and mask are read at every replay: a graph of `scan, then sort_rows` follows the column's contents. */
MI355_API int mi355_sort_rows_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const void *mask_dev, int descending,
                                  uint64_t first_row, uint64_t *rowids_dev, uint32_t *values_dev, uint64_t capacity, uint64_t *count_dev);

/* passes the call above makes at width c: 1 for c = 1..8, 2 for 9..16, 3 for 17..24, 4 for 25..32; 0 for a width the call would
 * refuse.  Pure arithmetic: needs no device and no context. */
MI355_API unsigned mi355_sort_rows_passes(unsigned c);

/* 64-bit words of the selection workspace the call above takes: the counters of the widest pass (2^min(c, 8) per span of 16384
 * rows of n) with their prefix, 8 words of state, and min(passes - 1, 2) item buffers of min(capacity, n) words each -- sized by
 * the capacity, not by n: sorting the 1e6 survivors of a 1e9-row top_k takes the counters and 8 MB per item buffer.  A one-pass width needs no
 * item buffer.  0 for n == 0 and for arguments the call would refuse.  Pure arithmetic. */
MI355_API uint64_t mi355_sort_rows_workspace_words(uint64_t n, uint64_t capacity, unsigned c);

#ifdef __cplusplus
}
#endif

#endif /* MI355_SORT_H */
