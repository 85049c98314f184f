/* mi355_topk.h -- the k largest or smallest rows of a packed column, as a bitmap (part of the C ABI of libmi355scan.so).
 *
 * ORDER BY v [DESC] LIMIT k, and the order statistics that rest on the same step (the k-th largest value, a median, a
 * percentile), without decompressing anything: a radix select over the packed column.  The result is a bitmap, so it feeds
 * mi355_compact_dev, mi355_bitmap_to_rowids_dev, mi355_aggregate_dev, mi355_group_aggregate_dev and every fused-mask scan
 * unchanged; sorting the k survivors is not this call's business.  Plain C99, like mi355_scan.h; the context and the status codes
 * are that header's.
 */
#ifndef MI355_TOPK_H
#define MI355_TOPK_H

#include "mi355_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Over the qualifying rows Q -- the i < n whose bit is set in mask_dev, every row when mask_dev is NULL --, q = |Q|, m = min(k, q):
 * the call selects exactly the m rows that come first in the order "value descending (largest != 0) or ascending (largest == 0),
 * then row id ascending".  Ties at the cut go to the lowest row ids.
 *
 *   bitmap_dev  receives exactly ceil(n / 8) bytes: bit i is set iff row i is selected.  The bits >= n of the last byte are zero
 *               and the bytes behind keep their values (the bitmaps' tail rule).  4 bytes aligned.
 *   result_dev  four words, 8 bytes aligned:
 *               [0] = m;
 *               [1] = T, the value of the m-th row in that order: the threshold, and the k-th order statistic;
 *               [2] = the number of selected rows whose value lies strictly beyond T;
 *               [3] = the number of qualifying rows equal to T.  The cut went through ties iff [3] > [0] - [2].
 *               When m == 0 all four words are 0 and the bitmap is zero.
 *   widths      c is 1..32; n is any size, columns beyond 2^32 rows included; k is any uint64_t, k >= q selects Q.
 *   packed_dev  as everywhere: 16 bytes aligned, with the pad of mi355_compressed_buffer_size.  What lies behind row n - 1 never
 *               reaches a result, so row-range views work.
 *   mask_dev    NULL, or a canonical bitmap of n rows (bits >= n of its last byte zero), 4 bytes aligned, read up to ceil(n / 8)
 *               bytes and no further.
 *   aliasing    bitmap_dev == mask_dev exactly is allowed: the filter's bitmap is narrowed to its top k in place.  Any other
 *               overlap of bitmap_dev or result_dev with the mask's bytes, the column's bytes or each other is refused.
 *   n == 0      nothing is read, the four result words are zeroed; packed_dev, mask_dev and bitmap_dev may be NULL.
 *   result      every output byte is a function of the inputs only: the same call gives the same bytes.
 *   kernels     mi355_top_k_passes(c) rounds of topk_hist_kernel (a histogram of one digit of at most 12 bits, most significant
 *               first, over the rows that share the digits found so far) and topk_pick_kernel (one block: the digit in which the
 *               running count reaches what is left of k); then topk_emit_kernel writes mask AND (v beyond T OR v == T) and counts
 *               the rows equal to T per chunk of 16384 rows, rowid_scan_kernel turns the counts into prefixes, and
 *               topk_trim_kernel clears the ties whose rank in row order is not below [0] - [2].  That is
 *               mi355_top_k_passes(c) + 1 reads of the column; the trim reads it again only in chunks behind the cut that hold
 *               ties.  No block ever waits for another: the passes are separate launches in stream order.
 *   errors      MI355_E_INVALID, nothing launched, outputs untouched: c outside 1..32; bitmap_dev (n > 0) or result_dev NULL;
 *               packed_dev NULL (n > 0); a misaligned pointer; an output overlapping the column, or the mask other than
 *               bitmap_dev == mask_dev.
 *   stores      option "scan_nt_stores" (mi355_scan.h) governs topk_emit_kernel's bitmap stores: -1 (the default) write-through up to
 *               768 MiB of bitmap, non-temporal beyond; 0 plain.  1 non-temporal, 2 write-through.  The bytes never depend on it.
 *   stream     asynchronous on the context's stream, without a host round trip: threshold, remaining k and every decision stay
 *               on the device.  The call holds the context's lock like every other.
 *   record      mi355_ctx_last_launch names the kernels the call launched.
 *   graph capture: capturable after a warm-up call of at least this size -- the call takes the context's selection
 *   workspace, like mi355_compact_dev: (ceil(n / 16384) + 1 + ceil(n / 16777216) + 8 + 4096 * mi355_top_k_passes(c)) words,
 *   grown outside capture only.  Under capture a call that would have to grow it is refused with MI355_E_INVALID, the message
 *   names graph capture and the capture stays intact.  Column and mask are read at every replay: a graph of `scan, then top_k`
 *   follows the column's contents. */
MI355_API int mi355_top_k_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const void *mask_dev, uint64_t k, int largest,
                              void *bitmap_dev, uint64_t *result_dev);

/* histogram passes over the column the call above makes at width c (it reads the column once more to write the bitmap): 1 for
 * c = 1..12, 2 for 13..24, 3 for 25..32; 0 for a width the call would refuse.  Pure arithmetic: needs no device and no context. */
MI355_API unsigned mi355_top_k_passes(unsigned c);

#ifdef __cplusplus
}
#endif

#endif /* MI355_TOPK_H */
