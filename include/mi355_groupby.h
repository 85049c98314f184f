/* mi355_groupby.h -- grouped aggregates over two packed columns (part of the C ABI of libmi355scan.so).
 *
 * mi355_aggregate_dev (mi355_scan.h) reduces one column to one sum / count / min / max, mi355_histogram_dev counts the rows
 * per value of one column.  The call below ends the query `SELECT g, sum(v), count(*), min(v), max(v) FROM t WHERE <bitmap>
 * GROUP BY g`, with g one dictionary-coded column and v another: both packed columns are read once, neither is
 * decompressed, no per-group bitmap is written.  Plain C99, like mi355_scan.h; the context and the status codes are that
 * header's.
 */
#ifndef MI355_GROUPBY_H
#define MI355_GROUPBY_H

#include "mi355_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI355_GROUP_MAX_KEY_BITS 12 /* 2^12 groups: their sums, counts, minima and maxima live in the LDS of a CU */

/* per group g in [0, 2^ck): out_dev[4*g + 0] = sum, [1] = count, [2] = min, [3] = max of values_i over the rows i < n with
 * keys_i == g (and mask bit i set, when mask_dev is given).  Values and keys are the unsigned decoded integers.  A group
 * with no row: sum 0, count 0, min UINT64_MAX, max 0 -- the empty result of mi355_aggregate_dev.  sum is exact modulo 2^64.
 *
 *   widths      ck is 1..MI355_GROUP_MAX_KEY_BITS (12), cv is 1..32, any pair: one aggregation launch behind a tiny launch
 *               that sets out_dev to the empty result, as mi355_aggregate_dev does.  ck above 12 is MI355_E_INVALID.
 *   same buffer keys_dev and values_dev may be the same buffer when ck == cv.
 *   alignment   keys_dev / values_dev: 16 bytes, each with the pad mi355_compressed_buffer_size gives.  What lies behind
 *               row n - 1 may be anything and never reaches a result: both may be row-range views into longer columns.
 *               mask_dev: nullable (every row counts), a canonical bitmap, 4 bytes, read up to ceil(n/8) bytes and no further.
 *               out_dev: 8 bytes, 4 * 2^ck uint64, overwritten completely by every successful call.
 *   n == 0      out_dev gets the empty result for every group; no aggregation kernel runs (keys_dev / values_dev may be NULL).
 *   errors      MI355_E_INVALID, nothing launched, out_dev untouched: a width out of range; keys_dev or values_dev NULL
 *               with n > 0 (count(*) per value of ONE column is mi355_histogram_dev); out_dev NULL; a misaligned pointer.
 *   stream      asynchronous on the context's stream; the call holds the context's lock like every other.
 *   record      mi355_ctx_last_launch names the kernels the call enqueued.
 *   graph capture: capturable -- the call enqueues its two kernels on the context's stream; it uploads nothing, takes no
 *   buffer of the context's pool and never synchronises, whatever its arguments. */
MI355_API int mi355_group_aggregate_dev(mi355_ctx *ctx, const void *keys_dev, unsigned ck, const void *values_dev, unsigned cv,
                                        uint64_t n, const void *mask_dev, uint64_t *out_dev);

#ifdef __cplusplus
}
#endif

#endif /* MI355_GROUPBY_H */
