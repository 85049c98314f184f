/* mi355_groupby_wide.h -- grouped aggregates for keys beyond 12 bits (part of the C ABI of libmi355scan.so).
 *
 * mi355_group_aggregate_dev (mi355_groupby.h) keeps every group's state in the LDS of a CU and therefore stops at 2^12 groups.
 * The call below ends the same query -- `SELECT g, sum(v), count(*), min(v), max(v) FROM t WHERE <bitmap> GROUP BY g` -- for a
 * DENSE key domain of up to 2^26 groups: the composite key `g1 * |g2| + g2` that mi355_arith_dev (mi355_arith.h) builds from
 * two dictionary columns, a looked-up attribute (mi355_lookup.h) with ten thousand values.  The result table lives in device
 * memory; each block keeps a first-come front of it in LDS, so the frequent keys of a block cost LDS atomics and only the
 * rest goes to memory row by row.  Both packed columns are read once, neither is decompressed.  Plain C99, like mi355_scan.h;
 * the context and the status codes are that header's.
 */
#ifndef MI355_GROUPBY_WIDE_H
#define MI355_GROUPBY_WIDE_H

#include "mi355_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI355_GROUP_WIDE_MAX_GROUPS 67108864 /* 2^26: 2 GiB of result */

/* per group g in [0, groups): out_dev[4*g + 0] = sum, [1] = count, [2] = min, [3] = max of values_i over the rows i < n with
 * keys_i == g (and mask bit i set, when mask_dev is given).  Values and keys are the unsigned decoded integers.  A group
 * with no row: sum 0, count 0, min UINT64_MAX, max 0 -- the layout and the empty result of mi355_group_aggregate_dev.  sum is
 * exact modulo 2^64.
 *
 *   widths      ck and cv are 1..32, any pair.
 *   groups      1 <= groups <= min(2^ck, MI355_GROUP_WIDE_MAX_GROUPS); it need not be a power of two (a composite key has
 *               |g1| * |g2| groups).
 *   out-of-domain keys  a counted row whose key is >= groups reaches no group: the `miss` of mi355_arith_dev, a dictionary's
 *               null code, 0xffffffff at ck = 32.  dropped_dev: nullable device uint64 (8 bytes aligned); when given, every
 *               successful call writes the number of such rows there (0 when there are none).  Rows >= n and rows the mask
 *               leaves out are counted nowhere.
 *   same buffer keys_dev and values_dev may be the same buffer when ck == cv.
 *   alignment   keys_dev / values_dev: 16 bytes, each with the pad mi355_compressed_buffer_size gives.  What lies behind
 *               row n - 1 may be anything and never reaches a result: both may be row-range views into longer columns.
 *               mask_dev: nullable (every row counts), a canonical bitmap, 4 bytes, read up to ceil(n/8) bytes and no further.
 *               out_dev: 8 bytes, 4 * groups uint64, overwritten completely by every successful call.
 *   n == 0      out_dev gets the empty result for every group and *dropped_dev 0; only the init kernel runs (keys_dev /
 *               values_dev may be NULL).
 *   errors      MI355_E_INVALID, nothing launched, out_dev and *dropped_dev untouched: a width out of range; groups == 0;
 *               groups > 2^ck; groups > MI355_GROUP_WIDE_MAX_GROUPS; keys_dev or values_dev NULL with n > 0; out_dev NULL;
 *               a misaligned pointer.
 *   stream      asynchronous on the context's stream; the call holds the context's lock like every other.
 *   record      mi355_ctx_last_launch names the kernels the call enqueued: group_aggregate_wide_init_kernel (the empty results,
 *               the zero in *dropped_dev) and group_aggregate_wide_kernel.
 *   graph capture: capturable -- the call enqueues its two kernels on the context's stream and nothing else: no memset node, no
 *   upload, no buffer of the context's pool, and it never synchronises, whatever its arguments.  Both columns and the mask are
 *   read at every replay. */
MI355_API int mi355_group_aggregate_wide_dev(mi355_ctx *ctx, const void *keys_dev, unsigned ck, const void *values_dev, unsigned cv,
                                             uint64_t n, const void *mask_dev, uint64_t groups, uint64_t *out_dev, uint64_t *dropped_dev);

/* slots of the LDS front a block of the call above keeps at these widths: 4096, 2048 or 1024, the most that fit a CU's LDS next
 * to the waves' tiles of both columns; 0 for a width outside 1..32.  Pure arithmetic: needs no device and no context. */
MI355_API uint32_t mi355_group_wide_front_slots(unsigned ck, unsigned cv);

#ifdef __cplusplus
}
#endif

#endif /* MI355_GROUPBY_WIDE_H */
