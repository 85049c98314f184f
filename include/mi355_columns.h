/* mi355_columns.h -- predicates that compare two packed columns row by row (part of the C ABI of libmi355scan.so).
 *
 * Every predicate of mi355_scan.h compares a row's value with a constant.  The call below compares a row of one column
 * with the same row of another -- `l_commitdate < l_receiptdate`, `receipt >= ship + 30`, `|a - b| <= 3`, `a == b` --
 * in one kernel launch that reads both packed columns once and decompresses neither.  Plain C99, like mi355_scan.h; the
 * context, status codes, MI355_CMP_* and MI355_BITMAP_* are that header's.
 */
#ifndef MI355_COLUMNS_H
#define MI355_COLUMNS_H

#include "mi355_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* For row i let d_i = v1_i - v2_i, the exact integer difference of the two decoded (unsigned) values: d_i lies in
 * [-(2^c2 - 1), 2^c1 - 1], inside [-(2^32 - 1), 2^32 - 1].
 *   p[i]      = (d_i OP a [, b])         OP: MI355_CMP_EQ .. MI355_CMP_NOT_BETWEEN; a, b any int64, compared exactly
 *   bitmap[i] = mask_dev ? COMBINE(p[i], mask[i]) : p[i]      mask_op as in mi355_scan_combine_dev
 * col1 < col2 is (MI355_CMP_LT, 0); col1 >= col2 + 30 is (MI355_CMP_GE, 30); |col1 - col2| <= 3 is (MI355_CMP_BETWEEN, -3, 3).
 * A constant outside the domain of d compares as what it is: BETWEEN 7 AND 3 matches nothing, NOT BETWEEN 7 AND 3 every
 * row; d < INT64_MIN matches nothing, d <= INT64_MAX every row; widths 31 and 32 included (the comparison is made in 64
 * bits there).
 *
 * packed1_dev / packed2_dev: columns of n rows and c1 / c2 bits (1..32, any pair, one launch), 16-byte aligned, with the
 * pad mi355_compressed_buffer_size gives; they may be the same buffer.
 * Everything else is the contract of mi355_scan_combine_dev: exactly ceil(n/8) bytes of bitmap are written, bits >= n are
 * zero; hits_dev is nullable; bitmap_dev == NULL is a count-only scan; mask_dev (nullable, >= ceil(n/8) bytes) may be
 * bitmap_dev itself (in place); mask_dev and bitmap_dev are 16-byte aligned; n == 0 stores a zero hit count and launches
 * nothing; both outputs NULL is MI355_E_INVALID.
 *   errors (MI355_E_INVALID, nothing launched, outputs untouched): op outside MI355_CMP_EQ .. MI355_CMP_NOT_BETWEEN,
 *   mask_op outside MI355_BITMAP_AND .. MI355_BITMAP_ANDNOT, a width outside 1..32, a misaligned or null column.
 *   stores  option "scan_nt_stores" (mi355_scan.h) governs the bitmap stores: -1 (the default) write-through up to 768 MiB of
 *   bitmap, non-temporal beyond; 0 plain.  1 non-temporal, 2 write-through.  The bytes never depend on it.
 *   graph capture: capturable -- the call enqueues one kernel on the context's stream; it uploads nothing, takes no buffer
 *   of the context's pool and never synchronises, whatever its arguments. */
MI355_API int mi355_scan_columns_dev(mi355_ctx *ctx, const void *packed1_dev, unsigned c1, const void *packed2_dev, unsigned c2,
                                     uint64_t n, int op, int64_t a, int64_t b, int mask_op, const void *mask_dev,
                                     void *bitmap_dev, uint64_t *hits_dev);

#ifdef __cplusplus
}
#endif

#endif /* MI355_COLUMNS_H */
