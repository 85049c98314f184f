/* mi355_arith.h -- a packed column computed row by row from two others (part of the C ABI of libmi355scan.so).
 *
 * The step between the calls that filter, map and shrink packed columns and the calls that aggregate them: the composite key
 * `a * |b| + b` of `GROUP BY a, b` for mi355_group_aggregate_dev (mi355_groupby.h), the product column under
 * `sum(l_extendedprice * l_discount)` for mi355_aggregate_dev, the difference `receipt - ship` as a column for
 * mi355_histogram_dev or mi355_lookup_dev (mi355_lookup.h).  Packed in, packed out: nothing is decompressed.  Plain C99,
 * like mi355_scan.h; the context and the status codes are that header's.
 */
#ifndef MI355_ARITH_H
#define MI355_ARITH_H

#include "mi355_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI355_ARITH_LINEAR 0 /* r = a*x + b*y + k            */
#define MI355_ARITH_MUL    1 /* r = a*x*y + k   (b must be 0) */

/* out_i = (0 <= r_i < 2^co) ? r_i : miss,  i < n.  x_i, y_i: the unsigned decoded values of row i of packed1_dev (c1 bits) and
 * packed2_dev (c2 bits); r_i: the exact integer result of `op` on them; the result is a packed column of n values of co bits at
 * out_dev.
 *
 *   range rule  decided on the host, in 128-bit arithmetic.  With X = 2^c1 - 1 and Y = 2^c2 - 1,
 *                 LINEAR  lo = min(0, a X) + min(0, b Y) + k     hi = max(0, a X) + max(0, b Y) + k
 *                 MUL     lo = min(0, a X Y) + k                 hi = max(0, a X Y) + k
 *               bound every r_i.  lo < INT64_MIN or hi > INT64_MAX is refused (MI355_E_INVALID); otherwise 64-bit wrap-around
 *               arithmetic yields the exact r_i.  For MUL this rules out essentially only c1 + c2 = 64.
 *   kernels     [lo, hi] within [0, 2^co - 1]: arith_exact_kernel -- no row can be out of range, so nothing is tested or
 *               counted; 32-bit wrap-around arithmetic with a, b, k reduced mod 2^32 (the true result lies in [0, 2^32)).
 *               Otherwise arith_checked_kernel: 64-bit arithmetic, the test (uint64_t)r < 2^co, `miss` selected without a
 *               branch.
 *   widths      c1, c2 and co are 1..32, in any combination.
 *   miss        must be < 2^co when co < 32.
 *   out_of_range_dev  nullable device uint64 (naturally aligned), overwritten: the number of rows i < n with r_i outside
 *               [0, 2^co).  It is zeroed on the stream in front of the kernel, whose waves add to it; arith_exact_kernel leaves
 *               the 0, and so does n == 0.
 *   inputs      as everywhere: 16 bytes aligned, with the pad of mi355_compressed_buffer_size.  They may be the same buffer when
 *               c1 == c2.  What lies behind row n - 1 never reaches a result, so row-range views work.
 *   out_dev     16 bytes aligned.  The call writes exactly ceil(n * co / 8) bytes; the bits behind value n - 1 in the last byte are
 *               zero (the bitmaps' tail rule, applied to a packed output); nothing beyond is touched, so out_dev may be a row-range
 *               slice of a longer column (starting on a 16-byte boundary).  To be consumed as a column the buffer must still be
 *               mi355_compressed_buffer_size(co, n) bytes.
 *   aliasing    none: out_dev must overlap neither input (the byte ranges [out_dev, out_dev + ceil(n * co / 8)),
 *               [packed1_dev, packed1_dev + ceil(n * c1 / 8)) and [packed2_dev, packed2_dev + ceil(n * c2 / 8))).
 *   n == 0      no output byte is written and no kernel launched; the inputs and out_dev may be NULL.
 *   errors      MI355_E_INVALID, nothing launched, outputs untouched: op outside the two; a width outside 1..32; b != 0 with
 *               MI355_ARITH_MUL; miss >= 2^co when co < 32; the range rule; out_of_range_dev misaligned; with n > 0 a null or
 *               misaligned packed1_dev, packed2_dev or out_dev, or out_dev overlapping an input.
 *   stores      option "scan_nt_stores" (mi355_scan.h) governs the stores to out_dev: -1 (the default) write-through up to 768 MiB of
 *               output, non-temporal beyond; 0 plain.  1 non-temporal, 2 write-through.  The bytes never depend on it.
 *   stream     asynchronous on the context's stream; the call holds the context's lock like every other.
 *   record      mi355_ctx_last_launch names the kernel the call launched.
 *   graph capture: capturable -- the call enqueues its one kernel on the context's stream and, when a counter is given, the
 *   8-byte zeroing of out_of_range_dev in front of it; it uploads nothing, takes no buffer of the context's pool and never
 *   synchronises, whatever its arguments.  Both inputs are read at every replay. */
MI355_API int mi355_arith_dev(mi355_ctx *ctx, int op, const void *packed1_dev, unsigned c1, const void *packed2_dev, unsigned c2, uint64_t n,
                              int32_t a, int32_t b, int64_t k, unsigned co, uint32_t miss, void *out_dev, uint64_t *out_of_range_dev);

/* kernel family the call above would launch: "arith_exact_kernel" | "arith_checked_kernel"; NULL for whatever the call would
 * refuse whatever its buffers (op, a width, b != 0 with MI355_ARITH_MUL, the range rule).  Pure arithmetic: needs no device and no
 * context. */
MI355_API const char *mi355_arith_kernel(int op, unsigned c1, unsigned c2, int32_t a, int32_t b, int64_t k, unsigned co);

#ifdef __cplusplus
}
#endif

#endif /* MI355_ARITH_H */
