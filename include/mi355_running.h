/* mi355_running.h -- prefix sums and differences of a packed column (part of the C ABI of libmi355scan.so).
 *
 * The two calls whose rows depend on the rows before them: mi355_running_sum_dev turns a column of bit-packed deltas into the
 * column they encode (the DELTA_BINARY_PACKED shape: b = the block's minimum delta, k = the first value), computes
 * `sum(v) OVER (ROWS UNBOUNDED PRECEDING)`, also under a filter's bitmap, and -- with a result bitmap as a 1-bit column -- every
 * row's position among the selected rows; mi355_delta_dev is the inverse: the encoder, the descent counter behind "is this column
 * sorted?", and the step that marks where the values of a sorted column change.  Packed in, packed out: nothing is decompressed.
 * Plain C99, like mi355_scan.h; the context and the status codes are that header's.
 */
#ifndef MI355_RUNNING_H
#define MI355_RUNNING_H

#include "mi355_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI355_RUNNING_INCLUSIVE 0 /* r_i = k + the terms of rows j <= i */
#define MI355_RUNNING_EXCLUSIVE 1 /* r_i = k + the terms of rows j <  i */

/* out_i = (0 <= r_i < 2^co) ? r_i : miss for EVERY i < n, selected or not, with
 *     r_i = k + sum of t_j over j <= i (MI355_RUNNING_EXCLUSIVE: j < i),   t_j = (mask_dev == NULL || bit j of mask_dev) ? x_j + b : 0.
 * x_j: the unsigned decoded value of row j of packed_dev (c bits); the result is a packed column of n values of co bits at out_dev.
 *
 *   range rule  decided on the host, in 128-bit arithmetic.  With lo_t = min(0, b) and hi_t = max(0, 2^c - 1 + b), every partial
 *               sum lies in [k + n lo_t, k + n hi_t].  That interval must lie within int64, else MI355_E_INVALID (so must
 *               n <= 2^62); otherwise 64-bit wrap-around arithmetic yields the exact r_i.
 *   kernels     the interval within [0, 2^co - 1]: running_sum_exact_kernel -- no row can be out of range, so nothing is tested or
 *               counted; 32-bit wrap-around arithmetic with b, k and the carry reduced mod 2^32.  The position case lands here
 *               (c = 1, n < 2^32, co = 32).  Otherwise running_sum_checked_kernel: 64-bit arithmetic, the test
 *               (uint64_t)r >> co == 0, `miss` selected without a branch.
 *   launches    three: running_sum_totals_kernel (a wave sums the terms of a chunk of 16384 rows into a 64-bit word of the
 *               workspace), rowid_scan_kernel over those words, the emitting kernel.  The column is read twice.
 *   widths      c and co are 1..32, in any combination.
 *   flags       MI355_RUNNING_INCLUSIVE or MI355_RUNNING_EXCLUSIVE.
 *   miss        must be < 2^co when co < 32.
 *   mask_dev    nullable: a bitmap of n rows (ceil(n / 8) bytes, 4 bytes aligned).  Bits behind row n - 1 are not read as rows.
 *   result_dev  nullable device uint64[2] (naturally aligned), overwritten.  Word 0: k + the sum of ALL terms, as a two's-complement
 *               int64 -- the inclusive value of row n - 1 under either flag, and the k of a call on the rows that follow.  Word 1:
 *               the number of rows i < n replaced by miss.  Both are zeroed on the stream in front of the kernels.
 *   ws_dev      the caller's workspace: mi355_running_sum_workspace_words(n) 64-bit words, 8 bytes aligned.  It need not hold
 *               zeros, or anything: every word the call reads it has written first, on the stream.  What it leaves there is
 *               unspecified.  The call takes no buffer from the context.
 *   inputs      as everywhere: packed_dev 16 bytes aligned.  The kernels read whole 16-byte pieces that START inside the
 *               ceil(n * c / 8) payload bytes, so at most 15 bytes behind them: the pad of mi355_compressed_buffer_size covers
 *               that, and so does the 32-byte pad of a result bitmap (mi355_scan_output_buffer_size), which is what lets a bitmap
 *               stand in as a column of c = 1.  What lies behind row n - 1 reaches neither an output byte nor a result word, so
 *               row-range views work.
 *   out_dev     16 bytes aligned.  The call writes exactly ceil(n * co / 8) bytes; the bits behind value n - 1 in the last byte
 *               are zero; nothing beyond is touched, so out_dev may be a row-range slice of a longer column.  To be consumed as a
 *               column the buffer must still be mi355_compressed_buffer_size(co, n) bytes.
 *   aliasing    none: out_dev must overlap neither the column, nor the mask, nor the workspace.
 *   n == 0      no kernel is launched and no output byte written; word 0 gets k and word 1 gets 0.  packed_dev, out_dev and
 *               ws_dev may be NULL.
 *   errors      MI355_E_INVALID, nothing launched, every output and the workspace untouched: a width outside 1..32; flags outside
 *               the two; miss >= 2^co when co < 32; the range rule; result_dev or mask_dev misaligned; with n > 0 a null or
 *               misaligned packed_dev, out_dev or ws_dev, or out_dev overlapping the column, the mask or the workspace.
 *   stores      option "scan_nt_stores" (mi355_scan.h) governs the stores to out_dev: -1 (the default) and 0 plain.  1 non-temporal,
 *               2 write-through.  The bytes never depend on it.
 *   stream     asynchronous on the context's stream; the call holds the context's lock like every other.
 *   record      mi355_ctx_last_launch names the three kernels in launch order.
 *   graph capture: capturable -- the call enqueues its three kernels and, when result_dev is given, the 16-byte zeroing of it on
 *   the context's stream; the chunk prefix lives in the caller's workspace, so it uploads nothing, takes no buffer of the context's
 *   pool, never synchronises and needs no warm-up call, whatever its arguments.  Column, mask and workspace are read at every
 *   replay. */
MI355_API int mi355_running_sum_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const void *mask_dev, int64_t b, int64_t k,
                                    unsigned flags, unsigned co, uint32_t miss, void *out_dev, uint64_t *result_dev, uint64_t *ws_dev);

/* kernel family the call above would launch last: "running_sum_exact_kernel" | "running_sum_checked_kernel"; NULL for whatever the
 * call would refuse whatever its buffers (a width, the range rule).  Pure arithmetic: needs no device and no context. */
MI355_API const char *mi355_running_sum_kernel(unsigned c, uint64_t n, int64_t b, int64_t k, unsigned co);

/* 64-bit words of workspace a call on n rows needs: ceil(n / 16384) + 1 + ceil(n / 16777216), the chunk prefix that mi355_compact.h
 * documents.  Pure arithmetic. */
MI355_API uint64_t mi355_running_sum_workspace_words(uint64_t n);

/* out_i = (0 <= r_i < 2^co) ? r_i : miss, i < n, with r_i = x_i - x_{i-1} + k and x_{-1} = first: the differences of consecutive
 * rows of packed_dev (c bits) as a packed column of n values of co bits at out_dev.  With k = 0 and co = c the counter is the number
 * of descents (rows with x_i < x_{i-1}); 0 means the column is sorted.  With k = 2^c - 1 and co = c + 1 no row is replaced, and
 * mi355_running_sum_dev with b = -(2^c - 1), k = first gives the column back.
 *
 *   kernels     k >= 2^c - 1 and k + 2^c - 1 < 2^co: delta_exact_kernel -- no row can be out of range, nothing is tested or counted,
 *               32-bit wrap-around arithmetic.  Otherwise delta_checked_kernel: 64-bit wrap-around arithmetic and the test
 *               (uint64_t)r >> co == 0.  No range rule is needed: a difference plus k beyond int64 wraps to a value whose
 *               magnitude is at least 2^63 - 2^32, which is replaced by miss as the true one would be.
 *   widths      c and co are 1..32, in any combination.
 *   first       must be < 2^c when c < 32.
 *   miss        must be < 2^co when co < 32.
 *   out_of_range_dev  nullable device uint64 (naturally aligned), overwritten: the number of rows i < n with r_i outside [0, 2^co).
 *               It is zeroed on the stream in front of the kernel, whose waves add to it; delta_exact_kernel leaves the 0, and so
 *               does n == 0.
 *   inputs, out_dev, aliasing: as above (there is no mask and no workspace).
 *   n == 0      no output byte is written and no kernel launched; packed_dev and out_dev may be NULL.
 *   errors      MI355_E_INVALID, nothing launched, outputs untouched: a width outside 1..32; first >= 2^c when c < 32;
 *               miss >= 2^co when co < 32; out_of_range_dev misaligned; with n > 0 a null or misaligned packed_dev or out_dev, or
 *               out_dev overlapping the column.
 *   stores      option "scan_nt_stores" (mi355_scan.h) governs the stores to out_dev: -1 (the default) and 0 plain.  1 non-temporal,
 *               2 write-through.  The bytes never depend on it.
 *   record     mi355_ctx_last_launch names the kernel the call launched.
 *   graph capture: capturable -- the call enqueues its one kernel on the context's stream and, when a counter is given, the
 *   8-byte zeroing of out_of_range_dev in front of it; it uploads nothing, takes no buffer of the context's pool and never
 *   synchronises, whatever its arguments.  The column is read at every replay. */
MI355_API int mi355_delta_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, uint32_t first, int64_t k, unsigned co, uint32_t miss,
                              void *out_dev, uint64_t *out_of_range_dev);

/* kernel family the call above would launch: "delta_exact_kernel" | "delta_checked_kernel"; NULL for a width outside 1..32.  Pure
 * arithmetic: needs no device and no context. */
MI355_API const char *mi355_delta_kernel(unsigned c, int64_t k, unsigned co);

#ifdef __cplusplus
}
#endif

#endif /* MI355_RUNNING_H */
