/* mi355_run_aggregate.h -- sum, count, min, max of a packed column per run of a table of run ends (part of the C ABI of
 * libmi355scan.so).
 *
 * The aggregates of a sort-based GROUP BY, and of run-length-coded data.  mi355_sort_rows_dev orders the rows,
 * mi355_run_encode_dev leaves one entry per group: the group's key and its END, the row behind its last row.  The
 * call below aggregates a second column over those runs -- per sorted key, per session, per day -- for keys without a dense
 * domain: sparse 32-bit surrogate keys, more groups than mi355_group_aggregate_wide_dev (mi355_groupby_wide.h) addresses.  Groups
 * are contiguous, so the call needs no hash front and almost no atomics.  The packed column is read once and not decompressed.
 * Plain C99, like mi355_scan.h; the context and the status codes are that header's.
 */
#ifndef MI355_RUN_AGGREGATE_H
#define MI355_RUN_AGGREGATE_H

#include "mi355_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per run j in [0, runs): out_dev[4*j + 0] = sum, [1] = count, [2] = min, [3] = max of values_i over the rows i < n with j(i) == j
 * (and mask bit i set, when mask_dev is given), where j(i) is the number of j < R with end_j <= i -- mi355_run_decode_dev's rule.
 * Values are the unsigned decoded integers; sum is exact modulo 2^64.  A run with no counted row: sum 0, count 0, min UINT64_MAX,
 * max 0 -- the layout and the empty result of mi355_group_aggregate_dev: a run of length zero (equal ends), a run the mask leaves
 * empty, every entry j with R <= j < runs.
 *
 *   R           `runs`, or min(runs, *runs_dev) when runs_dev (a nullable device uint64, naturally aligned) is given: it is read
 *               on the device, so run_encode -> run_aggregate never touches the host.  runs <= 2^32 - 1.
 *   ends        ends_dev at ce bits, non-decreasing over [0, R).  Runs that end beyond n are cut at n.  With ends that are not
 *               sorted the call still returns MI355_OK, reads nothing outside the table's R entries and writes nothing outside
 *               out_dev's 4 * runs words; no stronger claim is made.
 *   uncovered_dev  nullable device uint64 (naturally aligned), overwritten: the number of counted rows with j(i) == R, which are
 *               aggregated nowhere.
 *   widths      cv and ce are 1..32, any pair.  n is any size; a row beyond 2^32 - 1 lies behind every end.
 *   inputs      values_dev 16 bytes aligned; whole 16-byte pieces that START inside the ceil(n cv / 8) payload bytes are read, so
 *               at most 15 bytes behind them.  What lies behind row n - 1 reaches nothing, so row-range views work.  mask_dev:
 *               nullable (every row counts), a canonical bitmap, 4 bytes aligned, read up to ceil(n / 8) bytes and no further.
 *               ends_dev: 4 bytes aligned, read where it lies -- dwords 0 .. the one that holds the last bit of entry R - 1 and
 *               no more.
 *   out_dev     8 bytes aligned, 4 * runs uint64, overwritten completely by every successful call; nothing outside it is written.
 *               It may overlap no input.
 *   n == 0, R == 0  every entry gets the empty result; with n == 0 only the init kernel runs and values_dev, mask_dev and
 *               ends_dev may be NULL.
 *   errors      MI355_E_INVALID, nothing launched, out_dev and *uncovered_dev untouched: a width outside 1..32; runs > 2^32 - 1;
 *               out_dev NULL with runs > 0; a misaligned pointer; values_dev NULL with n > 0; ends_dev NULL with n > 0 and
 *               runs > 0; out_dev overlapping the column, the mask, the table, *runs_dev or *uncovered_dev.
 *   determinism every output word is a function of the inputs only: integer add, min and max commute.
 *   kernel      run_aggregate_kernel: a wave streams a chunk of 8 tiles of 2048 rows; it finds the runs of a tile's first and last
 *               row by a 64-way search over the ends.  One run: the lanes' rows are reduced in registers and carried to the next
 *               tile.  Up to mi355_run_aggregate_span_slots(cv) runs: one LDS atomic update per lane and run on a span table of
 *               the wave; the runs inside the tile leave by plain stores.  More: a lane stores the runs inside its 32 rows plainly
 *               and adds its first and last piece to memory.  The open run is carried from tile to tile and added to memory once
 *               per chunk.  No workspace, nothing of the context's.
 *   stream      asynchronous on the context's stream; the call holds the context's lock like every other.
 *   record      mi355_ctx_last_launch names the kernels the call enqueued: run_aggregate_init_kernel (the empty results, the zero
 *               in *uncovered_dev) and run_aggregate_kernel.
 *   graph capture: capturable -- the call enqueues its two kernels on the context's stream and nothing else: no memset node, no
 *   upload, no buffer of the context's pool, and it never synchronises, whatever its arguments; it needs no warm-up call.  The
 *   column, the mask, the ends and *runs_dev are read at every replay. */
MI355_API int mi355_run_aggregate_dev(mi355_ctx *ctx, const void *values_dev, unsigned cv, uint64_t n, const void *mask_dev, const void *ends_dev,
                                      unsigned ce, uint64_t runs, const uint64_t *runs_dev, uint64_t *out_dev, uint64_t *uncovered_dev);

/* name of the aggregating kernel of the call above: "run_aggregate_kernel"; NULL for a width outside 1..32.  Pure arithmetic:
 * needs no device and no context. */
MI355_API const char *mi355_run_aggregate_kernel(unsigned cv, unsigned ce);

/* slots S of the span table a wave of the call above keeps at value width cv: a power of two, the largest with which the images
 * and span tables of four blocks fit a CU's LDS and at least 128 (256 up to 8 bits, 128 beyond); 0 for a width outside 1..32.  A
 * tile that touches more than S runs takes the dense path.  Pure arithmetic. */
MI355_API uint32_t mi355_run_aggregate_span_slots(unsigned cv);

#ifdef __cplusplus
}
#endif

#endif /* MI355_RUN_AGGREGATE_H */
