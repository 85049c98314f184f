/* mi355_runs.h -- the runs of a packed column, and back (part of the C ABI of libmi355scan.so).
 *
 * Run-length coding, the third of the lightweight encodings of an integer column beside dictionary codes (mi355_distinct.h) and
 * deltas (mi355_running.h).  mi355_run_encode_dev turns a column of n rows into its r runs, as two small packed columns: the runs'
 * values and the runs' ENDS (the row behind a run's last row).  mi355_run_decode_dev expands such a pair back onto n rows; it is
 * also repeat_interleave (ends = the running sum of the counts), and, with a result bitmap over the runs as a 1-bit column of
 * values, the step that turns it into the bitmap over the rows.  Ends compose with what exists: mi355_delta_dev(ends, first = 0)
 * is the run lengths, mi355_running_sum_dev(lengths) the ends again.  Packed in, packed out: nothing is decompressed.
 * Plain C99, like mi355_scan.h; the context and the status codes are that header's.
 */
#ifndef MI355_RUNS_H
#define MI355_RUNS_H

#include "mi355_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Row i of the column x (n rows of c bits at packed_dev) is a TAIL when i == n - 1 or x_i != x_{i+1}.  r is the number of tails
 * (r == 0 exactly when n == 0); run j ends at the j-th tail i_j, its value is x_{i_j} and its end is i_j + 1.
 *
 *   outputs     values_dev: a packed column at c bits; ends_dev: a packed column at ce bits; both hold the first
 *               m = min(r, capacity) runs.  *count_dev (a device uint64, naturally aligned) is always r.  Either output pointer
 *               may be NULL: values only is SELECT DISTINCT of a sorted column, ends only its group boundaries.  capacity == 0
 *               counts only: both outputs may be NULL, nothing is written to them, and only run_count_kernel and
 *               rowid_scan_kernel run.
 *   widths      c and ce are 1..32, and n <= 2^ce - 1 (an end is at most n), hence n <= 2^32 - 1.
 *   bytes       exactly ceil(m c / 8) bytes of values_dev and ceil(m ce / 8) bytes of ends_dev are written; the bits behind the
 *               last value in the last byte are zero; every byte behind keeps its value.  As in mi355_compact.h the call stores
 *               whole dwords, so each output must be writable up to the dword that holds its last byte.
 *   launches    four kinds: run_count_kernel (a wave counts the tails of a chunk of 16384 rows into a word of the workspace and
 *               adds its chunks' counts to *count_dev), rowid_scan_kernel over those words, compact_edges_kernel once per output
 *               given (it zeroes the dwords that chunks share), run_emit_kernel.  The column is read twice.
 *   determinism every output byte is a function of the inputs only.
 *   inputs      as everywhere: packed_dev 16 bytes aligned; whole 16-byte pieces that START inside the ceil(n c / 8) payload
 *               bytes are read, so at most 15 bytes behind them.  What lies behind row n - 1 reaches nothing: row n - 1 is a
 *               tail whatever follows it, so row-range views work.
 *   aliasing    none: no output may overlap the column, the other output or the workspace.
 *   ws_dev      the caller's workspace: mi355_run_encode_workspace_words(n) 64-bit words, 8 bytes aligned.  It may hold
 *               anything: every word the call reads it has written first, on the stream.  What it leaves there is unspecified.
 *               The call takes no buffer from the context.
 *   n == 0      nothing is launched; *count_dev = 0; packed_dev, the outputs and ws_dev may be NULL.
 *   errors      MI355_E_INVALID, nothing launched, every output and the workspace untouched: a width outside 1..32;
 *               n > 2^ce - 1; count_dev NULL or misaligned; with n > 0 a null or misaligned packed_dev or ws_dev; with
 *               capacity > 0 both outputs NULL; an output not 16 bytes aligned; any overlap named above.
 *   stores      option "scan_nt_stores" (mi355_scan.h) governs run_emit_kernel's stores of whole dwords to both outputs: -1 (the
 *               default) and 0 plain.  1 non-temporal, 2 write-through.  The dwords that chunks share leave by atomic OR whatever
 *               it says, and the bytes never depend on it.
 *   stream     asynchronous on the context's stream; the call holds the context's lock like every other.
 *   record      mi355_ctx_last_launch names the kernels in launch order.
 *   graph capture: capturable -- the call enqueues its kernels and the 8-byte zeroing of count_dev on the context's stream; the
 *   chunk prefix lives in the caller's workspace, so it uploads nothing, takes no buffer of the context's pool, never synchronises
 *   and needs no warm-up call, whatever its arguments.  Column and workspace are read at every replay. */
MI355_API int mi355_run_encode_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, unsigned ce, void *values_dev, void *ends_dev,
                                   uint64_t capacity, uint64_t *count_dev, uint64_t *ws_dev);

/* name of the emitting kernel of the call above: "run_emit_kernel"; NULL for what the call would refuse whatever its buffers (a
 * width outside 1..32).  Pure arithmetic: needs no device and no context. */
MI355_API const char *mi355_run_encode_kernel(unsigned c, unsigned ce);

/* 64-bit words of workspace a call on n rows needs: ceil(n / 16384) + 1 + ceil(n / 16777216), the chunk prefix that mi355_compact.h
 * documents.  Pure arithmetic. */
MI355_API uint64_t mi355_run_encode_workspace_words(uint64_t n);

/* out_i = values[j(i)] when j(i) < R, else miss, for every i < n, where j(i) is the number of j < R with end_j <= i: the column
 * that the R runs (values_dev at cv bits, ends_dev at ce bits) encode, as a packed column of n values of cv bits at out_dev.
 *
 *   R           `runs`, or min(runs, *runs_dev) when runs_dev (a nullable device uint64, naturally aligned) is given: it is read
 *               on the device, as mi355_gather_dev reads its count, so run_encode -> run_decode never touches the host.
 *               runs <= 2^32 - 1.  R == 0 gives a column of miss.
 *   ends        must be non-decreasing over [0, R).  Equal neighbours are runs of length zero: they are skipped and the result
 *               is exact (repeat_interleave with zero counts).  Runs that end beyond n are cut at n.  With ends that are not
 *               sorted every out_i is still values[j] of some j < R, or miss, and nothing outside the two tables' R entries is
 *               read.
 *   uncovered_dev  nullable device uint64 (naturally aligned), overwritten: the number of rows i < n with j(i) == R.  It is
 *               zeroed on the stream in front of the kernel, whose waves add to it.
 *   widths      cv and ce are 1..32; n is any size; miss must be < 2^cv when cv < 32.
 *   tables      both are read where they lie (4 bytes aligned, dwords 0 .. the one that holds the last bit of entry R - 1 and no
 *               more), as mi355_lookup.h's global tier reads its table: the hot part lives in L2 and the Infinity Cache.
 *   out_dev     16 bytes aligned.  Exactly ceil(n cv / 8) bytes are written; the bits behind value n - 1 in the last byte are
 *               zero; nothing beyond is touched.  With cv = 1 a buffer of ceil(n / 8) bytes is a bitmap of n rows.
 *   kernel      run_decode_kernel: a wave owns tiles of 2048 rows; it finds the runs of a tile's first and last row by a 64-way
 *               search over the ends; one run: the tile is one value; several: a lane searches inside that span for its first
 *               row and walks its 32 rows.  No workspace, nothing of the context's.
 *   n == 0      nothing is launched and nothing written; the counter gets 0.
 *   errors      MI355_E_INVALID, nothing launched, outputs untouched: a width outside 1..32; miss >= 2^cv when cv < 32;
 *               runs > 2^32 - 1; runs_dev or uncovered_dev misaligned; with n > 0 a null or misaligned out_dev; with n > 0 and
 *               runs > 0 a null or misaligned values_dev or ends_dev, or out_dev overlapping a table.
 *   stores      option "scan_nt_stores" (mi355_scan.h) governs the stores to out_dev: -1 (the default) and 0 plain.  1 non-temporal,
 *               2 write-through.  The bytes never depend on it.
 *   record     mi355_ctx_last_launch names the kernel.
 *   graph capture: capturable -- the call enqueues its one kernel on the context's stream and, when a counter is given, the
 *   8-byte zeroing of uncovered_dev in front of it; it uploads nothing, takes no buffer of the context's pool and never
 *   synchronises, whatever its arguments.  Both tables and *runs_dev are read at every replay. */
MI355_API int mi355_run_decode_dev(mi355_ctx *ctx, const void *values_dev, unsigned cv, const void *ends_dev, unsigned ce, uint64_t runs,
                                   const uint64_t *runs_dev, uint64_t n, uint32_t miss, void *out_dev, uint64_t *uncovered_dev);

/* name of the kernel the call above would launch: "run_decode_kernel"; NULL for a width outside 1..32.  Pure arithmetic. */
MI355_API const char *mi355_run_decode_kernel(unsigned cv, unsigned ce);

#ifdef __cplusplus
}
#endif

#endif /* MI355_RUNS_H */
