/* mi355_compact.h -- the rows a result bitmap selects, as a packed column (part of the C ABI of libmi355scan.so).
 *
 * The materialisation step behind a selective WHERE: filter once, compact the few columns the rest of the query needs with the
 * one bitmap -- they stay row-aligned --, then run mi355_lookup_dev, the scans, mi355_group_aggregate_dev and mi355_semijoin_dev
 * on the m rows that qualified instead of all n.  Packed in, packed out: nothing is decompressed to memory, no row id is
 * written.  Plain C99, like mi355_scan.h; the context and the status codes are that header's.
 */
#ifndef MI355_COMPACT_H
#define MI355_COMPACT_H

#include "mi355_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out = the packed column, at c bits, of the values v_i of packed_dev for exactly those i < n whose bit is set in bitmap_dev, in
 * row order; *count_dev = the number of set bits over [0, n).
 *
 *   widths      c is 1..32; n is any size, columns beyond 2^32 rows included.
 *   capacity    in values: m = min(count, capacity) values are written; *count_dev is always the total (the rule of
 *               mi355_bitmap_to_rowids_dev).  capacity == 0 makes the call count-only: out_dev may be NULL, nothing is written.
 *   packed_dev  as everywhere: 16 bytes aligned, with the pad of mi355_compressed_buffer_size.  What lies behind row n - 1 never
 *               reaches a result, so row-range views work.
 *   bitmap_dev  4 bytes aligned (a row range that starts at a multiple of 32 rows, as for mi355_bitmap_to_rowids_dev).  It must
 *               be canonical -- bits >= n of its last byte zero -- and is read up to ceil(n / 8) bytes and no further.
 *   out_dev     16 bytes aligned.  The call writes exactly the first ceil(m * c / 8) bytes; the bits behind value m - 1 in the
 *               last byte are zero (the bitmaps' tail rule, applied to a packed output); every byte behind that keeps the value
 *               it had.  The buffer must be writable in whole dwords: ceil(capacity * c / 8) bytes rounded up to 4.  To be
 *               consumed as a column it must be mi355_compressed_buffer_size(c, m) bytes.
 *   aliasing    none: out_dev must overlap neither the column's bytes [packed_dev, packed_dev + ceil(n * c / 8)) nor the
 *               bitmap's [bitmap_dev, bitmap_dev + ceil(n / 8)).
 *   n == 0      nothing is read, *count_dev = 0; packed_dev and bitmap_dev may be NULL.
 *   result      every output byte is a function of the inputs only: the same call gives the same bytes.
 *   kernels     the chunk counts and their prefix are those of mi355_bitmap_to_rowids_dev (rowid_count_kernel,
 *               rowid_scan_kernel); compact_edges_kernel clears the output dwords that two chunks share, compact_kernel writes the
 *               values.  No block ever waits for another: the passes are separate launches in stream order.
 *   errors      MI355_E_INVALID, nothing launched, outputs untouched: c outside 1..32; count_dev NULL; packed_dev or bitmap_dev
 *               NULL (n > 0); out_dev NULL (n > 0 and capacity > 0); a misaligned pointer; out_dev overlapping packed_dev or
 *               bitmap_dev.
 *   stores      option "scan_nt_stores" (mi355_scan.h) governs compact_kernel's stores of whole dwords: -1 (the default) write-through
 *               up to 768 MiB of output, non-temporal beyond; 0 plain.  1 non-temporal, 2 write-through.  The dwords that chunks
 *               share leave by atomic OR whatever it says, and the bytes never depend on it.
 *   stream     asynchronous on the context's stream; the call holds the context's lock like every other.
 *   record      mi355_ctx_last_launch names the kernels the call launched; compact_kernel is among them when capacity > 0.
 *   graph capture: capturable after a warm-up call of at least this size -- the call takes the context's selection
 *   workspace, like mi355_bitmap_to_rowids_dev: (ceil(n / 16384) + 1 + ceil(n / 16777216)) words, grown outside capture only.
 *   Under capture a call that would have to grow it is refused with MI355_E_INVALID, the message names graph capture and the
 *   capture stays intact.  Column and bitmap are read at every replay: a graph of `scan, then compact` follows the column's
 *   contents. */
MI355_API int mi355_compact_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const void *bitmap_dev, void *out_dev,
                                uint64_t capacity, uint64_t *count_dev);

/* kernel the call above launches to write its values: "compact_kernel"; NULL for a width the call would refuse (c outside 1..32).
 * Pure arithmetic: needs no device and no context. */
MI355_API const char *mi355_compact_kernel(unsigned c);

#ifdef __cplusplus
}
#endif

#endif /* MI355_COMPACT_H */
