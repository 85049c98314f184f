/* mi355_lookup.h -- map a packed column through a packed table that lives in device memory (part of the C ABI of libmi355scan.so).
 *
 * The star-schema join `SELECT d.attr, ... FROM fact f JOIN dim d ON f.fk = d.pk ... GROUP BY d.attr` with dense keys: for every
 * fact row the attribute of the dimension row its foreign key points at, as a packed column that every other call consumes --
 * mi355_group_aggregate_dev (mi355_groupby.h) as its keys, any scan as its column.  The same call re-codes a dictionary: the
 * codes of one dictionary into another's, or into coarser buckets.  Packed in, packed out: nothing is decompressed.  Plain C99,
 * like mi355_scan.h; the context and the status codes are that header's.
 */
#ifndef MI355_LOOKUP_H
#define MI355_LOOKUP_H

#include "mi355_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of LDS a block's decoded table may take: 160 KiB minus the block's input images at the widest width (4 waves x 2 x 8 KiB
 * at c = 32) minus 64 bytes of bookkeeping, in whole 16 bytes.  The LDS tier holds min(table_rows, 2^c) + 1 entries (the table's
 * reachable part and `miss`) of 1 byte (ct <= 8), 2 bytes (ct <= 16) or 4 bytes each within it. */
#define MI355_LOOKUP_LDS_MAX_BYTES 98240

/* out_i = (v_i < table_rows) ? t[v_i] : miss,  i < n.  v_i: row i of packed_dev (c bits); t[j]: value j of table_dev, a packed
 * column of table_rows values of ct bits; the result is a packed column of n values of ct bits at out_dev.
 *
 *   widths      c and ct are 1..32, in any pair.  table_rows is 0 .. 2^32 and may be smaller or larger than 2^c: rows at index 2^c
 *               and above are unreachable and are never read.  table_rows == 0: table_dev may be NULL and every row gets miss.
 *   miss        must be < 2^ct when ct < 32.
 *   packed_dev  as everywhere: 16 bytes aligned, with the pad of mi355_compressed_buffer_size.  What lies behind row n - 1 never
 *               reaches a result, so row-range views work.
 *   table_dev   read like the column of mi355_gather_dev: 4 bytes aligned, in whole dwords, readable up to 8 bytes past the last
 *               value (the pad of mi355_compressed_buffer_size covers that).  No dword behind the one that holds the last bit of
 *               value min(table_rows, 2^c) - 1 is read.  The bits of the last payload byte behind value table_rows - 1, and
 *               everything after, may hold anything: they never reach a result.  The table is read, never written.
 *   out_dev     16 bytes aligned.  The call writes exactly ceil(n * ct / 8) bytes; the bits behind value n - 1 in the last byte are
 *               zero (the bitmaps' tail rule, applied to a packed output); nothing beyond is touched, so out_dev may be a row-range
 *               slice of a longer column (starting on a 16-byte boundary).  To be consumed as a column the buffer must still be
 *               mi355_compressed_buffer_size(ct, n) bytes.
 *   aliasing    none: out_dev must overlap neither packed_dev nor table_dev (the byte ranges [out_dev, out_dev + ceil(n * ct / 8)),
 *               [packed_dev, packed_dev + ceil(n * c / 8)) and [table_dev, table_dev + ceil(table_rows * ct / 8))).
 *   n == 0      nothing is read or written; packed_dev may be NULL.
 *   kernels     (min(table_rows, 2^c) + 1) entries within MI355_LOOKUP_LDS_MAX_BYTES: lookup_lds_kernel -- every block decodes the
 *               reachable table into LDS once, then one LDS read per value.  Larger tables: lookup_global_kernel -- one or two
 *               dword loads per value from the packed table where it lies (L2 / Infinity Cache); gather-bound.
 *   errors      MI355_E_INVALID, nothing launched, outputs untouched: c or ct outside 1..32; table_rows > 2^32; miss >= 2^ct;
 *               packed_dev or out_dev NULL (n > 0); table_dev NULL with table_rows > 0; a misaligned pointer; out_dev
 *               overlapping packed_dev or table_dev.
 *   stores      option "scan_nt_stores" (mi355_scan.h) governs the stores to out_dev: -1 (the default) write-through up to 768 MiB of
 *               output, non-temporal beyond; 0 plain.  1 non-temporal, 2 write-through.  The bytes never depend on it.
 *   stream     asynchronous on the context's stream; the call holds the context's lock like every other.
 *   record      mi355_ctx_last_launch names the kernel the call launched.
 *   graph capture: capturable -- the call enqueues its one kernel on the context's stream; it uploads nothing, takes no
 *   buffer of the context's pool and never synchronises, whatever its arguments.  The table is read at every replay: a graph of
 *   `lookup, then group_aggregate` follows the dimension table's contents. */
MI355_API int mi355_lookup_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const void *table_dev, uint64_t table_rows,
                               unsigned ct, uint32_t miss, void *out_dev);

/* kernel family the call above would launch: "lookup_lds_kernel" | "lookup_global_kernel"; NULL for arguments the call would
 * refuse (c or ct outside 1..32, table_rows > 2^32).  Pure arithmetic: needs no device and no context. */
MI355_API const char *mi355_lookup_kernel(unsigned c, uint64_t table_rows, unsigned ct);

#ifdef __cplusplus
}
#endif

#endif /* MI355_LOOKUP_H */
