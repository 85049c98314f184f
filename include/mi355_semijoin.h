/* mi355_semijoin.h -- filter a packed column by a set that lives in device memory (part of the C ABI of libmi355scan.so).
 *
 * The star-schema filter `SELECT ... FROM fact WHERE fact.fk IN (SELECT pk FROM dim WHERE <predicate>)`: with dense keys the
 * result bitmap of any scan over `dim` IS that set -- bit j set means key j qualifies -- and the call below consumes it where
 * it lies: no download, no key list, no decompression of the fact column.  mi355_scan_in_dev (mi355_scan.h) takes at most
 * 1024 keys from a host array per call; this call takes a set of up to 2^32 bits from device memory.  Plain C99, like
 * mi355_scan.h; the context and the status codes are that header's.
 */
#ifndef MI355_SEMIJOIN_H
#define MI355_SEMIJOIN_H

#include "mi355_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* largest set (in bits, after the cut at 2^c) that a block keeps in the LDS of its CU: 160 KiB minus the block's tiles (4 waves
 * x 16 KiB at the widest widths) and AND-mask images (4 x 1 KiB) minus 64 bytes of bookkeeping, in whole 16 bytes = 94144 bytes */
#define MI355_SEMIJOIN_LDS_MAX_BITS 753152

/* bitmap[i] = (v_i < set_bits && bit v_i of set_dev) XOR negate, then AND and_mask[i] when and_mask_dev is given; v_i the unsigned
 * decoded value of row i < n.  *hits_dev = number of set result bits.
 *
 *   set         set_dev is in bitmap format: bit j is byte j / 8, bit j % 8 -- exactly what every scan of a set_bits-row table
 *               writes.  set_bits is 0 .. 2^32.  A value v >= set_bits is not in the set, whatever c is: set_bits may be smaller or
 *               larger than 2^c (bits at 2^c and above are simply unreachable).  Bits >= set_bits of the last byte and everything
 *               behind byte ceil(set_bits/8) - 1 may hold anything: they never reach a result and the bytes behind are never
 *               read.  set_dev: 4 bytes aligned; NULL only when set_bits == 0.  set_bits == 0: no row is in the set (under
 *               negate every row is).  The set is read, never written.
 *   negate      != 0 gives NOT IN.
 *   and_mask    nullable; a canonical bitmap, 16 bytes aligned; may be bitmap_dev itself (in place), as in mi355_scan_in_dev.
 *   outputs     bitmap_dev NULL is the count-only form (only hits_dev is produced, no store is issued), as in
 *               mi355_scan_combine_dev; hits_dev is nullable; both NULL is an error.
 *   rows        the tail rule (bits >= n of the last byte zero, exactly ceil(n/8) bytes written), the alignment of packed_dev and
 *               bitmap_dev (16 bytes), row-range views (what lies behind row n - 1 never reaches a result) and n == 0 (nothing
 *               is read or written but *hits_dev = 0) are those of mi355_scan_where_dev.
 *   kernels     min(set_bits, 2^c) <= MI355_SEMIJOIN_LDS_MAX_BITS: semijoin_lds_kernel -- every block copies the set into LDS
 *               once, then one LDS byte lookup per value, as mi355_scan_in_dev's bitset form does.  Larger sets:
 *               semijoin_global_kernel -- one byte load per value from the set where it lies (L2 / Infinity Cache); gather-bound.
 *   errors      MI355_E_INVALID, nothing launched, outputs untouched: c outside 1..32; set_bits > 2^32; packed_dev NULL (n > 0);
 *               set_dev NULL with set_bits > 0; bitmap_dev and hits_dev both NULL; a misaligned pointer; set_dev overlapping
 *               bitmap_dev (the byte ranges [set_dev, set_dev + ceil(set_bits/8)) and [bitmap_dev, bitmap_dev + ceil(n/8))).
 *   stores      option "scan_nt_stores" (mi355_scan.h) governs the bitmap stores of both kernels: -1 (the default) write-through up
 *               to 768 MiB of bitmap, non-temporal beyond; 0 write-through too (the kernels have no plain form, like
 *               mi355_scan2_dev's).  1 non-temporal, 2 write-through.  The bytes never depend on it.
 *   stream     asynchronous on the context's stream; the call holds the context's lock like every other.
 *   record      mi355_ctx_last_launch names the kernel the call launched.
 *   graph capture: capturable -- the call enqueues its one kernel on the context's stream; it uploads nothing, takes no
 *   buffer of the context's pool and never synchronises, whatever its arguments.  The set is read at every replay: a graph of
 *   `scan the dimension table, then semi-join the fact column` follows the dimension table's contents. */
MI355_API int mi355_semijoin_dev(mi355_ctx *ctx, const void *packed_dev, uint64_t n, unsigned c, const void *set_dev, uint64_t set_bits,
                                 int negate, const void *and_mask_dev, void *bitmap_dev, uint64_t *hits_dev);

/* kernel family the call above would launch: "semijoin_lds_kernel" | "semijoin_global_kernel"; NULL for c outside 1..32 or
 * set_bits > 2^32.  Pure arithmetic: needs no device and no context. */
MI355_API const char *mi355_semijoin_kernel(unsigned c, uint64_t set_bits);

#ifdef __cplusplus
}
#endif

#endif /* MI355_SEMIJOIN_H */
