/* mi355_keyindex.h -- the row of every key of a packed column, as a packed table: the inverse of a key column, in the form
 * mi355_lookup_dev takes as its table (part of the C ABI of libmi355scan.so).
 *
 * The build side of a join.  mi355_lookup_dev computes out[i] = table[fk[i]], so the table's row number has to be the key; until
 * now only mi355_set_ranks_dev wrote such a table, and only of ranks.  mi355_key_index_dev writes, for every key, the row that
 * carries it -- from a dimension in any order, from one filtered by a mask, from one whose key is a column of its own.  One index
 * serves any number of attributes: lookup(fk, index) is the dimension row of every fact row, as a packed column, and lookup of that
 * column through any dimension column (a packed column is a table indexed by row) is the attribute.  The call counts the rows it
 * sees per key on the way: "is this column a key?" is word 2 == word 0 of its output, "the first / last row per key" is the table
 * itself, "which keys have a match?" is table[j] != miss.  Plain C99, like mi355_scan.h; the context and the status codes are that
 * header's.
 */
#ifndef MI355_KEYINDEX_H
#define MI355_KEYINDEX_H

#include "mi355_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* which of the rows that carry a key the table names: the lowest or the highest row number */
#define MI355_KEY_INDEX_FIRST 0
#define MI355_KEY_INDEX_LAST  1

/* largest reach min(table_rows, 2^ck), in entries, that a block of mi355_key_index_dev keeps as 4-byte slots in the LDS of its CU:
 * 64 KiB, the budget the bitset of mi355_value_set_dev has next to the tiles.  Every key column of up to 14 bits stays below it
 * with its full domain. */
#define MI355_KEY_INDEX_LDS_MAX_ROWS 16384

/* table[j] = first_row + the lowest (keep == MI355_KEY_INDEX_FIRST) or highest (MI355_KEY_INDEX_LAST) row i < n that mask_dev
 * selects (every row when NULL) and whose unsigned key is j, for every j < table_rows; `miss` where no such row exists.
 *
 *   widths      ck, the keys' width, and ct, the table's, are 1..32 each.  A row id r = first_row + i enters the table where
 *               r < 2^ct; a key whose row id does not fit gets `miss` and is counted in out_dev[3].  miss < 2^ct (any value when
 *               ct == 32).  n <= 2^32 - 1, first_row < 2^32; keep is one of the two constants above.
 *   rows        keys_dev: 16 bytes aligned, with the pad of mi355_compressed_buffer_size; NULL only when n == 0.  mask_dev:
 *               nullable, a bitmap over the n rows, 4 bytes aligned, read up to ceil(n / 8) bytes and no further; bits >= n of its
 *               last byte may hold anything.  What lies behind row n - 1 never reaches the table, neither pad bytes nor mask bits
 *               >= n, so row-range views work.  table_rows is 0 .. 2^32; it may be smaller or larger than 2^ck (entries at 2^ck and
 *               above are unreachable: they get `miss` and no workspace is read for them).
 *   outputs     table_dev: a packed column of table_rows values of ct bits, 16 bytes aligned, NULL only when table_rows == 0;
 *               exactly ceil(table_rows * ct / 8) bytes are written, the trailing bits of the last byte zero, nothing beyond is
 *               touched (the rules of mi355_set_ranks_dev).  It is what mi355_lookup_dev takes as table_dev.  out_dev: required,
 *               8 bytes aligned, four words.  out_dev[0] = members: the keys below table_rows that have a row.  out_dev[1] = the
 *               selected rows whose key is >= table_rows; they enter nothing (the "outside" of mi355_group_aggregate_wide_dev).
 *               out_dev[2] = the selected rows whose key is < table_rows: the key column is unique among the selected rows
 *               exactly when this equals out_dev[0].  out_dev[3] = the members whose row id did not fit ct bits.  All four are
 *               exact and the table is the same whatever the grid is.  n == 0 writes an all-`miss` table and {0, 0, 0, 0};
 *               table_rows == 0 writes no table byte and counts every selected row as outside.
 *   kernels     two phases over reach = min(table_rows, 2^ck) 4-byte slots of the context's selection workspace, zeroed on the
 *               stream at every call.  reach <= MI355_KEY_INDEX_LDS_MAX_ROWS: key_index_lds_kernel -- every block keeps the
 *               slots in LDS and merges its non-zero ones into the workspace at its end.  Larger: key_index_global_kernel -- per
 *               row a test of the slot where it lies, an atomic maximum only where the row wins; gather-bound.  Then
 *               key_index_pack_kernel turns the slots into the table, a lane per 32 entries.
 *   errors      MI355_E_INVALID, nothing launched, nothing written: ck or ct outside 1..32; table_rows > 2^32; n >= 2^32;
 *               first_row >= 2^32; miss >= 2^ct; a keep that is neither constant; keys_dev NULL (n > 0); table_dev NULL
 *               (table_rows > 0); out_dev NULL; a misaligned pointer; the table's bytes [table_dev, table_dev +
 *               ceil(table_rows * ct / 8)) overlapping the keys, the mask or out_dev.
 *   stores      option "scan_nt_stores" (mi355_scan.h) governs key_index_pack_kernel's stores to table_dev: -1 (the default)
 *               write-through up to 768 MiB of table, non-temporal beyond; 0 plain.  1 non-temporal, 2 write-through.  The bytes
 *               never depend on it.
 *   stream     asynchronous on the context's stream; the call holds the context's lock like every other.
 *   record      mi355_ctx_last_launch names the tier's kernel, then key_index_pack_kernel; with n == 0 only the latter (the table
 *               is all `miss`, no workspace is used), with table_rows == 0 only the former.
 *   graph capture: capturable after a warm-up call of at least the same table_rows -- the call takes the context's selection
 *   workspace, like mi355_set_ranks_dev: ceil(reach / 2) words, grown outside capture only.  Under capture a call that would have
 *   to grow it is refused with MI355_E_INVALID, the message names graph capture and the capture stays intact.  Keys and mask are
 *   read at every replay: a graph of `scan, key_index, lookup, lookup` follows the dimension's contents. */
MI355_API int mi355_key_index_dev(mi355_ctx *ctx, const void *keys_dev, uint64_t n, unsigned ck, const void *mask_dev, uint64_t first_row,
                                  int keep, void *table_dev, uint64_t table_rows, unsigned ct, uint32_t miss, uint64_t *out_dev);

/* kernel family the first phase of the call above would launch: "key_index_lds_kernel" | "key_index_global_kernel"; NULL for ck
 * outside 1..32 or table_rows > 2^32.  Pure arithmetic: needs no device and no context. */
MI355_API const char *mi355_key_index_kernel(unsigned ck, uint64_t table_rows);

#ifdef __cplusplus
}
#endif

#endif /* MI355_KEYINDEX_H */
