"""ctypes binding of the public headers under include/ (HEADERS).  No compute happens in Python; a missing library is an error."""
from __future__ import annotations

import ctypes as C
import os

from .build import LIB_PATH

_lib = None

OK = 0
LAYOUT_PER_PREDICATE = 0
LAYOUT_LINEAR = 1
GEN_MOD, GEN_SPLITMIX, GEN_INDEX = 0, 1, 2
COMM_ID_BYTES = 128

_vp, _u64, _u32, _i32, _sz, _int = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32, C.c_size_t, C.c_int
HEADERS = {}  # public header under include/ -> every symbol it declares, as (name, restype, argtypes), oldest header first; lib() binds them all
HEADERS["mi355_scan.h"] = [
    ("mi355_last_error", C.c_char_p, []),
    ("mi355_version", C.c_char_p, []),
    ("mi355_ctx_create", _int, [_int, _vp, C.POINTER(_vp)]),
    ("mi355_ctx_destroy", _int, [_vp]),
    ("mi355_ctx_synchronize", _int, [_vp]),
    ("mi355_device_count", _int, [C.POINTER(_int)]),
    ("mi355_ctx_set_option", _int, [_vp, C.c_char_p, _int]),
    ("mi355_ctx_set_stream", _int, [_vp, _vp]),
    ("mi355_tune_dev", _int, [_vp, _vp, _u64, C.c_uint, C.c_uint]),
    ("mi355_tuned_blocks_per_cu", _int, [_vp, C.c_uint, C.c_uint, _int]),
    ("mi355_shard_rows", _int, [_u64, C.c_uint, C.c_uint, C.POINTER(_u64), C.POINTER(_u64)]),
    ("mi355_compressed_buffer_size", _sz, [C.c_uint, _sz]),
    ("mi355_decompression_output_buffer_size", _sz, [_sz]),
    ("mi355_scan_output_buffer_size", _sz, [_sz]),
    ("mi355_bitmap_stride", _sz, [_sz]),
    ("mi355_dev_alloc", _int, [_vp, _sz, C.POINTER(_vp)]),
    ("mi355_dev_free", _int, [_vp, _vp]),
    ("mi355_dev_upload", _int, [_vp, _vp, _vp, _sz]),
    ("mi355_dev_download", _int, [_vp, _vp, _vp, _sz]),
    ("mi355_dev_memset", _int, [_vp, _vp, _int, _sz]),
    ("mi355_pack_u16", _int, [_vp, _vp, _u64, C.c_uint, _vp]),
    ("mi355_pack_u32", _int, [_vp, _vp, _u64, C.c_uint, _vp]),
    ("mi355_pack_u16_dev", _int, [_vp, _vp, _u64, C.c_uint, _vp]),
    ("mi355_pack_u32_dev", _int, [_vp, _vp, _u64, C.c_uint, _vp]),
    ("mi355_generate_dev", _int, [_vp, _int, _u64, _u64, C.c_uint, _u64, _vp]),
    ("mi355_decompress", _int, [_vp, _vp, _u64, C.c_uint, _vp]),
    ("mi355_decompress_dev", _int, [_vp, _vp, _u64, C.c_uint, _vp]),
    ("mi355_scan_eq", _int, [_vp, _vp, _u64, C.c_uint, _i32, _vp, C.POINTER(_u64)]),
    ("mi355_scan_eq_dev", _int, [_vp, _vp, _u64, C.c_uint, _i32, _vp, _vp]),
    ("mi355_scan_range", _int, [_vp, _vp, _u64, C.c_uint, _u32, _u32, _vp, C.POINTER(_u64)]),
    ("mi355_scan_range_dev", _int, [_vp, _vp, _u64, C.c_uint, _u32, _u32, _vp, _vp]),
    ("mi355_shared_scan_eq", _int, [_vp, _vp, _u64, C.c_uint, _vp, C.c_uint, _vp, _vp]),
    ("mi355_shared_scan_eq_linear", _int, [_vp, _vp, _u64, C.c_uint, _vp, C.c_uint, _vp, _vp]),
    ("mi355_shared_scan_eq_dev", _int, [_vp, _vp, _u64, C.c_uint, _vp, C.c_uint, _int, _vp, _u64, _vp]),
    ("mi355_shared_scan_where", _int, [_vp, _vp, _u64, C.c_uint, _vp, C.c_uint, _vp, _vp]),
    ("mi355_shared_scan_where_linear", _int, [_vp, _vp, _u64, C.c_uint, _vp, C.c_uint, _vp, _vp]),
    ("mi355_shared_scan_where_dev", _int, [_vp, _vp, _u64, C.c_uint, _vp, C.c_uint, _int, _vp, _u64, _vp]),
    ("mi355_scan_where_dev", _int, [_vp, _vp, _u64, C.c_uint, _int, C.c_int64, C.c_int64, _vp, _vp, _vp]),
    ("mi355_scan_combine_dev", _int, [_vp, _vp, _u64, C.c_uint, _int, C.c_int64, C.c_int64, _int, _vp, _vp, _vp]),
    ("mi355_scan2_dev", _int, [_vp, _vp, C.c_uint, _int, C.c_int64, C.c_int64, _vp, C.c_uint, _int, C.c_int64, C.c_int64, _u64, _int,
                         _vp, _vp]),
    ("mi355_scan_select_dev", _int, [_vp, _vp, _u64, C.c_uint, _int, C.c_int64, C.c_int64, _int, _vp, _u64, _vp, _u64, _vp]),
    ("mi355_scan_in_dev", _int, [_vp, _vp, _u64, C.c_uint, _vp, C.c_uint, _int, _vp, _vp, _vp]),
    ("mi355_bitmap_combine_dev", _int, [_vp, _int, _vp, _vp, _vp, _u64, _vp]),
    ("mi355_bitmap_count_dev", _int, [_vp, _vp, _u64, _vp]),
    ("mi355_bitmap_to_rowids_dev", _int, [_vp, _vp, _u64, _u64, _vp, _u64, _vp]),
    ("mi355_gather_dev", _int, [_vp, _vp, _u64, C.c_uint, _u64, _vp, _vp, _u64, _vp]),
    ("mi355_aggregate_dev", _int, [_vp, _vp, _u64, C.c_uint, _vp, _vp]),
    ("mi355_histogram_dev", _int, [_vp, _vp, _u64, C.c_uint, _vp, _vp]),
    ("mi355_comm_get_unique_id", _int, [_vp]),
    ("mi355_comm_create", _int, [_vp, _int, _int, _vp, C.POINTER(_vp)]),
    ("mi355_comm_destroy", _int, [_vp]),
    ("mi355_comm_info", _int, [_vp, C.POINTER(_int), C.POINTER(_int)]),
    ("mi355_gather_bitmaps_dev", _int, [_vp, _vp, _vp, _vp, _int, _vp]),
    ("mi355_gather_bitmaps_at_dev", _int, [_vp, _vp, _vp, _vp, _vp, _int, _vp]),
    ("mi355_allreduce_hits_dev", _int, [_vp, _vp, _vp, C.c_uint]),
    ("mi355_sharded_scan_eq_dev", _int, [_vp, _vp, _vp, C.c_uint, _i32, _vp, _vp, _int, _vp, _vp]),
    ("mi355_sharded_scan_range_dev", _int, [_vp, _vp, _vp, C.c_uint, _u32, _u32, _vp, _vp, _int, _vp, _vp]),
    ("mi355_kernel_name", C.c_char_p, [C.c_char_p, C.c_uint]),
    ("mi355_shared_scan_kernel", C.c_char_p, [_vp, C.c_uint, C.c_uint, _int, _int]),
    ("mi355_shared_where_kernel", C.c_char_p, [_vp, C.c_uint, C.c_uint, _int, _int]),
    ("mi355_ctx_last_launch", C.c_char_p, [_vp]),
    ("mi355_ctx_last_llc_divisor", C.c_int, [_vp]),
    ("mi355_tile_values", _u64, [C.c_uint]),
]

# predicates that compare two columns row by row
HEADERS["mi355_columns.h"] = [
    ("mi355_scan_columns_dev", _int, [_vp, _vp, C.c_uint, _vp, C.c_uint, _u64, _int, C.c_int64, C.c_int64, _int, _vp, _vp, _vp]),
]

# grouped aggregates over two columns
HEADERS["mi355_groupby.h"] = [
    ("mi355_group_aggregate_dev", _int, [_vp, _vp, C.c_uint, _vp, C.c_uint, _u64, _vp, _vp]),
]

# a column filtered by a device-resident bitmap set
HEADERS["mi355_semijoin.h"] = [
    ("mi355_semijoin_dev", _int, [_vp, _vp, _u64, C.c_uint, _vp, _u64, _int, _vp, _vp, _vp]),
    ("mi355_semijoin_kernel", C.c_char_p, [C.c_uint, _u64]),
]

# a column mapped through a device-resident packed table
HEADERS["mi355_lookup.h"] = [
    ("mi355_lookup_dev", _int, [_vp, _vp, _u64, C.c_uint, _vp, _u64, C.c_uint, C.c_uint32, _vp]),
    ("mi355_lookup_kernel", C.c_char_p, [C.c_uint, _u64, C.c_uint]),
]

# the rows a bitmap selects, as a packed column
HEADERS["mi355_compact.h"] = [
    ("mi355_compact_dev", _int, [_vp, _vp, _u64, C.c_uint, _vp, _vp, _u64, _vp]),
    ("mi355_compact_kernel", C.c_char_p, [C.c_uint]),
]

# a packed column computed row by row from two others
HEADERS["mi355_arith.h"] = [
    ("mi355_arith_dev", _int, [_vp, _int, _vp, C.c_uint, _vp, C.c_uint, _u64, _i32, _i32, C.c_int64, C.c_uint, _u32, _vp, _vp]),
    ("mi355_arith_kernel", C.c_char_p, [_int, C.c_uint, C.c_uint, _i32, _i32, C.c_int64, C.c_uint]),
]

# grouped aggregates for keys beyond 12 bits
HEADERS["mi355_groupby_wide.h"] = [
    ("mi355_group_aggregate_wide_dev", _int, [_vp, _vp, C.c_uint, _vp, C.c_uint, _u64, _vp, _u64, _vp, _vp]),
    ("mi355_group_wide_front_slots", _u32, [C.c_uint, C.c_uint]),
]

# the k largest or smallest rows of a column, as a bitmap
HEADERS["mi355_topk.h"] = [
    ("mi355_top_k_dev", _int, [_vp, _vp, _u64, C.c_uint, _vp, _u64, _int, _vp, _vp]),
    ("mi355_top_k_passes", C.c_uint, [C.c_uint]),
]

# the set of a column's values as a bitmap over the value domain, the members' ranks as a packed table.  (In front of mi355_sort.h:
# tests/test_sort_rows.py wants that header to stay the dict's last key.)
HEADERS["mi355_distinct.h"] = [
    ("mi355_value_set_dev", _int, [_vp, _vp, _u64, C.c_uint, _vp, _vp, _u64, _int, _vp]),
    ("mi355_value_set_kernel", C.c_char_p, [C.c_uint, _u64]),
    ("mi355_set_ranks_dev", _int, [_vp, _vp, _u64, C.c_uint, _u32, _vp, _vp]),
]

# the row of every key of a column, as the packed table lookup reads.  (In front of mi355_sort.h too.)
HEADERS["mi355_keyindex.h"] = [
    ("mi355_key_index_dev", _int, [_vp, _vp, _u64, C.c_uint, _vp, _u64, _int, _vp, _u64, C.c_uint, _u32, _vp]),
    ("mi355_key_index_kernel", C.c_char_p, [C.c_uint, _u64]),
]

# prefix sums and differences of a packed column.  (In front of mi355_sort.h too.)
HEADERS["mi355_running.h"] = [
    ("mi355_running_sum_dev", _int, [_vp, _vp, _u64, C.c_uint, _vp, C.c_int64, C.c_int64, C.c_uint, C.c_uint, _u32, _vp, _vp, _vp]),
    ("mi355_running_sum_kernel", C.c_char_p, [C.c_uint, _u64, C.c_int64, C.c_int64, C.c_uint]),
    ("mi355_running_sum_workspace_words", _u64, [_u64]),
    ("mi355_delta_dev", _int, [_vp, _vp, _u64, C.c_uint, _u32, C.c_int64, C.c_uint, _u32, _vp, _vp]),
    ("mi355_delta_kernel", C.c_char_p, [C.c_uint, C.c_int64, C.c_uint]),
]

# a packed column's positions in a sorted packed table.  (In front of mi355_runs.h: tests/test_runs.py wants that header and mi355_sort.h to stay the dict's last two keys.)
HEADERS["mi355_search.h"] = [
    ("mi355_search_sorted_dev", _int, [_vp, _vp, _u64, C.c_uint, _vp, C.c_uint, _u64, _vp, _int, _int, _u32, _vp, C.c_uint, _vp, _vp]),
    ("mi355_search_sorted_kernel", C.c_char_p, [C.c_uint, C.c_uint, C.c_uint, _u64]),
    ("mi355_search_sorted_stride", _u64, [_u64]),
]

# sum, count, min, max of a packed column per run of a table of run ends.  (In front of mi355_runs.h too.)
HEADERS["mi355_run_aggregate.h"] = [
    ("mi355_run_aggregate_dev", _int, [_vp, _vp, C.c_uint, _u64, _vp, _vp, C.c_uint, _u64, _vp, _vp, _vp]),
    ("mi355_run_aggregate_kernel", C.c_char_p, [C.c_uint, C.c_uint]),
    ("mi355_run_aggregate_span_slots", _u32, [C.c_uint]),
]

# a packed column's runs as two packed columns, and their expansion.  (In front of mi355_sort.h too.)
HEADERS["mi355_runs.h"] = [
    ("mi355_run_encode_dev", _int, [_vp, _vp, _u64, C.c_uint, C.c_uint, _vp, _vp, _u64, _vp, _vp]),
    ("mi355_run_encode_kernel", C.c_char_p, [C.c_uint, C.c_uint]),
    ("mi355_run_encode_workspace_words", _u64, [_u64]),
    ("mi355_run_decode_dev", _int, [_vp, _vp, C.c_uint, _vp, C.c_uint, _u64, _vp, _u64, _u32, _vp, _vp]),
    ("mi355_run_decode_kernel", C.c_char_p, [C.c_uint, C.c_uint]),
]

# the row ids of a column in value order
HEADERS["mi355_sort.h"] = [
    ("mi355_sort_rows_dev", _int, [_vp, _vp, _u64, C.c_uint, _vp, _int, _u64, _vp, _vp, _u64, _vp]),
    ("mi355_sort_rows_passes", C.c_uint, [C.c_uint]),
    ("mi355_sort_rows_workspace_words", _u64, [_u64, _u64, C.c_uint]),
]


class Predicate(C.Structure):
    """mi355_predicate: one comparison `v OP a [, b]` of a shared where-scan"""
    _fields_ = [("op", C.c_int32), ("reserved", C.c_int32), ("a", C.c_int64), ("b", C.c_int64)]


class Mi355Error(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load shared_simd_scan_amd/libmi355scan.so (built by build.py / __graft_entry__.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise Mi355Error(
                f"{LIB_PATH} not found: the HIP extension is not built (run `python -m shared_simd_scan_amd.build`). "
                "There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        for name, res, args in sum(HEADERS.values(), []):
            fn = getattr(L, name)  # AttributeError if the library does not export what the header declares
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc: int) -> None:
    if rc != OK:
        msg = lib().mi355_last_error()
        raise Mi355Error(f"mi355 error {rc}: {msg.decode() if msg else '?'}")
