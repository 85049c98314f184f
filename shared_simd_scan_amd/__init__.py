"""shared_simd_scan_amd -- MI355X-native bit-packed column decompress / predicate scan engine.

Drop-in for the hot path of RRr89/Shared_SIMD_Scan (src/simd_scan.hpp): compress, decompress,
equality / range scan and shared multi-predicate scan as hand-written gfx950 HIP kernels behind a C
ABI (include/mi355_scan.h, shared_simd_scan_amd/libmi355scan.so).  See DESIGN.md.
"""
from ._capi import Mi355Error, lib  # noqa: F401
from .engine import (PackedColumn, ScanEngine, arith_kernel, arith_range, arith_width, clamp_diff, compact_kernel, compressed_buffer_size, decompression_output_buffer_size,  # noqa: F401
                     delta_kernel, group_wide_front_slots, kernel_name, key_index_kernel, lookup_kernel, running_sum_kernel, running_sum_range,
                     running_sum_workspace_words, run_aggregate_kernel, run_aggregate_span_slots, run_decode_kernel, run_encode_kernel, run_encode_workspace_words, scan_output_buffer_size, search_sorted_kernel, search_sorted_stride, semi_join_kernel, shared_where_kernel, sort_rows_passes, tile_values, top_k_passes,
                     value_set_kernel)

__all__ = ["Mi355Error", "PackedColumn", "ScanEngine", "compressed_buffer_size", "decompression_output_buffer_size",
           "scan_output_buffer_size", "kernel_name", "shared_where_kernel", "tile_values", "lib", "clamp_diff", "semi_join_kernel",
           "lookup_kernel", "compact_kernel", "arith_kernel", "arith_range", "arith_width", "group_wide_front_slots", "top_k_passes", "sort_rows_passes",
           "value_set_kernel", "key_index_kernel", "running_sum_kernel", "running_sum_range", "running_sum_workspace_words", "delta_kernel",
           "run_encode_kernel", "run_encode_workspace_words", "run_decode_kernel", "run_aggregate_kernel", "run_aggregate_span_slots", "search_sorted_kernel", "search_sorted_stride"]
