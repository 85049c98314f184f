"""ScanEngine -- Python face of the C ABI for device-resident columns.

torch is plumbing here: it owns device memory (uint8 / int32 tensors), the HIP stream the kernels are
enqueued on, and (in sharded.py) the RCCL process group.  Every operation is one call into
libmi355scan.so; nothing is computed in Python and nothing falls back to the CPU.

Names follow the reference's surface (src/simd_scan.hpp): compress / decompress / scan / shared_scan.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi
from ._capi import check, lib


def compressed_buffer_size(c: int, n: int) -> int:
    """src/simd_scan.hpp:20-26"""
    return lib().mi355_compressed_buffer_size(c, n)


def decompression_output_buffer_size(n: int) -> int:
    """src/simd_scan.hpp:28-33"""
    return lib().mi355_decompression_output_buffer_size(n)


def scan_output_buffer_size(n: int) -> int:
    """src/simd_scan.hpp:35-40"""
    return lib().mi355_scan_output_buffer_size(n)


def tile_values(c: int) -> int:
    return int(lib().mi355_tile_values(c))


def kernel_name(op: str, c: int) -> str:
    s = lib().mi355_kernel_name(op.encode(), c)
    if s is None:
        raise ValueError(op)
    return s.decode()


# ---- predicate constants -> C ABI arguments --------------------------------------------------------------------------
# ctypes masks an int that does not fit the argument's C type without an error (c_uint32(-1) is 0xffffffff, c_int64(2**64 + 5)
# is 5), so every constant a caller passes goes through one of these first: they give the C side a value of its type that
# selects exactly the rows the Python int selects, or raise.
def clamp_const(x: int) -> int:
    """a comparison constant of scan_where / scan_combine / scan_select / scan2 (any int) -> [-1, 2^32]: every decoded
    value lies in [0, 2^32), so this changes no comparison, and the result fits c_int64 with room for the +-1 of < and >"""
    return min(max(int(x), -1), 1 << 32)


def clamp_diff(x: int) -> int:
    """a comparison constant of scan_columns (any int) -> [-2^32, 2^32]: the difference of two decoded values lies strictly
    inside that range, so this changes no comparison, and the result fits c_int64"""
    return min(max(int(x), -(1 << 32)), 1 << 32)


def range_bounds(lo: int, hi: int) -> Optional[Tuple[int, int]]:
    """scan_range's inclusive bounds (any ints) -> (lo, hi) within [0, 2^32), or None when no value can lie in between
    (the rules of the C++ drop-in scan(int, int) in include/simd_scan.hpp, extended to ints beyond 32 bits)"""
    lo, hi = int(lo), int(hi)
    if hi < 0 or lo > hi or lo >= 1 << 32:
        return None
    return max(lo, 0), min(hi, 0xFFFFFFFF)


def key32(key: int, c: int) -> int:
    """an equality / IN-list key -> the int32 the C ABI takes.  Keys in [-2^31, 2^32) keep their meaning: the unsigned
    32-bit pattern is compared with the decoded value, so at c = 32 a key in [-2^31, 0) matches key + 2^32, below c = 32 it
    matches nothing.  Any other key matches nothing below c = 32 (it becomes -1, i.e. 0xffffffff >= 2^c); at c = 32 every
    int32 pattern is a value of the column, so it raises ValueError."""
    k = int(key)
    if -(1 << 31) <= k < 1 << 31:
        return k
    if 1 << 31 <= k < 1 << 32:
        return k - (1 << 32)
    if c == 32:
        raise ValueError(f"key {k} is outside [-2^31, 2^32): at c = 32 no int32 key stands for it")
    return -1


def keys32(keys: Sequence[int], c: int) -> np.ndarray:
    """key32 over a key list -> contiguous int32 array"""
    return np.ascontiguousarray(np.array([key32(k, c) for k in keys], dtype=np.int32))


CMP = {"==": 0, "!=": 1, "<": 2, "<=": 3, ">": 4, ">=": 5, "between": 6, "not_between": 7}


def predicates(preds: Sequence[Tuple]) -> "C.Array":
    """(op, a) / (op, a, b) tuples, op spelled as scan_where spells it and a, b any ints -> the mi355_predicate array of
    mi355_shared_scan_where_dev.  Constants go through clamp_const; b is 0 where the op does not read it."""
    arr = (_capi.Predicate * max(len(preds), 1))()
    for i, p in enumerate(preds):
        if len(p) not in (2, 3):
            raise ValueError(f"predicate {i}: expected (op, a) or (op, a, b), got {p!r}")
        op = CMP[p[0]]
        arr[i].op = op
        arr[i].reserved = 0
        arr[i].a = clamp_const(p[1])
        arr[i].b = clamp_const(p[2]) if len(p) == 3 and op >= 6 else 0
    return arr


def shared_where_kernel(c: int, P: int, layout: str = "per_predicate", with_hits: bool = True) -> str:
    """kernel family a shared where-scan of P predicates at width c launches (mi355_shared_where_kernel; needs a device)"""
    code = {"per_predicate": _capi.LAYOUT_PER_PREDICATE, "linear": _capi.LAYOUT_LINEAR}[layout]
    s = lib().mi355_shared_where_kernel(None, c, P, code, 1 if with_hits else 0)
    if s is None:
        raise ValueError((c, P, layout))
    return s.decode()


def _table_kernel(query, count: int, what: tuple) -> str:
    """the kernel family by the size of a device-resident set or table: `count` outside 0..2^32 (ctypes would wrap it) or an
    answer of NULL (a width the library does not have) -> ValueError(what)"""
    if not 0 <= int(count) <= 1 << 32:
        raise ValueError(what)
    s = query()
    if s is None:
        raise ValueError(what)
    return s.decode()


def semi_join_kernel(c: int, set_bits: int) -> str:
    """kernel family ScanEngine.semi_join launches for a set of set_bits bits at width c (mi355_semijoin_kernel; arithmetic
    only, needs no device): 'semijoin_lds_kernel' | 'semijoin_global_kernel'"""
    return _table_kernel(lambda: lib().mi355_semijoin_kernel(c, int(set_bits)), set_bits, (c, set_bits))


def lookup_kernel(c: int, table_rows: int, ct: int) -> str:
    """kernel family ScanEngine.lookup launches for a column of width c and a table of table_rows values of width ct
    (mi355_lookup_kernel; arithmetic only, needs no device): 'lookup_lds_kernel' | 'lookup_global_kernel'"""
    return _table_kernel(lambda: lib().mi355_lookup_kernel(c, int(table_rows), ct), table_rows, (c, table_rows, ct))


def value_set_kernel(c: int, set_bits: int) -> str:
    """kernel family ScanEngine.value_set launches for a set of set_bits bits at width c (mi355_value_set_kernel; arithmetic
    only, needs no device): 'value_set_lds_kernel' | 'value_set_global_kernel'"""
    return _table_kernel(lambda: lib().mi355_value_set_kernel(c, int(set_bits)), set_bits, (c, set_bits))


def key_index_kernel(ck: int, table_rows: int) -> str:
    """kernel family the first phase of ScanEngine.key_index launches for a table of table_rows entries at key width ck
    (mi355_key_index_kernel; arithmetic only, needs no device): 'key_index_lds_kernel' | 'key_index_global_kernel'"""
    return _table_kernel(lambda: lib().mi355_key_index_kernel(ck, int(table_rows)), table_rows, (ck, table_rows))


def _width_query(symbol: str, *widths: int):
    """what the library's `symbol` answers for bit widths: a width outside 0..2^32 (ctypes would wrap it) or an answer of NULL
    or 0 (a width the library does not have) -> ValueError(the width, or the tuple of them)"""
    answer = getattr(lib(), symbol)(*widths) if all(0 <= int(w) < 1 << 32 for w in widths) else None
    if not answer:
        raise ValueError(widths[0] if len(widths) == 1 else widths)
    return answer


def compact_kernel(c: int) -> str:
    """kernel ScanEngine.compact launches to write its values at width c (mi355_compact_kernel; arithmetic only, needs no
    device): 'compact_kernel'; a width outside 1..32 -> ValueError"""
    return _width_query("mi355_compact_kernel", c).decode()


def top_k_passes(c: int) -> int:
    """histogram passes over the column ScanEngine.top_k makes at width c, before the one that writes the bitmap
    (mi355_top_k_passes; arithmetic only, needs no device): 1 | 2 | 3; a width outside 1..32 -> ValueError"""
    return int(_width_query("mi355_top_k_passes", c))


def sort_rows_passes(c: int) -> int:
    """passes ScanEngine.sort_rows makes at width c, one per 8-bit digit (mi355_sort_rows_passes; arithmetic only, needs no
    device): 1 | 2 | 3 | 4; a width outside 1..32 -> ValueError"""
    return int(_width_query("mi355_sort_rows_passes", c))


GROUP_WIDE_MAX_GROUPS = 1 << 26  # MI355_GROUP_WIDE_MAX_GROUPS


def group_wide_front_slots(ck: int, cv: int) -> int:
    """slots of the LDS front a block of ScanEngine.group_aggregate_wide keeps at key width ck and value width cv
    (mi355_group_wide_front_slots; arithmetic only, needs no device): 4096 | 2048 | 1024; a width outside 1..32 -> ValueError"""
    return int(_width_query("mi355_group_wide_front_slots", ck, cv))


ARITH_OPS = {"linear": 0, "mul": 1}  # MI355_ARITH_LINEAR, MI355_ARITH_MUL


def _arith_operands(op: str, c1: int, c2: int, a: int, b: Optional[int], k: int) -> Tuple[int, int, int, int]:
    """(op code, a, b, k) as the C ABI takes them: b defaults to 1 ("linear") or 0 ("mul"); an unknown op, a width outside
    1..32, a or b outside int32, k outside int64 (ctypes would wrap them silently) or b != 0 with "mul" -> ValueError"""
    if op not in ARITH_OPS:
        raise ValueError(f"op {op!r} is neither 'linear' nor 'mul'")
    if b is None:
        b = 0 if op == "mul" else 1
    a, b, k = int(a), int(b), int(k)
    if not (1 <= int(c1) <= 32 and 1 <= int(c2) <= 32):
        raise ValueError(f"widths {c1}, {c2} outside 1..32")
    if not (-(1 << 31) <= a < 1 << 31 and -(1 << 31) <= b < 1 << 31 and -(1 << 63) <= k < 1 << 63):
        raise ValueError(f"a={a}, b={b} must be int32 and k={k} int64")
    if op == "mul" and b != 0:
        raise ValueError(f"b={b} must be 0 with 'mul'")
    return ARITH_OPS[op], a, b, k


def arith_range(op: str, c1: int, c2: int, a: int = 1, b: Optional[int] = None, k: int = 0) -> Tuple[int, int]:
    """(lo, hi), in Python ints: the bounds of a x + b y + k ("linear") or a x y + k ("mul") over all x < 2^c1, y < 2^c2 -- the
    range rule of include/mi355_arith.h.  ScanEngine.arith needs both inside int64; inside [0, 2^co) no row can miss."""
    _, a, b, k = _arith_operands(op, c1, c2, a, b, k)
    X, Y = (1 << int(c1)) - 1, (1 << int(c2)) - 1
    terms = [a * X * Y] if op == "mul" else [a * X, b * Y]
    return sum(min(0, t) for t in terms) + k, sum(max(0, t) for t in terms) + k


def arith_kernel(op: str, c1: int, c2: int, a: int = 1, b: Optional[int] = None, k: int = 0, co: Optional[int] = None) -> str:
    """kernel family ScanEngine.arith launches (mi355_arith_kernel; arithmetic only, needs no device): 'arith_exact_kernel' when
    no row can leave [0, 2^co), else 'arith_checked_kernel'; co=None: the width ScanEngine.arith would pick.  What the call
    would refuse -> ValueError"""
    code, a, b, k = _arith_operands(op, c1, c2, a, b, k)
    if co is None:
        co = arith_width(op, c1, c2, a, b, k)
    s = lib().mi355_arith_kernel(code, c1, c2, a, b, k, co) if 0 <= int(co) < 1 << 32 else None
    if s is None:
        raise ValueError((op, c1, c2, a, b, k, co))
    return s.decode()


def arith_width(op: str, c1: int, c2: int, a: int = 1, b: Optional[int] = None, k: int = 0) -> int:
    """the smallest output width that holds every result: lo < 0 or hi >= 2^32 -> ValueError (name a width and a miss value)"""
    lo, hi = arith_range(op, c1, c2, a, b, k)
    if lo < 0 or hi >= 1 << 32:
        raise ValueError(f"results span [{lo}, {hi}]: no width of 1..32 bits holds them all; pass co (and miss)")
    return max(1, hi.bit_length())


RUNNING_CHUNK_ROWS = 16384  # rows a wave of ScanEngine.running_sum sums into one word of the workspace


def _int64_arg(x: int, name: str) -> int:
    """an int on its way to an int64 C argument (ctypes would wrap it silently)"""
    x = int(x)
    if not -(1 << 63) <= x < 1 << 63:
        raise ValueError(f"{name}={x} must be int64")
    return x


def running_sum_range(c: int, n: int, b: int = 0, k: int = 0) -> Tuple[int, int]:
    """(lo, hi), in Python ints: the bounds of every partial sum k + sum(x_j + b) over up to n rows of c bits -- the range rule
    of include/mi355_running.h.  ScanEngine.running_sum needs both inside int64; inside [0, 2^co) no row can miss."""
    if not 1 <= int(c) <= 32:
        raise ValueError(f"width {c} outside 1..32")
    n, b, k = int(n), int(b), int(k)
    return k + n * min(0, b), k + n * max(0, (1 << int(c)) - 1 + b)


def running_sum_workspace_words(n: int) -> int:
    """64-bit words of workspace ScanEngine.running_sum needs for n rows (mi355_running_sum_workspace_words; arithmetic only)"""
    return int(lib().mi355_running_sum_workspace_words(_unsigned(n, 1 << 64, "n {}")))


def running_sum_kernel(c: int, n: int, b: int = 0, k: int = 0, co: Optional[int] = None) -> str:
    """kernel family ScanEngine.running_sum launches last (mi355_running_sum_kernel; arithmetic only, needs no device):
    'running_sum_exact_kernel' when no partial sum can leave [0, 2^co), else 'running_sum_checked_kernel'; co=None: the width
    ScanEngine.running_sum would pick.  What the call would refuse -> ValueError"""
    b, k, n = _int64_arg(b, "b"), _int64_arg(k, "k"), _unsigned(n, 1 << 64, "n {}")
    if co is None:
        co = _running_sum_width(c, n, b, k)
    ok = all(0 <= int(w) < 1 << 32 for w in (c, co))
    s = lib().mi355_running_sum_kernel(int(c), n, b, k, int(co)) if ok else None
    if s is None:
        raise ValueError((c, n, b, k, co))
    return s.decode()


def _running_sum_width(c: int, n: int, b: int, k: int) -> int:
    """the smallest output width that holds every partial sum: lo < 0 or hi >= 2^32 -> ValueError"""
    lo, hi = running_sum_range(c, n, b, k)
    if lo < 0 or hi >= 1 << 32:
        raise ValueError(f"partial sums span [{lo}, {hi}]: no width of 1..32 bits holds them all; pass co (and miss)")
    return max(1, hi.bit_length())


def _delta_width(c: int, k: int) -> int:
    """the width that holds the largest possible difference k + 2^c - 1 (k = 0: c; k = 2^c - 1: c + 1): beyond 32 bits -> ValueError"""
    if not 1 <= int(c) <= 32:
        raise ValueError(f"width {c} outside 1..32")
    hi = int(k) + (1 << int(c)) - 1
    if hi >= 1 << 32:
        raise ValueError(f"differences reach {hi}: no width of 1..32 bits holds them all; pass co (and miss)")
    return max(1, hi.bit_length())


def delta_kernel(c: int, k: int = 0, co: Optional[int] = None) -> str:
    """kernel family ScanEngine.delta launches (mi355_delta_kernel; arithmetic only, needs no device): 'delta_exact_kernel' when
    k >= 2^c - 1 and k + 2^c - 1 < 2^co, else 'delta_checked_kernel'; co=None: the width ScanEngine.delta would pick.  A width
    outside 1..32 -> ValueError"""
    k = _int64_arg(k, "k")
    if co is None:
        co = _delta_width(c, k)
    s =lib().mi355_delta_kernel(int(c), k, int(co)) if all(0 <= int(w) < 1 << 32 for w in (c, co)) else None
    if s is None:
        raise ValueError((c, k, co))
    return s.decode()


def run_encode_workspace_words(n: int) -> int:
    """64-bit words of workspace ScanEngine.run_encode needs for n rows (mi355_run_encode_workspace_words; arithmetic only)"""
    return int(lib().mi355_run_encode_workspace_words(_unsigned(n, 1 << 64, "n {}")))


def run_encode_kernel(c: int, ce: int) -> str:
    """the emitting kernel of ScanEngine.run_encode (mi355_run_encode_kernel; arithmetic only, needs no device).  A width outside
    1..32 -> ValueError"""
    s = lib().mi355_run_encode_kernel(int(c), int(ce)) if all(0 <= int(w) < 1 << 32 for w in (c, ce)) else None
    if s is None:
        raise ValueError((c, ce))
    return s.decode()


def run_decode_kernel(cv: int, ce: int) -> str:
    """the kernel of ScanEngine.run_decode (mi355_run_decode_kernel; arithmetic only, needs no device).  A width outside 1..32 ->
    ValueError"""
    s = lib().mi355_run_decode_kernel(int(cv), int(ce)) if all(0 <= int(w) < 1 << 32 for w in (cv, ce)) else None
    if s is None:
        raise ValueError((cv, ce))
    return s.decode()


def run_aggregate_kernel(cv: int, ce: int) -> str:
    """the aggregating kernel of ScanEngine.run_aggregate (mi355_run_aggregate_kernel; arithmetic only, needs no device).  A width
    outside 1..32 -> ValueError"""
    return _width_query("mi355_run_aggregate_kernel", cv, ce).decode()


def run_aggregate_span_slots(cv: int) -> int:
    """slots S of the span table a wave of ScanEngine.run_aggregate keeps at value width cv (mi355_run_aggregate_span_slots;
    arithmetic only, needs no device): a power of two; a tile of 2048 rows that touches more than S runs takes the dense path.
    A width outside 1..32 -> ValueError"""
    return int(_width_query("mi355_run_aggregate_span_slots", cv))


def search_sorted_kernel(c: int, ct: int, co: int, rows: int) -> str:
    """kernel family ScanEngine.search_sorted launches for a column of width c, a table of `rows` entries of width ct and positions
    of width co (mi355_search_sorted_kernel; arithmetic only, needs no device): 'search_lds_kernel' | 'search_global_kernel'.
    A width outside 1..32 or rows outside 0..2^32 - 1 -> ValueError"""
    ok = all(0 <= int(w) < 1 << 32 for w in (c, ct, co)) and 0 <= int(rows) < 1 << 64
    s = lib().mi355_search_sorted_kernel(int(c), int(ct), int(co), int(rows)) if ok else None
    if s is None:
        raise ValueError((c, ct, co, rows))
    return s.decode()


def search_sorted_stride(rows: int) -> int:
    """the distance S of the table samples a block of ScanEngine.search_sorted keeps in LDS (mi355_search_sorted_stride;
    arithmetic only): 1 where the whole table fits"""
    return int(lib().mi355_search_sorted_stride(_unsigned(rows, 1 << 32, "rows {} beyond 2^32 - 1")))


def _ends_width(n: int, ends_width: Optional[int]) -> int:
    """the width of a column of run ends over n rows: the one that holds n itself (None), or the caller's when it does"""
    n = _unsigned(n, 1 << 32, "n {} beyond 2^32 - 1 rows: an end of at most 32 bits cannot hold it")
    if ends_width is None:
        return max(1, n.bit_length())
    ce = int(ends_width)
    if not 1 <= ce <= 32:
        raise ValueError(f"ends_width {ce} outside 1..32")
    if n > (1 << ce) - 1:
        raise ValueError(f"n {n} beyond 2^{ce} - 1: an end of {ce} bits cannot hold it")
    return ce


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """an optional tensor as a pointer argument: None travels as NULL"""
    return t.data_ptr() if t is not None else None


def _col_ptr(col: "PackedColumn") -> Optional[int]:
    """a column's data as a pointer argument: an empty column travels as NULL"""
    return col.data.data_ptr() if col.n else None


def _unsigned(x: int, limit: int, message: str) -> int:
    """an int on its way to an unsigned C argument -> int(x) where 0 <= x < limit, else ValueError(message, the value in the
    place of its {}): ctypes would wrap it silently"""
    x = int(x)
    if not 0 <= x < limit:
        raise ValueError(message.format(x))
    return x


class PackedColumn:
    """A bit-packed column resident in HBM: `n` values of `c` bits, reference stream format."""

    def __init__(self, data: torch.Tensor, n: int, c: int):
        assert data.dtype == torch.uint8 and data.is_cuda
        self.data, self.n, self.c = data, int(n), int(c)

    @property
    def payload_bytes(self) -> int:
        return (self.n * self.c + 7) // 8


class ScanEngine:
    def __init__(self, device: Optional[int] = None, stream: Optional[torch.cuda.Stream] = None):
        if not torch.cuda.is_available():
            raise _capi.Mi355Error("no GPU visible: shared_simd_scan_amd has no CPU fallback")
        self.device = torch.cuda.current_device() if device is None else int(device)
        with torch.cuda.device(self.device):
            self.stream = stream if stream is not None else torch.cuda.current_stream()
        self._ctx = C.c_void_p()
        check(lib().mi355_ctx_create(self.device, C.c_void_p(self.stream.cuda_stream), C.byref(self._ctx)))
        self._dev = torch.device("cuda", self.device)

    def close(self) -> None:
        if getattr(self, "_ctx", None) is not None and self._ctx:
            lib().mi355_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name: str, value: int) -> None:
        check(lib().mi355_ctx_set_option(self._ctx, name.encode(), int(value)))

    TUNE_KINDS = {"scan": 1, "count": 2, "mask": 4, "decompress": 8, "all": 15}

    def tune(self, col: "PackedColumn", what: str = "all") -> dict:
        """mi355_tune_dev: measure 1 / 2 / 4 resident blocks per CU on this column (>= 5e7 rows; blocks) and keep the
        fastest for later launches of that kind and width.  Returns what was kept ({} for a small column)."""
        mask = 0
        for kind in what.split("+"):
            mask |= self.TUNE_KINDS[kind]
        check(lib().mi355_tune_dev(self._ctx, col.data.data_ptr(), col.n, col.c, mask))
        return self.tuned(col.c)

    def tuned(self, c: int) -> dict:
        got = {"scan_eq": lib().mi355_tuned_blocks_per_cu(self._ctx, c, 1, 0), "scan_range": lib().mi355_tuned_blocks_per_cu(self._ctx, c, 1, 1),
               "count": lib().mi355_tuned_blocks_per_cu(self._ctx, c, 2, 0), "mask": lib().mi355_tuned_blocks_per_cu(self._ctx, c, 4, 0),
               "decompress": lib().mi355_tuned_blocks_per_cu(self._ctx, c, 8, 0)}
        return {k: v for k, v in got.items() if v}

    def use_stream(self, stream: torch.cuda.Stream) -> None:
        """enqueue subsequent work on `stream` (e.g. the capture stream inside torch.cuda.graph)"""
        self.stream = stream
        check(lib().mi355_ctx_set_stream(self._ctx, C.c_void_p(stream.cuda_stream)))

    def synchronize(self) -> None:
        check(lib().mi355_ctx_synchronize(self._ctx))

    # ---- allocation -----------------------------------------------------------------------
    def _empty(self, nbytes: int, dtype=torch.uint8) -> torch.Tensor:
        return torch.empty(nbytes, dtype=dtype, device=self._dev)

    def _int64(self, k: int = 1) -> torch.Tensor:
        """a device result of k counters"""
        return self._empty(k, torch.int64)

    def _packed_out(self, out: Optional[torch.Tensor], c: int, n: int, need: int) -> torch.Tensor:
        """the buffer of a packed result of n values of c bits: allocated with the stream format's pad when None, else checked
        against the `need` bytes the call writes at most"""
        if out is None:
            return self._empty(compressed_buffer_size(c, n))
        assert out.dtype == torch.uint8 and out.numel() >= need
        return out

    def alloc_packed(self, n: int, c: int) -> PackedColumn:
        return PackedColumn(self._empty(compressed_buffer_size(c, n)), n, c)

    # ---- compression (src/simd_scan_compression.cpp:53-104) ----------------------------------
    def compress(self, values: torch.Tensor, c: int) -> PackedColumn:
        """values: uint16 / int32 / uint32-as-int32 tensor on this device -> packed column."""
        values = values.to(self._dev).contiguous()
        n = values.numel()
        col = self.alloc_packed(n, c)
        if values.dtype in (torch.uint16, torch.int16):
            check(lib().mi355_pack_u16_dev(self._ctx, values.data_ptr(), n, c, col.data.data_ptr()))
        elif values.dtype in (torch.int32, torch.uint32):
            check(lib().mi355_pack_u32_dev(self._ctx, values.data_ptr(), n, c, col.data.data_ptr()))
        else:
            raise TypeError(f"values dtype {values.dtype}: need a 16- or 32-bit integer tensor")
        return col

    def slice_rows(self, col: PackedColumn, first: int, last: int) -> PackedColumn:
        """View of rows [first, last) of a resident column (no copy).  `first` must be a multiple of 128 rows so the
        slice starts on a whole value, 16-byte aligned; a slice that ends inside the column is followed by the next
        rows instead of the zero pad, which only feeds result bits >= n (masked by every kernel)."""
        if first % 128 or not (0 <= first <= last <= col.n):
            raise ValueError("slice_rows: first must be a multiple of 128 and 0 <= first <= last <= n")
        return PackedColumn(col.data[first * col.c // 8:], last - first, col.c)

    def generate(self, kind: str, n: int, c: int, param: int = 0, first_row: int = 0) -> PackedColumn:
        """Synthesise a packed column on the device: 'mod' | 'splitmix' | 'index' (SURVEY 8d)."""
        code = {"mod": _capi.GEN_MOD, "splitmix": _capi.GEN_SPLITMIX, "index": _capi.GEN_INDEX}[kind]
        col = self.alloc_packed(n, c)
        check(lib().mi355_generate_dev(self._ctx, code, first_row, n, c, param, col.data.data_ptr()))
        return col

    # ---- decompression (src/simd_scan_decompression.cpp) --------------------------------------
    def decompress(self, col: PackedColumn, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        if out is None:
            out = self._empty(col.n, torch.int32)
        assert out.dtype == torch.int32 and out.numel() >= col.n
        check(lib().mi355_decompress_dev(self._ctx, col.data.data_ptr(), col.n, col.c, out.data_ptr()))
        return out

    # ---- scans (src/simd_scan.cpp) -------------------------------------------------------------
    def alloc_bitmap(self, n: int) -> torch.Tensor:
        return self._empty((n + 7) // 8)

    def _outputs(self, n: int, bitmap, hits, count_only: bool = False):
        """the scans' output defaults -> (bitmap, hits): a bitmap of n rows unless one is given (none at all with count_only),
        one int64 hit count unless one is given"""
        if count_only:
            bitmap = None
        elif bitmap is None:
            bitmap = self.alloc_bitmap(n)
        if hits is None:
            hits = self._int64()
        return bitmap, hits

    def scan(self, key: int, col: PackedColumn, bitmap: Optional[torch.Tensor] = None,
             hits: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """value == key -> (bitmap uint8[ceil(n/8)], hits int64[1]); asynchronous on the stream."""
        bitmap, hits = self._outputs(col.n, bitmap, hits)
        check(lib().mi355_scan_eq_dev(self._ctx, col.data.data_ptr(), col.n, col.c, key32(key, col.c), bitmap.data_ptr(),
                                      hits.data_ptr()))
        return bitmap, hits

    def scan_range(self, lo: int, hi: int, col: PackedColumn, bitmap: Optional[torch.Tensor] = None,
                   hits: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """lo <= value <= hi (src/simd_scan.hpp:76-84); any ints, compared exactly."""
        bitmap, hits = self._outputs(col.n, bitmap, hits)
        lo, hi = range_bounds(lo, hi) or (1, 0)  # lo > hi: the C side stores the empty result
        check(lib().mi355_scan_range_dev(self._ctx, col.data.data_ptr(), col.n, col.c, lo, hi, bitmap.data_ptr(),
                                         hits.data_ptr()))
        return bitmap, hits

    # ---- beyond the reference: general comparisons, conjunctions, bitmap consumers -----
    _CMP = CMP
    _BOP = {"and": 0, "or": 1, "xor": 2, "andnot": 3}

    def scan_where(self, op: str, a: int, col: PackedColumn, b: int = 0, and_mask: Optional[torch.Tensor] = None,
                   bitmap: Optional[torch.Tensor] = None, hits: Optional[torch.Tensor] = None):
        """bitmap[i] = (value_i OP a [, b]) [& and_mask[i]]; op in == != < <= > >= between not_between."""
        bitmap, hits = self._outputs(col.n, bitmap, hits)
        check(lib().mi355_scan_where_dev(self._ctx, col.data.data_ptr(), col.n, col.c, self._CMP[op], clamp_const(a), clamp_const(b),
                                         _ptr(and_mask), bitmap.data_ptr(), hits.data_ptr()))
        return bitmap, hits

    def scan_combine(self, op: str, a: int, col: PackedColumn, b: int = 0, mask: Optional[torch.Tensor] = None,
                     mask_op: str = "and", bitmap: Optional[torch.Tensor] = None, hits: Optional[torch.Tensor] = None,
                     count_only: bool = False):
        """scan_where with the earlier bitmap combined by AND / OR / XOR / ANDNOT (mask & ~p) inside the scan;
        count_only=True stores no bitmap at all (returns (None, hits))."""
        bitmap, hits = self._outputs(col.n, bitmap, hits, count_only)
        check(lib().mi355_scan_combine_dev(self._ctx, col.data.data_ptr(), col.n, col.c, self._CMP[op], clamp_const(a), clamp_const(b),
                                           self._BOP[mask_op], _ptr(mask), _ptr(bitmap), hits.data_ptr()))
        return bitmap, hits

    def scan2(self, col1: PackedColumn, op1: str, a1: int, col2: PackedColumn, op2: str, a2: int, b1: int = 0, b2: int = 0,
              combine: str = "and", bitmap: Optional[torch.Tensor] = None, hits: Optional[torch.Tensor] = None,
              count_only: bool = False):
        """predicates over two columns of the same row count, combined (and / or / xor / andnot = p1 & ~p2) in one call;
        same-width columns run as a single launch"""
        assert col1.n == col2.n
        bitmap, hits = self._outputs(col1.n, bitmap, hits, count_only)
        check(lib().mi355_scan2_dev(self._ctx, col1.data.data_ptr(), col1.c, self._CMP[op1], clamp_const(a1), clamp_const(b1),
                                    col2.data.data_ptr(), col2.c, self._CMP[op2], clamp_const(a2), clamp_const(b2), col1.n, self._BOP[combine],
                                    _ptr(bitmap), hits.data_ptr()))
        return bitmap, hits

    def scan_columns(self, col1: PackedColumn, op: str, col2: PackedColumn, a: int = 0, b: int = 0, mask: Optional[torch.Tensor] = None,
                     mask_op: str = "and", bitmap: Optional[torch.Tensor] = None, hits: Optional[torch.Tensor] = None,
                     count_only: bool = False):
        """bitmap[i] = (col1_i - col2_i) OP a [, b], the exact integer difference of the two rows: col1 < col2 is ("<", a=0),
        col1 >= col2 + 30 is (">=", a=30), |col1 - col2| <= 3 is ("between", a=-3, b=3).  Any width pair, one launch; mask,
        mask_op, bitmap, hits and count_only as in scan_combine."""
        assert col1.n == col2.n
        bitmap, hits = self._outputs(col1.n, bitmap, hits, count_only)
        check(lib().mi355_scan_columns_dev(self._ctx, col1.data.data_ptr(), col1.c, col2.data.data_ptr(), col2.c, col1.n, self._CMP[op],
                                           clamp_diff(a), clamp_diff(b), self._BOP[mask_op], _ptr(mask), _ptr(bitmap), hits.data_ptr()))
        return bitmap, hits

    def scan_select(self, op: str, a: int, col: PackedColumn, capacity: int, b: int = 0, mask: Optional[torch.Tensor] = None,
                    mask_op: str = "and", first_row: int = 0):
        """predicate (optionally combined with an earlier bitmap) -> (int64 ascending row ids [capacity], count int64[1])
        in one launch, no bitmap in HBM; ids beyond `capacity` are dropped, count is the total."""
        rowids, count = self._int64(max(capacity, 1)), self._int64()
        check(lib().mi355_scan_select_dev(self._ctx, col.data.data_ptr(), col.n, col.c, self._CMP[op], clamp_const(a), clamp_const(b),
                                          self._BOP[mask_op], _ptr(mask), first_row,
                                          rowids.data_ptr(), capacity, count.data_ptr()))
        return rowids, count

    def scan_in(self, keys: Sequence[int], col: PackedColumn, negate: bool = False,
                and_mask: Optional[torch.Tensor] = None, bitmap: Optional[torch.Tensor] = None,
                hits: Optional[torch.Tensor] = None):
        """bitmap[i] = value_i in keys (NOT IN with negate=True) [& and_mask[i]].  Every P is uploaded per call; never
        capturable into a graph (refused while the stream is capturing)."""
        k = keys32(keys, col.c)
        bitmap, hits = self._outputs(col.n, bitmap, hits)
        check(lib().mi355_scan_in_dev(self._ctx, col.data.data_ptr(), col.n, col.c, k.ctypes.data, int(k.shape[0]),
                                      1 if negate else 0, _ptr(and_mask), bitmap.data_ptr(), hits.data_ptr()))
        return bitmap, hits

    def semi_join(self, col: PackedColumn, set_bitmap: Optional[torch.Tensor], set_bits: int, negate: bool = False,
                  and_mask: Optional[torch.Tensor] = None, bitmap=None, want_hits: bool = True):
        """bitmap[i] = (value_i < set_bits and bit value_i of set_bitmap) (NOT IN with negate=True) [& and_mask[i]] -> (bitmap,
        hits): `fk IN (SELECT pk FROM dim WHERE ...)` with set_bitmap the result bitmap of a scan over the set_bits rows of
        `dim`, consumed where it lies (uint8 device tensor of at least ceil(set_bits/8) bytes; None only with set_bits == 0).
        Capturable into a graph: the set is read at every replay.  bitmap=False: count only, no bitmap is stored (returns
        (None, hits)); want_hits=False: no count (returns (bitmap, None))."""
        set_bits = _unsigned(set_bits, (1 << 32) + 1, "set_bits {} outside 0..2^32")
        if set_bitmap is None:
            assert set_bits == 0
        else:
            assert set_bitmap.dtype == torch.uint8 and set_bitmap.numel() >= (set_bits + 7) // 8
        count_only = bitmap is False
        assert not (count_only and not want_hits), "neither a bitmap nor a count asked for"
        if bitmap is None:
            bitmap = self.alloc_bitmap(col.n)
        hits = self._int64() if want_hits else None
        check(lib().mi355_semijoin_dev(self._ctx, col.data.data_ptr(), col.n, col.c, _ptr(set_bitmap),
                                       set_bits, 1 if negate else 0, _ptr(and_mask),
                                       None if count_only else bitmap.data_ptr(), _ptr(hits)))
        return (None if count_only else bitmap), hits

    def lookup(self, col: PackedColumn, table: PackedColumn, miss: int = 0, out: Optional[torch.Tensor] = None) -> PackedColumn:
        """out[i] = table[value_i] if value_i < table.n else miss, as a packed column of col.n values of table.c bits: for every
        fact row the attribute of the dimension row its key points at (then `group_aggregate` by it, or any scan over it), or
        a dictionary re-code.  `out`: a uint8 device tensor of at least compressed_buffer_size(table.c, col.n) bytes that
        overlaps neither input (allocated when None).  Capturable into a graph: the table is read at every replay."""
        miss = _unsigned(miss, 1 << table.c, f"miss {{}} is no value of {table.c} bits")
        out = self._packed_out(out, table.c, col.n, (col.n * table.c + 7) // 8)
        check(lib().mi355_lookup_dev(self._ctx, col.data.data_ptr(), col.n, col.c, _col_ptr(table), table.n, table.c, miss, out.data_ptr()))
        return PackedColumn(out, col.n, table.c)

    def arith(self, op: str, col1: PackedColumn, col2: PackedColumn, a: int = 1, b: Optional[int] = None, k: int = 0,
              co: Optional[int] = None, miss: int = 0, out: Optional[torch.Tensor] = None,
              out_of_range: Optional[torch.Tensor] = None) -> PackedColumn:
        """out[i] = r_i if 0 <= r_i < 2^co else miss, r_i = a x_i + b y_i + k (op "linear", b defaults to 1) or a x_i y_i + k
        (op "mul", b must be 0) on the rows of col1 and col2, exact integers, as a packed column of co bits: the composite key
        g1 * |g2| + g2 for `group_aggregate`, the product under sum(price * discount) for `aggregate`, a difference as a
        column.  co=None: the smallest width that holds every possible result (arith_width; ValueError when none does).
        `out`: a uint8 device tensor of at least compressed_buffer_size(co, n) bytes that overlaps neither input (allocated
        when None).  `out_of_range`: an int64[1] device tensor that gets the number of rows replaced by miss (None: not
        counted).  The columns may be the same.  Capturable into a graph: both columns are read at every replay.  Measured
        (profiles/r11_arith.txt): 1e9 rows 9 x 9 -> 10 bit 5.8 x as fast as decompress -> torch -> compress, 9.6 x into 9 bit with
        half of the rows counted as out of range; 2.5e8 rows 20 x 4 -> 24 bit ("mul") only 1.86 x."""
        assert col1.n == col2.n
        code, a, b, k = _arith_operands(op, col1.c, col2.c, a, b, k)
        if co is None:
            co = arith_width(op, col1.c, col2.c, a, b, k)
        co, miss = int(co), int(miss)
        if not 1 <= co <= 32:
            raise ValueError(f"co {co} outside 1..32")
        miss = _unsigned(miss, 1 << co, f"miss {{}} is no value of {co} bits")
        out = self._packed_out(out, co, col1.n, (col1.n * co + 7) // 8)
        if out_of_range is not None:
            assert out_of_range.dtype == torch.int64 and out_of_range.numel() >= 1
        check(lib().mi355_arith_dev(self._ctx, code, col1.data.data_ptr(), col1.c, col2.data.data_ptr(), col2.c, col1.n, a, b, k, co, miss,
                                    out.data_ptr(), _ptr(out_of_range)))
        return PackedColumn(out, col1.n, co)

    def _running_workspace(self, words: int) -> torch.Tensor:
        """the engine's own grow-only workspace of running_sum (int64 words), kept between calls.  A call that needs more gets a
        larger one; the smaller ones stay alive as long as the engine, since a captured graph may still point at them"""
        kept = self.__dict__.setdefault("_running_ws", [])
        if not kept or kept[-1].numel() < words:
            kept.append(self._empty(max(words, 1), torch.int64))
        return kept[-1]

    def running_sum(self, col: PackedColumn, mask: Optional[torch.Tensor] = None, b: int = 0, k: int = 0, exclusive: bool = False,
                    co: Optional[int] = None, miss: int = 0, out: Optional[torch.Tensor] = None, result: Optional[torch.Tensor] = None,
                    workspace: Optional[torch.Tensor] = None) -> Tuple[PackedColumn, torch.Tensor]:
        """out[i] = r_i if 0 <= r_i < 2^co else miss for every row, r_i = k + the sum of x_j + b over the rows j <= i (j < i with
        exclusive=True) that `mask` selects (a result bitmap of col.n rows; None: all), exact integers, as a packed column of co
        bits -> (column, result int64[2]: k + the sum of all terms, the number of rows replaced by miss).  Delta decoding is
        b = the block's minimum delta and k = the value in front of the first row (delta_decode); a row's position among the
        selected rows is the exclusive sum of the bitmap as a 1-bit column (row_positions).  co=None: the smallest width that
        holds every possible partial sum (ValueError when none does, or when one can be negative).  `out`: a uint8 device tensor
        of at least compressed_buffer_size(co, n) bytes that overlaps no input (allocated when None).  `workspace`: an int64
        device tensor of at least running_sum_workspace_words(n) words, contents irrelevant (None: the engine's own grow-only
        one).  Nothing synchronises.  Capturable into a graph whatever its arguments and without a warm-up call (pass `out`,
        `result` and `workspace`, so that the graph's buffers are yours); column and mask are read at every replay.  Measured
        (profiles/r21_running_sum.txt): 1e9 rows of 2-bit deltas into 31 bit 13.6 x as fast as decompress -> torch.cumsum -> compress,
        the positions of a 1e9-row bitmap 16.3 x; 1.18 x a count-only scan plus arith into the same width."""
        b, k = _int64_arg(b, "b"), _int64_arg(k, "k")
        n = col.n
        if co is None:
            co = _running_sum_width(col.c, n, b, k)
        co = int(co)
        if not 1 <= co <= 32:
            raise ValueError(f"co {co} outside 1..32")
        miss = _unsigned(miss, 1 << co, f"miss {{}} is no value of {co} bits")
        if mask is not None:
            assert mask.dtype == torch.uint8 and mask.numel() >= (n + 7) // 8
        out = self._packed_out(out, co, n, (n * co + 7) // 8)
        if result is None:
            result = self._int64(2)
        assert result.dtype == torch.int64 and result.numel() >= 2
        words = running_sum_workspace_words(n)
        if workspace is None:
            workspace = self._running_workspace(words)
        assert workspace.dtype == torch.int64 and workspace.numel() >= words
        check(lib().mi355_running_sum_dev(self._ctx, _col_ptr(col), n, col.c, _ptr(mask), b, k, 1 if exclusive else 0, co, miss,
                                          out.data_ptr() if n else None, result.data_ptr(), workspace.data_ptr() if n else None))
        return PackedColumn(out, n, co), result

    def delta(self, col: PackedColumn, first: int = 0, k: int = 0, co: Optional[int] = None, miss: int = 0,
              out: Optional[torch.Tensor] = None, out_of_range: Optional[torch.Tensor] = None) -> PackedColumn:
        """out[i] = r_i if 0 <= r_i < 2^co else miss, r_i = x_i - x_{i-1} + k with x_{-1} = first, as a packed column of co bits:
        the encoder of a delta-coded column (k = 2^c - 1, co = c + 1 loses nothing; running_sum with b = -(2^c - 1), k = first
        gives the column back), and with k = 0, co = c the marks of where a sorted column's value changes (scan it with != 0).
        co=None: the width that holds the largest possible result k + 2^c - 1 (ValueError beyond 32 bits).  `out_of_range`: an
        int64[1] device tensor that gets the number of rows replaced by miss (None: not counted) -- with k = 0 the number of
        descents.  `out` as in arith.  Capturable into a graph whatever its arguments; the column is read at every replay."""
        k = _int64_arg(k, "k")
        if co is None:
            co = _delta_width(col.c, k)
        co = int(co)
        if not 1 <= co <= 32:
            raise ValueError(f"co {co} outside 1..32")
        first = _unsigned(first, 1 << col.c, f"first {{}} is no value of {col.c} bits")
        miss = _unsigned(miss, 1 << co, f"miss {{}} is no value of {co} bits")
        out = self._packed_out(out, co, col.n, (col.n * co + 7) // 8)
        if out_of_range is not None:
            assert out_of_range.dtype == torch.int64 and out_of_range.numel() >= 1
        check(lib().mi355_delta_dev(self._ctx, _col_ptr(col), col.n, col.c, first, k, co, miss, out.data_ptr() if col.n else None,
                                    _ptr(out_of_range)))
        return PackedColumn(out, col.n, co)

    def delta_decode(self, deltas: PackedColumn, first_value: int, min_delta: int = 0, co: int = 32):
        """the column a delta-coded one encodes: row i = first_value + the sum of delta_j + min_delta over j <= i, as
        running_sum(deltas, b=min_delta, k=first_value, co=co) -> (column, result int64[2]); result[1] counts the rows that did not
        fit co bits"""
        return self.running_sum(deltas, b=min_delta, k=first_value, co=co)

    def row_positions(self, bitmap: torch.Tensor, n: int):
        """for every row the number of selected rows in front of it -- row_number() - 1, and the slot `compact` gives a selected
        row: the exclusive running sum of the result bitmap read as a 1-bit column, at the width that holds n -> (column,
        result int64[2]; result[0] is the number of selected rows)"""
        n = _unsigned(n, 1 << 32, "n {} beyond what 32-bit positions hold")
        assert bitmap.dtype == torch.uint8 and bitmap.numel() >= (n + 7) // 8
        return self.running_sum(PackedColumn(bitmap, n, 1), exclusive=True, co=max(1, n.bit_length()))

    def is_sorted(self, col: PackedColumn, first: int = 0) -> torch.Tensor:
        """int64[1] on the device: the number of descents of the column (rows smaller than the row before; row 0 against
        `first`).  0 means sorted ascending.  No host read: the caller decides when to look"""
        counter = self._int64()
        self.delta(col, first=first, k=0, co=col.c, out_of_range=counter)
        return counter

    def run_encode(self, col: PackedColumn, capacity: Optional[int] = None, ends_width: Optional[int] = None, values=None, ends=None,
                   count: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
        """the runs of `col` -> (values, ends, count int64[1]): row i is a run's last row when i == n - 1 or x_i != x_{i+1}; `values`
        is a packed column's data at col.c bits with every run's value, `ends` one at ends_width bits with the row behind every
        run's last row, both in row order.  At most `capacity` runs are written (default col.n); count is always the number of
        runs.  ends_width=None: the width that holds n.  `values` / `ends`: uint8 device tensors of at least
        compressed_buffer_size(width, capacity) bytes that overlap nothing else (allocated when None); False: that output is not
        computed (values only is SELECT DISTINCT of a sorted column, ends only its group boundaries; None is returned in its
        place).  `workspace` as in running_sum.  delta(ends, first=0) is the run lengths (run_lengths), running_sum(lengths) the
        ends again; lookup(arith(ends - 1), running_sum(y)) -> delta is sum(y) per run.  Nothing synchronises.  Capturable into a
        graph whatever its arguments and without a warm-up call (pass the outputs, `count` and `workspace`); the column is read at
        every replay."""
        n = col.n
        ce = _ends_width(n, ends_width)
        capacity = _unsigned(n if capacity is None else capacity, 1 << 64, "capacity {}")
        most = min(capacity, n)
        if capacity and values is False and ends is False:
            raise ValueError("neither values nor ends asked for with capacity > 0")
        if values is not False:
            values = self._packed_out(values, col.c, most, (most * col.c + 31) // 32 * 4)  # whole dwords
        if ends is not False:
            ends = self._packed_out(ends, ce, most, (most * ce + 31) // 32 * 4)
        if count is None:
            count = self._int64()
        assert count.dtype == torch.int64 and count.numel() >= 1
        words = run_encode_workspace_words(n)
        if workspace is None:
            workspace = self._running_workspace(words)
        assert workspace.dtype == torch.int64 and workspace.numel() >= words
        given = lambda t: t.data_ptr() if (t is not False and capacity) else None
        check(lib().mi355_run_encode_dev(self._ctx, _col_ptr(col), n, col.c, ce, given(values), given(ends), capacity, count.data_ptr(),
                                         workspace.data_ptr() if n else None))
        return (None if values is False else values), (None if ends is False else ends), count

    def count_runs(self, col: PackedColumn) -> torch.Tensor:
        """int64[1] on the device: the number of runs of the column (rows that differ from the next row, and the last row).  Count
        only: two launches, no output column.  No host read: the caller decides when to look"""
        return self.run_encode(col, capacity=0, values=False, ends=False)[2]

    def run_lengths(self, ends_col: PackedColumn, co: Optional[int] = None) -> PackedColumn:
        """the run lengths of a column of run ends: delta(ends, first=0), at the ends' width unless `co` names one"""
        return self.delta(ends_col, first=0, k=0, co=ends_col.c if co is None else co)

    def run_decode(self, values_col: PackedColumn, ends_col: PackedColumn, n: int, runs=None, miss: int = 0, out: Optional[torch.Tensor] = None,
                   uncovered: Optional[torch.Tensor] = None) -> PackedColumn:
        """the column of n rows that the runs (values_col, ends_col) encode, packed at values_col.c bits: out[i] = values[j] for the
        first run j whose end lies behind row i, `miss` for the rows behind the last run.  `runs`: how many of the tables' entries
        count -- an int, or the int64[1] device tensor run_encode left (read on the device: nothing synchronises; at most
        min(values_col.n, ends_col.n) either way); None: all of them.  Ends must be non-decreasing; equal neighbours are runs of
        length zero (repeat).  `uncovered`: an int64[1] device tensor that gets the number of rows behind the last run (None:
        not counted).  `out` as in arith.  With values_col.c == 1 the result is the bitmap over the rows of a bitmap over the
        runs.  Capturable into a graph whatever its arguments; tables and `runs` are read at every replay."""
        n = _unsigned(n, 1 << 64, "n {}")
        table = min(values_col.n, ends_col.n)
        runs_dev = None
        if isinstance(runs, torch.Tensor):
            assert runs.dtype == torch.int64 and runs.numel() >= 1
            runs_dev, runs = runs, table
        else:
            runs = table if runs is None else _unsigned(runs, table + 1, f"runs {{}} beyond the tables' {table} entries")
        runs = _unsigned(runs, 1 << 32, "runs {} beyond 2^32 - 1")
        cv = values_col.c
        miss = _unsigned(miss, 1 << cv, f"miss {{}} is no value of {cv} bits")
        out = self._packed_out(out, cv, n, (n * cv + 7) // 8)
        if uncovered is not None:
            assert uncovered.dtype == torch.int64 and uncovered.numel() >= 1
        check(lib().mi355_run_decode_dev(self._ctx, _col_ptr(values_col) if runs else None, cv, _col_ptr(ends_col) if runs else None, ends_col.c, runs,
                                         _ptr(runs_dev), n, miss, out.data_ptr() if n else None, _ptr(uncovered)))
        return PackedColumn(out, n, cv)

    def repeat(self, values_col: PackedColumn, counts_col: PackedColumn, n: int, miss: int = 0, out: Optional[torch.Tensor] = None,
               uncovered: Optional[torch.Tensor] = None) -> PackedColumn:
        """repeat_interleave, packed: value j of values_col counts_col[j] times, on n rows -- running_sum(counts) at the width that
        holds every partial sum (32 bits at the most), then run_decode.  Runs that end beyond n are cut at n; the rows behind the
        sum of the counts get `miss`"""
        fits = counts_col.n * ((1 << counts_col.c) - 1) < 1 << 32  # else: 32 bits, and a sum beyond them ends behind every row
        ends, _ = self.running_sum(counts_col, co=None if fits else 32, miss=0 if fits else (1 << 32) - 1)
        return self.run_decode(values_col, ends, n, miss=miss, out=out, uncovered=uncovered)

    def runs_column(self, col: PackedColumn) -> Tuple[PackedColumn, PackedColumn]:
        """`run_encode` as two columns (values, ends): reads the count back (the one host read the row count of a new column needs)"""
        values, ends, count = self.run_encode(col)
        r = int(count.item())
        return PackedColumn(values, r, col.c), PackedColumn(ends, r, _ends_width(col.n, None))

    def run_aggregate(self, values: PackedColumn, ends: PackedColumn, runs=None, mask: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None, uncovered=False):
        """-> int64[runs, 4] device tensor: row j = (sum, count, min, max) of `values` over the rows of run j of `ends` (a column of
        run ends as run_encode leaves it: the row behind every run's last row, non-decreasing), among the rows of `mask` (a result
        bitmap; None = every row) -- the aggregates of a sort-based GROUP BY and of run-length-coded data: per sorted key, per
        session, per day.  `runs`: how many of the ends count -- an int, or the int64[1] device tensor run_encode left (read on
        the device: nothing synchronises; the table then has ends.n rows); None: all of them.  A run without a counted row -- a
        run of length zero, one the mask empties, an entry behind the device count -- reads (0, 0, -1, 0) like group_aggregate.
        Runs that end beyond values.n are cut there.  `uncovered`: True, or an int64[1] device tensor -> (table, counter): the
        number of counted rows behind the last run, which are aggregated nowhere.  One pass over the packed column; groups are
        contiguous, so the open run is carried in registers and memory sees atomics once per run and 16384 rows.  Capturable
        into a graph whatever its arguments and without a warm-up call (pass `out`); column, mask, ends and `runs` are read at
        every replay.  Measured (profiles/r24_run_aggregate.txt): 1e9 x 9 bit with mean run 4096 0.96 ms, mean run 64 2.82 ms,
        mean run 4 15.5 ms, against 1705 / 678 / 359 ms for decompress -> torch.repeat_interleave -> index_add_ /
        scatter_reduce_ / bincount; 4-5 x `aggregate` of the same column where runs are long, 14 x at mean run 64, 77 x at mean
        run 4: bound by dependent reads of the ends, not by bytes."""
        n = values.n
        runs_dev = None
        if isinstance(runs, torch.Tensor):
            assert runs.dtype == torch.int64 and runs.numel() >= 1
            runs_dev, runs = runs, ends.n
        else:
            runs = ends.n if runs is None else _unsigned(runs, ends.n + 1, f"runs {{}} beyond the table's {ends.n} entries")
        runs = _unsigned(runs, 1 << 32, "runs {} beyond 2^32 - 1")
        if mask is not None:
            assert mask.dtype == torch.uint8 and mask.numel() >= (n + 7) // 8
        if out is None:
            out = torch.empty((runs, 4), dtype=torch.int64, device=self._dev)
        assert tuple(out.shape) == (runs, 4) and out.dtype == torch.int64 and out.is_contiguous()
        if uncovered is True:
            uncovered = self._int64()
        counter = uncovered if isinstance(uncovered, torch.Tensor) else None
        if counter is not None:
            assert counter.dtype == torch.int64 and counter.numel() >= 1
        check(lib().mi355_run_aggregate_dev(self._ctx, _col_ptr(values), values.c, n, _ptr(mask) if n else None, _col_ptr(ends) if (n and runs) else None,
                                            ends.c, runs, _ptr(runs_dev), out.data_ptr() if runs else None, _ptr(counter)))
        return out if counter is None else (out, counter)

    def sorted_group_aggregate(self, keys: PackedColumn, values: PackedColumn, mask: Optional[torch.Tensor] = None):
        """SELECT k, sum(v), count(*), min(v), max(v) ... GROUP BY k for keys WITHOUT a dense domain (sparse 32-bit surrogate keys,
        more groups than group_aggregate_wide addresses) -> (group keys: a PackedColumn of keys.n entries at keys.c bits, ascending,
        of which the first `count` are set; aggregates int64[keys.n, 4] in that order; count int64[1]: the number of groups).  The
        sort-based plan, without a host read: sort_rows over all rows with its values -> compress -> run_encode; gather(values) in
        that order -> compress; with a `mask` the same gather of the mask as a 1-bit column, the bitmap in sorted order;
        run_aggregate.  Every key of the column is a group; one whose rows the mask leaves out shows count 0."""
        assert keys.n == values.n
        n = keys.n
        rowids, count, ordered = self.sort_rows(keys, with_values=True)
        sorted_keys = self.compress(ordered[:n], keys.c)
        group_keys, ends, groups = self.run_encode(sorted_keys)
        sorted_values = self.compress(self.gather(values, rowids, count)[:n], values.c)
        sorted_mask = None
        if mask is not None and n:
            assert mask.dtype == torch.uint8 and mask.numel() >= (n + 7) // 8
            bits = self._empty(compressed_buffer_size(1, n))  # the mask with a packed column's read pad behind it
            bits[: (n + 7) // 8].copy_(mask[: (n + 7) // 8])
            sorted_mask = self.compress(self.gather(PackedColumn(bits, n, 1), rowids, count)[:n], 1).data
        table = self.run_aggregate(sorted_values, PackedColumn(ends, n, _ends_width(n, None)), runs=groups, mask=sorted_mask)
        return PackedColumn(group_keys, n, keys.c), table, groups

    def compact(self, col: PackedColumn, bitmap: torch.Tensor, capacity: Optional[int] = None, out: Optional[torch.Tensor] = None):
        """the values of the rows of `col` whose bit is set in `bitmap` (a result bitmap of col.n rows), in row order, packed at
        col.c bits -> (uint8 device tensor: the data of a packed column, count int64[1]).  At most `capacity` values are written
        (default col.n); count is always the total.  `out`: a uint8 device tensor of at least
        compressed_buffer_size(col.c, capacity) bytes that overlaps neither input (allocated when None); exactly its first
        ceil(min(count, capacity) * col.c / 8) bytes are written.  Nothing synchronises.  Compact every column a query still needs
        with the one bitmap and they stay row-aligned.  Capturable into a graph after a warm-up call of at least this size;
        column and bitmap are read at every replay.  Measured (profiles/r10_compact.txt, 1e9 x 9 bit / 2.5e8 x 17 bit): faster than
        bitmap_to_rowids -> gather -> compress at density 1/2 (4.2 x / 2.3 x) and on clustered selections, 1.49 x / on par at
        1/8; at the measured densities 1/64 and 1/512 that route is the faster one (1.5-2 x and 2.7-3.5 x): it never reads the
        unselected rows."""
        capacity = _unsigned(col.n if capacity is None else capacity, 1 << 64, "capacity {}")
        assert bitmap.dtype == torch.uint8 and bitmap.numel() >= (col.n + 7) // 8
        out = self._packed_out(out, col.c, capacity, (capacity * col.c + 31) // 32 * 4)  # whole dwords
        count = self._int64()
        check(lib().mi355_compact_dev(self._ctx, _col_ptr(col), col.n, col.c, bitmap.data_ptr() if col.n else None,
                                      out.data_ptr() if capacity else None, capacity, count.data_ptr()))
        return out, count

    def compact_column(self, col: PackedColumn, bitmap: torch.Tensor) -> PackedColumn:
        """`compact` as a column: reads the count back (the one host read the row count of a new column needs)"""
        out, count = self.compact(col, bitmap)
        return PackedColumn(out, int(count.item()), col.c)

    def top_k(self, col: PackedColumn, k: int, largest: bool = True, mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
        """ORDER BY v [DESC] LIMIT k as a bitmap: of the rows of `col` whose bit is set in `mask` (every row when None) the
        min(k, their number) that come first by value -- descending with `largest`, else ascending -- then by row id; ties at the
        cut go to the lowest row ids -> (bitmap of col.n rows, result int64[4]: rows selected, the threshold value T = the k-th
        order statistic, selected rows strictly beyond T, qualifying rows equal to T).  `out`: a uint8 device tensor of at least
        ceil(col.n / 8) bytes for the bitmap (allocated when None); it may be `mask` itself -- the filter's bitmap narrowed in
        place -- and must not overlap it otherwise.  Nothing synchronises: k, threshold and ties stay on the device.  The bitmap
        feeds compact, bitmap_to_rowids, aggregate, group_aggregate and the fused-mask scans; the survivors are not sorted.
        Capturable into a graph after a warm-up call of at least this size; column and mask are read at every replay.  Measured
        (profiles/r13_top_k.txt, uniform values): 1e9 x 9 bit 0.71-0.84 ms against 38.7 ms for decompress -> torch.topk, 2.5e8 x 32 bit
        0.86-0.91 ms against 11.7 ms; an all-equal 1e9 x 9 bit column at k = n / 2 takes 3.83 ms."""
        k = _unsigned(k, 1 << 64, "k {}")
        nbytes = (col.n + 7) // 8
        if mask is not None:
            assert mask.dtype == torch.uint8 and mask.numel() >= nbytes
        if out is None:
            out = self.alloc_bitmap(col.n)
        else:
            assert out.dtype == torch.uint8 and out.numel() >= nbytes
        result = self._int64(4)
        check(lib().mi355_top_k_dev(self._ctx, _col_ptr(col), col.n, col.c, _ptr(mask) if col.n else None, k,
                                    1 if largest else 0, out.data_ptr() if col.n else None, result.data_ptr()))
        return out, result

    def kth_value(self, col: PackedColumn, k: int, largest: bool = True, mask: Optional[torch.Tensor] = None) -> int:
        """the k-th largest (smallest with largest=False) value among the rows `mask` selects, k counted from 1: a median, a
        percentile.  One `top_k`, then the threshold is read back: this SYNCHRONISES with the stream.  Fewer than k qualifying
        rows (or k < 1) -> ValueError."""
        _, result = self.top_k(col, k, largest=largest, mask=mask)
        m, threshold = (int(x) for x in result[:2].tolist())
        if k < 1 or m < k:
            raise ValueError(f"k {k} outside 1..{m}, the number of qualifying rows")
        return threshold

    def sort_rows(self, col: PackedColumn, descending: bool = False, mask: Optional[torch.Tensor] = None, capacity: Optional[int] = None,
                  first_row: int = 0, with_values: bool = False):
        """ORDER BY v [DESC] as row ids: the rows of `col` whose bit is set in `mask` (every row when None), ordered by value --
        descending or ascending -- then by row id (a stable sort, top_k's order) -> (rowids int64[capacity]: first_row + row,
        count int64[1]: the number of qualifying rows), with `with_values` also values (int32-viewed uint32 [capacity]: the
        values in that order).  All or nothing: with count > capacity (default col.n) nothing is written.  At most 2^32 rows.
        Nothing synchronises.  rowids and count are what `gather` takes; ORDER BY ... LIMIT k is `top_k`, then
        sort_rows(mask=its bitmap, capacity=k).  A stable LSD radix sort over the packed values, sort_rows_passes(col.c)
        passes of 8-bit digits.  Capturable into a graph after a warm-up call of at least this size; column and mask are read
        at every replay.  Measured (profiles/r16_sort_rows.txt, uniform values, ids and values out): 2.5e8 x 9 bit 3.44 ms against
        9.82 ms for decompress -> torch.sort, x 16 bit 5.06 ms against 10.40 ms, x 32 bit 11.44 ms against 11.44 ms (no gain); the top 1e6
        of 1e9 x 9 bit in order, top_k -> sort_rows, 1.93 ms against 38.2 ms for decompress -> torch.topk(sorted=True)."""
        capacity = _unsigned(col.n if capacity is None else capacity, 1 << 64, "capacity {}")
        first_row = _unsigned(first_row, 1 << 64, "first_row {}")
        if mask is not None:
            assert mask.dtype == torch.uint8 and mask.numel() >= (col.n + 7) // 8
        rowids, count = self._int64(max(capacity, 1)), self._int64()
        values = self._empty(max(capacity, 1), torch.int32) if with_values else None
        check(lib().mi355_sort_rows_dev(self._ctx, _col_ptr(col), col.n, col.c, _ptr(mask) if col.n else None, 1 if descending else 0,
                                        first_row, rowids.data_ptr() if capacity else None, _ptr(values) if capacity else None, capacity,
                                        count.data_ptr()))
        rowids = rowids[:capacity]
        return (rowids, count, values[:capacity]) if with_values else (rowids, count)

    def value_set(self, col: PackedColumn, set_bits: Optional[int] = None, mask: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None, accumulate: bool = False, counts: Optional[torch.Tensor] = None):
        """the set of values that occur in `col` among the rows `mask` selects (every row when None), as a bitmap over the value
        domain: bit v is set for every such row whose value v < set_bits (default 2^col.c) -> (set uint8 tensor, counts int64[2]:
        the bits this call turned from 0 to 1 -- the number of distinct values, without `accumulate` -- and the selected rows
        whose value is >= set_bits, which set nothing).  The set is what `semi_join` takes as set_bitmap (`a IN (SELECT b ...)`),
        what `bitmap_combine` intersects or subtracts and `bitmap_count` counts, and `bitmap_to_rowids` over it lists the
        distinct values in ascending order.  `out`: a uint8 device tensor of at least 4 * ceil(set_bits / 32) bytes, 4-byte
        aligned (allocated with scan_output_buffer_size(set_bits) bytes when None); exactly ceil(set_bits / 8) bytes are
        rewritten.  `accumulate`: only OR into what `out` holds -- the union over several columns or calls.  Nothing synchronises.
        Capturable into a graph: column and mask are read at every replay.  Measured (profiles/r19_value_set.txt, uniform values):
        1e9 x 9 bit 0.480 ms against 23.0 ms for decompress -> torch.unique, 2.5e8 x 24 bit 2.498 ms against 5.985; 1.4-1.7 x histogram
        on the same column; 2.5e8 x 32 bit into a 2^32-bit set 10.8 ms where that route takes 6.1 ms."""
        set_bits = _unsigned((1 << col.c) if set_bits is None else set_bits, (1 << 32) + 1, "set_bits {} outside 0..2^32")
        if mask is not None:
            assert mask.dtype == torch.uint8 and mask.numel() >= (col.n + 7) // 8
        if out is None:
            assert not accumulate, "accumulate needs the set to add to"
            out = self._empty(_capi.lib().mi355_scan_output_buffer_size(set_bits))
        assert out.dtype == torch.uint8 and out.numel() >= (set_bits + 31) // 32 * 4
        if counts is None:
            counts = self._int64(2)
        assert counts.dtype == torch.int64 and counts.numel() >= 2
        check(lib().mi355_value_set_dev(self._ctx, _col_ptr(col), col.n, col.c, _ptr(mask) if col.n else None,
                                        out.data_ptr() if set_bits else None, set_bits, 1 if accumulate else 0, counts.data_ptr()))
        return out, counts

    def count_distinct(self, col: PackedColumn, mask: Optional[torch.Tensor] = None) -> int:
        """count(DISTINCT v) over the rows `mask` selects: one `value_set` over the column's whole domain, then the count is read
        back: this SYNCHRONISES with the stream."""
        _, counts = self.value_set(col, mask=mask)
        return int(counts[0].item())

    def distinct_values(self, col: PackedColumn, mask: Optional[torch.Tensor] = None, capacity: Optional[int] = None):
        """SELECT DISTINCT v ORDER BY v over the rows `mask` selects -> (values int64[capacity], ascending; count int64[1]: the
        number of distinct values, of which min(count, capacity) are written).  `value_set`, then `bitmap_to_rowids` over the set;
        capacity defaults to min(2^col.c, col.n).  Nothing synchronises."""
        domain = 1 << col.c
        capacity = _unsigned(min(domain, col.n) if capacity is None else capacity, 1 << 64, "capacity {}")
        vset, _ = self.value_set(col, domain, mask=mask)
        return self.bitmap_to_rowids(vset, domain, capacity)

    def set_ranks(self, set_bitmap: Optional[torch.Tensor], set_bits: int, ct: int, miss: int = 0, out: Optional[torch.Tensor] = None):
        """the rank of every member of a bitmap set among the members, as a packed table of set_bits entries of ct bits:
        table[j] = the number of set bits below j if bit j is set, else `miss`; a member whose rank does not fit ct bits gets
        `miss` too -> (table PackedColumn, counts int64[2]: the members, and the members whose rank did not fit).  The table is
        what `lookup` takes: value_set -> set_ranks -> lookup re-codes a column to dense codes.  `out`: a uint8 device tensor of at
        least compressed_buffer_size(ct, set_bits) bytes (allocated when None).  Nothing synchronises.  Capturable into a graph
        after a warm-up call of at least this set_bits; the set is read at every replay."""
        set_bits = _unsigned(set_bits, (1 << 32) + 1, "set_bits {} outside 0..2^32")
        ct = int(ct)
        if not 1 <= ct <= 32:
            raise ValueError(f"ct {ct} outside 1..32")
        miss = _unsigned(miss, 1 << ct, f"miss {{}} is no value of {ct} bits")
        if set_bitmap is None:
            assert set_bits == 0
        else:
            assert set_bitmap.dtype == torch.uint8 and set_bitmap.numel() >= (set_bits + 7) // 8
        out = self._packed_out(out, ct, set_bits, (set_bits * ct + 7) // 8)
        counts = self._int64(2)
        check(lib().mi355_set_ranks_dev(self._ctx, _ptr(set_bitmap) if set_bits else None, set_bits, ct, miss,
                                        out.data_ptr() if set_bits else None, counts.data_ptr()))
        return PackedColumn(out, set_bits, ct), counts

    def dense_codes(self, col: PackedColumn, ct: Optional[int] = None, mask: Optional[torch.Tensor] = None, miss: int = 0):
        """`col` re-coded to dense codes: code_i = the rank of value_i among the distinct values of the rows `mask` selects ->
        (codes PackedColumn of col.n rows at ct bits, values int64[min(2^col.c, col.n)]: the distinct values ascending, so that
        values[code] decodes, count int64[1]: their number).  value_set -> set_ranks -> lookup; the key of a sparse GROUP BY for
        `group_aggregate_wide`, or a column narrowed after `compact`.  Rows whose value is not in the set (masked-out rows that
        alone carry a value) and, at a ct too narrow, values whose rank does not fit get `miss`.  ct=None: the distinct count is
        read back and the smallest width that holds count - 1 is taken: this SYNCHRONISES with the stream, once; with ct given
        nothing synchronises."""
        domain = 1 << col.c
        vset, counts = self.value_set(col, domain, mask=mask)
        if ct is None:
            ct = max(1, (int(counts[0].item()) - 1).bit_length())
        table, _ = self.set_ranks(vset, domain, ct, miss=miss)
        codes = self.lookup(col, table, miss=miss)
        values, count = self.bitmap_to_rowids(vset, domain, min(domain, col.n))
        return codes, values, count

    _KEEP = {"first": 0, "last": 1}  # MI355_KEY_INDEX_FIRST, MI355_KEY_INDEX_LAST

    def key_index(self, keys: PackedColumn, table_rows: Optional[int] = None, ct: Optional[int] = None, mask: Optional[torch.Tensor] = None,
                  keep: str = "first", first_row: int = 0, miss: Optional[int] = None, out: Optional[torch.Tensor] = None,
                  counts: Optional[torch.Tensor] = None):
        """the row of every key: table[j] = first_row + the first (keep="first") or last (keep="last") row of `keys` that `mask`
        selects (every row when None) and whose key is j, for every j < table_rows (default 2^keys.c); `miss` for a key no such
        row carries, and for one whose row id does not fit ct bits -> (table PackedColumn of table_rows entries of ct bits,
        counts int64[4]: the keys that have a row, the selected rows whose key is >= table_rows (they enter nothing), the
        selected rows whose key is below it, the keys whose row id did not fit).  The build side of a join: `lookup(fk, table)`
        is the dimension row of every fact row, and `lookup` of that column through any dimension column is the attribute -- from
        a dimension in any order, or filtered (`mask` = a scan over it).  The key column is unique among the selected rows
        exactly when counts[2] == counts[0]; the table itself is the first / last row per key.  Defaults: ct = the width that
        holds first_row + keys.n, miss = first_row + keys.n where that fits ct bits (an id no row has, which `lookup` through a
        dimension column of keys.n rows turns into its own miss), else 0.  `out`: a uint8 device tensor of at least
        compressed_buffer_size(ct, table_rows) bytes that overlaps neither input (allocated when None); `counts`: int64[4].
        Nothing synchronises.  Capturable into a graph after a warm-up call of at least this table_rows; keys and mask are read
        at every replay.  Measured (profiles/r20_key_index.txt, uniform keys, the table over the whole domain): 2.5e8 x 14 bit with
        keep="last" 0.344 ms against 53.5 ms for decompress -> scatter_reduce_(amax) -> compress, 2.5e8 x 24 bit 4.804 ms against
        18.4; 1.9-2.2 x value_set on the same column; a sorted 24-bit column under keep="last" only draws with that route."""
        table_rows = _unsigned((1 << keys.c) if table_rows is None else table_rows, (1 << 32) + 1, "table_rows {} outside 0..2^32")
        first_row = _unsigned(first_row, 1 << 32, "first_row {} outside 0..2^32 - 1")
        if keep not in self._KEEP:
            raise ValueError(f"keep {keep!r} is neither 'first' nor 'last'")
        if not 0 <= keys.n < 1 << 32:
            raise ValueError(f"{keys.n} rows: key_index takes at most 2^32 - 1")
        ct = max(1, (first_row + keys.n).bit_length()) if ct is None else int(ct)
        if not 1 <= ct <= 32:
            raise ValueError(f"ct {ct} outside 1..32")
        if miss is None:
            miss = first_row + keys.n if first_row + keys.n < 1 << ct else 0
        miss = _unsigned(miss, 1 << ct, f"miss {{}} is no value of {ct} bits")
        if mask is not None:
            assert mask.dtype == torch.uint8 and mask.numel() >= (keys.n + 7) // 8
        out = self._packed_out(out, ct, table_rows, (table_rows * ct + 7) // 8)
        if counts is None:
            counts = self._int64(4)
        assert counts.dtype == torch.int64 and counts.numel() >= 4
        check(lib().mi355_key_index_dev(self._ctx, _col_ptr(keys), keys.n, keys.c, _ptr(mask) if keys.n else None, first_row, self._KEEP[keep],
                                        out.data_ptr() if table_rows else None, table_rows, ct, miss, counts.data_ptr()))
        return PackedColumn(out, table_rows, ct), counts

    def build_table(self, keys: PackedColumn, values: PackedColumn, table_rows: Optional[int] = None, mask: Optional[torch.Tensor] = None,
                    keep: str = "first", miss: int = 0):
        """the table `lookup(fk, .)` takes, for one attribute: table[j] = the value of the first (or last) row of `keys` that
        `mask` selects and whose key is j, `miss` for a key without a row -> (table PackedColumn of table_rows entries of
        values.c bits, counts int64[4] as `key_index` gives them).  `key_index` with its defaults, then `lookup` of the index
        through `values` (a packed column is a table indexed by row; the index's own miss, keys.n, is no row of it).  For several
        attributes call `key_index` once and `lookup` per attribute.  Nothing synchronises.  Capturable into a graph after a
        warm-up call of at least this table_rows."""
        assert values.n == keys.n, "one value per key row"
        index, counts = self.key_index(keys, table_rows, mask=mask, keep=keep)
        return self.lookup(index, values, miss=miss), counts

    _SIDE = {"left": 0, "right": 1}  # MI355_SEARCH_LEFT, MI355_SEARCH_RIGHT

    def search_sorted(self, col: PackedColumn, table: PackedColumn, side: str = "left", rows=None, exact: bool = False, miss: int = 0,
                      co: Optional[int] = None, out=None, found=None, hits=False):
        """numpy.searchsorted, packed: for every row of `col` its position in the sorted packed column `table` -- the number of
        entries < the value (side="left") or <= it (side="right") -> (positions PackedColumn of col.n values of co bits, found,
        hits).  `rows`: how many of the table's entries count -- an int, or an int64[1] device tensor such as sort_rows,
        run_encode or value_set leave (read on the device: nothing synchronises; at most table.n either way); None: all.
        A row is FOUND when its value occurs in the table.  exact: a row that is not found gets `miss` for its position.
        co: the positions' width (None: the smallest that holds the row bound, and `miss` when exact).  out: a uint8 device
        tensor as in lookup (None: allocated; False: no positions, the first result is None).  found: a uint8 device tensor of
        ceil(col.n / 8) bytes for the bitmap of found rows (True: allocated; None: no bitmap).  hits: an int64[1] device tensor
        for the number of found rows (True: allocated; False: not counted).  Values compare as unsigned integers whatever the
        two widths.  The table must be non-decreasing; on one that is not, positions stay inside 0..rows and nothing outside
        the table is read.  Capturable into a graph whatever its arguments, with no warm-up; column, table and `rows` are read
        at every replay."""
        if side not in self._SIDE:
            raise ValueError(f"side {side!r} is neither 'left' nor 'right'")
        rows_dev = None
        if isinstance(rows, torch.Tensor):
            assert rows.dtype == torch.int64 and rows.numel() >= 1
            rows_dev, rows = rows, table.n
        else:
            rows = table.n if rows is None else _unsigned(rows, table.n + 1, f"rows {{}} beyond the table's {table.n} entries")
        rows = _unsigned(rows, 1 << 32, "rows {} beyond 2^32 - 1")
        miss = _unsigned(miss, 1 << 32, "miss {} is no value of 32 bits")
        if co is None:
            co = max(1, rows.bit_length(), miss.bit_length() if exact else 0)
        co = int(co)
        if not 1 <= co <= 32:
            raise ValueError(f"co {co} outside 1..32")
        with_out = out is not False
        if with_out:
            if rows >= 1 << co:
                raise ValueError(f"rows {rows} beyond 2^{co} - 1: a position is no value of {co} bits")
            miss = _unsigned(miss, 1 << co, f"miss {{}} is no value of {co} bits")
            out = self._packed_out(out, co, col.n, (col.n * co + 7) // 8)
        if found is True:
            found = self.alloc_bitmap(col.n)
        if found is not None:
            assert found.dtype == torch.uint8 and found.numel() >= (col.n + 7) // 8
        if hits is True:
            hits = self._int64()
        elif hits is False:
            hits = None
        if hits is not None:
            assert hits.dtype == torch.int64 and hits.numel() >= 1
        assert with_out or found is not None or hits is not None, "neither positions, nor a bitmap, nor a count asked for"
        check(lib().mi355_search_sorted_dev(self._ctx, _col_ptr(col), col.n, col.c, _col_ptr(table) if rows else None, table.c, rows, _ptr(rows_dev),
                                            self._SIDE[side], 1 if exact else 0, miss, out.data_ptr() if with_out else None, co, _ptr(found), _ptr(hits)))
        return (PackedColumn(out, col.n, co) if with_out else None), found, hits

    def bucketize(self, col: PackedColumn, edges: PackedColumn, co: Optional[int] = None) -> PackedColumn:
        """the bin of every row among sorted `edges`: the number of edges <= the value (0 below the first edge, edges.n from the last
        on) -- width_bucket, a CASE WHEN ladder, an uneven histogram's keys (then `group_aggregate`)"""
        return self.search_sorted(col, edges, side="right", co=co)[0]

    def index_of(self, col: PackedColumn, table: PackedColumn, miss: int, rows=None, co: Optional[int] = None) -> PackedColumn:
        """the first position of every row's value in the sorted `table`, `miss` where it does not occur: what `lookup` takes"""
        return self.search_sorted(col, table, side="left", rows=rows, exact=True, miss=miss, co=co)[0]

    def is_member(self, col: PackedColumn, table: PackedColumn, rows=None):
        """`col IN (sorted table)` -> (bitmap of col.n rows, hits int64[1]); no positions are written"""
        return self.search_sorted(col, table, rows=rows, out=False, found=True, hits=True)[1:]

    def sorted_keys(self, keys: PackedColumn, mask: Optional[torch.Tensor] = None):
        """the keys of the rows `mask` selects in ascending order, as the table `search_sorted` takes -> (PackedColumn of keys.n
        entries at keys.c bits of which the first `count` are set, rowids int64[keys.n]: the row each came from, count int64[1]).
        `sort_rows` with its values, packed; nothing synchronises.  Equal keys keep their row order."""
        rowids, count, values = self.sort_rows(keys, mask=mask, with_values=True)
        return self.compress(values, keys.c), rowids, count

    def sparse_lookup(self, fk: PackedColumn, dim_keys: PackedColumn, dim_attr: PackedColumn, miss: int = 0,
                      mask: Optional[torch.Tensor] = None) -> PackedColumn:
        """`lookup` for keys without a dense domain: for every row of `fk` the value of `dim_attr` in the row of the dimension
        whose key in `dim_keys` equals it (among the rows `mask` selects; the lowest such row where keys repeat), `miss` where
        there is none, packed at dim_attr.c bits.  sorted_keys -> gather(dim_attr) in that order, packed -> index_of with the
        dimension's row count for its miss -> lookup, which turns that into `miss`.  Nothing synchronises."""
        assert dim_attr.n == dim_keys.n, "one attribute per dimension row"
        table, rowids, count = self.sorted_keys(dim_keys, mask)
        attr = self.compress(self.gather(dim_attr, rowids, count)[:dim_keys.n], dim_attr.c)
        return self.lookup(self.index_of(fk, table, miss=dim_keys.n, rows=count), attr, miss=miss)

    def bitmap_combine(self, op: str, a: torch.Tensor, b: torch.Tensor, n: int, out: Optional[torch.Tensor] = None):
        if out is None:
            out = self.alloc_bitmap(n)
        count = self._int64()
        check(lib().mi355_bitmap_combine_dev(self._ctx, self._BOP[op], a.data_ptr(), b.data_ptr(), out.data_ptr(), n,
                                             count.data_ptr()))
        return out, count

    def bitmap_count(self, bitmap: torch.Tensor, n: int) -> torch.Tensor:
        count = self._int64()
        check(lib().mi355_bitmap_count_dev(self._ctx, bitmap.data_ptr(), n, count.data_ptr()))
        return count

    def bitmap_to_rowids(self, bitmap: torch.Tensor, n: int, capacity: int, first_row: int = 0):
        """-> (int64 row ids [capacity], count int64[1]); ids beyond `capacity` are dropped, count is the total."""
        rowids, count = self._int64(max(capacity, 1)), self._int64()
        check(lib().mi355_bitmap_to_rowids_dev(self._ctx, bitmap.data_ptr(), n, first_row, rowids.data_ptr(), capacity,
                                               count.data_ptr()))
        return rowids, count

    def gather(self, col: PackedColumn, rowids: torch.Tensor, count, first_row: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """values of `col` at the row ids a selection produced ("take"): out[i] = value of row rowids[i] for
        i < min(count, len(rowids)); `count` is the int64[1] device tensor the selection left behind (no host round trip) or
        an int.  Ids outside the column give -1."""
        cap = int(rowids.numel())
        if not torch.is_tensor(count):
            count = torch.tensor([int(count)], dtype=torch.int64, device=self._dev)
        if out is None:
            out = self._empty(max(cap, 1), torch.int32)
        assert rowids.dtype == torch.int64 and out.dtype == torch.int32 and out.numel() >= cap
        check(lib().mi355_gather_dev(self._ctx, col.data.data_ptr(), col.n, col.c, first_row, rowids.data_ptr(), count.data_ptr(), cap,
                                     out.data_ptr()))
        return out

    def aggregate(self, col: PackedColumn, mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> int64[4] device tensor (sum, count, min, max) of the column's values over the rows of `mask` (a result bitmap;
        None = every row): one pass over the column, nothing decoded to memory.  count = 0: min is -1 (UINT64_MAX)."""
        if out is None:
            out = self._int64(4)
        check(lib().mi355_aggregate_dev(self._ctx, col.data.data_ptr(), col.n, col.c, _ptr(mask), out.data_ptr()))
        return out

    def histogram(self, col: PackedColumn, mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> int64[2^c] device tensor: how often each value occurs among the rows of `mask` (None = all rows); c <= 14"""
        if out is None:
            out = torch.empty(1 << col.c, dtype=torch.int64, device=self._dev)
        assert out.numel() >= (1 << col.c) and out.dtype == torch.int64
        check(lib().mi355_histogram_dev(self._ctx, col.data.data_ptr(), col.n, col.c, _ptr(mask), out.data_ptr()))
        return out

    def group_aggregate(self, keys: PackedColumn, values: PackedColumn, mask: Optional[torch.Tensor] = None,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> int64[2^keys.c, 4] device tensor: row g = (sum, count, min, max) of `values` over the rows whose key is g, among
        the rows of `mask` (a result bitmap; None = every row) -- SELECT g, sum(v), count(*), min(v), max(v) ... GROUP BY g in
        one pass over both packed columns.  keys.c <= 12; a group without rows reads (0, 0, -1, 0) like aggregate().  For
        keys.c > 12 (a composite key from `arith`, a looked-up attribute) use `group_aggregate_wide`."""
        assert keys.n == values.n
        groups = 1 << keys.c
        if out is None:
            out = torch.empty((groups, 4), dtype=torch.int64, device=self._dev)
        assert tuple(out.shape) == (groups, 4) and out.dtype == torch.int64 and out.is_contiguous()
        check(lib().mi355_group_aggregate_dev(self._ctx, keys.data.data_ptr(), keys.c, values.data.data_ptr(), values.c, keys.n, _ptr(mask), out.data_ptr()))
        return out

    def group_aggregate_wide(self, keys: PackedColumn, values: PackedColumn, groups: int, mask: Optional[torch.Tensor] = None,
                             out: Optional[torch.Tensor] = None, dropped: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> int64[groups, 4] device tensor: row g = (sum, count, min, max) of `values` over the rows whose key is g, among the
        rows of `mask` (a result bitmap; None = every row), for a dense key domain [0, groups) of up to 2^26 groups and keys of
        any width: `group_aggregate` beyond 12 bits -- the composite key g1 * |g2| + g2 from `arith`, an attribute from `lookup`.
        One pass over both packed columns; the result table lives in device memory behind a first-come front in each block's
        LDS.  1 <= groups <= min(2^keys.c, 2^26), not necessarily a power of two.  A counted row whose key is >= groups (the
        `miss` of `arith`, a null code) reaches no group; `dropped`: an int64[1] device tensor that gets the number of such rows
        (None: not counted).  A group without rows reads (0, 0, -1, 0).  Capturable into a graph: both columns and the mask are
        read at every replay.  Measured (profiles/r12_group_aggregate_wide.txt, 2.5e8 rows x 17 bit): on uniform keys over 2^18 /
        2^20 groups 22 ms, 2.47 x / 2.16 x as fast as decompress x 2 -> torch index_add_ / bincount / scatter_reduce_, and bound by
        its global atomics, not its bytes; 14.6 ms with half of the rows in one key, 2.2 ms on sorted keys; at 4096 groups 51 ms
        where `group_aggregate` takes 0.5 ms -- up to 12 bits use that."""
        assert keys.n == values.n  # (so the two column pointers below are NULL together, for the empty column)
        groups = int(groups)
        if not 1 <= groups <= min(1 << keys.c, GROUP_WIDE_MAX_GROUPS):
            raise ValueError(f"groups {groups} outside 1..min(2^{keys.c}, 2^26)")  # (ctypes would wrap a negative count silently)
        if out is None:
            out = torch.empty((groups, 4), dtype=torch.int64, device=self._dev)
        assert tuple(out.shape) == (groups, 4) and out.dtype == torch.int64 and out.is_contiguous()
        if dropped is not None:
            assert dropped.dtype == torch.int64 and dropped.numel() >= 1
        check(lib().mi355_group_aggregate_wide_dev(self._ctx, _col_ptr(keys), keys.c, _col_ptr(values), values.c, keys.n, _ptr(mask), groups,
                                                   out.data_ptr(), _ptr(dropped)))
        return out

    # ---- shared scans (src/simd_scan_shared.cpp, src/simd_scan_shared_linear.cpp) -----------------
    def _shared_outputs(self, n: int, P: int, layout: str, out, hits):
        """the outputs of a shared scan of P keys / predicates by layout -> (out, hits, hits pointer, layout code, stride)"""
        if hits is None:
            hits = self._int64(P)
        hits_ptr = 0 if hits is False else hits.data_ptr()  # hits=False: bitmaps only, no counting
        if layout == "per_predicate":
            stride = int(lib().mi355_bitmap_stride(n))  # whole 128-byte lines per bitmap: up to 2x faster than a 16-byte-multiple stride
            if out is None:
                out = torch.empty((P, stride), dtype=torch.uint8, device=self._dev)
            return out, hits, hits_ptr, _capi.LAYOUT_PER_PREDICATE, stride
        if layout == "linear":
            if out is None:
                out = self._empty((n + 7) // 8 * P)
            return out, hits, hits_ptr, _capi.LAYOUT_LINEAR, 0
        raise ValueError(layout)

    def shared_scan(self, keys: Sequence[int], col: PackedColumn, layout: str = "per_predicate",
                    out: Optional[torch.Tensor] = None, hits: Optional[torch.Tensor] = None):
        """per_predicate -> uint8[P, stride] (row k = bitmap of keys[k], stride = mi355_bitmap_stride(n): ceil(n/8) rounded up to 256);
        linear -> uint8[ceil(n/8) * P] with the byte of 8-value group g and key k at g*P + k.
        hits: int64[P] device tensor to fill (allocated when None); False skips the hit counts."""
        k = keys32(keys, col.c)
        P = int(k.shape[0])
        out, hits, hits_ptr, code, stride = self._shared_outputs(col.n, P, layout, out, hits)
        check(lib().mi355_shared_scan_eq_dev(self._ctx, col.data.data_ptr(), col.n, col.c, k.ctypes.data, P, code,
                                             out.data_ptr(), stride, hits_ptr))
        return out, (None if hits is False else hits)

    def shared_scan_where(self, preds: Sequence[Tuple], col: PackedColumn, layout: str = "per_predicate",
                          out: Optional[torch.Tensor] = None, hits: Optional[torch.Tensor] = None):
        """shared_scan over comparison predicates: preds = (op, a) / (op, a, b) tuples, op in == != < <= > >= between
        not_between, constants any ints; predicate k is scan_where(op_k, a_k, col, b_k).  Outputs, `hits` and the return
        value as shared_scan."""
        arr = predicates(preds)
        P = len(preds)
        out, hits, hits_ptr, code, stride = self._shared_outputs(col.n, P, layout, out, hits)
        check(lib().mi355_shared_scan_where_dev(self._ctx, col.data.data_ptr(), col.n, col.c, C.cast(arr, C.c_void_p), P, code,
                                                out.data_ptr(), stride, hits_ptr))
        return out, (None if hits is False else hits)
