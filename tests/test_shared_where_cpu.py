"""No device: the kernels of csrc/predicates/ against the case table of tests/test_shared_where.py, and the Python side of
the predicate marshalling (engine.predicates -> mi355_predicate) against plain integer comparison."""
import glob
import os
import re

import pytest

from kernel_cases import WHERE_COUNT_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRED_DIR = os.path.join(ROOT, "shared_simd_scan_amd", "csrc", "predicates")
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
OPS = ["==", "!=", "<", "<=", ">", ">=", "between", "not_between"]


def predicate_sources():
    return sorted(glob.glob(os.path.join(PRED_DIR, "*.hpp")) + glob.glob(os.path.join(PRED_DIR, "*.hip")))


def global_kernels():
    names = set()
    for path in glob.glob(os.path.join(PRED_DIR, "*.hpp")):
        text = open(path).read()
        names |= set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", text))
    return names


def test_every_predicates_kernel_has_a_case():
    """the contract of test_kernel_paths.test_every_kernel_has_a_case for the new directory: every __global__ under
    csrc/predicates/ is the expected kernel of at least one case of the GPU file's table (kernel_cases.WHERE_COUNT_CASES), and the
    table names no kernel that does not exist"""
    kernels = global_kernels()
    assert kernels, "no __global__ kernel found under csrc/predicates/"
    named = {family.split("(")[0] for _, _, family in WHERE_COUNT_CASES}
    assert kernels <= named, f"kernels without a case: {sorted(kernels - named)}"
    assert named - kernels == {"scan_burst_kernel"}, f"cases name unknown kernels: {sorted(named - kernels)}"
    scan_hpp = open(os.path.join(ROOT, "shared_simd_scan_amd", "csrc", "kernels", "scan.hpp")).read()
    assert re.search(r"__global__[^;{]*?\bvoid\s+scan_burst_kernel\s*\(", scan_hpp)
    # both forms of the table kernel occur
    fams = {family for _, _, family in WHERE_COUNT_CASES}
    assert {"shared_where_lut_kernel", "shared_where_lut_kernel(multi-pass)", "shared_where_chain_kernel"} <= fams


def test_predicates_kernels_read_no_flag_bits():
    for path in predicate_sources():
        text = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(path).read(), flags=re.S)
        assert not re.search(r"flags\s*&", text), f"{os.path.relpath(path, ROOT)} tests a kernel_flags bit"


def py_pred(v, op, a, b):
    if op == "==":
        return v == a
    if op == "!=":
        return v != a
    if op == "<":
        return v < a
    if op == "<=":
        return v <= a
    if op == ">":
        return v > a
    if op == ">=":
        return v >= a
    inside = a <= v <= b
    return inside if op == "between" else not inside


def c_pred(v, p):
    """what the C side computes from a mi355_predicate: plain integer comparison of the decoded value with its int64 fields"""
    op, a, b = int(p.op), int(p.a), int(p.b)
    return py_pred(v, OPS[op], a, b)


@pytest.mark.parametrize("c", [1, 5, 9, 32])
def test_python_predicate_marshalling(c):
    from shared_simd_scan_amd.engine import predicates

    top = 1 << c
    consts = [INT64_MIN, -5, -1, 0, 1, top - 1, top, top + 3, 1 << 32, INT64_MAX]
    if c <= 9:
        domain = list(range(top))
    else:
        domain = [0, 1, 2, 5, 1000, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, top - 4, top - 2, top - 1]
    for op in OPS:
        for a in consts:
            for b in (consts if op in ("between", "not_between") else [0]):
                spec = (op, a, b) if op in ("between", "not_between") else (op, a)
                arr = predicates([spec, spec + (12345,)] if len(spec) == 2 else [spec])
                for p in arr:
                    assert p.reserved == 0 and OPS[p.op] == op
                    assert INT64_MIN <= p.a <= INT64_MAX and INT64_MIN <= p.b <= INT64_MAX
                    for v in domain:
                        assert c_pred(v, p) == py_pred(v, op, a, b), (c, op, a, b, v)


def test_python_predicate_marshalling_refuses_malformed_tuples():
    from shared_simd_scan_amd.engine import predicates

    with pytest.raises(ValueError):
        predicates([("==",)])
    with pytest.raises(KeyError):
        predicates([("=", 3)])
    arr = predicates([("between", 1 << 70, -(1 << 70)), ("<", 3)])
    assert (arr[0].a, arr[0].b, arr[1].b) == (1 << 32, -1, 0)
