"""csrc/predicate_norm.hpp turns (op, a, b) into what the kernels compare with; it is plain host arithmetic, so it is checked here
without a GPU.

tests/cpp/predicate_norm_check.cpp is a stand-alone program (its own main, plain g++, never loaded into Python) built with
-fsanitize=undefined,address.  Over every width 1..32, every comparison, constants at every boundary of the arithmetic (INT64_MIN,
+-2^33, +-2^32, 2^31, the ends of the domain, each +-1) and values at both ends and in the middle of the domain it asserts that

* the kernels' test ((uint32)(x - lo) <= span) != invert equals the comparison on int64;
* the same for the difference of two columns over the width pairs (c1, c2 in {1, 2, c1, 30, 31, 32}): the 64-bit test everywhere,
  the 32-bit test where both widths are <= 30, and lo <= hi inside the domain always;
* a predicate is handed to the equality-key path only with a key that (uint32)key == x answers as the predicate does.
"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shared_simd_scan_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "predicate_norm_check.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "build", "predicate_norm_check")


def build_binary():
    newest = max(os.path.getmtime(f) for f in (SRC, os.path.join(CSRC, "predicate_norm.hpp")))
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < newest:
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-I", CSRC,
                        SRC, "-o", BIN], check=True)
    return BIN


def test_header_needs_no_hip():
    text = open(os.path.join(CSRC, "predicate_norm.hpp")).read()
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', text)
    assert includes and not [i for i in includes if "hip" in i or i.endswith(".hpp")], includes
    assert "ScanArgs" not in re.sub(r"//.*", "", text)


def test_normalised_tests_equal_the_int64_comparisons():
    res = subprocess.run([build_binary()], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    m = re.fullmatch(r"(\d+) comparisons, 0 failed\n", res.stdout)
    assert m and int(m.group(1)) > 5_000_000, res.stdout
