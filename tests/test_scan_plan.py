"""csrc/scan_plan.hpp holds the rules by which the three group units plan a launch: the Infinity Cache divisor of the eq / range scan
(llc_divisor), the tiles per store burst (burst_k), the store policies, the AUX word each kernel is launched with, the blocks per CU
and the grid.  They are pure functions of numbers, so they are checked here without a GPU.

tests/cpp/scan_plan_check.cpp is a stand-alone program (its own main, plain g++, never loaded into Python) built with
-fsanitize=undefined,address.  It asserts the divisors that the rule's own comment states (1e9 x 9 bit: budgets 190 / 205 / 220 / 240
MiB give 17 / 13 / 11 / 9; auto on a repeat 13, 5 and 3 at 1e9, 5e8 and 2.5e8 rows), every exit of llc_divisor, burst_k at every width
with the scan_burst override, the table (dma_aux, store policy) -> AUX of the four kernels, the two store policies at their size
thresholds with the option at -1, 0 and 1, the clamps of scan_want_bpc and of the column scan, the IN-list's second block, decompress's
two blocks, and grid_for at its edges.
"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shared_simd_scan_amd", "csrc")
HEADER = os.path.join(CSRC, "scan_plan.hpp")
SRC = os.path.join(ROOT, "tests", "cpp", "scan_plan_check.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "build", "scan_plan_check")


def build_binary():
    newest = max(os.path.getmtime(f) for f in (SRC, HEADER))
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < newest:
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-I", CSRC,
                        SRC, "-o", BIN], check=True)
    return BIN


def test_header_needs_no_hip():
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', open(HEADER).read())
    assert sorted(includes) == ["stddef.h", "stdint.h"], includes
    # ... and the check includes nothing of the project but that header
    assert re.findall(r'#include\s+"([^"]+)"', open(SRC).read()) == ["scan_plan.hpp"]


def test_the_rules_live_in_the_header_only():
    """one copy of each rule: no other source defines them, and the 40 KiB formula is written once"""
    names = ("llc_divisor", "burst_k", "scan_want_bpc", "cap_bpc", "grid_for", "one_pass_store_policy", "multi_pass_nt_stores")
    for folder, _, files in os.walk(CSRC):
        for name in files:
            if name.endswith((".hip", ".hpp")):
                text = re.sub(r"//.*", "", open(os.path.join(folder, name)).read())
                defined = [n for n in names if re.search(r"\b(?:int|bool|unsigned|uint32_t)\s+%s\s*\(" % n, text)]
                assert defined == (list(names) if name == "scan_plan.hpp" else []), (name, defined)
                assert len(re.findall(r"40\s*\*\s*1024", text)) == (1 if name == "scan_plan.hpp" else 0), name


def test_launcher_reports_the_planned_divisor():
    """through launch_group_N itself (tests/cpp/launch_dry_run.cpp with its two trailing columns): the divisors of the rule's comment.
    The dry run passes no bitmap, so the budgets are the comment's less the 1e9-row bitmap's 119.2 MiB, rounded down to whole MiB
    where the divisor stays: 70 / 85 / 100 / 120 MiB give 17 / 13 / 11 / 9 (1.125e9 bytes of column over the budget, rounded up, made odd)."""
    from kernel_cases import build_binary as build_dry_run

    n, MIB = 10**9, 1 << 20
    col = (n * 9 + 7) // 8
    want = {mib: -(-col // (mib * MIB)) | 1 for mib in (70, 85, 100, 120)}
    assert want == {70: 17, 85: 13, 100: 11, 120: 9}
    #        op c P layout hits n flags vpl nts bpc aux burst single | llc_resident_mib llc_repeat -> divisor
    rows = [((0, 9, 1, 0, 1, n, 0, 0, -1, 0, 18, 0, 0, mib, rep), d) for mib, d in want.items() for rep in (0, 1)]
    rows += [((1, 9, 1, 0, 1, n, 0, 0, -1, 0, 18, 0, 0, -1, 0), 0),      # auto acts on a repeat only
             ((1, 9, 1, 0, 1, n, 0, 0, -1, 0, 18, 0, 0, -1, 1), 7),      # ... with 205 MiB: 5.2 -> 6 -> 7
             ((0, 9, 1, 0, 1, n, 0, 0, -1, 0, 18, 0, 0, 0, 1), 0),       # off
             ((0, 9, 1, 0, 1, n, 0, 0, -1, 0, 0, 0, 0, 100, 1), 0),      # default-policy loads
             ((0, 9, 1, 0, 1, 10**8, 0, 0, -1, 0, 18, 0, 0, -1, 1), 0),  # the column fits whole: nothing in auto,
             ((0, 9, 1, 0, 1, 10**8, 0, 0, -1, 0, 18, 0, 0, 205, 1), 1),  # all of it with an explicit budget
             ((4, 9, 40, 0, 1, n, 0, 0, -1, 0, 18, 0, 0, 100, 1), -1)]   # the IN-list reports none
    text = "".join(" ".join(str(v) for v in row) + "\n" for row, _ in rows)
    res = subprocess.run([build_dry_run()], input=text, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    got = [ln.split("\t") for ln in res.stdout.splitlines()]
    assert len(got) == len(rows) and all(len(g) == 3 for g in got), res.stdout[-2000:]
    for (row, d), (fam, rec, llc_d) in zip(rows, got):
        assert int(fam) == -1 and int(llc_d) == d, (row, rec, llc_d)
        assert rec.startswith("in_kernel<9, 34, " if row[0] == 4 else f"scan_burst_kernel<9, {row[0]}, {34 if row[10] else 0}, 128, 4> "), rec


def test_rules_value_by_value():
    res = subprocess.run([build_binary()], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    m = re.fullmatch(r"(\d+) checks, 0 failed\n", res.stdout)
    assert m and int(m.group(1)) > 300, res.stdout
