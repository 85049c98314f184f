"""csrc/llc_repeat.hpp decides whether an eq / range scan repeats the launch that runs directly before it (option "llc_resident_mib"
= -1 acts on repeats only) and what mi355_ctx_last_llc_divisor reports; it is plain host bookkeeping over the launch record, so it
is checked here without a GPU.

tests/cpp/llc_repeat_check.cpp is a stand-alone program (its own main, plain g++, never loaded into Python) built with
-fsanitize=undefined,address.  It drives the struct as ctx.hpp's Entry and capi.hip's launch() do and asserts "repeat" and the
reported divisor after every step: a first scan, an identical one, one of column / bitmap / mask / n / c changed; an identical scan
after another launch in a call of its own, after another launch later in the scan's own outermost call, after a call that launched
nothing (all three end the repeat) and after a transparent call (kKeepRecord / Locked: it stays); the host-pointer flavour's nested
scan repeated; identical scans inside one outermost call; a capture id that changes, that stays, and that is unknown.
"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shared_simd_scan_amd", "csrc")
HEADER = os.path.join(CSRC, "llc_repeat.hpp")
SRC = os.path.join(ROOT, "tests", "cpp", "llc_repeat_check.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "build", "llc_repeat_check")


def build_binary():
    newest = max(os.path.getmtime(f) for f in (SRC, HEADER))
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < newest:
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-I", CSRC,
                        SRC, "-o", BIN], check=True)
    return BIN


def test_header_needs_no_hip():
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', open(HEADER).read())
    assert includes and not [i for i in includes if "hip" in i or i.endswith(".hpp")], includes
    # ... and the check includes nothing of the project but that header
    assert [i for i in re.findall(r'#include\s+"([^"]+)"', open(SRC).read())] == ["llc_repeat.hpp"]


def test_no_launcher_but_the_scan_path_mentions_the_state():
    """the struct's callers: the entry prologue (ctx.hpp) and the eq / range path and the introspection call of capi.hip"""
    users = set()
    for folder, _, names in os.walk(CSRC):
        for name in names:
            if name.endswith((".hip", ".hpp")) and name != "llc_repeat.hpp":
                text = re.sub(r"//.*", "", open(os.path.join(folder, name)).read())
                if re.search(r"\bllc\s*\.|->\s*llc\b|LlcRepeat|LlcScan", text):
                    users.add(name)
    assert users == {"ctx.hpp", "capi.hip"}, users


def test_scripted_call_sequences():
    res = subprocess.run([build_binary()], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    m = re.fullmatch(r"(\d+) checks, 0 failed\n", res.stdout)
    assert m and int(m.group(1)) > 150, res.stdout
