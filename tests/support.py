"""What the test files share: where things are, the library and engine fixtures, what a public header declares, a recording
stand-in for the library, packed uploads, and the checks every feature header and feature source directory gets.

A plain module, not a conftest: a test file imports what it uses by name, fixtures included (pytest takes an imported fixture as
the importing module's own, so the module-scoped ones still live once per test file).  A copy that differs from what is here
stays in its test file, with a comment that says how."""
import ctypes as C
import glob
import os
import re
import subprocess
import types

import numpy as np
import pytest

from test_kernel_paths import parse_record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "shared_simd_scan_amd", "csrc")


@pytest.fixture(scope="module")
def L():
    """the library, built first where it is missing"""
    from shared_simd_scan_amd import build, lib

    if not os.path.exists(build.LIB_PATH):
        build.build()
    return lib()


@pytest.fixture(scope="module")
def eng():
    """an engine on device 0, closed behind the module's last test"""
    from shared_simd_scan_amd import ScanEngine

    e = ScanEngine(0)
    yield e
    e.close()


# ---- public headers ---------------------------------------------------------------------------------------------------------

def header_text(header):
    return open(os.path.join(INCLUDE, header)).read()


def declared(header):
    """the entry points a public header declares, sorted"""
    return sorted(set(re.findall(r"^MI355_API [^;(]*?\b(mi355_\w+)\(", header_text(header), flags=re.M)))


def header_macro(header, name):
    m = re.search(rf"^#define {name}\s+(\d+)", header_text(header), flags=re.M)
    assert m, name
    return int(m.group(1))


def check_header_is_plain_c99(header):
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(INCLUDE, header)],
                   check=True)


def check_header_binds(L, header):
    """`header` declares exactly what its list in _capi.HEADERS binds, the loaded library carries those argument types, and neither
    an earlier header nor an earlier list (what precedes it in HEADERS) knows any of the names -> (names, {name: argtypes})"""
    from shared_simd_scan_amd._capi import HEADERS

    symbols = HEADERS[header]
    earlier_headers = list(HEADERS)[:list(HEADERS).index(header)]
    earlier_symbols = [s for h in earlier_headers for s in HEADERS[h]]
    names = declared(header)
    assert names == sorted(s[0] for s in symbols)
    sigs = dict((s[0], s[2]) for s in symbols)
    for name in names:
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes == sigs[name]  # lib() applied the list
    for other in earlier_headers:
        assert not set(names) & set(declared(other)), other
        assert header not in header_text(other), f"{other} includes {header}"
    assert not set(names) & {s[0] for s in earlier_symbols}
    return names, sigs


def check_capture_verdict(header, *more):
    text = header_text(header)
    for pattern in (r"graph capture: capturable\b",) + more:
        assert re.search(pattern, text), pattern


# ---- a recording stand-in for the library -------------------------------------------------------------------------------------

class RecordingLib:
    """stand-in for libmi355scan.so: converts the arguments through the real argtypes (as ctypes would) and records them;
    `real`: the library that answers the buffer-size arithmetic, for the wrappers that ask it"""

    def __init__(self, real=None):
        from shared_simd_scan_amd import _capi

        self.calls = []
        if real is not None:
            self.mi355_compressed_buffer_size = real.mi355_compressed_buffer_size
        self._sig = {name: args for symbols in _capi.HEADERS.values() for name, _, args in symbols}

    def __getattr__(self, name):
        argtypes = self._sig[name]

        def call(*args):
            assert len(args) == len(argtypes), name
            conv = []
            for t, a in zip(argtypes, args):
                if t in (C.c_int32, C.c_uint32, C.c_int64, C.c_uint64, C.c_int, C.c_uint) and isinstance(a, int):
                    a = t(a).value
                conv.append(a)
            self.calls.append((name, conv))
            return 0

        return call


def fake_engine(monkeypatch, rec):
    """an engine without a device whose library is `rec` -> (engine, rec, col(c, n): a stand-in for a packed column)"""
    import torch

    from shared_simd_scan_amd import engine

    monkeypatch.setattr(engine, "lib", lambda: rec)
    monkeypatch.setattr(engine, "check", lambda rc: None)
    eng = object.__new__(engine.ScanEngine)
    eng._ctx, eng._dev = None, torch.device("cpu")

    def col(c, n=1000):
        return types.SimpleNamespace(data=torch.zeros(64, dtype=torch.uint8), n=n, c=c)

    return eng, rec, col


@pytest.fixture
def fake(monkeypatch, L):
    """fake_engine over a RecordingLib whose buffer-size arithmetic is the real library's, with a PackedColumn that takes any tensor
    (the real one wants a device tensor)"""
    from shared_simd_scan_amd import engine

    monkeypatch.setattr(engine, "PackedColumn", lambda data, n, c: types.SimpleNamespace(data=data, n=int(n), c=int(c)))
    return fake_engine(monkeypatch, RecordingLib(L))


# ---- GPU cases ----------------------------------------------------------------------------------------------------------------

def record(L, eng):
    """the launch record of the engine's last call, parsed"""
    return parse_record((L.mi355_ctx_last_launch(eng._ctx) or b"").decode())


def plain_pack(O, values, c):
    """the oracle's packed image of `values` -> device tensor"""
    import torch

    return torch.from_numpy(O.pack(np.ascontiguousarray(values, dtype=np.uint32), c)).cuda()


upload = plain_pack


def hostile_pack(O, values, c, offset=0):
    """the oracle's packed image of `values` in hostile surroundings -> device tensor (a view at `offset` bytes, a multiple of 4,
    behind a 16-byte boundary): ones in the bits behind the last value and in every byte of the pad, 0xFF in front of the view"""
    import torch

    n = len(values)
    img = O.pack(np.ascontiguousarray(values, dtype=np.uint32), c).copy()
    nb = (n * c + 7) // 8
    if (n * c) % 8:
        img[nb - 1] |= (0xFF << ((n * c) % 8)) & 0xFF
    img[nb:] = 0xFF
    buf = torch.full((16 + offset + len(img),), 0xFF, dtype=torch.uint8, device="cuda")
    buf = buf[(-buf.data_ptr()) % 16:]
    buf[offset: offset + len(img)] = torch.from_numpy(img).cuda()
    view = buf[offset: offset + len(img)]
    assert view.data_ptr() % 16 == offset % 16
    return view


# ---- the sources of a feature directory (csrc/<feature>/) -----------------------------------------------------------------------

def feature_sources(feature):
    return sorted(glob.glob(os.path.join(CSRC, feature, "*.hpp")) + glob.glob(os.path.join(CSRC, feature, "*.hip")))


def global_kernels_of(feature):
    """the name of every __global__ under csrc/<feature>/"""
    kernels = set()
    for path in feature_sources(feature):
        kernels |= set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", open(path).read()))
    return kernels


def gpu_part_of(test_file):
    """a test file's text from its "# GPU" banner on"""
    me = open(test_file).read()
    return me[me.index("# GPU\n"):]


def check_gpu_part_asserts(test_file, *names):
    """each of the kernel-name constants `names` stands in an assert of the file's GPU part"""
    gpu_part = gpu_part_of(test_file)
    for const in names:
        assert re.search(rf"assert [^\n]*\b{const}\b", gpu_part), f"no GPU case asserts {const} from the launch record"


def check_sources_read_no_flag_bits(feature):
    assert feature_sources(feature)
    for path in feature_sources(feature):
        text = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(path).read(), flags=re.S)
        assert not re.search(r"flags\s*&", text), f"{os.path.relpath(path, ROOT)} tests a kernel_flags bit"
