"""What the test files share: where things are, the library and engine fixtures, what a public header declares, a recording
stand-in for the library, launch records, guarded buffers and the exact image of one, packed and hostile uploads, the runtime of
the alignment tables, what the unit tables compute their inputs and expectations with (numpy and the CPU oracle), the rank-process
helpers, the checks every feature header and feature source directory gets, which entry points' launchers reach a piece of the
context's state, and which kernels of a feature directory take a store policy.  capture.py (graph capture),
kernel_cases.py (the kernel-path case table) and large_routes.py (the torch routes of test_large_columns.py) stand beside it; no
test file imports from another test file.

A plain module, not a conftest: a test file imports what it uses by name, fixtures included (pytest takes an imported fixture as
the importing module's own, so the module-scoped ones still live once per test file).  A copy that differs from what is here
stays in its test file, with a comment that says how."""
import ctypes as C
import glob
import os
import queue
import re
import socket
import subprocess
import time
import types
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "shared_simd_scan_amd", "csrc")

E_INVALID = -1   # MI355_E_INVALID
SENTINEL = 0xEE  # the fill of every guard byte and of every output in front of a call


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


# ---- launch records -----------------------------------------------------------------------------------------------------------

RECORD_LINE = re.compile(r"(?P<label>\S.*?) grid=(?P<grid>\d+) lds=(?P<lds>\d+) flags=0x(?P<flags>[0-9a-f]+)")


def parse_record(text):
    lines = [ln for ln in text.split("\n") if ln]
    out = []
    for ln in lines:
        m = RECORD_LINE.fullmatch(ln)
        assert m, f"malformed launch record line {ln!r}"
        out.append((m["label"], int(m["grid"]), int(m["lds"]), int(m["flags"], 16)))
    return out


def label_matches(pattern, label):
    rx = re.escape(pattern).replace(r"\*", r"[^,<>]+")
    return re.fullmatch(rx, label) is not None


def base_name(label):
    return label.split("<", 1)[0]


# ---- GPU cases ----------------------------------------------------------------------------------------------------------------

class Guarded:
    """a device buffer of `nbytes` inside 0xEE guard regions (`front` / `back` bytes, front a multiple of 16)"""

    def __init__(self, nbytes, back=4096, front=4096):
        import torch

        self.nbytes, self.front, self.back = int(nbytes), front, back
        self.t = torch.full((front + self.nbytes + back,), SENTINEL, dtype=torch.uint8, device="cuda")

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + self.front)

    @property
    def body(self):
        """the buffer between the guards, as a view"""
        return self.t[self.front: self.front + self.nbytes]

    def guards_intact(self):
        """both guard regions still hold 0xEE, compared on the device: for a buffer too large for fetch()"""
        return bool((self.t[: self.front] == SENTINEL).all().item()) and bool((self.t[self.front + self.nbytes:] == SENTINEL).all().item())

    def fetch(self):
        h = self.t.cpu().numpy()
        assert (h[: self.front] == SENTINEL).all(), "guard in front of the buffer overwritten"
        tail = h[self.front + self.nbytes:]
        assert (tail == SENTINEL).all(), f"guard behind the buffer overwritten at +{int(np.argmax(tail != SENTINEL))}"
        return h[self.front: self.front + self.nbytes]


class Expected:
    """a Guarded output and every byte a call must leave in it: `body` is the whole buffer as the call leaves it, SENTINEL where it
    must not write.  The buffer and its image (guards, body, guards) are made on the device at the first reset(); check() compares
    them there in one pass and fetches the buffer only to say where they differ"""

    def __init__(self, body):
        self.want = np.ascontiguousarray(body, dtype=np.uint8)
        self.g = self.image = None

    @property
    def ptr(self):
        return self.g.ptr if len(self.want) else None

    def reset(self):
        import torch

        if self.g is None:
            self.g = Guarded(len(self.want))
            guard = lambda k: np.full(k, SENTINEL, dtype=np.uint8)
            self.image = torch.from_numpy(np.concatenate([guard(self.g.front), self.want, guard(self.g.back)])).cuda()
        self.g.t.fill_(SENTINEL)

    def untouched(self):
        return bool((self.g.t == SENTINEL).all().item())

    def check(self, what):
        import torch

        if torch.equal(self.g.t, self.image):
            return
        have = self.g.fetch()  # (asserts the guard bytes on both sides)
        bad = np.nonzero(have != self.want)[0]
        assert bad.size == 0, (what, "byte", int(bad[0]), "of", len(have), "have", int(have[bad[0]]), "want", int(self.want[bad[0]]), "wrong bytes", int(bad.size))
        raise AssertionError((what, "the buffer and its image differ, but not in a byte"))


def packbits(mask):
    return np.packbits(mask.astype(bool), bitorder="little")


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


def hostile_bitmap(bits, offset=0, front=None):
    """the canonical bitmap of `bits` -> device tensor of exactly ceil(n/8) bytes, a view with 0xFF bytes directly behind it (and
    `front` bytes, default 0xFF, before it) that starts `offset` bytes (a multiple of 4) behind a 16-byte boundary"""
    import torch

    img = packbits(bits)
    lead = np.full(offset, 0xFF, dtype=np.uint8) if front is None else np.asarray(front, dtype=np.uint8)
    assert len(lead) % 16 == offset % 16
    buf = torch.full((16 + len(lead) + len(img) + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    buf = buf[(-buf.data_ptr()) % 16:]
    buf[: len(lead)] = torch.from_numpy(lead.copy()).cuda()
    buf[len(lead): len(lead) + len(img)] = torch.from_numpy(img.copy()).cuda()
    view = buf[len(lead): len(lead) + len(img)]
    assert view.data_ptr() % 16 == offset % 16
    return view, buf


# ---- what the unit tables (test_shared_state, test_store_policies) compute their inputs and expectations with: numpy and the CPU
# oracle only ----

CMP = {"==": 0, "!=": 1, "<": 2, "<=": 3, ">": 4, ">=": 5, "between": 6, "not_between": 7}  # MI355_CMP_*
BOP = {"and": 0, "or": 1, "xor": 2, "andnot": 3}                                             # MI355_BITMAP_*


def oracle():
    from oracle import oracle as get

    return get()


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def u64s(*xs):
    return np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in xs], dtype=np.uint64).view(np.uint8)


def packed(vals, c):
    """the column as the calls read it: the oracle's image, pad included"""
    return oracle().pack(np.ascontiguousarray(vals, dtype=np.uint32), c)


def payload(vals, c):
    """the bytes a call that writes len(vals) values of c bits leaves: trailing bits of the last byte zero"""
    return packed(vals, c)[: (len(vals) * c + 7) // 8].copy()


def prefix_body(nbytes, written):
    """a buffer of nbytes whose first len(written) bytes a call writes; the rest stays as it was"""
    body = np.full(nbytes, SENTINEL, dtype=np.uint8)
    body[: len(written)] = written
    return body


def random_values(rng, n, c):
    return rng.integers(0, 1 << c, n, dtype=np.uint64).astype(np.uint32)


def pred(v, op, a, b=0):
    v = v.astype(np.int64)
    between = (v >= a) & (v <= b)
    return {"==": v == a, "!=": v != a, "<": v < a, "<=": v <= a, ">": v > a, ">=": v >= a, "between": between, "not_between": ~between}[op]


def combine(p, m, op):
    return {"and": p & m, "or": p | m, "xor": p ^ m, "andnot": m & ~p}[op]


def top_k_expect(vals, qual, k, largest):
    """-> (the bitmap's rows, [m, threshold, selected rows beyond it, qualifying rows equal to it]): by value, then by row id"""
    idx = np.nonzero(qual)[0]
    v = vals[idx].astype(np.int64)
    m = min(k, len(idx))
    bits = np.zeros(len(vals), dtype=bool)
    if m == 0:
        return bits, [0, 0, 0, 0]
    order = np.lexsort((idx, -v if largest else v))
    bits[idx[order[:m]]] = True
    T = int(v[order[m - 1]])
    return bits, [m, T, int((v > T).sum() if largest else (v < T).sum()), int((v == T).sum())]


def key_index_expect(keys, qual, table_rows, keep, first_row, ct, miss):
    """-> (table, [members, selected rows outside the table, selected rows inside it, members whose row id did not fit])"""
    rows = np.nonzero(qual & (keys < table_rows))[0]
    winner = np.full(table_rows, -1, dtype=np.int64)
    if keep == "first":
        winner[keys[rows[::-1]]] = rows[::-1]
    else:
        winner[keys[rows]] = rows
    member = winner >= 0
    ids = winner + first_row
    fits = member & (ids < (1 << ct))
    table = np.where(fits, ids, miss).astype(np.uint32)
    return table, [int(member.sum()), int((qual & (keys >= table_rows)).sum()), len(rows), int((member & ~fits).sum())]


def corner_rows(n, R=2048):
    """rows that carry the corner values (tiles of R rows: 64 lanes x 32 rows): the first four of the first tile, the last four of
    the last full tile, the last four of the ragged tail (as far as they exist)"""
    rows = [list(range(min(4, n)))]
    nfull = n // R
    if nfull >= 1:
        rows.append(list(range(nfull * R - 4, nfull * R)))
    if n % R >= 4 and n > 4:
        rows.append(list(range(n - 4, n)))
    return rows


def grouped(keys, values, groups, sel=None):
    """numpy's sum, count, min, max of values per key, in group_aggregate's layout (an empty group: 0, 0, ~0, 0)"""
    want = np.zeros((groups, 4), dtype=np.uint64)
    want[:, 2] = (1 << 64) - 1
    if sel is None:
        sel = np.ones(len(keys), dtype=bool)
    k, v = keys[sel].astype(np.int64), values[sel].astype(np.uint64)
    np.add.at(want[:, 0], k, v)
    want[:, 1] = np.bincount(k, minlength=groups).astype(np.uint64)
    np.minimum.at(want[:, 2], k, v)
    np.maximum.at(want[:, 3], k, v)
    return want


# ---- the runtime of the minimum-alignment and refusal tables (test_min_contract, test_argument_refusals) ----------------------

HOSTILE_BYTES = 256  # 0xFF bytes in front of and behind a mask


class Runtime:
    def __init__(self, L, O):
        import torch

        from shared_simd_scan_amd import ScanEngine

        self.L, self.O, self.torch = L, O, torch
        self.default = ScanEngine()
        self.capped = ScanEngine()  # 4 waves: a wave reaches the tail tile with a previous tile's values still in its LDS
        self.capped.set_option("grid_cus", 1)
        self.capped.set_option("max_blocks_per_cu", 1)

    def close(self):
        self.default.close()
        self.capped.close()

    def place(self, raw, shift, offset, align):
        """raw bytes `shift` bytes into a fresh allocation -> (tensor, address of raw[offset]); the address is `align` mod 2 * align"""
        host = np.concatenate([np.full(shift, 0xFF, dtype=np.uint8), raw])
        t = self.torch.from_numpy(host).cuda()
        ptr = t.data_ptr() + shift + offset
        assert ptr % (2 * align) == align, f"pointer {ptr:#x} is not {align} mod {2 * align}"
        return t, ptr

    def column(self, model, j, align=16):
        vals, a = model.columns[j]
        w = model.case.widths[j]
        raw = self.O.pack(vals.astype(np.uint32), w)
        assert (a * w) % 8 == 0
        return self.place(raw, 0 if w % 2 else align, a * w // 8, align)

    def bitmap(self, model, j, align=16):
        body = packbits(model.B[j])
        side = np.full(HOSTILE_BYTES, model.hostile_byte[j], dtype=np.uint8)
        return self.place(np.concatenate([side, body, side]), align, HOSTILE_BYTES, align)

    def out(self, nbytes, align=16):
        g = Guarded(nbytes, front=4096 + align)
        assert g.ptr.value % (2 * align) == align
        return g

    def word(self):
        return Guarded(8, back=64, front=64)


@pytest.fixture(scope="module")
def rt(O):
    """library, oracle, torch and two engines (the default grid and a 4-wave one), closed behind the module's last test"""
    import torch

    from shared_simd_scan_amd import lib

    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    r = Runtime(lib(), O)
    yield r
    r.close()


# ---- rank processes and the two-rank benchmark (test_sharded_gloo, test_exchange_loopback) ------------------------------------

def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def join_or_kill(procs, timeout, q=None):
    """Wait up to `timeout` seconds in all for the rank processes; a rank that failed ends the wait at once (its peers
    may be blocked in a collective waiting for it).  Survivors are terminated, then killed, before the test fails: a
    hung rank must not stay on the GPU.  Returns what the ranks put on `q` meanwhile (drained while waiting, so that no
    child blocks on a full queue at exit)."""
    deadline = time.monotonic() + timeout
    got = []

    def drain():
        while q is not None:
            try:
                got.append(q.get_nowait())
            except queue.Empty:
                return

    while any(p.is_alive() for p in procs) and time.monotonic() < deadline:
        drain()
        if any(p.exitcode not in (None, 0) for p in procs):
            break
        time.sleep(0.1)
    survivors = [p for p in procs if p.is_alive()]
    for p in survivors:
        p.terminate()
    for p in survivors:
        p.join(10)
        if p.is_alive():
            p.kill()
            p.join(10)
    for p in procs:
        p.join(1)
    drain()
    codes = [p.exitcode for p in procs]
    if any(c != 0 for c in codes):
        msg = f"rank exit codes {codes}"
        if survivors:
            msg += f"; {len(survivors)} rank(s) still running after {timeout} s were terminated"
        reports = [m for m in got if isinstance(m, str)]  # e.g. a rank's traceback
        pytest.fail("\n".join([msg] + reports))
    return got


def _bench_2ranks(extra_env, extra_args=()):
    import json
    import sys

    env = dict(os.environ, BENCH_BACKEND="gloo", **extra_env)
    env.pop("WORLD_SIZE", None)
    # --full: the weak partition and the exchange step are not part of a plain run
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--rows", "40000000", "--steps", "5",
                          "--warmup", "2", "--full", *extra_args], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    return res, (json.loads(lines[-1]) if lines else None)


# ---- the sources of a feature directory (csrc/<feature>/) -----------------------------------------------------------------------

def feature_sources(feature):
    return sorted(glob.glob(os.path.join(CSRC, feature, "*.hpp")) + glob.glob(os.path.join(CSRC, feature, "*.hip")))


def global_kernels_of(feature):
    """the name of every __global__ under csrc/<feature>/"""
    kernels = set()
    for path in feature_sources(feature):
        kernels |= set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", open(path).read()))
    return kernels


def hip_functions():
    """[(name, file, body)] of every function a .hip file under csrc/ defines at file level: a definition's line starts in column 0
    and ends with its argument list, `{` and `}` stand alone in column 0 (the sources' one style; the parse fails loudly below where
    a file has a `{` line it did not match)"""
    found = []
    for path in sorted(glob.glob(os.path.join(CSRC, "**", "*.hip"), recursive=True)):
        text = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(path).read(), flags=re.S)
        defs = list(re.finditer(r"^(?![ \t#}])[^\n;{}]*?\b(\w+)\((?:[^;{}]*?)\)\n(?:#[^\n]*\n)*\{\n(.*?)\n\}", text, flags=re.M | re.S))
        opened = [m for m in re.finditer(r"^\{$", text, flags=re.M)]
        assert len(defs) == len(opened), f"{os.path.relpath(path, ROOT)}: {len(opened)} bodies, {len(defs)} parsed"
        for m in defs:
            found.append((m.group(1), os.path.relpath(path, CSRC), m.group(2)))
    return found


def entry_points_reaching(*needles):
    """every exported mi355_*_dev whose launcher source mentions one of `needles`: in its own body, or in that of a function it calls
    -- a helper of its translation unit or another entry point -- to any depth; sorted"""
    funcs = hip_functions()
    reach = {(name, path) for name, path, body in funcs if any(s in body for s in needles)}
    while True:
        more = {(name, path) for name, path, body in funcs if (name, path) not in reach
                and any(re.search(rf"\b{callee}\s*(?:<[^;()]*>)?\(", body) for callee, where in reach if callee.startswith("mi355_") or where == path)}
        if not more:
            break
        reach |= more
    reach = {name for name, _ in reach}
    exported = {s for header in sorted(os.listdir(INCLUDE)) if header.endswith(".h") for s in declared(header)}
    return sorted(s for s in reach & exported if s.endswith("_dev"))


def feature_directories():
    """the directories under csrc/ that hold a feature's own kernels and launcher (kernels/ and extras/ are the shared ones)"""
    return sorted(d for d in os.listdir(CSRC) if os.path.isdir(os.path.join(CSRC, d)) and d not in ("kernels", "extras"))


def store_policy_kernels(feature):
    """the name of every __global__ under csrc/<feature>/ that takes a struct with an `nts` field, or an AUX template argument"""
    text = "\n".join(re.sub(r"//[^\n]*|/\*.*?\*/", "", open(path).read(), flags=re.S) for path in feature_sources(feature))
    with_field = {m.group(1) for m in re.finditer(r"^struct (\w+) \{\n(.*?)\n\};", text, flags=re.M | re.S) if re.search(r"\bnts;", m.group(2))}
    found = set()
    for m in re.finditer(r"(?:template <([^>]*)>\s*)?(?:static )?__global__[^;{]*?\bvoid\s+(\w+)\s*\(\s*(\w+)\s+\w+\s*\)", text):
        if m.group(3) in with_field or re.search(r"\bint AUX", m.group(1) or ""):
            found.add(m.group(2))
    return found


def assignments_to(field):
    """[(function, file, right-hand side)] of every `.<field> = ...;` in a function that a .hip file under csrc/ defines"""
    return [(name, path, rhs.strip()) for name, path, body in hip_functions() for rhs in re.findall(rf"\.{field}\s*=\s*([^;]+);", body)]


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
