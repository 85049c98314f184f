"""Every kernel path of the launcher, by name: CASES is the one list of (call, options) -> kernel (with its template
arguments) that the call must launch, as mi355_ctx_last_launch reports it.

CPU: every __global__ kernel of csrc/kernels/*.hpp and csrc/extras/*.hpp is the expected kernel of some case; the variant
axes the launcher picks between are covered; every kernel-side `flags &` test names a switch of csrc/switches.hpp whose
option value is in the matrix, the table maps option values as the shifts it replaced did, and every option bit of the matrix has a case.
GPU (-m gpu): each case runs, its launch record matches, and every output byte equals numpy, inside 0xEE guard bytes that
must stay untouched.  A shared scan also asks mi355_shared_scan_kernel under its options: the family named is the one launched.  A case with an option bit also runs without that bit: the record must change (the launcher really
took the other path) and the results must not.  The counter-flush cases run on a 4-wave grid (grid_cus = 1,
max_blocks_per_cu = 1) so that every wave walks more than 1100 tiles: the packed 16-bit hit counters flush at least twice.
"""
import ctypes as C
import glob
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

from kernel_cases import (CASES, FLUSH_TILES, LAUNCHER_SET, N_SMALL, SELECT_BITS, SHARED_BITS, SHARED_TILE_ROWS, TIMING_ABLATIONS, UNUSED_BITS,
                          WAVES_PER_BLOCK, build_binary, check_select, column, dry_run, family_of)
from support import CSRC, ROOT, SENTINEL, Guarded, base_name, label_matches, packbits, parse_record

EXEMPT_KERNELS = {}  # kernel name -> reason; none today

# the variant axes the launcher picks between: (regex over a case's expected label, flags set, flags clear, what)
REQUIRED_VARIANTS = [
    (r"shared_wide3_kernel<\d+, \d+, 0, false>", 0, 0, "wide3 RC 0"),
    (r"shared_wide3_kernel<\d+, \d+, 1, false>", 0, 0, "wide3 RC 1"),
    (r"shared_wide3_kernel<\d+, \d+, 2, false>", 0, 0, "wide3 RC 2"),
    (r"shared_wide3_kernel<\d+, \d+, 0, true>", 0, 0, "wide3 RC 0 BIG"),
    (r"shared_wide3_kernel<\d+, \d+, 1, true>", 0, 0, "wide3 RC 1 BIG"),
    (r"shared_wide3_kernel<\d+, \d+, 2, true>", 0, 0, "wide3 RC 2 BIG"),
    (r"shared_wide3_kernel<\d+, 2, .*>", 0, 0, "wide3 plain stores"),
    (r"shared_wide3_kernel<\d+, 18, .*>", 0, 0, "wide3 nt stores"),
    (r"shared_wide2_kernel<\d+, \d+, 64, 0, .*>", 0, 0, "wide2 RC 0"),
    (r"shared_wide2_kernel<\d+, \d+, 64, 1, .*>", 0, 0, "wide2 RC 1"),
    (r"shared_wide2_kernel<\d+, \d+, 64, 2, .*>", 0, 0, "wide2 RC 2"),
    (r"shared_wide2_kernel<\d+, \d+, 64, 0, true>", 0, 0, "wide2 BIG"),
    (r"shared_wide2_kernel<\d+, 2, .*>", 0, 0, "wide2 plain stores"),
    (r"shared_wide2_kernel<\d+, 18, .*>", 0, 0, "wide2 nt stores"),
    (r"shared_wide_kernel<\d+, 2, 64, 0>", 0, 0, "wide per-predicate plain"),
    (r"shared_wide_kernel<\d+, 18, 64, 0>", 0, 0, "wide per-predicate nt"),
    (r"shared_wide_kernel<\d+, 2, 64, 1>", 0, 0, "wide linear"),
    (r"shared_linear_kernel<\d+, 2, 1>", 0x100000, 0, "linear with the aligned image"),
    (r"shared_linear_kernel<\d+, 2, 1>", 0, 0x100000, "linear without the aligned image"),
    (r"shared_linear_kernel<\d+, 2, 2>", 0, 0, "linear, two rows per piece"),
    (r"shared_linear2_kernel<\d+, 2>", 0x20000, 0, "linear2, short table attached"),
    (r"shared_linear2_kernel<\d+, 2>", 0, 0x20000, "linear2, short table detached"),
    (r"shared_linear3_kernel<\d+, 2, 0, .*>", 0, 0, "linear3 RC 0"),
    (r"shared_linear3_kernel<\d+, 2, 1, .*>", 0, 0, "linear3 RC 1"),
    (r"shared_linear3_kernel<\d+, 2, 2, .*>", 0, 0, "linear3 RC 2"),
    (r"shared_linear3_kernel<\d+, 2, \d, true>", 0, 0, "linear3 BIG"),
    (r"shared_lut_kernel<\d+, 34, \d+, 0, false>", 0, 0, "lut per-predicate write-through"),
    (r"shared_lut_kernel<\d+, 18, \d+, 0, false>", 0, 0, "lut per-predicate nt"),
    (r"shared_lut_kernel<\d+, 2, \d+, 0, false>", 0, 0, "lut per-predicate plain"),
    (r"shared_lut_kernel<\d+, 34, \d+, 1, false>", 0, 0, "lut linear write-through"),
    (r"shared_lut_kernel<\d+, 18, \d+, 1, false>", 0, 0, "lut linear nt"),
    (r"shared_lut_kernel<\d+, 2, \d+, 1, false>", 0, 0, "lut linear plain"),
    (r"shared_lut_kernel<\d+, \d+, 128, 0, false>", 0, 0, "lut 128 values per lane"),
    (r"shared_lut_kernel<\d+, \d+, 64, 0, false>", 0, 0, "lut 64 values per lane"),
    (r"shared_lut_kernel<\d+, 2, 64, 1, true>", 0, 0, "lut multi-pass"),
    (r"shared_pair_kernel<\d+, 34, .*>", 0, 0, "pair write-through"),
    (r"shared_pair_kernel<\d+, 18, .*>", 0, 0, "pair nt"),
    (r"scan_burst_kernel<\d+, 0, 0, .*>", 0, 0, "scan default loads"),
    (r"scan_burst_kernel<\d+, 0, 2, .*>", 0, 0, "scan plain stores"),
    (r"scan_burst_kernel<\d+, 0, 18, .*>", 0, 0, "scan nt stores"),
    (r"scan_burst_kernel<\d+, 0, 34, .*>", 0, 0, "scan write-through stores"),
    (r"scan_burst_kernel<\d+, \d, \d+, \d+, 4>", 0, 0, "scan store bursts of 4 tiles"),
    (r"scan_burst_kernel<9, \d, \d+, \d+, 1>", 0, 0, "scan one tile per burst (option)"),
    (r"in_kernel<\d+, 34, .*>", 0, 0, "in write-through"),
    (r"in_kernel<\d+, 18, .*>", 0, 0, "in nt"),
    (r"in_kernel<\d+, 2, .*>", 0, 0, "in plain"),
    (r"scan2_kernel<\d+, 34, .*>", 0, 0, "scan2 write-through"),
    (r"scan2_kernel<\d+, 18, .*>", 0, 0, "scan2 nt"),
    (r"decompress_kernel<\d+, 0>", 0, 0, "decompress dma_aux 0"),
    (r"decompress_kernel<\d+, 2>", 0, 0, "decompress dma_aux 2"),
    (r"decompress_kernel<\d+, 18>", 0, 0, "decompress dma_aux 18"),
    (r"decompress_kernel<\d+, 34>", 0, 0, "decompress dma_aux 34"),
    (r"select_kernel<.*>", 0, 0, "selection, single-role kernel"),
    (r"select2_kernel<.*>", 0, 0, "selection, decoder / expander kernel"),
]


def case_by_id(cid):
    return next(c for c in CASES if c.id == cid)


# ------------------------------------------------------------------------------------------------------------------------
# CPU: the table covers every kernel, every variant axis and every option bit
# ------------------------------------------------------------------------------------------------------------------------

def kernel_sources():
    return sorted(glob.glob(os.path.join(CSRC, "kernels", "*.hpp")) + glob.glob(os.path.join(CSRC, "extras", "*.hpp")))


def global_kernels():
    names = set()
    for f in kernel_sources():
        text = open(f).read()
        names |= set(re.findall(r"__global__[^;{}]*?\bvoid\s+(\w+)\s*\(", text))
    return names


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def strip_debug_blocks(text):
    # the selection's look-back diagnostics exist only in -DMI355_SELECT_DEBUG builds: not a switch of the library
    return re.sub(r"#ifdef MI355_SELECT_DEBUG.*?#endif", "", text, flags=re.S)


def test_case_ids_unique():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))


def test_every_kernel_has_a_case():
    kernels = global_kernels()
    assert len(kernels) >= 20, kernels  # the parse found the kernels
    covered = {base_name(p) for c in CASES for p in c.expect}
    missing = sorted(kernels - covered - set(EXEMPT_KERNELS))
    assert not missing, f"__global__ kernels no case of CASES expects: {missing}"
    stale = sorted((covered | set(EXEMPT_KERNELS)) - kernels)
    assert not stale, f"CASES / EXEMPT_KERNELS name kernels that do not exist: {stale}"


@pytest.mark.parametrize("pattern,set_bits,clear_bits,what", REQUIRED_VARIANTS, ids=[v[3] for v in REQUIRED_VARIANTS])
def test_every_variant_has_a_case(pattern, set_bits, clear_bits, what):
    hits = [c.id for c in CASES for p in c.expect if re.fullmatch(pattern, p)
            and (c.set_bits & set_bits) == set_bits and (c.clear_bits & clear_bits) == clear_bits]
    assert hits, f"no case covers {what} ({pattern})"


def switch_table():
    """csrc/switches.hpp as tests/cpp/launch_dry_run --switches prints it: [(name, option value, kernel-side bit, receiver)]"""
    out = subprocess.run([build_binary(), "--switches"], capture_output=True, text=True, timeout=60, check=True).stdout
    return [(name, int(opt), int(kbit, 16), recv) for name, opt, kbit, recv in (ln.split("\t") for ln in out.splitlines())]


def switch_words(options):
    """[(shared scans' word, selection's word)] of kernel_switch_word() per option value, read from the flags=0x... of the launch
    record of an equality scan (every launch but the selection's carries the shared scans' word) and of a selection"""
    recs = dry_run([(op, 9, 1, 0, 1, N_SMALL, v, 0, -1, 0, 18, 0, 0) for v in options for op in (0, 5)])
    words = [parse_record(text)[0][3] for _, text in recs]
    return list(zip(words[0::2], words[1::2]))


def test_flag_shifts_keep_the_selection_apart():
    rows = switch_table()
    assert len({r[0] for r in rows}) == len(rows) and {r[3] for r in rows} == {"shared", "select", "launcher-set", "reserved"}, rows
    options = {recv: {r[1] for r in rows if r[3] == recv} for recv in ("shared", "select", "launcher-set", "reserved")}
    kbits = {recv: {r[2] for r in rows if r[3] == recv} for recv in options}
    assert not options["select"] & options["shared"], "an option bit reaches both the shared scans and the selection"
    assert options["select"] == set(SELECT_BITS[:2]) | set(TIMING_ABLATIONS) == {512, 1024, 2048, 4096}, sorted(options["select"])
    assert options["shared"] == set(SHARED_BITS), sorted(options["shared"])
    assert options["launcher-set"] == {0}, "a launcher-set switch has an option value"
    assert kbits["launcher-set"] == set(LAUNCHER_SET), kbits["launcher-set"]
    assert options["reserved"] == set(UNUSED_BITS), options["reserved"]
    # neither the launcher's own rows (no option value) nor the reserved one give a receiver anything, and no option bit at all
    # brings about a launcher-set or reserved kernel bit, or one of the other receiver
    for v, (shared, select) in zip([0] + sorted(UNUSED_BITS), switch_words([0] + sorted(UNUSED_BITS))):
        assert shared == 0 and select == 0, f"option value {v} reaches the kernels: {shared:#x} / {select:#x}"
    singles = [1 << b for b in range(32)]
    for v, (shared, select) in zip(singles, switch_words(singles)):
        assert not shared & ~sum(kbits["shared"]) and not select & ~sum(kbits["select"]), f"option bit {v}: {shared:#x} / {select:#x}"
        assert not (shared and select), f"option bit {v} reaches both the shared scans and the selection"


# what capi.hip's launch() computed before csrc/switches.hpp held the table (recorded old behaviour): select, everything else
OLD_SWITCH_WORD = (lambda v: (v >> 8) & 0x1e, lambda v: (v & 0x1ff) | ((v >> 4) & 0xdee00))


def test_switch_word_is_what_the_shifts_gave():
    """the mapping is bitwise, so the 32 single-bit option values cover it"""
    singles = [1 << b for b in range(32)]
    for v, (shared, select) in zip(singles, switch_words(singles)):
        assert select == OLD_SWITCH_WORD[0](v), f"option bit {v}, selection: {select:#x}"
        assert shared == OLD_SWITCH_WORD[1](v), f"option bit {v}, shared scans: {shared:#x}"


FLAGS_AND = r"\bflags\s*&(?!&)"


def kernel_flag_tests():
    """(file, switch name) for every `flags & <name>` / `flags & (<name> | <name>)` of width_group.hip, shared_plan.hpp and
    kernels/*.hpp; whatever else follows a `flags &` fails here"""
    out = []
    for f in [os.path.join(CSRC, "width_group.hip"), os.path.join(CSRC, "shared_plan.hpp")] + sorted(glob.glob(os.path.join(CSRC, "kernels", "*.hpp"))):
        text = strip_comments(strip_debug_blocks(open(f).read()))
        assert not re.search(FLAGS_AND + r"[\s(]*(0x[0-9a-fA-F]+|\d)", text), f"{os.path.basename(f)}: a numeric literal next to `flags &`"
        found = re.findall(FLAGS_AND + r"\s*(?:\(([^()]*)\)|([A-Za-z_]\w*))", text)
        assert len(found) == len(re.findall(FLAGS_AND, text)), f"{os.path.basename(f)}: a `flags &` without a switch name behind it"
        for group, one in found:
            out += [(os.path.basename(f), name.strip()) for name in (group.split("|") if group else [one])]
    return out


def test_kernel_flag_tests_are_in_the_matrix():
    tests = kernel_flag_tests()
    assert len(tests) >= 20, tests  # the parse found the launcher's switches
    table = {name: (opt, kbit, recv) for name, opt, kbit, recv in switch_table()}
    documented = set(SHARED_BITS) | set(SELECT_BITS) | set(TIMING_ABLATIONS)
    for fname, name in tests:
        assert name in table, f"{fname}: `flags & {name}`: not a switch of csrc/switches.hpp"
        opt, kbit, recv = table[name]
        if fname in ("select.hpp", "select2.hpp"):
            assert recv == "select", f"{fname}: {name} is a switch of receiver {recv}"
        else:
            assert recv in ("shared", "launcher-set"), f"{fname}: {name} is a switch of receiver {recv}"
            if recv == "launcher-set":
                assert kbit in LAUNCHER_SET, f"{fname}: {name} = {kbit:#x}"
                continue
        assert opt in documented, f"{fname}: {name} = option bit {opt}: not in the option-bit matrix"


def test_design_lists_every_switch():
    """DESIGN.md's "A/B switches" section has every row of the table, name and option value on one line"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    start = text.index("**A/B switches.**")
    section = text[start:text.index("\n## 9.", start)].splitlines()
    for name, opt, kbit, recv in switch_table():
        cell = str(opt) if opt else "—"
        assert any(re.search(rf"\|\s*`{name}`\s*\|\s*{cell}\s*\|\s*{recv}\s*\|", ln) for ln in section), f"DESIGN.md section 8: no row for {name} ({cell}, {recv})"


def test_every_option_bit_has_a_case():
    for b in SHARED_BITS + list(UNUSED_BITS):
        got = [c.id for c in CASES if c.bit == b and c.opt("kernel_flags") & b and c.op == "shared"]
        assert got, f"option bit {b}: no shared-scan case"
    for b in SELECT_BITS:
        for single in (0, 1):
            got = [c.id for c in CASES if c.op == "select" and c.bit == b and c.opt("kernel_flags") == b and c.opt("select_kernel") == single]
            assert got, f"option bit {b}: no case on {'select_kernel' if single else 'select2_kernel'}"
    for c in CASES:
        if c.bit:
            assert c.opt("kernel_flags") & c.bit, c.id
            assert c.bit in SHARED_BITS + SELECT_BITS or c.bit in UNUSED_BITS, c.id


def test_flush_cases_walk_enough_tiles():
    flush = [c for c in CASES if c.min_tiles == FLUSH_TILES]
    assert {(c.c, c.P, c.layout) for c in flush} >= {(9, 33, 0), (9, 48, 0), (9, 63, 0), (17, 33, 0), (17, 48, 0), (17, 64, 0),
                                                      (9, 33, 1), (9, 40, 1)}
    for c in flush + [c for c in CASES if c.min_tiles]:
        ntiles = (c.n + SHARED_TILE_ROWS - 1) // SHARED_TILE_ROWS
        assert ntiles // WAVES_PER_BLOCK > c.min_tiles, c.id
        assert c.n % SHARED_TILE_ROWS != 0, c.id  # ragged tail
        assert c.opt("grid_cus") == 1 and c.opt("max_blocks_per_cu") == 1, c.id


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------


class Runner:
    def __init__(self, L, O):
        self.L, self.O = L, O

    def ok(self, rc):
        assert rc == 0, self.L.mi355_last_error()

    def run(self, case, opts):
        """run the case with these options; check every output byte; -> the launch record"""
        import torch

        from shared_simd_scan_amd import ScanEngine

        eng = ScanEngine()
        self.last_record = ""
        try:
            for name, value in opts:
                eng.set_option(name, value)
            rng = np.random.default_rng(zlib.crc32(case.id.encode()))
            getattr(self, "op_" + case.op)(eng, case, rng, torch)  # reads the record before it checks the outputs
            return self.last_record
        finally:
            eng.close()

    def record(self, eng):
        eng.synchronize()
        self.last_record = (self.L.mi355_ctx_last_launch(eng._ctx) or b"").decode()

    def upload(self, torch, vals, c):
        return torch.from_numpy(self.O.pack(vals, c)).cuda()

    # ---- shared scans ----
    def op_shared(self, eng, case, rng, torch):
        n, c, P = case.n, case.c, case.P
        vals, keys = column(case, rng)
        packed = self.upload(torch, vals, c)
        nb = (n + 7) // 8
        stride = (nb + 15) // 16 * 16 + 16  # a guard gap behind every bitmap of the per-predicate layout
        out = Guarded(P * stride if case.layout == 0 else P * nb)
        hits = Guarded(8 * P) if case.hits else None
        k = np.ascontiguousarray(np.asarray(keys, dtype=np.uint32).view(np.int32))
        named = self.L.mi355_shared_scan_kernel(eng._ctx, c, P, case.layout, int(case.hits))  # under the case's options
        self.ok(self.L.mi355_shared_scan_eq_dev(eng._ctx, C.c_void_p(packed.data_ptr()), n, c, k.ctypes.data_as(C.c_void_p), P,
                                                case.layout, out.ptr, stride, hits.ptr if hits else None))
        self.record(eng)
        launched = parse_record(self.last_record)
        assert len(launched) == 1 and named is not None and named.decode() == family_of(launched[0][0]), \
            f"the library names {named}, launched:\n{self.last_record}"
        body = out.fetch()
        uniq = {}
        for key in keys:
            if key not in uniq:
                uniq[key] = (packbits(vals == key), int((vals == key).sum()))
        if case.layout == 0:
            seg = body.reshape(P, stride)
            for j, key in enumerate(keys):
                assert np.array_equal(seg[j, :nb], uniq[key][0]), f"bitmap of key {j} differs"
            assert (seg[:, nb:] == SENTINEL).all(), "bytes between the per-predicate bitmaps overwritten"
        else:
            lin = body.reshape(nb, P)
            for j, key in enumerate(keys):
                assert np.array_equal(lin[:, j], uniq[key][0]), f"linear column of key {j} differs"
        if hits:
            got = hits.fetch().view(np.uint64)
            assert got.tolist() == [uniq[key][1] for key in keys]

    # ---- scans ----
    def _scan(self, eng, case, rng, torch, call):
        vals, keys = column(case, rng)
        packed = self.upload(torch, vals, case.c)
        bm, hits = Guarded((case.n + 7) // 8), Guarded(8, back=64, front=64)
        expect = call(C.c_void_p(packed.data_ptr()), vals, keys, bm, hits)
        self.record(eng)
        assert np.array_equal(bm.fetch(), packbits(expect))
        assert int(hits.fetch().view(np.uint64)[0]) == int(expect.sum())

    def op_scan_eq(self, eng, case, rng, torch):
        def call(p, vals, keys, bm, hits):
            self.ok(self.L.mi355_scan_eq_dev(eng._ctx, p, case.n, case.c, keys[0], bm.ptr, hits.ptr))
            return vals == keys[0]
        self._scan(eng, case, rng, torch, call)

    def op_scan_range(self, eng, case, rng, torch):
        def call(p, vals, keys, bm, hits):
            lo, hi = sorted((keys[0], (keys[0] * 7 + 5) % (1 << case.c)))
            self.ok(self.L.mi355_scan_range_dev(eng._ctx, p, case.n, case.c, lo, hi, bm.ptr, hits.ptr))
            return (vals >= lo) & (vals <= hi)
        self._scan(eng, case, rng, torch, call)

    def op_combine(self, eng, case, rng, torch):
        mask_bits = rng.random(case.n) < 0.5
        mask = torch.from_numpy(packbits(mask_bits)).cuda()

        def call(p, vals, keys, bm, hits):
            lo, hi = 100, 300
            self.ok(self.L.mi355_scan_combine_dev(eng._ctx, p, case.n, case.c, 6, lo, hi, 0, C.c_void_p(mask.data_ptr()), bm.ptr, hits.ptr))
            return (vals >= lo) & (vals <= hi) & mask_bits
        self._scan(eng, case, rng, torch, call)

    def op_in(self, eng, case, rng, torch):
        def call(p, vals, keys, bm, hits):
            k = np.ascontiguousarray(np.asarray(keys, dtype=np.int32))
            self.ok(self.L.mi355_scan_in_dev(eng._ctx, p, case.n, case.c, k.ctypes.data_as(C.c_void_p), len(keys), 0, None, bm.ptr, hits.ptr))
            return np.isin(vals, np.asarray(keys, dtype=np.uint32))
        self._scan(eng, case, rng, torch, call)

    def op_scan2(self, eng, case, rng, torch):
        vals2 = rng.integers(0, 1 << case.c, case.n).astype(np.uint32)
        packed2 = self.upload(torch, vals2, case.c)

        def call(p, vals, keys, bm, hits):
            self.ok(self.L.mi355_scan2_dev(eng._ctx, p, case.c, 0, keys[0], 0, C.c_void_p(packed2.data_ptr()), case.c, 2, 256, 0, case.n,
                                           0, bm.ptr, hits.ptr))
            return (vals == keys[0]) & (vals2 < 256)
        self._scan(eng, case, rng, torch, call)

    # ---- selection ----
    def op_select(self, eng, case, rng, torch):
        vals, keys = column(case, rng)
        packed = self.upload(torch, vals, case.c)
        check_select(self.L, eng, packed, vals, case.n, case.c, 2, 1 << (case.c - 2), "gt", after=lambda: self.record(eng))

    # ---- decompress / pack ----
    def op_decompress(self, eng, case, rng, torch):
        vals, _ = column(case, rng)
        packed = self.upload(torch, vals, case.c)
        out = Guarded(4 * case.n)
        self.ok(self.L.mi355_decompress_dev(eng._ctx, C.c_void_p(packed.data_ptr()), case.n, case.c, out.ptr))
        self.record(eng)
        assert np.array_equal(out.fetch().view(np.int32), vals.astype(np.int32))

    def op_generate(self, eng, case, rng, torch):
        size = self.L.mi355_compressed_buffer_size(case.c, case.n)
        out = Guarded(size)
        self.ok(self.L.mi355_generate_dev(eng._ctx, 1, 0, case.n, case.c, 42, out.ptr))
        self.record(eng)
        assert np.array_equal(out.fetch(), self.O.pack(self.O.gen_values("splitmix", case.n, case.c, 42), case.c))

    def op_pack_u32(self, eng, case, rng, torch):
        vals, _ = column(case, rng)
        dv = torch.from_numpy(vals.view(np.int32)).cuda()
        out = Guarded(self.L.mi355_compressed_buffer_size(case.c, case.n))
        self.ok(self.L.mi355_pack_u32_dev(eng._ctx, C.c_void_p(dv.data_ptr()), case.n, case.c, out.ptr))
        self.record(eng)
        assert np.array_equal(out.fetch(), self.O.pack(vals, case.c))

    # ---- bitmap consumers ----
    def _bitmaps(self, case, rng, torch):
        a, b = rng.random(case.n) < 0.4, rng.random(case.n) < 0.6
        return a, b, torch.from_numpy(packbits(a)).cuda(), torch.from_numpy(packbits(b)).cuda()

    def op_bitmap_and(self, eng, case, rng, torch):
        a, b, da, db = self._bitmaps(case, rng, torch)
        out = Guarded((case.n + 7) // 8)
        self.ok(self.L.mi355_bitmap_combine_dev(eng._ctx, 0, C.c_void_p(da.data_ptr()), C.c_void_p(db.data_ptr()), out.ptr, case.n, None))
        self.record(eng)
        assert np.array_equal(out.fetch(), packbits(a & b))

    def op_bitmap_count(self, eng, case, rng, torch):
        a, _, da, _ = self._bitmaps(case, rng, torch)
        cnt = Guarded(8, back=64, front=64)
        self.ok(self.L.mi355_bitmap_count_dev(eng._ctx, C.c_void_p(da.data_ptr()), case.n, cnt.ptr))
        self.record(eng)
        assert int(cnt.fetch().view(np.uint64)[0]) == int(a.sum())

    def op_rowids(self, eng, case, rng, torch):
        a, _, da, _ = self._bitmaps(case, rng, torch)
        want = np.nonzero(a)[0].astype(np.uint64) + 5
        ids, cnt = Guarded(8 * len(want)), Guarded(8, back=64, front=64)
        self.ok(self.L.mi355_bitmap_to_rowids_dev(eng._ctx, C.c_void_p(da.data_ptr()), case.n, 5, ids.ptr, len(want), cnt.ptr))
        self.record(eng)
        assert np.array_equal(ids.fetch().view(np.uint64), want)
        assert int(cnt.fetch().view(np.uint64)[0]) == len(want)

    def op_gather(self, eng, case, rng, torch):
        vals, _ = column(case, rng)
        packed = self.upload(torch, vals, case.c)
        rows = rng.integers(0, case.n, 3000).astype(np.uint64)
        drows = torch.from_numpy(rows.view(np.int64)).cuda()
        dcnt = torch.tensor([len(rows)], dtype=torch.int64, device="cuda")
        out = Guarded(4 * len(rows))
        self.ok(self.L.mi355_gather_dev(eng._ctx, C.c_void_p(packed.data_ptr()), case.n, case.c, 0, C.c_void_p(drows.data_ptr()),
                                        C.c_void_p(dcnt.data_ptr()), len(rows), out.ptr))
        self.record(eng)
        assert np.array_equal(out.fetch().view(np.int32), vals[rows.astype(np.int64)].astype(np.int32))

    def op_aggregate(self, eng, case, rng, torch):
        vals, _ = column(case, rng)
        packed = self.upload(torch, vals, case.c)
        out = Guarded(32, back=64, front=64)
        self.ok(self.L.mi355_aggregate_dev(eng._ctx, C.c_void_p(packed.data_ptr()), case.n, case.c, None, out.ptr))
        self.record(eng)
        v = vals.astype(np.uint64)
        assert out.fetch().view(np.uint64).tolist() == [int(v.sum()), case.n, int(v.min()), int(v.max())]

    def op_histogram(self, eng, case, rng, torch):
        vals, _ = column(case, rng)
        packed = self.upload(torch, vals, case.c)
        out = Guarded(8 << case.c)
        self.ok(self.L.mi355_histogram_dev(eng._ctx, C.c_void_p(packed.data_ptr()), case.n, case.c, None, out.ptr))
        self.record(eng)
        assert np.array_equal(out.fetch().view(np.uint64), np.bincount(vals, minlength=1 << case.c).astype(np.uint64))


# differs from support.L: a missing library is an error here, it is not built
@pytest.fixture(scope="module")
def L():
    from shared_simd_scan_amd import lib

    return lib()


@pytest.fixture(scope="module")
def runner(L, O):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return Runner(L, O)


def expected_tiles_per_wave(case, launch):
    _, grid, _, _ = launch
    ntiles = (case.n + SHARED_TILE_ROWS - 1) // SHARED_TILE_ROWS
    return ntiles // (grid * WAVES_PER_BLOCK)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_kernel_path(runner, cid):
    case = case_by_id(cid)
    text = runner.run(case, case.opts)
    rec = parse_record(text)
    assert len(rec) == len(case.expect) and all(label_matches(p, r[0]) for p, r in zip(case.expect, rec)), \
        f"{cid}: expected {list(case.expect)}, launched:\n{text}"
    flags = rec[-1][3]
    assert flags & case.set_bits == case.set_bits and not flags & case.clear_bits, f"{cid}: flags {flags:#x}\n{text}"
    if case.min_tiles:
        assert rec[-1][1] == 1, f"{cid}: grid_cus = 1, max_blocks_per_cu = 1 should give one block:\n{text}"
        assert expected_tiles_per_wave(case, rec[-1]) > case.min_tiles
    if case.bit:
        opts = tuple((k, v & ~case.bit) if k == "kernel_flags" else (k, v) for k, v in case.opts)
        base = runner.run(case, opts)
        if case.bit in UNUSED_BITS:
            assert base == text, f"unused option bit {case.bit} changed the launch:\n{base}\n->\n{text}"
        else:
            assert base != text, f"option bit {case.bit} did not change the launch:\n{text}"


SELECT_GUARD_BITS = [0] + SHARED_BITS + SELECT_BITS + list(UNUSED_BITS) + list(TIMING_ABLATIONS)


@pytest.mark.gpu
@pytest.mark.parametrize("capacity", ["lt", "eq", "gt"])
@pytest.mark.parametrize("bit", SELECT_GUARD_BITS)
@pytest.mark.parametrize("single", [0, 1], ids=["select2", "select_single"])
def test_select_stays_inside_its_buffers(runner, O, single, bit, capacity):
    """every option bit, both kernels: nothing is written past rowids[capacity] or count_dev[0] (the timing ablations give
    wrong ids by construction: only the guards are checked under them)"""
    import torch

    from shared_simd_scan_amd import ScanEngine

    n, c = N_SMALL, 9
    vals = np.random.default_rng(bit + 7 * single).integers(0, 1 << c, n).astype(np.uint32)
    packed = torch.from_numpy(O.pack(vals, c)).cuda()
    eng = ScanEngine()
    try:
        eng.set_option("select_kernel", single)
        eng.set_option("kernel_flags", bit)
        check_select(runner.L, eng, packed, vals, n, c, 2, 200, capacity, check_ids=bit not in TIMING_ABLATIONS)
        rec = parse_record(runner.L.mi355_ctx_last_launch(eng._ctx).decode())
        assert len(rec) == 1 and base_name(rec[0][0]) == ("select_kernel" if single else "select2_kernel")
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("density", ["dense", "sparse"])
@pytest.mark.parametrize("grid_cus", [1, 2, 3])
@pytest.mark.parametrize("single", [0, 1], ids=["select2", "select_single"])
@pytest.mark.parametrize("chunks", [8, 24])
def test_select_lookback_small_grid(runner, O, chunks, single, grid_cus, density):
    """a grid of one to three blocks: every block walks several chunks (65536 rows at c = 9), the look-back crosses its own
    earlier chunks"""
    import torch

    from shared_simd_scan_amd import ScanEngine

    n, c = 65536 * (chunks - 1) + 77, 9
    vals = np.random.default_rng(grid_cus).integers(0, 1 << c, n).astype(np.uint32)
    packed = torch.from_numpy(O.pack(vals, c)).cuda()
    eng = ScanEngine()
    try:
        eng.set_option("select_kernel", single)
        eng.set_option("grid_cus", grid_cus)
        eng.set_option("max_blocks_per_cu", 1)
        op, a = (2, 300) if density == "dense" else (0, 77)
        check_select(runner.L, eng, packed, vals, n, c, op, a, "gt")
        rec = parse_record(runner.L.mi355_ctx_last_launch(eng._ctx).decode())
        assert len(rec) == 1 and rec[0][1] == min(grid_cus, (chunks + WAVES_PER_BLOCK - 1) // WAVES_PER_BLOCK), rec  # grid_for()
    finally:
        eng.close()


@pytest.mark.gpu
def test_grid_cus_option_range(runner):
    import torch

    from shared_simd_scan_amd import Mi355Error, ScanEngine

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    eng = ScanEngine()
    try:
        for bad in (-1, cus + 1):
            with pytest.raises(Mi355Error):
                eng.set_option("grid_cus", bad)
        for good in (1, cus, 0):
            eng.set_option("grid_cus", good)
    finally:
        eng.close()


@pytest.mark.gpu
def test_launch_record_scope(runner, O):
    """a call starts a new record; a compound call records all of its launches; a call that launches nothing leaves it empty"""
    import torch

    from shared_simd_scan_amd import ScanEngine

    L = runner.L
    n = N_SMALL
    rng = np.random.default_rng(5)
    v9, v12 = rng.integers(0, 512, n).astype(np.uint32), rng.integers(0, 4096, n).astype(np.uint32)
    p9, p12 = torch.from_numpy(O.pack(v9, 9)).cuda(), torch.from_numpy(O.pack(v12, 12)).cuda()
    bm, hits = Guarded((n + 7) // 8), Guarded(8, back=64, front=64)
    eng = ScanEngine()
    try:
        assert L.mi355_ctx_last_launch(eng._ctx) == b""
        runner.ok(L.mi355_scan2_dev(eng._ctx, C.c_void_p(p9.data_ptr()), 9, 0, 5, 0, C.c_void_p(p12.data_ptr()), 12, 2, 99, 0, n, 0,
                                    bm.ptr, hits.ptr))
        rec = parse_record(L.mi355_ctx_last_launch(eng._ctx).decode())
        assert [r[0] for r in rec] == ["scan_burst_kernel<9, 1, 34, 128, 4>", "scan_burst_kernel<12, 1, 34, 128, 4>"], rec
        eng.synchronize()
        assert np.array_equal(bm.fetch(), packbits((v9 == 5) & (v12 < 99)))
        eng.set_option("kernel_flags", 0)  # options leave the record alone
        assert len(parse_record(L.mi355_ctx_last_launch(eng._ctx).decode())) == 2
        runner.ok(L.mi355_scan_eq_dev(eng._ctx, C.c_void_p(p9.data_ptr()), 0, 9, 5, bm.ptr, hits.ptr))  # n = 0: nothing launched
        assert L.mi355_ctx_last_launch(eng._ctx) == b""
    finally:
        eng.close()
