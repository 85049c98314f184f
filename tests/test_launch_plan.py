"""The width-group launchers decide on the host, so what they would launch is checked here without a GPU.

tests/cpp/launch_dry_run.cpp links against csrc/build/width_group_*.o and calls launch_group_N with LaunchReq::choice_out
set: nothing is launched, the launcher reports the kernel family and writes the launch-record line.

* every case of kernel_cases.CASES that passes through the width groups: the recorded label matches `expect`, the flags
  word carries `set_bits` / `clear_bits`, and the reported family (what mi355_shared_scan_kernel names) is the family of the
  recorded label;
* every width, every key count, both layouts, with and without hit counts at kernel_flags = 0: reported family == family of
  the recorded label.

Grids are not asserted: the occupancy queries have no device to ask.
"""
from kernel_cases import CASES, N_SMALL, dry_run, family_of
from support import label_matches, parse_record

# launch_dry_run.cpp's `op` (dispatch.hpp enum Op) of the cases that go through launch_group_N
WIDTH_OPS = {"scan_eq": 0, "scan_range": 1, "combine": 1, "shared": 2, "decompress": 3, "in": 4, "select": 5, "scan2": 6}
# SharedFamily (shared_plan.hpp) -> the name mi355_shared_scan_kernel returns
FAMILIES = ["shared_lut_kernel", "shared_lut_kernel(multi-pass)", "shared_wide_kernel", "shared_general_kernel", "shared_linear_kernel",
            "shared_pair_kernel"]
# (c, P, layout, hits) the sweep leaves out, with the reason; none
SWEEP_EXCLUSIONS = {}


def test_kernel_path_cases_without_a_gpu():
    cases = [c for c in CASES if c.op in WIDTH_OPS]
    assert len(cases) >= 90 and {c.op for c in cases} == set(WIDTH_OPS), len(cases)
    rows = [(WIDTH_OPS[c.op], c.c, c.P, c.layout, c.hits, c.n, c.opt("kernel_flags"), c.opt("shared_vpl"), c.opt("scan_nt_stores", -1),
             c.opt("max_blocks_per_cu"), c.opt("dma_aux", 18), c.opt("scan_burst"), c.opt("select_kernel") == 1) for c in cases]
    for case, (fam, text) in zip(cases, dry_run(rows)):
        rec = parse_record(text)
        assert len(rec) == 1 == len(case.expect) and label_matches(case.expect[0], rec[0][0]), f"{case.id}: expected {case.expect}, recorded {text}"
        flags = rec[0][3]
        assert flags & case.set_bits == case.set_bits and not flags & case.clear_bits, f"{case.id}: flags {flags:#x}"
        if case.op == "shared":
            assert case.P >= 2, case.id  # (P = 1 is the equality scan: capi.hip never plans it)
            assert FAMILIES[fam] == family_of(rec[0][0]), f"{case.id}: named {FAMILIES[fam]}, recorded {text}"
        else:
            assert fam == -1, f"{case.id}: a family reported for op {case.op}"


def test_named_family_is_the_launched_family_everywhere():
    points = [(c, P, layout, hits) for c in range(1, 33) for P in range(2, 1025) for layout in (0, 1) for hits in (0, 1)
              if (c, P, layout, hits) not in SWEEP_EXCLUSIONS]
    assert len(points) == 32 * 1023 * 4 - len(SWEEP_EXCLUSIONS)
    got = dry_run([(2, c, P, layout, hits, N_SMALL, 0, 0, -1, 0, 18, 0, 0) for c, P, layout, hits in points])
    bad = []
    for point, (fam, text) in zip(points, got):
        label = text.split(" grid=")[0]
        if not 0 <= fam < len(FAMILIES) or FAMILIES[fam] != family_of(label):
            bad.append((point, fam, label))
    assert not bad, f"{len(bad)} points name a family they do not launch, e.g. {bad[:5]}"
