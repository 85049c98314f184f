#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two builds kernel by kernel: registers, static LDS, scratch, instruction stream.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -DMI355_GROUP=0 -DMI355_WLO=c -DMI355_WHI=c \\
          width_group.hip -o before/width_group_c.s          (and predicates/where_group.hip; the same into after/)
    tools/compare_kernel_asm.py before after [--filter shared_]

Prints one line per kernel whose resources or instruction stream differ (with both instruction counts) and a summary;
exit status 1 if any resource differs.  "REGRESSION" marks a kernel that gained scratch or lost a wave per SIMD by its VGPR count
alone (SGPRs, LDS and launch bounds can limit occupancy further: the mark is a lower bound on what went wrong, equal resources
are the proof).  Reads only the .amdhsa_* resource lines and the instruction text."""
import argparse
import glob
import os
import re
import subprocess
import sys

RES = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def waves_per_simd(res):
    """what the 512 unified registers per lane admit (allocated in eights), 8 waves at the most"""
    regs = -(-int(res.get("next_free_vgpr", "1")) // 8) * 8
    return min(8, 512 // max(regs, 8))


def kernels_of(path):
    """{symbol: (resources, [instructions])}"""
    out, body, name = {}, {}, None
    for line in open(path):
        line = line.split(";")[0].rstrip()
        m = re.match(r"^(_Z\w+):$", line)
        if m:
            name, body[name] = m.group(1), []
            continue
        if re.match(r"^\.Lfunc_end", line):
            name = None
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            out[m.group(1)] = ({}, body.get(m.group(1), []))
            cur = out[m.group(1)][0]
            continue
        m = re.match(r"^\s*\.amdhsa_(\w+)\s+(\S+)", line)
        if m and m.group(1) in RES:
            cur[m.group(1)] = m.group(2)
        text = line.strip()
        if name and text and not text.startswith(".") and not text.endswith(":"):
            body[name].append(re.sub(r"\.LBB\d+_\d+", ".L", text))
    return out


def demangle(names):
    try:
        res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, res))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--filter", default="shared_", help="only kernels whose symbol contains this")
    a = ap.parse_args()
    total = same = res_diff = worse = 0
    for fb in sorted(glob.glob(os.path.join(a.before, "*.s"))):
        fa = os.path.join(a.after, os.path.basename(fb))
        if not os.path.exists(fa):
            print(f"missing: {fa}")
            res_diff += 1
            continue
        kb, ka = kernels_of(fb), kernels_of(fa)
        kb = {k: v for k, v in kb.items() if a.filter in k}
        ka = {k: v for k, v in ka.items() if a.filter in k}
        if set(kb) != set(ka):
            print(f"{os.path.basename(fb)}: kernel sets differ: {sorted(set(kb) ^ set(ka))}")
            res_diff += 1
        names = demangle(sorted(set(kb) & set(ka)))
        for k in sorted(set(kb) & set(ka)):
            total += 1
            (rb, ib), (ra, ia) = kb[k], ka[k]
            if rb == ra and ib == ia:
                same += 1
                continue
            what = "" if rb == ra else "  RESOURCES " + " ".join(f"{r}={rb.get(r)}->{ra.get(r)}" for r in RES if rb.get(r) != ra.get(r))
            res_diff += rb != ra
            if waves_per_simd(ra) < waves_per_simd(rb) or int(ra.get("private_segment_fixed_size", 0)) > int(rb.get("private_segment_fixed_size", 0)):
                what += "  REGRESSION (fewer waves per SIMD or more scratch)"
                worse += 1
            print(f"{os.path.basename(fb)}: {names[k]}: instructions {len(ib)} -> {len(ia)}{what}")
    print(f"{total} kernels, {same} identical, {total - same} differ, {res_diff} with different resources, {worse} with fewer waves or more scratch")
    sys.exit(1 if res_diff else 0)


if __name__ == "__main__":
    main()
