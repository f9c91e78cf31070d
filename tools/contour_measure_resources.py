#!/usr/bin/env python3
"""VGPRs, SGPRs, LDS and scratch of every kernel of fraytracer_amd/csrc/contour_measure.hip, from the compiler's own resource remarks for gfx950 with the
Makefile's flags (needs no GPU) -> profiles/contour_measure_kernel_resources.txt.  Every kernel's launch bound is FT_CONTOUR_BLOCK threads: one wave on each
of a compute unit's four SIMDs per workgroup, and a SIMD lane has 512 VGPRs.

    python tools/contour_measure_resources.py [--out profiles/contour_measure_kernel_resources.txt]
"""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fraytracer_amd", "csrc")
sys.path.insert(0, CSRC)
import source_hash  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contour_measure_kernel_resources.txt"))
args = ap.parse_args()

mk = open(os.path.join(CSRC, "Makefile")).read()
common = re.search(r"^COMMON := (.*)$", mk, flags=re.M).group(1).split()
hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
cmd = [hipcc, "--offload-arch=gfx950", *common, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "contour_measure.hip", "-o", os.devnull]
err = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, check=True).stderr
filt = subprocess.run(["c++filt"], input=err, capture_output=True, text=True, check=True).stdout

rows, cur = [], None
for line in filt.splitlines():
    m = re.search(r"remark: .*?Function Name: (.*?)(?: \[-Rpass|$)", line)
    if m:
        cur = {"name": re.sub(r"\(anonymous namespace\)::|void |\(FtContourArgs\)", "", m.group(1)).strip()}
        rows.append(cur)
        continue
    for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("sgpr", r"TotalSGPRs: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
        m = re.search(pat, line)
        if m and cur is not None and key not in cur:
            cur[key] = int(m.group(1))

threads = int(re.search(r"#define FT_CONTOUR_BLOCK (\d+)", open(os.path.join(CSRC, "ft_contour_measure.h")).read()).group(1))
with open(args.out, "w") as f:
    f.write(f"# contour_measure.hip for gfx950, source {source_hash.source_hash()}: registers per lane, LDS bytes per workgroup, scratch bytes per lane, launch bound\n")
    f.write("# resident: workgroups per compute unit by VGPRs alone = 512 / (vgpr rounded up to 8 * waves per SIMD of one workgroup)\n")
    for r in sorted(rows, key=lambda r: r["name"]):
        resident = 512 // (-(-max(r["vgpr"], 1) // 8) * 8 * max(1, threads // 256))
        f.write(f"{r['name']:<48} vgpr {r['vgpr']:>3} sgpr {r['sgpr']:>3} lds {r['lds']:>5} scratch {r['scratch']:>3} threads {threads:>4} resident {resident:>2}\n")
print(open(args.out).read())
