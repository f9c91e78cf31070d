#!/usr/bin/env python3
"""VGPRs, SGPRs, LDS and scratch of every kernel of fraytracer_amd/csrc/shells.hip, from the compiler's own resource remarks for gfx950 with the
Makefile's flags (needs no GPU) -> profiles/shells_kernel_resources.txt.  `threads` is the kernel's launch bound: a workgroup of T threads puts
max(1, T / 256) waves on each of a compute unit's four SIMDs, and a SIMD lane has 512 VGPRs.

    python tools/shells_resources.py [--out profiles/shells_kernel_resources.txt]
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shells_kernel_resources.txt"))
args = ap.parse_args()

mk = open(os.path.join(CSRC, "Makefile")).read()
common = re.search(r"^COMMON := (.*)$", mk, flags=re.M).group(1).split()
hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
cmd = [hipcc, "--offload-arch=gfx950", *common, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "shells.hip", "-o", os.devnull]
err = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, check=True).stderr
filt = subprocess.run(["c++filt"], input=err, capture_output=True, text=True, check=True).stdout

rows, cur = [], None
for line in filt.splitlines():
    m = re.search(r"remark: .*?Function Name: (.*?)(?: \[-Rpass|$)", line)
    if m:
        name = re.sub(r"\(anonymous namespace\)::|void |\(FtShellsArgs\)", "", m.group(1)).strip()
        cur = {"name": name}
        rows.append(cur)
        continue
    for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("sgpr", r"TotalSGPRs: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
        m = re.search(pat, line)
        if m and cur is not None and key not in cur:
            cur[key] = int(m.group(1))

src = open(os.path.join(CSRC, "shells.hip")).read()
head = open(os.path.join(CSRC, "ft_shells.h")).read()
scan_block = int(re.search(r"#define FT_SHELLS_SCAN_BLOCK (\d+)", head).group(1))
flat_block = int(re.search(r"#define FT_SHELLS_FLAT_BLOCK (\d+)", head).group(1))


def threads(name):
    m = re.search(r"<(\d+)>", name)
    if m:
        return int(m.group(1))
    bound = re.search(r"__launch_bounds__\((\w+)\) void " + re.escape(name) + r"\(", src).group(1)
    return {"FT_SHELLS_SCAN_BLOCK": scan_block, "FT_SHELLS_FLAT_BLOCK": flat_block}[bound]


with open(args.out, "w") as f:
    f.write(f"# shells.hip for gfx950, source {source_hash.source_hash()}: registers per lane, LDS bytes per workgroup, scratch bytes per lane, launch bound\n")
    f.write("# resident: workgroups per compute unit by VGPRs alone = 512 / (vgpr rounded up to 8 * waves per SIMD of one workgroup)\n")
    for r in sorted(rows, key=lambda r: r["name"]):
        t = threads(r["name"])
        per_simd = max(1, t // 256)
        resident = 512 // (-(-max(r["vgpr"], 1) // 8) * 8 * per_simd)
        f.write(f"{r['name']:<48} vgpr {r['vgpr']:>3} sgpr {r['sgpr']:>3} lds {r['lds']:>5} scratch {r['scratch']:>3} threads {t:>4} resident {resident:>2}\n")
print(open(args.out).read())
