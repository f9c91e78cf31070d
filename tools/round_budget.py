#!/usr/bin/env python3
"""Static instruction budget of one trace kernel, per region of its round, from the device assembly.
Usage: make -C fraytracer_amd/csrc kernels.dev.s && python3 tools/round_budget.py [--kernel ft_trace_kernel_smooth_spheres] [--json] fraytracer_amd/csrc/kernels.dev.s
The assembly carries line tables (the Makefile's kernels.dev.s target), so every instruction names the line of kernels.hip it was compiled from, inlined
code included.  A region is a function of kernels.hip, and within ft_trace_body the part of the round under each of its `// ---- ` headings.  Instructions
are classed by mnemonic prefix alone (v_ VALU, s_ SALU with its loads, waits, no-ops and branches apart, ds_ LDS, global_ / flat_ / buffer_ / scratch_ VMEM);
the only instructions looked at by name are v_readlane / v_writelane on the registers the compiler spills SGPRs into.  Then the code object's own figures:
SGPRs, VGPRs, spilled SGPRs, scratch bytes, code bytes."""
import argparse, collections, json, os, re, sys

ap = argparse.ArgumentParser()
ap.add_argument("asm")
ap.add_argument("--kernel", default="ft_trace_kernel_smooth_spheres")
ap.add_argument("--source", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fraytracer_amd", "csrc", "kernels.hip"))
ap.add_argument("--json", action="store_true")
args = ap.parse_args()

# ---- regions of kernels.hip: (first line, name), ascending ----
src = open(args.source).read().split("\n")
starts = []
body = None
for n, line in enumerate(src, 1):
    m = re.match(r"__device__ __forceinline__ [^(]*?\b(\w+)\s*\(", line)
    if m:
        starts.append((n, m.group(1)))
        body = m.group(1)
    elif body == "ft_trace_body" and line.startswith("}"):
        body = None
    elif body == "ft_trace_body" and (m2 := re.match(r"\s+// ---- (.*?)[ -]*$", line)):
        starts.append((n, ("round: " + re.sub(r"\s*[(:].*", "", m2.group(1)))[:43]))
first = [s[0] for s in starts]


def region(line):
    import bisect
    i = bisect.bisect_right(first, line) - 1
    return starts[i][1] if i >= 0 else "(header)"


CLASSES = ("VALU", "SALU", "SMEM", "LDS", "VMEM", "wait/nop", "branch")


def classify(mn):
    if mn.startswith("v_"): return "VALU"
    if mn.startswith("ds_"): return "LDS"
    if mn.startswith(("global_", "flat_", "buffer_", "scratch_")): return "VMEM"
    if mn.startswith(("s_load", "s_buffer_load", "s_memtime", "s_memrealtime")): return "SMEM"
    if mn.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_sleep")): return "wait/nop"
    if mn.startswith(("s_branch", "s_cbranch", "s_endpgm")): return "branch"
    if mn.startswith("s_"): return "SALU"
    return None


# ---- the kernel's text ----
text = open(args.asm).read().split("\n")
try:
    i0 = text.index(args.kernel + ":" + " " * 9 + "; @" + args.kernel)
except ValueError:
    i0 = next(i for i, l in enumerate(text) if l.startswith(args.kernel + ":"))
counts = collections.defaultdict(collections.Counter)
spill_regs, files, cur, own = set(), {}, 0, None
for l in text:                                                         # the file number of kernels.hip in the line tables
    m = re.match(r"\s+\.file\s+(\d+)\s+(?:\"[^\"]*\"\s+)?\"([^\"]*)\"", l)
    if m and os.path.basename(m.group(2)) == os.path.basename(args.source):
        own = m.group(1)
code_bytes = None
for l in text[i0 + 1:]:
    if l.startswith(".Lfunc_end"):
        break
    m = re.match(r"\s+\.loc\s+(\d+)\s+(\d+)", l)
    if m:
        if (own is None or m.group(1) == own) and int(m.group(2)) != 0:     # line 0: compiler-made code stays with the line before it
            cur = int(m.group(2))
        continue
    m = re.search(r"implicit-def: \$(vgpr\d+) : SGPR spill to VGPR lane", l)
    if m:
        spill_regs.add("v" + m.group(1)[4:])
        continue
    m = re.match(r"\t([a-z_0-9]+)\b(.*)", l)
    if not m or classify(m.group(1)) is None:
        continue
    r = region(cur) if cur else "(no line)"
    counts[r][classify(m.group(1))] += 1
    if m.group(1).startswith(("v_readlane", "v_writelane")) and any(re.search(r"\b" + v + r"\b", m.group(2)) for v in spill_regs):
        counts[r]["spill " + ("reload" if m.group(1).startswith("v_readlane") else "store")] += 1
for l in text[i0:]:
    m = re.match(r"; codeLenInByte = (\d+)", l)
    if m:
        code_bytes = int(m.group(1))
        break

# ---- the code object's metadata entry of the kernel ----
meta = {}
entry = {}
for l in text:
    if re.match(r"\s+- \.agpr_count:", l):
        entry = {}
    m = re.match(r"\s+(?:- )?\.([a-z_]+):\s+(\S+)\s*$", l)
    if m:
        entry[m.group(1)] = m.group(2)
        if m.group(1) == "wavefront_size" and entry.get("name") == args.kernel:
            meta = dict(entry)
res = {"kernel": args.kernel, "sgpr_count": int(meta["sgpr_count"]), "vgpr_count": int(meta["vgpr_count"]), "sgpr_spill_count": int(meta["sgpr_spill_count"]),
       "vgpr_spill_count": int(meta["vgpr_spill_count"]), "scratch_bytes": int(meta["private_segment_fixed_size"]), "code_bytes": code_bytes,
       "regions": {r: dict(c) for r, c in counts.items()}}
if args.json:
    print(json.dumps(res))
    sys.exit(0)
cols = CLASSES + ("spill reload", "spill store")
print(f"{args.kernel}: static instructions per region")
print(f"{'region':44s}" + "".join(f"{c:>13s}" for c in cols))
order = [s[1] for s in starts if s[1] in counts] + [r for r in counts if r not in {s[1] for s in starts}]
tot = collections.Counter()
for r in dict.fromkeys(order):
    print(f"{r:44s}" + "".join(f"{counts[r][c]:13d}" for c in cols))
    tot.update(counts[r])
print(f"{'total':44s}" + "".join(f"{tot[c]:13d}" for c in cols))
print(f"sgprs {res['sgpr_count']}  vgprs {res['vgpr_count']}  spilled sgprs {res['sgpr_spill_count']}  spilled vgprs {res['vgpr_spill_count']}  "
      f"scratch {res['scratch_bytes']} bytes  code {res['code_bytes']} bytes")
