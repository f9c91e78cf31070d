#!/usr/bin/env python3
"""What the fixed part of a lean-kernel round costs, pass by pass, on the C3 frame (256 spheres, smooth union 0.25, 4096^2, 1 spp).

    round_fixed_probe.py run [--size 4096] [--tag T]        one line of JSON per launch: the launch's option column, kernel_ms, wave_evals, sdf_evals ...
    round_fixed_probe.py table LINES.jsonl PMC_DIR [...]    the same lines joined with the counters rocprofv3 --pmc wrote for the same launches

`run` renders the frame under the defaults and then with one option changed at a time through the existing words (cull, cert_policy, occl, escape,
tail_k).  Every column is launched twice — the first launch of a column records the tile order its second launch follows — and both are printed.
Under `rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_SMEM SQ_WAVE_CYCLES GRBM_GUI_ACTIVE -- python3 tools/round_fixed_probe.py run` (a run of its
own: no tracing beside the counters) the k-th ft_trace_kernel dispatch of the counter file is the k-th line printed, which is how `table` joins them.
Kernel times come from a run without the profiler.  Switching a pass off changes the rounds a frame takes, so `table` prices per evaluation round
(wave_evals), and beside the whole round it gives the round without its sphere loop: 25.5 VALU per child evaluated, children per round taken from
culled_fraction (the loop's own price: DESIGN.md section 5)."""
import argparse, csv, glob, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# a C3 4096^2 frame's tiles are narrower than the certificate's margin, so word 0 means "the bundle alone" there (include/fraytracer_hip.h, FT_OPT_CERT_POLICY):
# the columns spell the words out.  bits 0-7 / 8-15: 255 = no per-lane tries; bits 30-31: 0 the shipped bundle schedule, 3 the bundle off
BUNDLE_ONLY = 255 | 255 << 8 | 16 << 16 | 6 << 24
COLUMNS = [
    ("defaults", {}),
    ("cull=0", {"cull": 0}),
    ("cert_policy: bundle off", {"cert_policy": BUNDLE_ONLY | 3 << 30}),
    ("cert_policy: per-lane tries on", {"cert_policy": 0 | 6 << 8 | 16 << 16 | 6 << 24}),
    ("cert_policy: per-lane tries off (= word 0 here)", {"cert_policy": BUNDLE_ONLY}),
    ("occl=0", {"occl": 0}),
    ("escape=0", {"escape": 0}),
    ("tail_k=0", {"tail_k": 0}),
]
COUNTERS = ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_SMEM", "SQ_WAVE_CYCLES", "GRBM_GUI_ACTIVE")
LOOP_VALU_PER_CHILD = 25.5


def s32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


def run(args):
    import torch
    import fraytracer_amd as ft
    from fraytracer_amd import synthetic as syn
    dev = ft.Device(0)
    ds = dev.scene(syn.config3(n=args.spheres)[0])
    size = ft.ImageSize(args.size, args.size)
    cam = syn.default_camera()
    buf = torch.empty((args.size, args.size, 3), dtype=torch.float32, device="cuda")
    build = ft.build_info()["src"]
    for label, opts in COLUMNS:
        saved = {k: dev.get_option(k) for k in opts}
        for k, v in opts.items():
            dev.set_option(k, s32(v))
        for launch in range(2):
            ds.render_device(syn.EPSILON, syn.RAY_LENGTH, size, cam, buf.data_ptr())
            st = ds.collect_stats()
            print(json.dumps({"tag": args.tag, "build": build, "column": label, "launch": launch, "spheres": args.spheres, "size": args.size,
                              "kernel_ms": round(st["kernel_ms"], 3), "wave_evals": st["wave_evals"], "sdf_evals": st["sdf_evals"],
                              "rays": st["rays_primary"] + st["rays_shadow"], "culled_fraction": round(st["culled_fraction"], 4),
                              "tail_fraction": round(st["tail_fraction"], 4), "flags": st["flags"]}), flush=True)
        for k, v in saved.items():
            dev.set_option(k, v)
    dev.close()


def dispatches(pmc_dir):
    """-> [{counter: value}] of the ft_trace_kernel dispatches, in dispatch order"""
    acc = {}
    for f in glob.glob(os.path.join(pmc_dir, "**", "*counter_collection.csv"), recursive=True):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                if "ft_trace_kernel" in r.get("Kernel_Name", ""):
                    key = int(r.get("Dispatch_Id") or r.get("Correlation_Id"))
                    acc.setdefault(key, {}).setdefault(r["Counter_Name"], 0.0)
                    acc[key][r["Counter_Name"]] += float(r["Counter_Value"])
    return [acc[k] for k in sorted(acc)]


def table(args):
    for lines_file, pmc_dir in zip(args.pairs[0::2], args.pairs[1::2]):
        lines = [json.loads(l) for l in open(lines_file) if l.startswith("{")]
        disp = dispatches(pmc_dir)
        if len(disp) != len(lines):
            raise SystemExit(f"{pmc_dir}: {len(disp)} ft_trace_kernel dispatches for {len(lines)} lines of {lines_file}")
        print(f"# {lines[0]['tag']} (build {lines[0]['build']}): counters per launch and per evaluation round; second launch of every column")
        print(f"{'column':50s}{'wave_evals':>11s}{'sdf_evals':>11s}{'children':>9s}" + "".join(f"{c[3:] if c.startswith('SQ_') else c:>17s}" for c in COUNTERS)
              + f"{'VALU/round':>11s}{'less loop':>10s}{'SALU/round':>11s}{'SMEM/round':>11s}{'cyc/round':>10s}")
        base = None
        for ln, d in zip(lines, disp):
            if ln["launch"] != 1:
                continue
            rounds = ln["wave_evals"]
            kids = ln["spheres"] * (1.0 - ln["culled_fraction"])
            valu = d["SQ_INSTS_VALU"] / rounds
            fixed = valu - LOOP_VALU_PER_CHILD * kids
            row = (f"{ln['column']:50s}{rounds:11d}{ln['sdf_evals']:11d}{kids:9.1f}" + "".join(f"{d.get(c, float('nan')):17.0f}" for c in COUNTERS)
                   + f"{valu:11.1f}{fixed:10.1f}{d['SQ_INSTS_SALU'] / rounds:11.1f}{d['SQ_INSTS_SMEM'] / rounds:11.2f}{d['SQ_WAVE_CYCLES'] / rounds:10.1f}")
            if base is None:
                base = fixed
            else:
                row += f"   fixed part against the defaults {fixed - base:+.1f} VALU per round"
            print(row)


ap = argparse.ArgumentParser()
sub = ap.add_subparsers(dest="cmd", required=True)
r = sub.add_parser("run")
r.add_argument("--size", type=int, default=4096)
r.add_argument("--spheres", type=int, default=256)
r.add_argument("--tag", default="")
t = sub.add_parser("table")
t.add_argument("pairs", nargs="+")
args = ap.parse_args()
run(args) if args.cmd == "run" else table(args)
