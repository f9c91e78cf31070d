#!/usr/bin/env python3
"""Field sampling (ft_sample_lattice_device, ft_sample_points_device) against the route it replaces.  Appends one JSON line per scene to --out
(profiles/field_probe.jsonl).

Scenes and lattices (over +-0.6 boundary radii around the boundary centre):
  C3 (256 spheres)             lean     256^3
  console_scene (1000 tori)    carved   256^3
  combinator_crowd             general  128^3

Per scene, every variant below is timed ROUNDS times, the variants ALTERNATING within a round, so that the spread of one variant is known before
a difference between two is believed.  One figure is the mean kernel time of enough back-to-back launches to fill WINDOW seconds, from the device
events the library records around each launch on the context's stream (ft_collect_stats' kernel_ms).
  distance / all          distance only; distance + normal + material (four evaluation rounds per point)
  cull 0 / 1              FT_OPT_CULL
  brick 0 / 1 / 2         4x4x4, 2x4x8, 2x2x16 lattice points per wave (internal ft_ctx_field_brick); the rows without a shape in their name ran 2x4x8
  points                  ft_sample_points_device on the same points uploaded as a buffer
  eval_distance           the parent's route: ft_eval_distance (host form: upload, ft_eval_points_kernel, download) — WALL time per call

--eval-only runs nothing but ft_eval_distance, EVAL_CALLS times per scene: the run to put under `rocprofv3 --kernel-trace --stats`, whose
kernel trace --rocprof-csv then turns into per-scene ft_eval_points_kernel times (dispatches in scene order).
Not the contract bench (that is bench.py)."""
import argparse
import ctypes as C
import csv
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch                              # before the library: torch's HIP runtime is the one the process loads first

import fraytracer_amd as ft
from fraytracer_amd import _lib
from fraytracer_amd import synthetic as syn

ROUNDS, WINDOW, EVAL_CALLS = 5, 0.3, 3
NORMAL_EPS = 0.00125
BRICKS = {0: "4x4x4", 1: "2x4x8", 2: "2x2x16"}
SCENES = (("C3 smooth256", lambda: syn.config3()[0], 256), ("console_scene 1000 tori", lambda: syn.console_scene()[0], 256),
          ("combinator_crowd", lambda: syn.combinator_crowd()[0], 128))


def lattice_of(ds, n):
    b = np.asarray(ds.boundary(), np.float32)
    origin = b[0:3] - np.float32(0.6) * b[3]
    step = np.float32(1.2) * b[3] / np.float32(n - 1)
    return tuple(float(v) for v in origin), (float(step),) * 3, (n, n, n)


def stat(v):
    return {"median_ms": round(statistics.median(v), 4), "range_ms": [round(min(v), 4), round(max(v), 4)], "runs_ms": [round(x, 4) for x in v]}


def eval_only(dev):
    for name, make, n in SCENES:
        ds = dev.scene(make())
        pts = ft.lattice_points(*lattice_of(ds, n)).reshape(-1, 3)
        for _ in range(EVAL_CALLS):
            ds.eval_distance(pts)
        ds.close()


def rocprof_times(path):
    """per scene, the ft_eval_points_kernel durations (ms) of an --eval-only run's kernel trace"""
    rows = list(csv.DictReader(open(path)))
    col = {k.lower(): k for k in rows[0]}
    name, t0, t1 = col["kernel_name"], col["start_timestamp"], col["end_timestamp"]
    runs = sorted((int(r[t0]), (int(r[t1]) - int(r[t0])) / 1e6) for r in rows if r[name].startswith("ft_eval_points_kernel"))
    assert len(runs) == EVAL_CALLS * len(SCENES), len(runs)
    return {SCENES[i][0]: [round(ms, 4) for _, ms in runs[EVAL_CALLS * i:EVAL_CALLS * (i + 1)]] for i in range(len(SCENES))}


def probe_scene(dev, torch, name, scene, n, brick):
    ds = dev.scene(scene)
    origin, step, counts = lattice_of(ds, n)
    total = n ** 3
    pts = ft.lattice_points(origin, step, counts).reshape(-1, 3)
    dpts = torch.from_numpy(pts).cuda()
    dist = torch.empty(total, dtype=torch.float32, device="cuda")
    nrm = torch.empty((total, 3), dtype=torch.float32, device="cuda")
    mat = torch.empty(total, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    want = torch.from_numpy(ds.eval_distance(pts)[0]).cuda()

    def lattice(all_outputs):
        if all_outputs:
            return lambda: ds.sample_lattice_device(origin, step, counts, dist.data_ptr(), nrm.data_ptr(), mat.data_ptr(), normal_epsilon=NORMAL_EPS)
        return lambda: ds.sample_lattice_device(origin, step, counts, dist.data_ptr())

    variants = []                     # (label, options to set, brick, launch)
    for what in ("distance", "all"):
        variants.append((what, {}, 1, lattice(what == "all")))
        variants.append((what + " cull=0", {"cull": 0}, 1, lattice(what == "all")))
        for b in (0, 2):
            variants.append((f"{what} brick {BRICKS[b]}", {}, b, lattice(what == "all")))
    variants.append(("points distance", {}, 1, lambda: ds.sample_points_device(dpts.data_ptr(), total, dist.data_ptr())))
    variants.append(("points all", {}, 1, lambda: ds.sample_points_device(dpts.data_ptr(), total, dist.data_ptr(), nrm.data_ptr(), mat.data_ptr(), normal_epsilon=NORMAL_EPS)))

    def run(v, reps):
        label, opts, b, launch = v
        for k, val in opts.items():
            dev.set_option(k, val)
        brick(dev._ctx, b)
        try:
            for _ in range(reps):
                launch()
            return ds.collect_stats()["kernel_ms"] / reps
        finally:
            for k in opts:
                dev.set_option(k, 1)
            brick(dev._ctx, -1)                   # the shipped rule

    res = {"scene": name, "lattice": n, "points": total, "fast_path": ds.info()["fast_path"], "window_s": WINDOW, "rounds": ROUNDS, "variants": {}}
    reps, same = {}, {}
    for v in variants:                # warm-up, the repetitions that fill the window, and the bits
        dist.fill_(float("nan")); torch.cuda.synchronize()
        one = run(v, 1)
        same[v[0]] = bool(torch.equal(dist.view(torch.int32), want.view(torch.int32)))
        reps[v[0]] = max(1, math.ceil(WINDOW * 1e3 / max(one, 1e-3)))
    figures = {v[0]: [] for v in variants}
    walls = []
    for _ in range(ROUNDS):
        for v in variants:
            figures[v[0]].append(run(v, reps[v[0]]))
        t0 = time.perf_counter()
        ds.eval_distance(pts)
        walls.append((time.perf_counter() - t0) * 1e3)
    for v in variants:
        res["variants"][v[0]] = dict(stat(figures[v[0]]), launches_per_figure=reps[v[0]], same_distance_bits_as_eval_distance=same[v[0]])
    res["eval_distance_wall"] = stat(walls)
    ds.close()
    return res


ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "field_probe.jsonl"))
ap.add_argument("--eval-only", action="store_true")
ap.add_argument("--rocprof-csv", help="kernel trace of an --eval-only run under rocprofv3: append its ft_eval_points_kernel times to --out")
ap.add_argument("--scale", type=int, default=1, help="divide every lattice edge by this (rehearsals)")
args = ap.parse_args()
if args.scale != 1:
    SCENES = tuple((name, make, max(2, n // args.scale)) for name, make, n in SCENES)
if args.rocprof_csv:
    with open(args.out, "a") as f:
        f.write(json.dumps({"probe": "field", "ft_eval_points_kernel_ms_under_rocprofv3": rocprof_times(args.rocprof_csv), "calls": EVAL_CALLS}) + "\n")
    sys.exit(0)
dev = ft.Device(0)
if args.eval_only:
    eval_only(dev)
    dev.close()
    sys.exit(0)
brick = _lib.lib.ft_ctx_field_brick                                  # internal: not in the header
brick.restype, brick.argtypes = C.c_int, [C.c_void_p, C.c_int32]
for name, make, n in SCENES:
    case = {"probe": "field", "build": ft.build_info()["src"], "device": torch.cuda.get_device_name(0)}
    case.update(probe_scene(dev, torch, name, make(), n, brick))
    with open(args.out, "a") as f:
        f.write(json.dumps(case) + "\n")
    print(json.dumps(case), flush=True)
    torch.cuda.empty_cache()
dev.close()
