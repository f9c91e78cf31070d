#!/usr/bin/env python3
"""Slicing (ft_slice_lattice, ft_slice_values_device) stage by stage, against the field evaluation it follows, the mesher's extraction of the same
lattice and the route it replaces.  Appends one JSON line per case to --out (profiles/slice_probe.jsonl).

Cases (lattices over +-1.25 boundary radii around the boundary centre):
  C3 (256 spheres), console_scene (1000 tori), combinator_crowd: a stack of 256 slices of 256^2 for each axis, and one single slice of 4096^2
  through the boundary centre (axis 2).

One process, the library's event pairs (ft_collect_stats' kernel_ms).  Per case every variant is timed ROUNDS times, the variants ALTERNATING within
a round, median and range reported.  The rule for reading them: two figures whose ranges overlap are not told apart.
  field                   ft_sample_lattice_device, distance only: the evaluation the extraction follows
  slice to link           ft_slice_values_device on the distances kept from it, ended after count + scan + emit + link (internal ft_ctx_slice_probe)
  slice to jumps          the same, ended after the 2 R jump rounds (lead + R, cut + R)
  slice whole             the same, whole: + tail, heads, scan, records, scatter (the lay-out)
  mesh extract            ft_mesh_values_device on the same distances: the mesher's count + scan + emit (3D lattices only)
The stages are differences of medians: jumps = "to jumps" - "to link", lay-out = "whole" - "to jumps".
  wall slice_lattice      DeviceScene.slice_lattice to host arrays: field + extraction + the contours' download — WALL time per call
  wall sample_lattice     DeviceScene.sample_lattice to a host array: the route it replaces (its chaining on the host is not timed) — WALL time
Not the contract bench (that is bench.py)."""
import argparse
import ctypes as C
import json
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

ROUNDS, REPS, WALL_CALLS = 5, 5, 2
SCENES = (("C3 smooth256", lambda: syn.config3()[0]), ("console_scene 1000 tori", lambda: syn.console_scene()[0]), ("combinator_crowd", lambda: syn.combinator_crowd()[0]))
L = _lib.lib
probe = L.ft_ctx_slice_probe                                         # internal: not in the header
probe.restype, probe.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]


def lattice_of(ds, counts):
    """counts over +-1.25 boundary radii; an axis with one point lies at the boundary's centre"""
    b = np.asarray(ds.boundary(), np.float32)
    origin = [float(b[a] - np.float32(1.25) * b[3]) if counts[a] > 1 else float(b[a]) for a in range(3)]
    step = [float(np.float32(2.5) * b[3] / np.float32(counts[a] - 1)) if counts[a] > 1 else 0.0 for a in range(3)]
    return tuple(origin), tuple(step), tuple(counts)


def stat(v):
    return {"median_ms": round(statistics.median(v), 4), "range_ms": [round(min(v), 4), round(max(v), 4)], "runs_ms": [round(x, 4) for x in v]}


def probe_case(dev, ds, name, counts, axis):
    origin, step, counts = lattice_of(ds, counts)
    lat, _ = ft.api._lattice(origin, step, counts)
    dist = torch.empty(int(np.prod(counts)), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def field():
        ds.sample_lattice_device(origin, step, counts, dist.data_ptr())

    def slices():
        h = C.c_void_p()
        _lib.check(L.ft_slice_values_device(dev._ctx, C.byref(lat), C.c_void_p(dist.data_ptr()), axis, 0.0, C.byref(h)))
        L.ft_slices_destroy(h)

    def mesh():
        h = C.c_void_p()
        _lib.check(L.ft_mesh_values_device(dev._ctx, C.byref(lat), C.c_void_p(dist.data_ptr()), 0.0, C.byref(h)))
        L.ft_mesh_destroy(h)

    def timed(launch, stop=0):
        _lib.check(probe(dev._ctx, stop, None))
        try:
            for _ in range(REPS):
                launch()
            return ds.collect_stats()["kernel_ms"] / REPS
        finally:
            _lib.check(probe(dev._ctx, 0, None))

    field()
    whole = ds.slice_lattice(origin, step, counts, axis=axis)           # to host: the totals of the case
    last = (C.c_int64 * 2)()
    _lib.check(probe(dev._ctx, 0, last))
    ds.collect_stats()
    variants = [("field", field, 0), ("slice to link", slices, 1), ("slice to jumps", slices, 2), ("slice whole", slices, 0)]
    if min(counts) > 1:
        variants.append(("mesh extract", mesh, 0))
    figures = {label: [] for label, _, _ in variants}
    walls = {"wall slice_lattice": [], "wall sample_lattice": []}
    for _ in range(ROUNDS):
        for label, launch, stop in variants:
            figures[label].append(timed(launch, stop))
        for label, call in (("wall slice_lattice", lambda: ds.slice_lattice(origin, step, counts, axis=axis)), ("wall sample_lattice", lambda: ds.sample_lattice(origin, step, counts))):
            t0 = time.perf_counter()
            for _ in range(WALL_CALLS):
                call()
            walls[label].append((time.perf_counter() - t0) * 1e3 / WALL_CALLS)
        ds.collect_stats()
    med = {k: statistics.median(v) for k, v in figures.items()}
    stages = {"count + scan + emit + link": round(med["slice to link"], 4), "jump rounds": round(med["slice to jumps"] - med["slice to link"], 4),
              "lay-out": round(med["slice whole"] - med["slice to jumps"], 4)}
    return {"scene": name, "counts": list(counts), "axis": axis, "points": int(np.prod(counts)), "fast_path": ds.info()["fast_path"], "vertices": int(last[0]),
            "jump_rounds_R": int(last[1]), "contour_points": len(whole.points), "polylines": len(whole.polylines), "closed": whole.closed, "skipped": whole.skipped,
            "rounds": ROUNDS, "launches_per_figure": REPS, "rule": "two figures whose ranges overlap are not told apart",
            "kernel_ms": {k: stat(v) for k, v in figures.items()}, "stage_ms_from_medians": stages, "wall_ms": {k: stat(v) for k, v in walls.items()}}


ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "slice_probe.jsonl"))
ap.add_argument("--scale", type=int, default=1, help="divide every lattice edge by this (rehearsals)")
args = ap.parse_args()
n, big = max(2, 256 // args.scale), max(2, 4096 // args.scale)
dev = ft.Device(0)
for name, make in SCENES:
    ds = dev.scene(make())
    for counts, axis in (((n, n, n), 0), ((n, n, n), 1), ((n, n, n), 2), ((big, big, 1), 2)):
        case = {"probe": "slice", "build": ft.build_info()["src"], "device": torch.cuda.get_device_name(0)}
        case.update(probe_case(dev, ds, name, counts, axis))
        with open(args.out, "a") as f:
            f.write(json.dumps(case) + "\n")
        print(json.dumps(case), flush=True)
        torch.cuda.empty_cache()
    ds.close()
dev.close()
