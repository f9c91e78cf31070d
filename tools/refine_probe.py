#!/usr/bin/env python3
"""Refinement (ft_mesh_lattice_refined, ft_slice_lattice_refined) against the unrefined constructors and against the only other route to a smaller
residual, a lattice with twice the points per axis.  Appends one JSON line per scene to --out (profiles/refine_probe.jsonl).

Scenes and lattices as tools/mesh_probe.py's (over +-1.25 boundary radii around the boundary centre):
  C3 (256 spheres)             lean     256^3
  console_scene (1000 tori)    carved   256^3
  combinator_crowd             general  128^3

One process, the library's event pairs (ft_collect_stats' kernel_ms: every launch of a call, the lattice's field evaluation included).  Per scene every
variant is timed ROUNDS times, the variants ALTERNATING within a round, median and range reported.  The rule for reading them: two figures whose
ranges overlap are not told apart.
  mesh                    ft_mesh_lattice
  mesh R                  ft_mesh_lattice_refined with R = 4, 8, 12
  mesh R no field         the same without its R field launches (internal ft_ctx_refine_probe; the positions are then not the rule's): the bracket and
                          round launches alone are this minus `mesh`, the field rounds are `mesh R` minus this
  slice, slice R, ...     the same for ft_slice_lattice(_refined), axis 2, on the same lattice (a 256^3 stack)
  mesh 2x                 ft_mesh_lattice on the lattice with twice the points per axis over the same box: the yardstick
and, from ft_sample_points_device at the vertices, max and median |D(v) - iso| of every mesh.
Not the contract bench (that is bench.py)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch                              # before the library: torch's HIP runtime is the one the process loads first

import fraytracer_amd as ft
from fraytracer_amd import _lib
from fraytracer_amd import synthetic as syn

ROUNDS, REPS = 5, 3
STEPS = (4, 8, 12)
ISO = 0.0
SCENES = (("C3 smooth256", lambda: syn.config3()[0], 256), ("console_scene 1000 tori", lambda: syn.console_scene()[0], 256),
          ("combinator_crowd", lambda: syn.combinator_crowd()[0], 128))
L = _lib.lib


def lattice_of(ds, n):
    b = np.asarray(ds.boundary(), np.float32)
    origin = b[0:3] - np.float32(1.25) * b[3]
    step = np.float32(2.5) * b[3] / np.float32(n - 1)
    return tuple(float(v) for v in origin), (float(step),) * 3, (n, n, n)


def stat(v):
    return {"median_ms": round(statistics.median(v), 4), "range_ms": [round(min(v), 4), round(max(v), 4)], "runs_ms": [round(x, 4) for x in v]}


def probe_scene(dev, name, scene, n, skip_field):
    ds = dev.scene(scene)
    like = torch.zeros(1, device="cuda")
    origin, step, counts = lattice_of(ds, n)
    lat, _ = ft.api._lattice(origin, step, counts)
    origin2, step2, counts2 = lattice_of(ds, 2 * n)
    lat2, _ = ft.api._lattice(origin2, step2, counts2)

    def mesh(R, lattice=lat):
        h = C.c_void_p()
        if R is None:
            _lib.check(L.ft_mesh_lattice(dev._ctx, ds._scene, C.byref(lattice), ISO, 0.0, 0, C.byref(h)))
        else:
            _lib.check(L.ft_mesh_lattice_refined(dev._ctx, ds._scene, C.byref(lattice), ISO, 0.0, 0, R, C.byref(h)))
        L.ft_mesh_destroy(h)

    def slices(R):
        h = C.c_void_p()
        if R is None:
            _lib.check(L.ft_slice_lattice(dev._ctx, ds._scene, C.byref(lat), 2, ISO, 0.0, 0, C.byref(h)))
        else:
            _lib.check(L.ft_slice_lattice_refined(dev._ctx, ds._scene, C.byref(lat), 2, ISO, 0.0, 0, R, C.byref(h)))
        L.ft_slices_destroy(h)

    def timed(call, reps, skip=0):
        skip_field(dev._ctx, skip)
        try:
            for _ in range(reps):
                call()
            return ds.collect_stats()["kernel_ms"] / reps
        finally:
            skip_field(dev._ctx, 0)

    def residual(m):
        if not len(m.vertices):
            return {"max": None, "median": None}
        d = (ds.sample_points(m.vertices).distance - ISO).abs()
        torch.cuda.synchronize()
        return {"max": float(d.max()), "median": float(d.median())}

    # sizes and residuals, once
    sizes, residuals = {}, {}
    for label, m in [("mesh", ds.mesh_lattice(origin, step, counts, iso=ISO, like=like))] + \
                    [(f"mesh {R}", ds.mesh_lattice(origin, step, counts, iso=ISO, like=like, refine=R)) for R in STEPS] + \
                    [("mesh 2x", ds.mesh_lattice(origin2, step2, counts2, iso=ISO, like=like))]:
        sizes[label] = {"vertices": len(m.vertices), "triangles": len(m.triangles)}
        residuals[label] = residual(m)
        del m
    contours = ds.slice_lattice(origin, step, counts, axis=2, iso=ISO, like=like)
    sizes["slice"] = {"points": len(contours.points), "polylines": len(contours.polylines)}
    del contours
    torch.cuda.empty_cache()
    ds.collect_stats()

    variants = [("mesh", lambda: mesh(None), 0), ("slice", lambda: slices(None), 0), ("mesh 2x", lambda: mesh(None, lat2), 0)]
    for R in STEPS:
        variants += [(f"mesh {R}", lambda R=R: mesh(R), 0), (f"mesh {R} no field", lambda R=R: mesh(R), 1),
                     (f"slice {R}", lambda R=R: slices(R), 0), (f"slice {R} no field", lambda R=R: slices(R), 1)]
    for _, call, skip in variants:                                     # warm every shape the timed window uses
        timed(call, 1, skip)
    figures = {label: [] for label, _, _ in variants}
    for _ in range(ROUNDS):
        for label, call, skip in variants:
            figures[label].append(timed(call, REPS, skip))
    med = {k: statistics.median(v) for k, v in figures.items()}
    split = {}
    for kind in ("mesh", "slice"):
        for R in STEPS:
            own, field = med[f"{kind} {R} no field"] - med[kind], med[f"{kind} {R}"] - med[f"{kind} {R} no field"]
            split[f"{kind} {R}"] = {"bracket_and_round_launches_ms": round(own, 4), "field_rounds_ms": round(field, 4),
                                    "share_outside_the_field_launches": round(own / (own + field), 4) if own + field > 0 else None}
    res = {"scene": name, "lattice": n, "points": n ** 3, "iso": ISO, "fast_path": ds.info()["fast_path"], "sizes": sizes, "residual_abs_D_minus_iso": residuals,
           "rounds": ROUNDS, "launches_per_figure": REPS, "rule": "two figures whose ranges overlap are not told apart",
           "kernel_ms": {k: stat(v) for k, v in figures.items()}, "refinement_split_of_medians": split}
    ds.close()
    return res


ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "refine_probe.jsonl"))
ap.add_argument("--scale", type=int, default=1, help="divide every lattice edge by this (rehearsals)")
args = ap.parse_args()
if args.scale != 1:
    SCENES = tuple((name, make, max(2, n // args.scale)) for name, make, n in SCENES)
dev = ft.Device(0)
skip_field = L.ft_ctx_refine_probe                                   # internal: not in the header
skip_field.restype, skip_field.argtypes = C.c_int, [C.c_void_p, C.c_int32]
for name, make, n in SCENES:
    case = {"probe": "refine", "build": ft.build_info()["src"], "device": torch.cuda.get_device_name(0)}
    case.update(probe_scene(dev, name, make(), n, skip_field))
    with open(args.out, "a") as f:
        f.write(json.dumps(case) + "\n")
    print(json.dumps(case), flush=True)
    torch.cuda.empty_cache()
dev.close()
