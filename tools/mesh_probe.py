#!/usr/bin/env python3
"""Meshing (ft_mesh_lattice, ft_mesh_values_device) against the field evaluation it follows and the route it replaces.  Appends one JSON line per
scene to --out (profiles/mesh_probe.jsonl).

Scenes and lattices (over +-1.25 boundary radii around the boundary centre, so that the whole surface lies inside):
  C3 (256 spheres)             lean     256^3
  console_scene (1000 tori)    carved   256^3
  combinator_crowd             general  128^3

One process, the library's event pairs (ft_collect_stats' kernel_ms).  Per scene every variant is timed ROUNDS times, the variants ALTERNATING
within a round, median and range reported.  The rule for reading them: two figures whose ranges overlap are not told apart.
  field                   ft_sample_lattice_device, distance only: the evaluation the extraction follows
  extract tile T          ft_mesh_values_device on the distances kept from it: count + scan + emit vertices + emit triangles, with T = 128, 256,
                          512, 1024 lattice points per workgroup (internal ft_ctx_mesh_tile; every tile gives the same mesh, checked here)
  wall mesh_lattice       DeviceScene.mesh_lattice to host arrays: field + extraction + the mesh's download — WALL time per call
  wall sample_lattice     DeviceScene.sample_lattice to a host array: the route it replaces (its extraction on the host is not timed) — WALL time
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

ROUNDS, REPS, WALL_CALLS = 5, 10, 2
TILES = (128, 256, 512, 1024)
SHIPPED_TILE = 512                        # ft_mesh.h FT_MESH_TILE_DEFAULT
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


def probe_scene(dev, name, scene, n, set_tile):
    ds = dev.scene(scene)
    origin, step, counts = lattice_of(ds, n)
    lat, _ = ft.api._lattice(origin, step, counts)
    dist = torch.empty(n ** 3, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def field():
        ds.sample_lattice_device(origin, step, counts, dist.data_ptr())

    def extract():
        h = C.c_void_p()
        _lib.check(L.ft_mesh_values_device(dev._ctx, C.byref(lat), C.c_void_p(dist.data_ptr()), 0.0, C.byref(h)))
        return h

    def info_of(h):
        info = _lib.MeshInfo()
        _lib.check(L.ft_mesh_get_info(h, C.byref(info)))
        return info

    def timed(launch, reps, tile=SHIPPED_TILE):
        set_tile(dev._ctx, tile)
        try:
            for _ in range(reps):
                h = launch()
                if h is not None:
                    L.ft_mesh_destroy(h)
            return ds.collect_stats()["kernel_ms"] / reps
        finally:
            set_tile(dev._ctx, SHIPPED_TILE)

    field()
    ds.collect_stats()
    whole = ds.mesh_lattice(origin, step, counts)                      # the shipped tile, to host: what every tile must give
    same = {}
    for t in TILES:
        set_tile(dev._ctx, t)
        try:
            h = extract()
            i = info_of(h)
            v, tr = np.empty((i.n_vertices, 3), np.float32), np.empty((i.n_triangles, 3), np.int32)
            _lib.check(L.ft_mesh_read(h, v.ctypes.data_as(C.c_void_p), tr.ctypes.data_as(C.c_void_p), None, None))
            L.ft_mesh_destroy(h)
            same[t] = bool(np.array_equal(v.view(np.uint32), whole.vertices.view(np.uint32)) and np.array_equal(tr, whole.triangles))
        finally:
            set_tile(dev._ctx, SHIPPED_TILE)
    ds.collect_stats()
    figures = {"field": []}
    figures.update({f"extract tile {t}": [] for t in TILES})
    walls = {"wall mesh_lattice": [], "wall sample_lattice": []}
    for _ in range(ROUNDS):
        figures["field"].append(timed(field, REPS))
        for t in TILES:
            figures[f"extract tile {t}"].append(timed(extract, REPS, t))
        for label, call in (("wall mesh_lattice", lambda: ds.mesh_lattice(origin, step, counts)), ("wall sample_lattice", lambda: ds.sample_lattice(origin, step, counts))):
            t0 = time.perf_counter()
            for _ in range(WALL_CALLS):
                call()
            walls[label].append((time.perf_counter() - t0) * 1e3 / WALL_CALLS)
        ds.collect_stats()
    res = {"scene": name, "lattice": n, "points": n ** 3, "fast_path": ds.info()["fast_path"], "vertices": len(whole.vertices), "triangles": len(whole.triangles),
           "skipped": whole.skipped, "rounds": ROUNDS, "launches_per_figure": REPS, "rule": "two figures whose ranges overlap are not told apart",
           "kernel_ms": {k: stat(v) for k, v in figures.items()}, "same_mesh_as_shipped_tile": same, "wall_ms": {k: stat(v) for k, v in walls.items()}}
    ds.close()
    return res


ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mesh_probe.jsonl"))
ap.add_argument("--scale", type=int, default=1, help="divide every lattice edge by this (rehearsals)")
args = ap.parse_args()
if args.scale != 1:
    SCENES = tuple((name, make, max(2, n // args.scale)) for name, make, n in SCENES)
dev = ft.Device(0)
set_tile = L.ft_ctx_mesh_tile                                        # internal: not in the header
set_tile.restype, set_tile.argtypes = C.c_int, [C.c_void_p, C.c_int32]
for name, make, n in SCENES:
    case = {"probe": "mesh", "build": ft.build_info()["src"], "device": torch.cuda.get_device_name(0)}
    case.update(probe_scene(dev, name, make(), n, set_tile))
    with open(args.out, "a") as f:
        f.write(json.dumps(case) + "\n")
    print(json.dumps(case), flush=True)
    torch.cuda.empty_cache()
dev.close()
