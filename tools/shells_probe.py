#!/usr/bin/env python3
"""Shell labelling (ft_mesh_shells) and selection (ft_mesh_select) against the extraction they follow and the route they replace.  Appends one JSON
line per scene to --out (profiles/shells_probe.jsonl).

Scenes and lattices: tools/mesh_probe.py's (C3 256^3, console_scene 256^3, combinator_crowd 128^3, over +-1.25 boundary radii).

One process, the library's event pairs (ft_collect_stats' kernel_ms), the mean of REPS calls, ROUNDS rounds with the variants ALTERNATING within a
round, median and range reported.  The rule for reading them: two figures whose ranges overlap are not told apart.
  extract                 ft_mesh_values_device on the distances kept from ft_sample_lattice_device: the mesh the shells are of
  shells tile T           ft_mesh_shells on that mesh, whole, with T = 128, 256, 512, 1024 items per workgroup of the tiled kernels (internal
                          ft_ctx_shells_tile; every tile gives the same shells, checked here)
  stage 1 / 2 / 3         the labelling cut short after the incidence lists / the iterations / the vertex labels (internal ft_ctx_shells_probe), so
                          that per group: incidence = stage 1, iterate = stage 2 - stage 1, records = stage 3 - stage 2 (smallest members, numbering,
                          vertex labels and counts), border = whole - stage 3 (triangle labels and counts, border edges, totals)
  select largest          ft_mesh_select keeping the shell with the most triangles
  wall host route         ft_mesh_read to host arrays + the labelling on the host (scipy.sparse.csgraph.connected_components where present, else the
                          tests' restatement) — WALL time, the route the device labelling replaces
  wall shells             ft_mesh_shells + ft_shells_read to host arrays — WALL time
Not the contract bench (that is bench.py)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch                              # before the library: torch's HIP runtime is the one the process loads first

import fraytracer_amd as ft
from fraytracer_amd import _lib
from fraytracer_amd import synthetic as syn

try:
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
except ImportError:                       # the tests' restatement instead
    connected_components = None
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import shells_restatement

ROUNDS, REPS, WALL_CALLS = 5, 10, 2
TILES = (128, 256, 512, 1024)
SHIPPED_TILE = 512                        # ft_shells.h FT_SHELLS_TILE_DEFAULT
SCENES = (("C3 smooth256", lambda: syn.config3()[0], 256), ("console_scene 1000 tori", lambda: syn.console_scene()[0], 256),
          ("combinator_crowd", lambda: syn.combinator_crowd()[0], 128))
L = _lib.lib
for fn, args_ in ((L.ft_ctx_shells_tile, [C.c_void_p, C.c_int32]), (L.ft_ctx_shells_probe, [C.c_void_p, C.c_int32]), (L.ft_ctx_shells_last, [C.c_void_p, C.POINTER(C.c_int64)])):
    fn.restype, fn.argtypes = C.c_int, args_           # internal: not in the header


def lattice_of(ds, n):
    b = np.asarray(ds.boundary(), np.float32)
    origin = b[0:3] - np.float32(1.25) * b[3]
    step = np.float32(2.5) * b[3] / np.float32(n - 1)
    return tuple(float(v) for v in origin), (float(step),) * 3, (n, n, n)


def stat(v):
    return {"median_ms": round(statistics.median(v), 4), "range_ms": [round(min(v), 4), round(max(v), 4)], "runs_ms": [round(x, 4) for x in v]}


def host_labels(triangles, n_vertices):
    if connected_components is None:
        return shells_restatement.shells(triangles, n_vertices).info["n_shells"]
    t = triangles.astype(np.int64)
    rows, cols = np.concatenate([t[:, 0], t[:, 1]]), np.concatenate([t[:, 1], t[:, 2]])
    n, _ = connected_components(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n_vertices, n_vertices)), directed=False)
    return n - (n_vertices - len(np.unique(t)))                        # unused vertices are components of their own there


def probe_scene(dev, name, scene, n):
    ds = dev.scene(scene)
    origin, step, counts = lattice_of(ds, n)
    lat, _ = ft.api._lattice(origin, step, counts)
    dist = torch.empty(n ** 3, dtype=torch.float32, device="cuda")
    ds.sample_lattice_device(origin, step, counts, dist.data_ptr())
    torch.cuda.synchronize()

    def extract():
        h = C.c_void_p()
        _lib.check(L.ft_mesh_values_device(dev._ctx, C.byref(lat), C.c_void_p(dist.data_ptr()), 0.0, C.byref(h)))
        return h

    mesh = extract()                                                   # kept: every labelling below is of this mesh
    info = _lib.MeshInfo()
    _lib.check(L.ft_mesh_get_info(mesh, C.byref(info)))
    nv, nt = int(info.n_vertices), int(info.n_triangles)

    def shells():
        h = C.c_void_p()
        _lib.check(L.ft_mesh_shells(mesh, C.byref(h)))
        return h

    def read(h):
        i = _lib.ShellsInfo()
        _lib.check(L.ft_shells_get_info(h, C.byref(i)))
        parts = np.empty(nv, np.int32), np.empty(nt, np.int32), np.empty((int(i.n_shells), 4), np.int32)
        _lib.check(L.ft_shells_read(h, *[p.ctypes.data_as(C.c_void_p) for p in parts]))
        return parts

    def timed(launch, destroy, reps, tile=SHIPPED_TILE, stop=0):
        L.ft_ctx_shells_tile(dev._ctx, tile)
        L.ft_ctx_shells_probe(dev._ctx, stop)
        try:
            for _ in range(reps):
                destroy(launch())
            return ds.collect_stats()["kernel_ms"] / reps
        finally:
            L.ft_ctx_shells_tile(dev._ctx, SHIPPED_TILE)
            L.ft_ctx_shells_probe(dev._ctx, 0)

    whole = shells()
    labels = read(whole)
    last = (C.c_int64 * 2)()
    L.ft_ctx_shells_last(dev._ctx, last)
    records = labels[2]
    keep = np.zeros(len(records), np.uint8)
    if len(records):
        keep[min(range(len(records)), key=lambda s: (-int(records[s, 2]), s))] = 1

    def select():
        h = C.c_void_p()
        _lib.check(L.ft_mesh_select(mesh, whole, keep.ctypes.data_as(C.c_void_p), len(keep), C.byref(h)))
        return h

    same = {}
    for t in TILES:
        L.ft_ctx_shells_tile(dev._ctx, t)
        try:
            h = shells()
            same[t] = all(bool(np.array_equal(a, b)) for a, b in zip(read(h), labels))
            L.ft_shells_destroy(h)
        finally:
            L.ft_ctx_shells_tile(dev._ctx, SHIPPED_TILE)

    def host_route():
        v, tr = np.empty((nv, 3), np.float32), np.empty((nt, 3), np.int32)
        _lib.check(L.ft_mesh_read(mesh, v.ctypes.data_as(C.c_void_p), tr.ctypes.data_as(C.c_void_p), None, None))
        return host_labels(tr, nv)

    def device_route():
        h = shells()
        read(h)
        L.ft_shells_destroy(h)

    host_shells = host_route()
    ds.collect_stats()
    figures = {"extract": [], "select largest": []}
    figures.update({f"shells tile {t}": [] for t in TILES})
    figures.update({f"stage {s}": [] for s in (1, 2, 3)})
    walls = {"wall host route": [], "wall shells": []}
    for _ in range(ROUNDS):
        figures["extract"].append(timed(extract, L.ft_mesh_destroy, REPS))
        for t in TILES:
            figures[f"shells tile {t}"].append(timed(shells, L.ft_shells_destroy, REPS, t))
        for s in (1, 2, 3):
            figures[f"stage {s}"].append(timed(shells, L.ft_shells_destroy, REPS, SHIPPED_TILE, s))
        figures["select largest"].append(timed(select, L.ft_mesh_destroy, REPS))
        for label, call in (("wall host route", host_route), ("wall shells", device_route)):
            t0 = time.perf_counter()
            for _ in range(WALL_CALLS):
                call()
            walls[label].append((time.perf_counter() - t0) * 1e3 / WALL_CALLS)
        ds.collect_stats()
    med = lambda k: statistics.median(figures[k])
    whole_ms = med(f"shells tile {SHIPPED_TILE}")
    groups = {"incidence": med("stage 1"), "iterate": med("stage 2") - med("stage 1"), "records": med("stage 3") - med("stage 2"), "border": whole_ms - med("stage 3")}
    sh_info = _lib.ShellsInfo()
    _lib.check(L.ft_shells_get_info(whole, C.byref(sh_info)))
    res = {"scene": name, "lattice": n, "fast_path": ds.info()["fast_path"], "vertices": nv, "triangles": nt,
           "shells": {k: int(getattr(sh_info, k)) for k, _ in sh_info._fields_}, "largest_shell_triangles": int(records[:, 2].max()) if len(records) else 0,
           "host_route": "scipy connected_components" if connected_components is not None else "the tests' restatement", "host_route_shells": int(host_shells),
           "iterations": int(last[0]), "synchronisations": int(last[1]), "rounds": ROUNDS, "launches_per_figure": REPS,
           "rule": "two figures whose ranges overlap are not told apart", "kernel_ms": {k: stat(v) for k, v in figures.items()},
           "group_ms_from_medians": {k: round(v, 4) for k, v in groups.items()}, "shells_over_extract": round(whole_ms / med("extract"), 3),
           "same_shells_as_shipped_tile": same, "wall_ms": {k: stat(v) for k, v in walls.items()}}
    L.ft_shells_destroy(whole)
    L.ft_mesh_destroy(mesh)
    ds.close()
    return res


ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shells_probe.jsonl"))
ap.add_argument("--scale", type=int, default=1, help="divide every lattice edge by this (rehearsals)")
args = ap.parse_args()
if args.scale != 1:
    SCENES = tuple((name, make, max(2, n // args.scale)) for name, make, n in SCENES)
dev = ft.Device(0)
for name, make, n in SCENES:
    case = {"probe": "shells", "build": ft.build_info()["src"], "device": torch.cuda.get_device_name(0)}
    case.update(probe_scene(dev, name, make(), n))
    with open(args.out, "a") as f:
        f.write(json.dumps(case) + "\n")
    print(json.dumps(case), flush=True)
    torch.cuda.empty_cache()
dev.close()
