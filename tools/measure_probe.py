#!/usr/bin/env python3
"""Per-shell measures (ft_shells_measure, ft_mesh_measure) against the labelling they follow and the host route they replace.  Appends one JSON line
per scene to --out (profiles/measure_probe.jsonl).

Scenes and lattices: tools/mesh_probe.py's (C3 256^3, console_scene 256^3, combinator_crowd 128^3, over +-1.25 boundary radii).

One process, the library's event pairs (ft_collect_stats' kernel_ms), the mean of REPS calls, ROUNDS rounds with the variants ALTERNATING within a
round, median and range reported.  The rule for reading them: two figures whose ranges overlap are not told apart.
  shells measure / mesh measure      the whole call, records to device memory (no copy, no synchronisation inside the figure)
  ... stage 1 / stage 2              the call cut short after the extent + box kernel / after the terms kernel (internal ft_ctx_measure_probe), so that
                                     extent + box = stage 1, terms = stage 2 - stage 1, finish = whole - stage 2 (memsets are not kernels: not counted)
  shells measure eager stage 2       the terms kernel flushing every lane's partial sums at every iteration: the form without the accumulation in
                                     registers (same bytes, checked here); eager terms = this - stage 1
  shells                             ft_mesh_shells on the same mesh: the labelling the measures follow — a yardstick
  wall host route                    ft_mesh_read + ft_shells_read to host arrays + the same five sums and the boxes in numpy float64 — WALL time,
                                     the route the device measures replace
  wall measure                       ft_shells_measure to host records — WALL time
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

ROUNDS, REPS, WALL_CALLS = 5, 10, 2
SCENES = (("C3 smooth256", lambda: syn.config3()[0], 256), ("console_scene 1000 tori", lambda: syn.console_scene()[0], 256),
          ("combinator_crowd", lambda: syn.combinator_crowd()[0], 128))
L = _lib.lib
L.ft_ctx_measure_probe.restype, L.ft_ctx_measure_probe.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.c_int32]      # internal: not in the header
RECORD = np.dtype(_lib.SHELL_MEASURE_DTYPE)


def lattice_of(ds, n):
    b = np.asarray(ds.boundary(), np.float32)
    origin = b[0:3] - np.float32(1.25) * b[3]
    step = np.float32(2.5) * b[3] / np.float32(n - 1)
    return tuple(float(v) for v in origin), (float(step),) * 3, (n, n, n)


def stat(v):
    return {"median_ms": round(statistics.median(v), 4), "range_ms": [round(min(v), 4), round(max(v), 4)], "runs_ms": [round(x, 4) for x in v]}


def host_sums(v, t, vl, tl, n_shells):
    """area, six volumes, moments and boxes per shell in plain numpy float64: what a caller would write after ft_mesh_read"""
    p = v.astype(np.float64)
    a, b, c = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
    n = np.cross(b - a, c - a)
    six = np.einsum("ij,ij->i", a, np.cross(b, c))
    out = [np.bincount(tl, 0.5 * np.sqrt((n * n).sum(axis=1)), n_shells), np.bincount(tl, six, n_shells)]
    out += [np.bincount(tl, six * (a[:, i] + b[:, i] + c[:, i]), n_shells) for i in range(3)]
    used = vl >= 0
    order = np.argsort(vl[used], kind="stable")
    starts = np.searchsorted(vl[used][order], np.arange(n_shells))
    pts = v[used][order]
    return out, np.minimum.reduceat(pts, starts, axis=0), np.maximum.reduceat(pts, starts, axis=0)


def probe_scene(dev, name, scene, n):
    ds = dev.scene(scene)
    origin, step, counts = lattice_of(ds, n)
    lat, _ = ft.api._lattice(origin, step, counts)
    dist = torch.empty(n ** 3, dtype=torch.float32, device="cuda")
    ds.sample_lattice_device(origin, step, counts, dist.data_ptr())
    torch.cuda.synchronize()
    mesh = C.c_void_p()
    _lib.check(L.ft_mesh_values_device(dev._ctx, C.byref(lat), C.c_void_p(dist.data_ptr()), 0.0, C.byref(mesh)))
    info = _lib.MeshInfo()
    _lib.check(L.ft_mesh_get_info(mesh, C.byref(info)))
    nv, nt = int(info.n_vertices), int(info.n_triangles)
    shells = C.c_void_p()
    _lib.check(L.ft_mesh_shells(mesh, C.byref(shells)))
    sh_info = _lib.ShellsInfo()
    _lib.check(L.ft_shells_get_info(shells, C.byref(sh_info)))
    S = int(sh_info.n_shells)
    d_records = torch.empty((max(S, 1), 18), dtype=torch.float32, device="cuda")
    out = C.c_void_p(d_records.data_ptr())

    def timed(call, reps, stop=0, eager=0):
        L.ft_ctx_measure_probe(dev._ctx, stop, eager)
        try:
            for _ in range(reps):
                call()
            return ds.collect_stats()["kernel_ms"] / reps
        finally:
            L.ft_ctx_measure_probe(dev._ctx, 0, 0)

    shells_measure = lambda: _lib.check(L.ft_shells_measure(mesh, shells, out))
    mesh_measure = lambda: _lib.check(L.ft_mesh_measure(mesh, out))

    def label():
        h = C.c_void_p()
        _lib.check(L.ft_mesh_shells(mesh, C.byref(h)))
        L.ft_shells_destroy(h)

    def records(eager):
        rec = np.zeros(S, RECORD)
        L.ft_ctx_measure_probe(dev._ctx, 0, eager)
        try:
            _lib.check(L.ft_shells_measure(mesh, shells, rec.ctypes.data_as(C.c_void_p)))
        finally:
            L.ft_ctx_measure_probe(dev._ctx, 0, 0)
        return rec

    def host_route():
        v, tr = np.empty((nv, 3), np.float32), np.empty((nt, 3), np.int32)
        vl, tl = np.empty(nv, np.int32), np.empty(nt, np.int32)
        _lib.check(L.ft_mesh_read(mesh, v.ctypes.data_as(C.c_void_p), tr.ctypes.data_as(C.c_void_p), None, None))
        _lib.check(L.ft_shells_read(shells, vl.ctypes.data_as(C.c_void_p), tl.ctypes.data_as(C.c_void_p), None))
        return host_sums(v, tr, vl, tl, S)

    rec = records(0)
    same_eager = rec.tobytes() == records(1).tobytes()
    sums, lo, hi = host_route()
    with np.errstate(all="ignore"):
        agreement = {"area_max_rel": float(np.max(np.abs(sums[0] - rec["area"]) / np.maximum(rec["area"], 1e-300))),
                     "volume_max_abs_over_area": float(np.max(np.abs(sums[1] / 6.0 - rec["volume"]) / np.maximum(rec["area"], 1e-300))),
                     "boxes_equal": bool(np.array_equal(lo, rec["bbox_min"]) and np.array_equal(hi, rec["bbox_max"]))}
    ds.collect_stats()
    names = ("shells measure", "shells measure stage 1", "shells measure stage 2", "shells measure eager stage 2", "mesh measure", "mesh measure stage 1",
             "mesh measure stage 2", "shells")
    figures = {k: [] for k in names}
    walls = {"wall host route": [], "wall measure": []}
    for _ in range(ROUNDS):
        figures["shells measure"].append(timed(shells_measure, REPS))
        figures["shells measure stage 1"].append(timed(shells_measure, REPS, 1))
        figures["shells measure stage 2"].append(timed(shells_measure, REPS, 2))
        figures["shells measure eager stage 2"].append(timed(shells_measure, REPS, 2, 1))
        figures["mesh measure"].append(timed(mesh_measure, REPS))
        figures["mesh measure stage 1"].append(timed(mesh_measure, REPS, 1))
        figures["mesh measure stage 2"].append(timed(mesh_measure, REPS, 2))
        figures["shells"].append(timed(label, REPS))
        for key, call in (("wall host route", host_route), ("wall measure", lambda: records(0))):
            t0 = time.perf_counter()
            for _ in range(WALL_CALLS):
                call()
            walls[key].append((time.perf_counter() - t0) * 1e3 / WALL_CALLS)
        ds.collect_stats()
    med = lambda k: statistics.median(figures[k])
    split = {}
    for what in ("shells measure", "mesh measure"):
        split[what] = {"extent_box": round(med(what + " stage 1"), 4), "terms": round(med(what + " stage 2") - med(what + " stage 1"), 4),
                       "finish": round(med(what) - med(what + " stage 2"), 4)}
    split["shells measure"]["terms_eager"] = round(med("shells measure eager stage 2") - med("shells measure stage 1"), 4)
    res = {"scene": name, "lattice": n, "fast_path": ds.info()["fast_path"], "vertices": nv, "triangles": nt,
           "shells": {k: int(getattr(sh_info, k)) for k, _ in sh_info._fields_}, "extent_exponent": int(rec["extent_exponent"][0]) if S else 0,
           "unmeasured": int(rec["n_unmeasured"].sum()), "rounds": ROUNDS, "launches_per_figure": REPS,
           "rule": "two figures whose ranges overlap are not told apart", "kernel_ms": {k: stat(v) for k, v in figures.items()},
           "split_ms_from_medians": split, "measure_over_shells": round(med("shells measure") / med("shells"), 4),
           "eager_gives_the_same_bytes": same_eager, "host_numpy_agreement": agreement, "wall_ms": {k: stat(v) for k, v in walls.items()}}
    L.ft_shells_destroy(shells)
    L.ft_mesh_destroy(mesh)
    ds.close()
    return res


ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "measure_probe.jsonl"))
ap.add_argument("--scale", type=int, default=1, help="divide every lattice edge by this (rehearsals)")
args = ap.parse_args()
if args.scale != 1:
    SCENES = tuple((name, make, max(2, n // args.scale)) for name, make, n in SCENES)
dev = ft.Device(0)
for name, make, n in SCENES:
    case = {"probe": "measure", "build": ft.build_info()["src"], "device": torch.cuda.get_device_name(0)}
    case.update(probe_scene(dev, name, make(), n))
    with open(args.out, "a") as f:
        f.write(json.dumps(case) + "\n")
    print(json.dumps(case), flush=True)
    torch.cuda.empty_cache()
dev.close()
