#!/usr/bin/env python3
"""Contour measures (ft_slices_measure) against the slice that produced the contours and the host route they replace.  Appends one JSON line per
lattice to --out (profiles/contour_measure_probe.jsonl).

Scene: the console scene (examples/slice.py's defaults: 1000 tori, 256 x 256 points x 64 layers, axis 2, +-1.05 boundary radii), and the same at
1024 x 1024 points x 256 layers.

One process, the library's event pairs (ft_collect_stats' kernel_ms), the mean of REPS calls, ROUNDS rounds with the variants ALTERNATING within a
round, median and range reported.  The rule for reading them: two figures whose ranges overlap are not told apart.
  slice            ft_slice_lattice of the scene: the call whose contours are measured — a yardstick (one call per round)
  measure          ft_slices_measure, both record arrays to device memory (no copy, no synchronisation inside the figure)
  measure eager    the same with the terms kernel adding every lane's terms by itself (internal ft_ctx_contour_measure_probe): the form without the
                   segmented reduction across the wave (same bytes, checked here)
  wall measure     ft_slices_measure to host records — WALL time
  wall host route  ft_slices_read of points and polylines to host arrays + a numpy float64 shoelace per polyline (np.add.reduceat) — WALL time, the
                   route the device measures replace; its sums depend on their order and are not the rule's
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
LATTICES = ((256, 64), (1024, 256))
L = _lib.lib
L.ft_ctx_contour_measure_probe.restype, L.ft_ctx_contour_measure_probe.argtypes = C.c_int, [C.c_void_p, C.c_int32]      # internal: not in the header


def stat(v):
    return {"median_ms": round(statistics.median(v), 4), "range_ms": [round(min(v), 4), round(max(v), 4)], "runs_ms": [round(x, 4) for x in v]}


def host_route(handle, n_points, n_polylines, axis):
    """ft_slices_read + per polyline length, shoelace area and moments in plain numpy float64: what a caller would write today"""
    p, rec = np.empty((n_points, 3), np.float32), np.empty((n_polylines, 4), np.int32)
    _lib.check(L.ft_slices_read(handle, p.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p), None, None))
    u, v = p[:, (axis + 1) % 3].astype(np.float64), p[:, (axis + 2) % 3].astype(np.float64)
    nxt = np.arange(1, n_points + 1)
    last = rec[:, 0] + rec[:, 1] - 1
    nxt[last] = rec[:, 0]                                              # the closing segment (an open polyline's is dropped below)
    own = np.ones(n_points, bool)
    own[last[rec[:, 3] == 0]] = False
    qu, qv = u[nxt], v[nxt]
    cross = np.where(own, u * qv - qu * v, 0.0)
    length = np.where(own, np.sqrt((qu - u) ** 2 + (qv - v) ** 2), 0.0)
    first = rec[:, 0]
    return (np.add.reduceat(length, first), np.add.reduceat(cross, first) / 2.0, np.add.reduceat(cross * (u + qu), first) / 6.0,
            np.add.reduceat(cross * (v + qv), first) / 6.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contour_measure_probe.jsonl"))
    args = ap.parse_args()
    dev = ft.Device(0)
    ctx = dev._ctx
    ds = dev.scene(syn.console_scene(seed=19, n=1000)[0])
    cx, cy, cz, radius = ds.boundary()
    axis, half = 2, 1.05 * radius
    for points, layers in LATTICES:
        counts = [points, points, layers]
        step = [2.0 * half / (n - 1) for n in counts]
        origin = [c - half for c in (cx, cy, cz)]
        lat, _ = ft.api._lattice(origin, step, counts)

        def slice_once():
            h = C.c_void_p()
            _lib.check(L.ft_slice_lattice(ctx, ds._scene, C.byref(lat), axis, 0.0, 0.0, 0, C.byref(h)))
            return h

        def kernel_ms(call, reps):
            ds.collect_stats()                                         # drop what earlier calls left
            for _ in range(reps):
                call()
            return ds.collect_stats()["kernel_ms"] / reps

        handle = slice_once()
        info = _lib.SlicesInfo()
        _lib.check(L.ft_slices_get_info(handle, C.byref(info)))
        nP, nL, nW = int(info.n_points), int(info.n_polylines), int(info.n_slices)
        d_lines, d_slices = torch.empty((nL, 14), device="cuda"), torch.empty((nW, 18), device="cuda")
        measure = lambda: _lib.check(L.ft_slices_measure(handle, C.c_void_p(d_lines.data_ptr()), C.c_void_p(d_slices.data_ptr())))
        measure()
        torch.cuda.synchronize()
        reduced = (d_lines.cpu().numpy().tobytes(), d_slices.cpu().numpy().tobytes())
        _lib.check(L.ft_ctx_contour_measure_probe(ctx, 1))
        measure()
        torch.cuda.synchronize()
        same = (d_lines.cpu().numpy().tobytes(), d_slices.cpu().numpy().tobytes()) == reduced
        _lib.check(L.ft_ctx_contour_measure_probe(ctx, 0))
        runs = {"slice": [], "measure": [], "measure eager": [], "wall measure": [], "wall host route": []}
        for _ in range(ROUNDS):
            runs["slice"].append(kernel_ms(lambda: L.ft_slices_destroy(slice_once()), 1))
            runs["measure"].append(kernel_ms(measure, REPS))
            _lib.check(L.ft_ctx_contour_measure_probe(ctx, 1))
            runs["measure eager"].append(kernel_ms(measure, REPS))
            _lib.check(L.ft_ctx_contour_measure_probe(ctx, 0))
            h_lines, h_slices = np.empty(nL, np.dtype(_lib.CONTOUR_MEASURE_DTYPE)), np.empty(nW, np.dtype(_lib.SLICE_MEASURE_DTYPE))
            t0 = time.perf_counter()
            for _ in range(WALL_CALLS):
                _lib.check(L.ft_slices_measure(handle, h_lines.ctypes.data_as(C.c_void_p), h_slices.ctypes.data_as(C.c_void_p)))
            runs["wall measure"].append((time.perf_counter() - t0) * 1e3 / WALL_CALLS)
            t0 = time.perf_counter()
            for _ in range(WALL_CALLS):
                route = host_route(handle, nP, nL, axis)
            runs["wall host route"].append((time.perf_counter() - t0) * 1e3 / WALL_CALLS)
        line = {"scene": "console_scene 1000 tori", "lattice": counts, "axis": axis, "points": nP, "polylines": nL, "slices": nW, "closed": int(info.n_closed),
                "eager gives the same bytes": bool(same), "largest |area - numpy area|": float(np.abs(h_lines["area"] - route[1]).max()) if nL else 0.0,
                "volume of the stack": float(h_slices["area"].sum() * abs(step[axis])), "build": ft.build_info()["src"],
                **{k: stat(v) for k, v in runs.items()}}
        L.ft_slices_destroy(handle)
        print(json.dumps(line))
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    dev.close()


if __name__ == "__main__":
    main()
