#!/usr/bin/env python3
"""The scene of the reference's console program (src/FrayTracer.Console/Program.fs: System.Random(19), 1000 tori) as a stack of SVG layers, the way
a 3D-printing slicer sees it: the distance field is evaluated on a lattice around the scene, and per lattice plane the contour {distance = 0} is
extracted and chained into ordered, oriented loops on the GPU (DeviceScene.slice_lattice), then drawn one file per layer.

    python examples/slice.py [--tori 1000] [--points 256] [--layers 64] [--axis 2] [--span 1.05] [--refine 8] [--measure] [--out layers]

--measure: per layer the enclosed area, the perimeter, the outer loops, the holes and the centroid, and the stack's volume, measured on the GPU where
the contours lie (ft_slices_measure: exact sums, the same bytes on every run).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fraytracer_amd as ft
from fraytracer_amd import synthetic as syn

ap = argparse.ArgumentParser()
ap.add_argument("--tori", type=int, default=1000)
ap.add_argument("--points", type=int, default=256, help="lattice points per in-plane axis")
ap.add_argument("--layers", type=int, default=64, help="lattice planes along the axis")
ap.add_argument("--axis", type=int, default=2, choices=(0, 1, 2), help="the planes' normal: 0 x, 1 y, 2 z")
ap.add_argument("--span", type=float, default=1.05, help="half-width of the lattice in boundary radii")
ap.add_argument("--refine", type=int, default=None, help="bisection rounds (0 .. 32) that move every vertex along its lattice edge onto the surface")
ap.add_argument("--measure", action="store_true", help="print a table per layer (area, perimeter, outer loops, holes, centroid) and the stack's volume")
ap.add_argument("--out", default="layers", help="directory of the layer_NNNN.svg files")
args = ap.parse_args()

scene, _ = syn.console_scene(seed=19, n=args.tori)                         # Program.fs:14-83
ds = ft.Device.default(0).scene(scene)
cx, cy, cz, radius = ds.boundary()
half = args.span * radius
counts = [args.points] * 3
counts[args.axis] = args.layers
step = [2.0 * half / (n - 1) if n > 1 else 0.0 for n in counts]
origin = [c - half if n > 1 else c for c, n in zip((cx, cy, cz), counts)]

t0 = time.perf_counter()
contours = ds.slice_lattice(origin, step, counts, axis=args.axis, refine=args.refine, measures=args.measure)
print(f"{len(contours.polylines)} polylines ({contours.closed} closed), {len(contours.points)} points in {contours.slices} layers "
      f"in {time.perf_counter() - t0:.3f} s")
if args.measure:
    per, u, v = contours.layer_measures, "xyz"[(args.axis + 1) % 3], "xyz"[(args.axis + 2) % 3]
    area, length, centre = per.area, per.length, per.centroid
    print(f"{'layer':>5} {'area':>12} {'perimeter':>12} {'outer':>5} {'holes':>5} {'centroid ' + u:>12} {'centroid ' + v:>12}")
    for w in range(contours.slices):
        where = f"{centre[w, 0]:12.6f} {centre[w, 1]:12.6f}" if area[w] != 0 else f"{'-':>12} {'-':>12}"
        print(f"{w:5d} {area[w]:12.6f} {length[w]:12.6f} {per.n_outer[w]:5d} {per.n_holes[w]:5d} {where}")
    print(f"volume of the stack: {float(area.sum()) * abs(step[args.axis]):.6f} (the layers' areas times the layer distance {abs(step[args.axis]):.6f}); "
          f"{int(per.n_unmeasured.sum())} unmeasured segments")
os.makedirs(args.out, exist_ok=True)
for w in range(contours.slices):
    contours.write_svg(os.path.join(args.out, f"layer_{w:04d}.svg"), w)
print("wrote", contours.slices, "layers to", args.out)
