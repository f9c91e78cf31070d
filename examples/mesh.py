#!/usr/bin/env python3
"""The scene of the reference's console program (src/FrayTracer.Console/Program.fs: System.Random(19), 1000 tori) as a triangle mesh: the
distance field is evaluated on a lattice around the scene and the surface is extracted on the GPU (DeviceScene.mesh_lattice), then written as
Wavefront OBJ (or binary STL).

    python examples/mesh.py [--tori 1000] [--points 256] [--span 1.05] [--normals] [--refine 8] [--shells] [--measure]
                            [--keep-largest K | --keep-closed | --keep-bodies] [--out scene.obj]
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
ap.add_argument("--points", type=int, default=256, help="lattice points per axis")
ap.add_argument("--span", type=float, default=1.05, help="half-width of the lattice in boundary radii")
ap.add_argument("--normals", action="store_true", help="per-vertex SdfForm.normal (epsilon = a hundredth of the lattice step)")
ap.add_argument("--refine", type=int, default=None, help="bisection rounds (0 .. 32) that move every vertex along its lattice edge onto the surface")
ap.add_argument("--shells", action="store_true", help="label the mesh's connected pieces on the GPU and print a table of them")
ap.add_argument("--keep-largest", type=int, default=None, metavar="K", help="keep only the K shells with the most triangles")
ap.add_argument("--keep-closed", action="store_true", help="keep only the shells without a border edge")
ap.add_argument("--keep-bodies", action="store_true", help="keep only the closed shells of positive volume: no cavities, no open debris")
ap.add_argument("--measure", action="store_true", help="measure every shell and the whole mesh on the GPU: area, volume, centroid, box")
ap.add_argument("--out", default="scene.obj", help="*.obj or *.stl")
args = ap.parse_args()
if (args.keep_largest is not None) + args.keep_closed + args.keep_bodies > 1:
    ap.error("--keep-largest, --keep-closed and --keep-bodies exclude each other")
keep = args.keep_largest if args.keep_largest is not None else ("closed" if args.keep_closed else ("bodies" if args.keep_bodies else None))

scene, _ = syn.console_scene(seed=19, n=args.tori)                         # Program.fs:14-83
ds = ft.Device.default(0).scene(scene)
cx, cy, cz, radius = ds.boundary()
half = args.span * radius
step = 2.0 * half / (args.points - 1)

t0 = time.perf_counter()
mesh = ds.mesh_lattice((cx - half, cy - half, cz - half), (step,) * 3, (args.points,) * 3,
                       normal_epsilon=0.01 * step if args.normals else None, refine=args.refine, shells=args.shells, keep=keep, measures=args.measure)
print(f"{len(mesh.vertices)} vertices, {len(mesh.triangles)} triangles in {time.perf_counter() - t0:.3f} s")
if mesh.shells is not None:
    sh = mesh.shells
    print(f"{len(sh)} shells, {sh.info['n_closed']} closed, {sh.info['n_unused_vertices']} unused vertices, {sh.info['n_border_edges']} border edges")
    if args.shells:
        print(f"{'shell':>6} {'vertices':>10} {'triangles':>10} {'border':>8} {'closed':>7} {'euler':>6}")
        for s, (rec, closed, chi) in enumerate(zip(sh.records.tolist(), sh.closed.tolist(), sh.euler.tolist())):
            print(f"{s:>6} {rec[1]:>10} {rec[2]:>10} {rec[3]:>8} {'yes' if closed else 'no':>7} {chi:>6}")
if args.measure:
    def line(what, triangles, closed, r, c):
        box = " ".join(f"[{lo:.4g}, {hi:.4g}]" for lo, hi in zip(r["bbox_min"].tolist(), r["bbox_max"].tolist()))
        print(f"{what:>6} {triangles:>10} {closed:>7} {r['area']:>12.6g} {r['volume']:>12.6g}  ({c[0]:.4g}, {c[1]:.4g}, {c[2]:.4g})  {box}")

    print(f"{'shell':>6} {'triangles':>10} {'closed':>7} {'area':>12} {'volume':>12}  centroid  box")
    records, centroid = mesh.shells.measures.host(), mesh.shells.measures.centroid
    for s, (rec, closed) in enumerate(zip(ft.Mesh._host(mesh.shells.records).tolist(), mesh.shells.closed.tolist())):
        line(s, rec[2], "yes" if closed else "no", records[s], centroid[s])
    if len(mesh.measure):
        line("all", len(mesh.triangles), "-", mesh.measure.host()[0], mesh.measure.centroid[0])
(mesh.save_stl if args.out.lower().endswith(".stl") else mesh.save_obj)(args.out)
print("wrote", args.out)
