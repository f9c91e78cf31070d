#!/usr/bin/env python3
"""Miss-certificate schedules on the C3 frame (FT_OPT_CERT_POLICY, include/fraytracer_hip.h): HIP-event kernel ms through Scene.render_device for a
list of policy words, the words alternated over several rounds; per word the median, the spread, sdf_evals and evaluation rounds per frame.
Usage: cert_policy_probe.py [--size 4096] [--spheres 256] [--strength 0.25] [--fov 60] [--distance 10] [--rounds 3] [--frames 4] word[=label] ...
(a word as a Python integer literal, e.g. 0x4001ffff; word/occl sets FT_OPT_OCCL_POLICY = occl beside it, occl = off switches FT_OPT_OCCL off: 0/1 is
the shipped miss-certificate schedule with the occlusion certificate tried every round).  Every line carries tile_over_margin: the side of an 8x8 pixel tile at the far side of the support
sphere over the certificate's margin — at most 1 is where word 0 leaves the per-lane tries out (capi.cpp launchTrace)."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import fraytracer_amd as ft
from fraytracer_amd import synthetic as syn

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--spheres", type=int, default=256)
ap.add_argument("--strength", type=float, default=0.25)
ap.add_argument("--fov", type=float, default=60.0)
ap.add_argument("--distance", type=float, default=10.0)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--frames", type=int, default=4)
ap.add_argument("--tag", default="")
ap.add_argument("words", nargs="+")
args = ap.parse_args()


def s32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


def parse(w):
    """word[/occl][=label] -> ((FT_OPT_CERT_POLICY, FT_OPT_OCCL, FT_OPT_OCCL_POLICY), label)"""
    spec = w.split("=")[0]
    cert, _, occl = spec.partition("/")
    return (s32(int(cert, 0)), 0 if occl == "off" else 1, int(occl, 0) if occl not in ("", "off") else 0), w.split("=")[1] if "=" in w else w


words = [parse(w) for w in args.words]
dev = ft.Device(0)
import numpy as np
ds = dev.scene(syn.config3(n=args.spheres, strength=args.strength)[0])
size = ft.ImageSize(args.size, args.size)
cam = ft.Camera.lookAt(Position=(0.0, 0.0, -args.distance), LookAt=(0.0, 0.0, 0.0), Up=(0.0, 1.0, 0.0), Lens=ft.Lens.create(args.fov))     # fov 60, distance 10: Program.fs
ca, sup = cam.as_array().astype(np.float64), ds.support_sphere()
norm = lambda v: float(np.sqrt((v * v).sum()))
tile = 8.0 * max(norm(ca[6:9]), norm(ca[9:12])) / args.size * (norm(ca[0:3] - np.array(sup[:3])) + sup[3]) / norm(ca[3:6])
ratio = tile / ds.miss_certificate()["margin"]
buf = torch.empty((args.size, args.size, 3), dtype=torch.float32, device="cuda")
ds.render_device(syn.EPSILON, syn.RAY_LENGTH, size, cam, buf.data_ptr()); ds.collect_stats()     # warm-up
ms = {w: [] for w, _ in words}
last = {}
for _ in range(args.rounds):
    for w, _ in words:
        dev.set_option("cert_policy", w[0]); dev.set_option("occl", w[1]); dev.set_option("occl_policy", w[2])
        for _ in range(args.frames):
            ds.render_device(syn.EPSILON, syn.RAY_LENGTH, size, cam, buf.data_ptr())
        st = ds.collect_stats()
        ms[w].append(st["kernel_ms"] / args.frames)
        last[w] = st
for w, label in words:
    st = last[w]
    print(json.dumps({"build": args.tag, "scene": f"C3 n={args.spheres} s={args.strength} {args.size}^2 fov {args.fov:g} at {args.distance:g}", "tile_over_margin": round(ratio, 3), "policy": f"{w[0] & 0xFFFFFFFF:#010x}", "occl": w[1], "occl_policy": f"{w[2]:#x}", "label": label, "kernel_ms_median": round(statistics.median(ms[w]), 3),
                      "kernel_ms_runs": [round(v, 3) for v in ms[w]], "sdf_evals_per_frame": st["sdf_evals"] // args.frames,
                      "wave_rounds_per_frame": st["wave_evals"] // args.frames, "shader_mhz": round(st["shader_mhz"], 1)}), flush=True)
