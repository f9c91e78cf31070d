#!/usr/bin/env python3
"""Relighting without re-tracing (ft_scene_relight, ft_shade_hits_device).  Prints one JSON line (profiles/shade_hits_probe.jsonl).

The reference's own scene (Program.fs) and C3 at N x N (N = 1024 and 4096) under the relit lights of tests/test_gpu_shade_hits.py; the
records are those ft_render_hits_device wrote for the scene as it was.

  shade   kernel time of ONE shade_hits_device of the relit scene over the frame's records, per run; the colours are compared with the relit
          scene's render_device (same bits).
  render  kernel time of render_device of the relit scene built from scratch (ft_scene_create), per run: what a relit frame costs without
          ft_shade_hits.  --part render needs nothing of this feature, so it runs on an older tree as well: alternate the two trees.
  setup   wall time of ft_scene_relight against ft_scene_create for the Program.fs scene (1000 tori), the light handles made beforehand.

Medians over RUNS after WARMUP, with the range.  Not the contract bench (that is bench.py)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import fraytracer_amd as ft
from fraytracer_amd import _lib
from fraytracer_amd import synthetic as syn
from fraytracer_amd.api import realise

WARMUP, RUNS = 2, 7
EPS, LEN = syn.EPSILON, syn.RAY_LENGTH
BG = (0.02, 0.03, 0.05)
LIGHTS = (ft.SdfLight.directional((0.6, -1.0, -0.3), (0.9, 0.8, 0.7)), ft.SdfLight.point((3.0, 4.0, -6.0), (30.0, 40.0, 50.0)),
          ft.SdfLight.directional((0.0, 1.0, 0.2), (0.3, 0.3, 0.3)))


def stat(ms):
    return {"median_ms": round(statistics.median(ms), 3), "range_ms": [round(min(ms), 3), round(max(ms), 3)], "runs_ms": [round(v, 3) for v in ms]}


def render_case(fresh, n, cam):
    out = torch.full((n, n, 3), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ms = []
    for i in range(WARMUP + RUNS):
        fresh.render_device(EPS, LEN, ft.ImageSize(n, n), cam, out.data_ptr())
        st = fresh.collect_stats()
        if i >= WARMUP:
            ms.append(st["kernel_ms"])
    return {"render_device_kernel": stat(ms), "rays_primary": st["rays_primary"], "rays_shadow": st["rays_shadow"], "sdf_evals": st["sdf_evals"]}, out


def shade_case(ds, n, cam, want):
    rec = torch.full((n, n, 16), float("nan"), dtype=torch.float32, device="cuda")
    out = torch.full((n, n, 3), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ds.render_hits_device(EPS, LEN, ft.ImageSize(n, n), cam, rec.data_ptr())
    ds.collect_stats()
    relit = ds.relight(BG, LIGHTS)
    ms = []
    for i in range(WARMUP + RUNS):
        relit.shade_hits_device(rec.data_ptr(), n * n, out.data_ptr())
        st = relit.collect_stats()
        if i >= WARMUP:
            ms.append(st["kernel_ms"])
    res = {"shade_hits_device_kernel": stat(ms), "rays_shadow": st["rays_shadow"], "hits_shadow": st["hits_shadow"], "sdf_evals": st["sdf_evals"],
           "hit_fraction": round(float((rec[..., 14].view(torch.int32) != 0).float().mean().item()), 3),
           "same_bits_as_render": bool(torch.equal(out.view(torch.int32), want.view(torch.int32))), "fast_path": relit.info()["fast_path"]}
    relit.close()
    return res


def setup_case(dev, ds):
    lights = [realise(l, dev) for l in LIGHTS]
    hs = (C.c_int32 * 3)(*lights)
    bg = (C.c_float * 3)(*BG)
    lib = _lib.lib

    def timed(call):
        ms = []
        for i in range(WARMUP + RUNS):
            p = C.c_void_p()
            t = time.perf_counter()
            _lib.check(call(p))
            dt = (time.perf_counter() - t) * 1e3
            lib.ft_scene_destroy(p)
            if i >= WARMUP:
                ms.append(dt)
        return ms
    create = timed(lambda p: lib.ft_scene_create(dev._ctx, ds._object, bg, hs, 3, C.byref(p)))
    relight = timed(lambda p: lib.ft_scene_relight(ds._scene, bg, hs, 3, C.byref(p)))
    return {"scene_create_wall": stat(create), "scene_relight_wall": stat(relight),
            "create_over_relight": round(statistics.median(create) / statistics.median(relight), 1)}


ap = argparse.ArgumentParser()
ap.add_argument("--part", choices=("all", "render", "setup"), default="all")
ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
args = ap.parse_args()
dev = ft.Device(0)
cam = syn.default_camera()
res = {"probe": "shade_hits", "part": args.part, "build": ft.build_info()["src"], "device": torch.cuda.get_device_name(0), "warmup": WARMUP, "runs": RUNS,
       "cases": []}
for name, scene in (("Program.fs scene", syn.console_scene()[0]), ("C3 smooth256", syn.config3()[0])):
    ds = dev.scene(scene)
    fresh = dev.scene(ft.SdfScene(scene.Object, BG, LIGHTS))
    if args.part in ("all", "setup") and name.startswith("Program.fs"):
        res["setup"] = setup_case(dev, ds)
        print(json.dumps(res["setup"]), file=sys.stderr, flush=True)
    for n in args.sizes if args.part != "setup" else []:
        case = {"scene": name, "frame": n}
        case["render"], want = render_case(fresh, n, cam)
        if args.part == "all":
            case["shade"] = shade_case(ds, n, cam, want)
            case["shade_over_render"] = round(case["shade"]["shade_hits_device_kernel"]["median_ms"] / case["render"]["render_device_kernel"]["median_ms"], 3)
        res["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
        del want
        torch.cuda.empty_cache()
    ds.close(); fresh.close()
dev.close()
print(json.dumps(res))
