#!/usr/bin/env python3
"""Per-pixel hit buffers (ft_render_hits_device): median kernel time of the plain frame, the hit buffers alone and the frame with its hit
buffers, per scene and size, plus the wall time of the host form against the device form.  One JSON line per (scene, size, mode).
Not the contract bench (that is bench.py)."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import fraytracer_amd as ft
from fraytracer_amd import synthetic as syn

WARMUP, RUNS = 1, 5
dev = ft.Device(0)
cam = syn.default_camera()
EPS, LEN = syn.EPSILON, syn.RAY_LENGTH
cases = [("C3 smooth256", syn.config3()[0], 4096), ("Program.fs scene", syn.console_scene()[0], 1000),
         ("Program.fs scene", syn.console_scene()[0], 4000), ("C2 union32", syn.config2()[0], 1024)]
only = sys.argv[1:]


def median_ms(launch, ds):
    for _ in range(WARMUP):
        launch(); ds.collect_stats()
    ms, walls = [], []
    for _ in range(RUNS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        launch()
        st = ds.collect_stats()
        walls.append((time.perf_counter() - t0) * 1e3)
        ms.append(st["kernel_ms"])
    return statistics.median(ms), statistics.median(walls), st


for name, scene, n in cases:
    if only and not any(o in name for o in only):
        continue
    ds = dev.scene(scene)
    size = ft.ImageSize(n, n)
    img = torch.empty((n, n, 3), dtype=torch.float32, device="cuda")
    hits = torch.empty((n, n, 16), dtype=torch.float32, device="cuda")
    mat = torch.empty((n, n), dtype=torch.int32, device="cuda")
    modes = {"render": lambda: ds.render_device(EPS, LEN, size, cam, img.data_ptr()),
             "hits_only": lambda: ds.render_hits_device(EPS, LEN, size, cam, hits.data_ptr(), mat.data_ptr()),
             "shade_hits": lambda: ds.render_hits_device(EPS, LEN, size, cam, hits.data_ptr(), mat.data_ptr(), img.data_ptr())}
    base = None
    for mode, launch in modes.items():
        ms, wall, st = median_ms(launch, ds)
        base = ms if mode == "render" else base
        rays = st["rays_primary"] + st["rays_shadow"] + st["rays_ext"]
        print(json.dumps({"scene": name, "size": n, "mode": mode, "kernel_ms": round(ms, 3), "vs_render": round(ms / base, 3),
                          "Mrays/s": round(rays / ms / 1e3, 1), "device_wall_ms": round(wall, 3), "fast_path": ds.info()["fast_path"]}), flush=True)
    del img, hits, mat
    torch.cuda.empty_cache()
    # host form: the whole frame on lane 0, then the copies; wall time of the call against the device form's (above)
    walls = []
    for i in range(WARMUP + RUNS):
        t0 = time.perf_counter()
        _, _, st = ds.render_hits(EPS, LEN, size, cam, shade=True)
        if i >= WARMUP:
            walls.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"scene": name, "size": n, "mode": "shade_hits_host", "host_wall_ms": round(statistics.median(walls), 3),
                      "kernel_ms": round(st["kernel_ms"], 3)}), flush=True)
    ds.close()
dev.close()
