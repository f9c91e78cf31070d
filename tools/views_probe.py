#!/usr/bin/env python3
"""Batches of camera views (ft_render_views_device): kernel time of one batch launch of K orbit cameras against the summed kernel time of K
sequential render_device calls of the same cameras, and whether the images are the same bits.  The reference's own scene (Program.fs) at
1000^2 with K = 1, 4, 16 and C3 at 1024^2 with K = 16; medians over RUNS after WARMUP.  Prints one JSON line.
Not the contract bench (that is bench.py)."""
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import fraytracer_amd as ft
from fraytracer_amd import synthetic as syn

WARMUP, RUNS = 2, 7
EPS, LEN = syn.EPSILON, syn.RAY_LENGTH


def orbit(k, n):
    """camera k of n on a circle of radius 10 around the scene, k = 0 the Program.fs camera (0, 0, -10)"""
    a = 2.0 * math.pi * k / n
    return ft.Camera.lookAt(Position=(10.0 * math.sin(a), 0.0, -10.0 * math.cos(a)), LookAt=(0.0, 0.0, 0.0), Up=(0.0, 1.0, 0.0),
                            Lens=ft.Lens.create(60.0))


def median_kernel_ms(launch, ds):
    for _ in range(WARMUP):
        launch(); ds.collect_stats()
    ms = []
    for _ in range(RUNS):
        launch()
        ms.append(ds.collect_stats()["kernel_ms"])
    return statistics.median(ms), min(ms), max(ms)


dev = ft.Device(0)
cases = []
for name, scene, n, views in (("Program.fs scene", syn.console_scene()[0], 1000, (1, 4, 16)), ("C3 smooth256", syn.config3()[0], 1024, (16,))):
    ds = dev.scene(scene)
    size = ft.ImageSize(n, n)
    for K in views:
        cams = [orbit(k, K) for k in range(K)]
        batch = torch.empty((K, n, n, 3), dtype=torch.float32, device="cuda")
        seq = torch.empty((K, n, n, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        b_ms, b_lo, b_hi = median_kernel_ms(lambda: ds.render_views_device(EPS, LEN, size, cams, batch.data_ptr()), ds)
        s_ms, s_lo, s_hi = median_kernel_ms(lambda: [ds.render_device(EPS, LEN, size, c, seq[k].data_ptr()) for k, c in enumerate(cams)], ds)
        same = bool(torch.equal(batch.view(torch.int32), seq.view(torch.int32)))
        cases.append({"scene": name, "size": n, "views": K, "fast_path": ds.info()["fast_path"],
                      "batch_kernel_ms": round(b_ms, 3), "batch_ms_range": [round(b_lo, 3), round(b_hi, 3)],
                      "sequential_kernel_ms": round(s_ms, 3), "sequential_ms_range": [round(s_lo, 3), round(s_hi, 3)],
                      "speedup": round(s_ms / b_ms, 3), "ms_per_view": round(b_ms / K, 3), "images_equal": same})
        print(json.dumps(cases[-1]), file=sys.stderr, flush=True)
        del batch, seq
        torch.cuda.empty_cache()
    ds.close()
dev.close()
print(json.dumps({"probe": "views", "build": ft.build_info()["src"], "device": torch.cuda.get_device_name(0), "warmup": WARMUP, "runs": RUNS,
                  "cases": cases}))
