#!/usr/bin/env python3
"""Hit buffers of batches of camera views (ft_render_views_hits).  Prints one JSON line (profiles/views_hits_probe.jsonl).

  hits  kernel time of one hits-only batch of K orbit cameras (render_views_hits_device) against the summed kernel time of K sequential
        render_hits_device calls of the same cameras, and whether records and material planes are the same bits: the reference's own scene
        (Program.fs) at 1000^2 with K = 4, 16 and C3 at 1024^2 with K = 16; plus the host form's wall time (render_views_hits against K
        render_hits calls) for the Program.fs scene, K = 16.
  ext   kernel time of plain render_views_device batches that run the EXTENSION *_views kernels (spp 4, ambient occlusion), K = 16: the
        builds whose hit stores changed.  Runs on a tree without ft_render_views_hits too (--part ext), for a before / after comparison.

Medians over RUNS after WARMUP.  Not the contract bench (that is bench.py)."""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import fraytracer_amd as ft
from fraytracer_amd import synthetic as syn

WARMUP, RUNS = 2, 7
EPS, LEN = syn.EPSILON, syn.RAY_LENGTH


def orbit(k, n):
    """camera k of n on a circle of radius 10 around the scene, k = 0 the Program.fs camera (0, 0, -10) (as tools/views_probe.py)"""
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


def median_wall_ms(call):
    for _ in range(WARMUP):
        call()
    ms = []
    for _ in range(RUNS):
        t = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms)


def hits_cases(dev):
    cases = []
    for name, scene, n, views in (("Program.fs scene", syn.console_scene()[0], 1000, (4, 16)), ("C3 smooth256", syn.config3()[0], 1024, (16,))):
        ds = dev.scene(scene)
        size = ft.ImageSize(n, n)
        for K in views:
            cams = [orbit(k, K) for k in range(K)]
            rec = [torch.full((K, n, n, 16), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]    # batch, sequential
            mat = [torch.full((K, n, n), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
            torch.cuda.synchronize()
            b_ms, b_lo, b_hi = median_kernel_ms(lambda: ds.render_views_hits_device(EPS, LEN, size, cams, rec[0].data_ptr(), mat[0].data_ptr()), ds)
            s_ms, s_lo, s_hi = median_kernel_ms(lambda: [ds.render_hits_device(EPS, LEN, size, c, rec[1][k].data_ptr(), mat[1][k].data_ptr())
                                                         for k, c in enumerate(cams)], ds)
            same = bool(torch.equal(rec[0].view(torch.int32), rec[1].view(torch.int32)) and torch.equal(mat[0], mat[1]))
            case = {"scene": name, "size": n, "views": K, "fast_path": ds.info()["fast_path"],
                    "batch_kernel_ms": round(b_ms, 3), "batch_ms_range": [round(b_lo, 3), round(b_hi, 3)],
                    "sequential_kernel_ms": round(s_ms, 3), "sequential_ms_range": [round(s_lo, 3), round(s_hi, 3)],
                    "speedup": round(s_ms / b_ms, 3), "ms_per_view": round(b_ms / K, 3), "hits_equal": same}
            del rec, mat
            torch.cuda.empty_cache()
            if name == "Program.fs scene" and K == 16:        # the host form, records and material planes copied into host arrays
                out = [(np.empty((K, n, n, 16), np.float32), np.empty((K, n, n), np.int32)) for _ in range(2)]
                ctx, sc, arr = dev._ctx, ds._scene, ds._cameras(cams)[0]
                p = ds._params(size, EPS, LEN)
                lib, C = ft._lib.lib, ft._lib.C
                st = ft._lib.Stats()
                ptr = lambda a: a.ctypes.data_as(C.c_void_p)
                hb = median_wall_ms(lambda: ft._lib.check(lib.ft_render_views_hits(ctx, sc, arr, K, C.byref(p), None, ptr(out[0][0]), ptr(out[0][1]), C.byref(st))))
                hs = median_wall_ms(lambda: [ft._lib.check(lib.ft_render_hits(ctx, sc, C.byref(c._c), C.byref(p), None, ptr(out[1][0][k]), ptr(out[1][1][k]), C.byref(st)))
                                             for k, c in enumerate(cams)])
                case.update({"host_batch_wall_ms": round(hb, 2), "host_sequential_wall_ms": round(hs, 2),
                             "host_equal": bool(np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32)) and np.array_equal(out[0][1], out[1][1]))})
                del out
            cases.append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
        ds.close()
    return cases


def ext_cases(dev):
    cases = []
    K = 16
    for name, scene, n, ext in (("Program.fs scene", syn.console_scene()[0], 1000, dict(spp=4)), ("Program.fs scene", syn.console_scene()[0], 1000, dict(ao_samples=4, ao_radius=0.75)),
                                ("C3 smooth256", syn.config3()[0], 1024, dict(spp=4))):
        ds = dev.scene(scene)
        size = ft.ImageSize(n, n)
        cams = [orbit(k, K) for k in range(K)]
        out = torch.empty((K, n, n, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ms, lo, hi = median_kernel_ms(lambda: ds.render_views_device(EPS, LEN, size, cams, out.data_ptr(), **ext), ds)
        cases.append({"scene": name, "size": n, "views": K, "ext": ext, "batch_kernel_ms": round(ms, 3), "batch_ms_range": [round(lo, 3), round(hi, 3)],
                      "image_sum": float(out.double().sum().item())})
        print(json.dumps(cases[-1]), file=sys.stderr, flush=True)
        del out
        torch.cuda.empty_cache()
        ds.close()
    return cases


ap = argparse.ArgumentParser()
ap.add_argument("--part", choices=("all", "hits", "ext"), default="all")
args = ap.parse_args()
dev = ft.Device(0)
res = {"probe": "views_hits", "build": ft.build_info()["src"], "device": torch.cuda.get_device_name(0), "warmup": WARMUP, "runs": RUNS}
if args.part in ("all", "hits"):
    res["hits"] = hits_cases(dev)
if args.part in ("all", "ext"):
    res["ext"] = ext_cases(dev)
dev.close()
print(json.dumps(res))
