#!/usr/bin/env python3
"""Ray buffers in device memory (ft_trace_rays_device, ft_trace_rays_hits_device).  Prints one JSON line (profiles/rays_device_probe.jsonl).

The ray buffer is the pixel rays of an N x N frame of the Program.fs camera (N = 1024 and 4096), for the reference's own scene (Program.fs)
and for C3.

  host    wall time of ft_trace_rays (rays and colours in host memory, staged through device scratch) against ft_trace_rays_device on
          rays that already lie in device memory plus one collect_stats (which synchronises); the colours are the same bits.
  hits    kernel time of ONE trace_rays_hits_device (colours + records + material handles) against the two launches it replaces,
          trace_rays_device + object_try_trace_device, alternated in the same loop; colours and records are the same bits.
  plain   kernel time of plain ft_trace_rays (host form, which every tree has) with its run-to-run range: run on two trees to compare
          the kernels that must not have changed (--part plain needs nothing of this pull request).

Medians over RUNS after WARMUP.  Not the contract bench (that is bench.py)."""
import argparse
import json
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


def pixel_rays(n):
    """the rays Camera.uniformPixelToRay makes for an n x n frame (Camera.fs:48-52, Image.fs:20-23), float32 [n * n, 8], x-major.  Vectorised, so
    the last bit of a direction may differ from the library's own pixel path: the probe compares ray-buffer calls with each other only."""
    cam = syn.default_camera().as_array().astype(np.float32)
    pos, fw, up, rt = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    t = (np.arange(n, dtype=np.float32) / np.float32(n)) - np.float32(0.5)
    d = fw[None, None, :] + t[:, None, None] * rt[None, None, :] + t[None, :, None] * up[None, None, :]
    d = (d / np.sqrt((d * d).sum(-1, keepdims=True, dtype=np.float32))).astype(np.float32)
    rays = np.empty((n, n, 8), np.float32)
    rays[..., 0:3] = pos
    rays[..., 3:6] = d
    rays[..., 6] = LEN
    rays[..., 7] = EPS
    return rays.reshape(-1, 8)


def stat(ms):
    return {"median_ms": round(statistics.median(ms), 3), "range_ms": [round(min(ms), 3), round(max(ms), 3)]}


def wall(call):
    for _ in range(WARMUP):
        call()
    ms = []
    for _ in range(RUNS):
        t = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t) * 1e3)
    return ms


def host_case(ds, rays):
    n = len(rays)
    out = np.empty((n, 3), np.float32)
    lib, C = ft._lib.lib, ft._lib.C
    st = ft._lib.Stats()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    host = wall(lambda: ft._lib.check(lib.ft_trace_rays(ds.device._ctx, ds._scene, ptr(rays), n, ptr(out), C.byref(st))))
    d_rays = torch.from_numpy(rays).cuda()
    d_out = torch.full((n, 3), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def device():
        ds.trace_rays_device(d_rays.data_ptr(), n, d_out.data_ptr())
        ds.collect_stats()
    dev = wall(device)
    same = bool(np.array_equal(d_out.cpu().numpy().view(np.uint32), out.view(np.uint32)))
    return {"host_wall": stat(host), "device_wall": stat(dev), "speedup": round(statistics.median(host) / statistics.median(dev), 2), "same_bits": same}


def hits_case(ds, rays):
    n = len(rays)
    d_rays = torch.from_numpy(rays).cuda()
    nan = float("nan")
    rgb = [torch.full((n, 3), nan, dtype=torch.float32, device="cuda") for _ in range(2)]
    rec = [torch.full((n, 16), nan, dtype=torch.float32, device="cuda") for _ in range(2)]
    mat = [torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    one, two_rgb, two_rec = [], [], []
    for i in range(WARMUP + RUNS):                         # alternated: one launch, then the two it replaces
        ds.trace_rays_hits_device(d_rays.data_ptr(), n, rgb[0].data_ptr(), rec[0].data_ptr(), mat[0].data_ptr())
        a = ds.collect_stats()["kernel_ms"]
        ds.trace_rays_device(d_rays.data_ptr(), n, rgb[1].data_ptr())
        b = ds.collect_stats()["kernel_ms"]
        ds.object_try_trace_device(d_rays.data_ptr(), n, rec[1].data_ptr(), mat[1].data_ptr())
        c = ds.collect_stats()["kernel_ms"]
        if i >= WARMUP:
            one.append(a); two_rgb.append(b); two_rec.append(c)
    same = bool(torch.equal(rgb[0].view(torch.int32), rgb[1].view(torch.int32)) and torch.equal(rec[0].view(torch.int32), rec[1].view(torch.int32))
                and torch.equal(mat[0], mat[1]))
    two = [b + c for b, c in zip(two_rgb, two_rec)]
    return {"one_launch": stat(one), "two_launches": stat(two), "trace_rays_device": stat(two_rgb), "object_try_trace_device": stat(two_rec),
            "two_over_one": round(statistics.median(two) / statistics.median(one), 3), "same_bits": same,
            "hit_fraction": round(float((mat[0] >= 0).float().mean().item()), 3)}


def plain_case(ds, rays):
    ms = []
    for i in range(WARMUP + RUNS):
        _, st = ds.trace_rays(rays)
        if i >= WARMUP:
            ms.append(st["kernel_ms"])
    return {"trace_rays_kernel": stat(ms), "fast_path": ds.info()["fast_path"]}


ap = argparse.ArgumentParser()
ap.add_argument("--part", choices=("all", "host", "hits", "plain"), default="all")
ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
args = ap.parse_args()
dev = ft.Device(0)
res = {"probe": "rays_device", "build": ft.build_info()["src"], "device": torch.cuda.get_device_name(0), "warmup": WARMUP, "runs": RUNS, "cases": []}
for name, scene in (("Program.fs scene", syn.console_scene()[0]), ("C3 smooth256", syn.config3()[0])):
    ds = dev.scene(scene)
    for n in args.sizes:
        rays = pixel_rays(n)
        case = {"scene": name, "frame": n, "rays": len(rays)}
        if args.part in ("all", "plain"):
            case["plain"] = plain_case(ds, rays)
        if args.part in ("all", "host"):
            case["host"] = host_case(ds, rays)
        if args.part in ("all", "hits"):
            case["hits"] = hits_case(ds, rays)
        res["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
        del rays
        torch.cuda.empty_cache()
    ds.close()
dev.close()
print(json.dumps(res))
