#!/usr/bin/env python3
"""Hand-out orders on the C3 frame (FT_OPT_ORDER, include/fraytracer_hip.h; kernels.hip "Tile order"): HIP-event kernel ms and wall ms per frame through
Scene.render_device, the variants alternated over several rounds in one call, each after one untimed launch that records the tile costs.
  off: FT_OPT_ORDER = 0;  record: 2 (index order, costs written);  sort: every tile by descending cost;  mean / 2mean: the tiles at or above 1 x / 2 x the
  mean cost first by descending cost, the rest in index order (mean is the shipped rule).
kernel ms is the trace kernel alone; wall ms also holds the three order-building launches behind every frame.
Usage: tile_order_probe.py [--size 4096] [--spheres 256] [--rounds 3] [--frames 4] [--tag TEXT] [variant ...]"""
import argparse, ctypes as C, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import fraytracer_amd as ft
from fraytracer_amd import _lib
from fraytracer_amd import synthetic as syn

VARIANTS = {"off": (0, 1, 1), "record": (2, 1, 1), "sort": (1, 0, 1), "mean": (1, 1, 1), "2mean": (1, 2, 1)}      # FT_OPT_ORDER, heavy from num / den of the mean
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--spheres", type=int, default=256)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--frames", type=int, default=4)
ap.add_argument("--tag", default="")
ap.add_argument("variants", nargs="*", default=["off", "sort", "mean", "2mean"])
args = ap.parse_args()

dev = ft.Device(0)
rule = _lib.lib.ft_ctx_tile_order_rule                      # internal: not in the header
rule.restype, rule.argtypes = C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]
ds = dev.scene(syn.config3(n=args.spheres, size=args.size)[0])
size, cam = ft.ImageSize(args.size, args.size), syn.default_camera()
buf = torch.empty((args.size, args.size, 3), dtype=torch.float32, device="cuda")


def frame():
    ds.render_device(syn.EPSILON, syn.RAY_LENGTH, size, cam, buf.data_ptr())


frame(); ds.collect_stats()                                 # warm-up
kms, wms, last = {v: [] for v in args.variants}, {v: [] for v in args.variants}, {}
for _ in range(args.rounds):
    for v in args.variants:
        opt, num, den = VARIANTS[v]
        dev.set_option("order", opt)
        _lib.check(rule(dev._ctx, num, den))
        frame(); ds.collect_stats()                         # records the costs the timed frames' order is built from
        t0 = time.perf_counter()
        for _ in range(args.frames):
            frame()
        st = ds.collect_stats()                             # waits for the stream
        wms[v].append((time.perf_counter() - t0) * 1e3 / args.frames)
        kms[v].append(st["kernel_ms"] / args.frames)
        last[v] = st
_lib.check(rule(dev._ctx, 1, 1))
for v in args.variants:
    st = last[v]
    print(json.dumps({"build": args.tag, "scene": f"C3 n={args.spheres} {args.size}^2", "variant": v, "kernel_ms_median": round(statistics.median(kms[v]), 3),
                      "kernel_ms_runs": [round(x, 3) for x in kms[v]], "wall_ms_median": round(statistics.median(wms[v]), 3), "wall_ms_runs": [round(x, 3) for x in wms[v]],
                      "sdf_evals_per_frame": st["sdf_evals"] // args.frames, "wave_rounds_per_frame": st["wave_evals"] // args.frames,
                      "shader_mhz": round(st["shader_mhz"], 1)}), flush=True)
dev.close()
