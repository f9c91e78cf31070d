#!/usr/bin/env python3
"""Generates tests/golden/launch_counters.json: the counters of small launches under every rule launchTrace (capi.cpp) applies — the kernel plan,
the grid size, the hand-out, the two certificate policy words with the tile-width rule, the occlusion schedule, the tile order — one option at a
time from the defaults, on one scene per kernel family, plus the other launch forms at the defaults.  Needs the GPU.

The table pins what the launches counted before launchTrace was cut into named steps, so it is recorded from the library of the commit whose
behaviour is to be kept, not from the code under test:

    python tests/golden/make_launch_counters.py --commit <commit>

records twice and keeps the cells whose two recordings agree (the others are named in "left_out").  Every cell is repeatable by construction:
chunk = refillMin = 64 and no guided hand-out, so a wave owns one tile between two grabs and everything counted is a function of the tile.
wave_evals, times and clocks are not recorded.  culled_fraction and tail_fraction are the ABI's form of the cull and latency-mode counters
(cull_skipped / cull_total, coop_evals / sdf_evals): kept as float32 bit patterns.

tests/test_gpu_parity.py replays cells() against the library in the tree.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "launch_counters.json")

COUNTERS = ("rays_primary", "rays_shadow", "rays_ext", "hits_primary", "hits_shadow", "sdf_evals", "flags")
FRACTIONS = ("culled_fraction", "tail_fraction")


def s32(v):
    return v - (1 << 32) if v & (1 << 31) else v


SHIPPED_LANES = 0 | (6 << 8) | (16 << 16) | (6 << 24)          # capi.cpp FT_CERT_POLICY_DEFAULT
# one option at a time; every other option is at its default (DEFAULTS)
DEFAULTS = {"cert": 1, "escape": 1, "occl": 1, "cert_policy": 0, "occl_policy": 0, "tail_k": -1, "max_blocks_per_cu": 0, "order": 1}
VARIED = [("cert", 0), ("escape", 0), ("occl", 0),
          ("cert_policy", 255 | (255 << 8) | (16 << 16)),        # per-lane tries off
          ("cert_policy", s32(SHIPPED_LANES | (1 << 30))),       # bundle every round
          ("cert_policy", s32(SHIPPED_LANES | (3 << 30))),       # bundle off
          ("occl_policy", 1), ("occl_policy", 255), ("occl_policy", 2 | (3 << 8) | (4 << 16)),
          ("tail_k", 0), ("max_blocks_per_cu", 2)]
ORDERS = (0, 1, 2)                                               # two frames in a row each


def scenes():
    """(name, scene, W, H): the smallest frames at which each rule can still go wrong — a cull site and clusters need >= 32 children, and 160^2
    is where the certificate bites on C3; one carved and one general scene"""
    from fraytracer_amd import synthetic as syn
    c3 = syn.config3(n=64)[0]
    return [("config3(n=64) 96x96", c3, 96, 96), ("config3(n=64) 160x160", c3, 160, 160),
            ("console_like(n=200) 96x96", syn.console_like(n=200)[0], 96, 96), ("mixed_nested 48x40", syn.mixed_nested()[0], 48, 40)]


def pixel_rays(W, H):
    """float32 [W * H, 8] rays of the default camera through a W x H frame, x-major (vectorised: a ray buffer of its own, not the library's pixels)"""
    from fraytracer_amd import synthetic as syn
    cam = syn.default_camera().as_array().astype(np.float32)
    pos, fw, up, rt = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    tx = (np.arange(W, dtype=np.float32) / np.float32(W)) - np.float32(0.5)
    ty = (np.arange(H, dtype=np.float32) / np.float32(H)) - np.float32(0.5)
    d = fw[None, None, :] + tx[:, None, None] * rt[None, None, :] + ty[None, :, None] * up[None, None, :]
    n2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    d = (d / np.sqrt(n2)[..., None]).astype(np.float32)
    rays = np.empty((W, H, 8), np.float32)
    rays[..., 0:3] = pos
    rays[..., 3:6] = d
    rays[..., 6] = syn.RAY_LENGTH
    rays[..., 7] = syn.EPSILON
    return rays.reshape(-1, 8)


def counters(st):
    out = {k: int(st[k]) for k in COUNTERS}
    for k in FRACTIONS:
        out[k] = int(np.float32(st[k]).view(np.uint32))
    return out


def cells(dev):
    """{cell name: counters} of every cell, in a fixed order, on the fraytracer_amd.Device `dev`; leaves its options at DEFAULTS"""
    import fraytracer_amd as ft
    from fraytracer_amd import synthetic as syn
    eps, length = syn.EPSILON, syn.RAY_LENGTH
    cam = syn.default_camera()
    cam2 = ft.Camera.lookAt(Position=(3.0, 2.0, -9.0), LookAt=(0.0, 0.5, 0.0), Up=(0.0, 1.0, 0.0), Lens=ft.Lens.create(60.0))
    out = {}
    for k, v in DEFAULTS.items():
        dev.set_option(k, v)
    try:
        for name, scene, W, H in scenes():
            ds = dev.scene(scene)
            size = ft.ImageSize(W, H)
            out[f"{name} render"] = counters(ds.render(eps, length, size, cam)[1])
            for k, v in VARIED:
                dev.set_option(k, v)
                out[f"{name} render {k}={v}"] = counters(ds.render(eps, length, size, cam)[1])
                dev.set_option(k, DEFAULTS[k])
            for order in ORDERS:
                fresh = ds.relight(scene.BackgroundColor, scene.Lights)   # the same scene with empty tile-order slots: frame 1 records, frame 2 may use the order
                dev.set_option("order", order)
                for frame in (1, 2):
                    out[f"{name} render order={order} frame {frame}"] = counters(fresh.render(eps, length, size, cam)[1])
                dev.set_option("order", DEFAULTS["order"])
                fresh.close()
            out[f"{name} render_views"] = counters(ds.render_views(eps, length, size, [cam, cam2])[1])
            out[f"{name} trace_rays"] = counters(ds.trace_rays(pixel_rays(W, H))[1])
            hits = ds.render_hits(eps, length, size, cam)[0]
            out[f"{name} shade_hits"] = counters(ds.shade_hits(hits)[1])
            out[f"{name} light_visibility"] = counters(ds.light_visibility(hits)[1])
    finally:
        for k, v in DEFAULTS.items():
            dev.set_option(k, v)
    return out


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import fraytracer_amd as ft
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=TABLE)
    args = ap.parse_args()
    dev = ft.Device(0)
    first, second = cells(dev), cells(dev)
    dev.close()
    assert list(first) == list(second)
    left_out = [k for k in first if first[k] != second[k]]
    single = [k for k in left_out if " render" in k and "render_views" not in k]
    for k in left_out:
        print("differs between the two recordings:", k, first[k], second[k])
    table = {
        "header": "counters of small launches as recorded twice on an MI355X from commit %s (tests/golden/make_launch_counters.py)" % args.commit,
        "recorded_from_commit": args.commit,
        "build": ft.build_info(),
        "left_out": left_out,
        "single_camera_render_cells_that_do_not_repeat": single,
        "cells": {k: v for k, v in first.items() if k not in left_out},
    }
    with open(args.out, "w") as f:
        json.dump(table, f, indent=0)
        f.write("\n")
    print(f"{len(first)} cells, {len(left_out)} left out -> {args.out}")


if __name__ == "__main__":
    main()
