#!/usr/bin/env python3
"""Light visibility masks (ft_light_visibility_device, ft_shade_visible_device).  Prints one JSON line (profiles/light_visibility_probe.jsonl).

The reference's own scene (Program.fs) and C3 at N x N (N = 1024 and 4096) under the relit lights of tests/test_gpu_shade_hits.py; the records
are those ft_render_hits_device wrote for the scene as it was.

  marches  kernel time of ONE light_visibility_device over the frame's records with every light selected, and of shade_hits_device on the same
           records in the same process: the same marches.  (The parent tree's figure is tools/shade_hits_probe.py run there: alternate.)
  one      the same with select = 1 << j for each light j, with the shadow rays cast beside the time.
  stream   kernel time of ONE shade_visible_device (80 B per record: 64 + 4 read, 12 written) and, as the yardstick, a device-to-device copy
           that moves the same 80 B per record (40 B read + 40 B written), in the same process; the colours are compared with the relit
           scene's render_device (same bits).
  render   kernel time of render_device of the relit scene: what a recolour costs without masks.

Medians over RUNS after WARMUP, with the range.  Not the contract bench (that is bench.py)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import fraytracer_amd as ft
from fraytracer_amd import synthetic as syn

WARMUP, RUNS = 2, 7
EPS, LEN = syn.EPSILON, syn.RAY_LENGTH
BG = (0.02, 0.03, 0.05)
LIGHTS = (ft.SdfLight.directional((0.6, -1.0, -0.3), (0.9, 0.8, 0.7)), ft.SdfLight.point((3.0, 4.0, -6.0), (30.0, 40.0, 50.0)),
          ft.SdfLight.directional((0.0, 1.0, 0.2), (0.3, 0.3, 0.3)))


def stat(ms):
    return {"median_ms": round(statistics.median(ms), 4), "range_ms": [round(min(ms), 4), round(max(ms), 4)], "runs_ms": [round(v, 4) for v in ms]}


def timed(ds, launch):
    """kernel ms of WARMUP + RUNS launches, one collect_stats each -> (times of the runs, the last statistics)"""
    ms = []
    for i in range(WARMUP + RUNS):
        launch()
        st = ds.collect_stats()
        if i >= WARMUP:
            ms.append(st["kernel_ms"])
    return ms, st


def copy_case(n_bytes):
    src = torch.empty(n_bytes // 4, dtype=torch.int32, device="cuda").random_()
    dst = torch.empty_like(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for i in range(WARMUP + RUNS):
        e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
        if i >= WARMUP:
            ms.append(e0.elapsed_time(e1))
    return ms


def case_of(dev, scene, n, cam):
    ds = dev.scene(scene)
    relit = ds.relight(BG, LIGHTS)
    px = n * n
    rec = torch.full((n, n, 16), float("nan"), dtype=torch.float32, device="cuda")
    want = torch.full((n, n, 3), float("nan"), dtype=torch.float32, device="cuda")
    out = torch.full((n, n, 3), float("nan"), dtype=torch.float32, device="cuda")
    vis = torch.full((n, n), -1, dtype=torch.int32, device="cuda")
    one = torch.full((n, n), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ds.render_hits_device(EPS, LEN, ft.ImageSize(n, n), cam, rec.data_ptr())
    ds.collect_stats()
    res = {"hit_fraction": round(float((rec[..., 14].view(torch.int32) != 0).float().mean().item()), 3), "fast_path": relit.info()["fast_path"]}
    ms, st = timed(relit, lambda: relit.render_device(EPS, LEN, ft.ImageSize(n, n), cam, want.data_ptr()))
    res["render"] = {"render_device_kernel": stat(ms), "rays_shadow": st["rays_shadow"], "sdf_evals": st["sdf_evals"]}
    ms, st = timed(relit, lambda: relit.shade_hits_device(rec.data_ptr(), px, out.data_ptr()))
    res["shade_hits"] = {"shade_hits_device_kernel": stat(ms), "rays_shadow": st["rays_shadow"], "sdf_evals": st["sdf_evals"]}
    ms, sv = timed(relit, lambda: relit.light_visibility_device(rec.data_ptr(), px, vis.data_ptr()))
    res["marches"] = {"light_visibility_device_kernel": stat(ms), "rays_shadow": sv["rays_shadow"], "hits_shadow": sv["hits_shadow"], "sdf_evals": sv["sdf_evals"],
                      "same_counters_as_shade_hits": all(sv[k] == st[k] for k in ("rays_shadow", "hits_shadow", "flags", "rays_primary"))}
    res["one"] = []
    for j in range(len(LIGHTS)):
        ms, so = timed(relit, lambda: relit.light_visibility_device(rec.data_ptr(), px, one.data_ptr(), 1 << j))
        res["one"].append({"light": j, "light_visibility_device_kernel": stat(ms), "rays_shadow": so["rays_shadow"], "sdf_evals": so["sdf_evals"],
                           "same_bit_as_all": bool(torch.equal(one, vis & (1 << j)))})
    out.fill_(float("nan")); torch.cuda.synchronize()
    ms, ss = timed(relit, lambda: relit.shade_visible_device(rec.data_ptr(), vis.data_ptr(), px, out.data_ptr()))
    cp = copy_case(40 * px)
    med, cmed = statistics.median(ms), statistics.median(cp)
    res["stream"] = {"shade_visible_device_kernel": stat(ms), "bytes": 80 * px, "gb_per_s": round(80 * px / med / 1e6, 1),
                     "copy_40B_in_40B_out": stat(cp), "copy_gb_per_s": round(80 * px / cmed / 1e6, 1), "shade_visible_over_copy": round(med / cmed, 3),
                     "same_bits_as_render": bool(torch.equal(out.view(torch.int32), want.view(torch.int32))), "sdf_evals": ss["sdf_evals"]}
    res["render_over_shade_visible"] = round(res["render"]["render_device_kernel"]["median_ms"] / med, 1)
    relit.close(); ds.close()
    return res


ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
args = ap.parse_args()
dev = ft.Device(0)
cam = syn.default_camera()
res = {"probe": "light_visibility", "build": ft.build_info()["src"], "device": torch.cuda.get_device_name(0), "warmup": WARMUP, "runs": RUNS, "cases": []}
for name, scene in (("Program.fs scene", syn.console_scene()[0]), ("C3 smooth256", syn.config3()[0])):
    for n in args.sizes:
        case = {"scene": name, "frame": n}
        case.update(case_of(dev, scene, n, cam))
        res["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
dev.close()
print(json.dumps(res))
