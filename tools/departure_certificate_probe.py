#!/usr/bin/env python3
"""Departure certificate on the C3 frame (FT_OPT_DEPART, include/fraytracer_hip.h; scene.cpp "Departure certificate"): HIP-event kernel ms per frame
through Scene.render_device for a still camera, one row per schedule, the rows alternated over several rounds in one call.  Every timed run follows
three untimed frames, so the rows on word 0 are hint-following frames.  Rows on an explicit FT_OPT_CERT_POLICY word follow no hint (an explicit word
never does): they compare schedules of the tilted tries with one another and with the flat margin on the same word, not with the shipped frame.
The frame of every row is compared with the first row's, on the device, bit for bit.
Usage: departure_certificate_probe.py [--size 4096] [--spheres 256] [--rounds 3] [--frames 4] [--tag TEXT]"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import fraytracer_amd as ft
from fraytracer_amd import synthetic as syn

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--spheres", type=int, default=256)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--frames", type=int, default=4)
ap.add_argument("--tag", default="")
args = ap.parse_args()


def word(shadow, lanes, repeat):
    """FT_OPT_CERT_POLICY: primary rays never, shadow rays due from `shadow` steps, `lanes` due lanes, again `repeat` steps after a failure; bundle as shipped"""
    return 255 | shadow << 8 | lanes << 16 | repeat << 24


ROWS = (("word 0, depart 0 (hinted, the parent's frame)", 0, 0), ("word 0, depart 1 (shipped)", 0, 1),
        ("birth only, 8 lanes, tilted", word(1, 8, 0), 2), ("birth only, 16 lanes, tilted", word(1, 16, 0), 2), ("birth + repeat 2, 8 lanes, tilted", word(1, 8, 2), 2),
        ("birth + repeat 2, 1 lane, tilted", word(1, 1, 2), 2), ("birth + repeat 2, 16 lanes, tilted", word(1, 16, 2), 2),
        ("birth + repeat 1, 16 lanes, tilted", word(1, 16, 1), 2), ("birth + repeat 3, 16 lanes, tilted", word(1, 16, 3), 2),
        ("birth + repeat 4, 16 lanes, tilted", word(1, 16, 4), 2), ("birth + repeat 2, 32 lanes, tilted", word(1, 32, 2), 2),
        ("step 2 + repeat 2, 16 lanes, tilted", word(2, 16, 2), 2),
        ("birth + repeat 2, 8 lanes, flat margin", word(1, 8, 2), 0), ("no per-lane tries, unhinted", word(255, 16, 6), 0))
PRE = 3

dev = ft.Device(0)
scene = syn.config3(n=args.spheres, size=args.size)[0]
size = ft.ImageSize(args.size, args.size)
buf = torch.empty((args.size, args.size, 3), dtype=torch.float32, device="cuda")
ref = torch.empty_like(buf)
cam = syn.default_camera()
ds = dev.scene(scene)
ds.render_device(syn.EPSILON, syn.RAY_LENGTH, size, cam, buf.data_ptr()); ds.collect_stats()                    # warm-up
kms, last, same = {r[0]: [] for r in ROWS}, {}, {r[0]: True for r in ROWS}
for _ in range(args.rounds):
    for i, (name, policy, depart) in enumerate(ROWS):
        dev.set_option("cert_policy", policy); dev.set_option("depart", depart)
        for _ in range(PRE):
            ds.render_device(syn.EPSILON, syn.RAY_LENGTH, size, cam, buf.data_ptr())
        ds.collect_stats()
        for _ in range(args.frames):
            ds.render_device(syn.EPSILON, syn.RAY_LENGTH, size, cam, buf.data_ptr())
        st = ds.collect_stats()                                       # waits for the stream
        kms[name].append(st["kernel_ms"] / args.frames)
        last[name] = st
        if i == 0:
            ref.copy_(buf)
            torch.cuda.synchronize()                                  # the copy runs on another stream than the frames
        else:
            same[name] = same[name] and bool(torch.equal(buf.view(torch.int32), ref.view(torch.int32)))
dev.set_option("cert_policy", 0); dev.set_option("depart", 1)
for name, policy, depart in ROWS:
    st = last[name]
    print(json.dumps({"build": args.tag, "scene": f"C3 n={args.spheres} {args.size}^2", "row": name, "cert_policy": policy, "depart": depart,
                      "kernel_ms_median": round(statistics.median(kms[name]), 3), "kernel_ms_runs": [round(x, 3) for x in kms[name]],
                      "sdf_evals_per_frame": st["sdf_evals"] // args.frames, "wave_rounds_per_frame": st["wave_evals"] // args.frames,
                      "same_frame_as_first_row": same[name], "flags": st["flags"], "shader_mhz": round(st["shader_mhz"], 1)}), flush=True)
ds.close()
dev.close()
