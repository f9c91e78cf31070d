#!/usr/bin/env python3
"""Try hints on the C3 frame (FT_OPT_TRY_HINT, include/fraytracer_hip.h; kernels.hip "Try hints"): HIP-event kernel ms per frame through
Scene.render_device for a still camera and for cameras turned about their position by 1, 8 and 64 pixels' worth of rotation per frame (back and forth
over eight steps, so that the cloud stays in the frame), each with the option 0 (off), 1 (on) and 2 (record only), the options alternated over several
rounds in one call.  Every timed run follows three untimed frames of the same motion.  The frame of every (motion, option) pair is compared with the
one option 0 gave for the same camera, on the device, bit for bit.
Then the convergence of a still camera: kernel ms, sdf_evals and evaluation rounds of frames 1 .. 6 of a fresh scene, per option.
Usage: try_hint_probe.py [--size 4096] [--spheres 256] [--rounds 3] [--frames 4] [--tag TEXT]"""
import argparse, json, math, os, statistics, sys
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

PIXEL = 2.0 * math.tan(math.radians(30.0)) / args.size            # the angle of one pixel at the frame's centre (60-degree lens)
MOTIONS = (("still", 0), ("1 px", 1), ("8 px", 8), ("64 px", 64))
OPTIONS = (0, 1, 2)
PRE = 3

dev = ft.Device(0)
scene = syn.config3(n=args.spheres, size=args.size)[0]
size = ft.ImageSize(args.size, args.size)
buf = torch.empty((args.size, args.size, 3), dtype=torch.float32, device="cuda")
ref = torch.empty_like(buf)


def camera(k, px):
    """the Program.fs camera turned about its position by px pixels' worth per frame, frame k of a sweep that turns back after eight steps"""
    t = k % 16
    a = (t if t <= 8 else 16 - t) * px * PIXEL
    return ft.Camera.lookAt(Position=(0.0, 0.0, -10.0), LookAt=(10.0 * math.sin(a), 0.0, -10.0 + 10.0 * math.cos(a)), Up=(0.0, 1.0, 0.0), Lens=ft.Lens.create(60.0))


def frame(ds, cam, out=buf):
    ds.render_device(syn.EPSILON, syn.RAY_LENGTH, size, cam, out.data_ptr())


ds = dev.scene(scene)
frame(ds, camera(0, 0)); ds.collect_stats()                       # warm-up
for name, px in MOTIONS:
    kms, last, same = {o: [] for o in OPTIONS}, {}, {o: True for o in OPTIONS}
    for _ in range(args.rounds):
        for o in OPTIONS:
            dev.set_option("try_hint", o)
            for k in range(PRE):
                frame(ds, camera(k, px))
            ds.collect_stats()
            for k in range(PRE, PRE + args.frames):
                frame(ds, camera(k, px))
            st = ds.collect_stats()                               # waits for the stream
            kms[o].append(st["kernel_ms"] / args.frames)
            last[o] = st
            if o == 0:
                ref.copy_(buf)
                torch.cuda.synchronize()                          # the copy runs on another stream than the frames
            else:
                same[o] = same[o] and bool(torch.equal(buf.view(torch.int32), ref.view(torch.int32)))
    for o in OPTIONS:
        st = last[o]
        print(json.dumps({"build": args.tag, "scene": f"C3 n={args.spheres} {args.size}^2", "camera": name, "try_hint": o,
                          "kernel_ms_median": round(statistics.median(kms[o]), 3), "kernel_ms_runs": [round(x, 3) for x in kms[o]],
                          "sdf_evals_per_frame": st["sdf_evals"] // args.frames, "wave_rounds_per_frame": st["wave_evals"] // args.frames,
                          "same_frame_as_option_0": same[o], "flags": st["flags"], "shader_mhz": round(st["shader_mhz"], 1)}), flush=True)
ds.close()

for o in OPTIONS:                                                 # convergence: a fresh scene has no hints
    dev.set_option("try_hint", o)
    ds = dev.scene(scene)
    rows = []
    for k in range(6):
        frame(ds, camera(0, 0))
        st = ds.collect_stats()
        rows.append({"frame": k + 1, "kernel_ms": round(st["kernel_ms"], 3), "sdf_evals": st["sdf_evals"], "wave_rounds": st["wave_evals"]})
    print(json.dumps({"build": args.tag, "convergence": "still camera, fresh scene", "try_hint": o, "frames": rows}), flush=True)
    ds.close()
dev.set_option("try_hint", 1)
dev.close()
