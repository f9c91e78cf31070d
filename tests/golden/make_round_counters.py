#!/usr/bin/env python3
"""Generates tests/golden/round_counters.json: the counters of small C3 frames whose runs of children take the paths of the lean kernel's round that the
64-child scenes of launch_counters.json cannot reach — several passes of the culling pass and of the bundle and occlusion certificates, a ragged last
pass, a run longer than the culling pass looks at.  Needs the GPU.

The table pins what those launches counted before the round's fixed cost was cut, so it is recorded from the library of the commit whose behaviour is
to be kept, not from the code under test (FRAYTRACER_HIP_LIB names that library where it is not the one in the tree):

    python tests/golden/make_round_counters.py --commit <commit>

records twice and keeps the cells whose two recordings agree (the others are named in "left_out").  The cells repeat for the reason those of
make_launch_counters.py do — a wave owns one tile between two grabs — and hold the same counters in the same form: sdf_evals moves with every
decision of a certificate or of the culling pass, culled_fraction and tail_fraction (float32 bit patterns) with what the pass drops and with when
the latency mode starts.

tests/test_gpu_round_overhead.py replays cells() against the library in the tree.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_launch_counters as pin  # noqa: E402

TABLE = os.path.join(HERE, "round_counters.json")

DEFAULTS = dict(pin.DEFAULTS, cull=1)
# the columns of make_launch_counters.VARIED that concern the certificates, the culling pass and the latency mode, and the culling pass switched off
VARIED = [(k, v) for k, v in pin.VARIED if k in ("cert", "occl", "cert_policy", "occl_policy", "tail_k")] + [("cull", 0)]


def scenes():
    """(name, scene, W, H): 130 children are three passes with a ragged last one, 257 leave one child behind FT_CULL_MAX = 256, which the evaluation
    takes in full, and 256 at 160^2 are the benchmark's four whole passes on a frame where the certificates bite"""
    from fraytracer_amd import synthetic as syn
    return [("config3(n=130) 96x96", syn.config3(n=130)[0], 96, 96), ("config3(n=257) 96x96", syn.config3(n=257)[0], 96, 96),
            ("config3(n=256) 160x160", syn.config3(n=256)[0], 160, 160)]


def cells(dev):
    """{cell name: counters} of every cell, in a fixed order, on the fraytracer_amd.Device `dev`; leaves its options at DEFAULTS"""
    import fraytracer_amd as ft
    from fraytracer_amd import synthetic as syn
    cam = syn.default_camera()
    out = {}
    for k, v in DEFAULTS.items():
        dev.set_option(k, v)
    try:
        for name, scene, W, H in scenes():
            ds = dev.scene(scene)
            size = ft.ImageSize(W, H)
            out[f"{name} render"] = pin.counters(ds.render(syn.EPSILON, syn.RAY_LENGTH, size, cam)[1])
            for k, v in VARIED:
                dev.set_option(k, v)
                out[f"{name} render {k}={v}"] = pin.counters(ds.render(syn.EPSILON, syn.RAY_LENGTH, size, cam)[1])
                dev.set_option(k, DEFAULTS[k])
            ds.close()
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
    for k in left_out:
        print("differs between the two recordings:", k, first[k], second[k])
    table = {
        "header": "counters of small C3 launches as recorded twice on an MI355X from commit %s (tests/golden/make_round_counters.py)" % args.commit,
        "recorded_from_commit": args.commit,
        "build": ft.build_info(),
        "left_out": left_out,
        "cells": {k: v for k, v in first.items() if k not in left_out},
    }
    with open(args.out, "w") as f:
        json.dump(table, f, indent=0)
        f.write("\n")
    print(f"{len(first)} cells, {len(left_out)} left out -> {args.out}")


if __name__ == "__main__":
    main()
