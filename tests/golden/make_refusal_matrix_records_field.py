#!/usr/bin/env python3
"""Generates tests/golden/refusal_matrix_records_field.json: the status and the message of the record forms (ft_shade_hits, ft_light_visibility,
ft_shade_visible), the field forms (ft_sample_points, ft_sample_lattice), each with its *_device form, and ft_eval_distance, for a fixed grid of
calls on a host-only context (ft_ctx_create(-1)) and with a NULL context.  No GPU is needed and no buffer is ever dereferenced: every call is
refused or has nothing to do (n = 0), and the buffer "addresses" are plain integers.  Beside refusal_matrix.json, which covers the sixteen render
and ray-buffer entry points (make_refusal_matrix.py).

The table pins the ORDER of the argument checks and the TEXT of every refusal, so it is recorded from the library of the commit whose behaviour is
to be kept, not from the code under test:

    git worktree add /tmp/base <commit> && make -C /tmp/base/fraytracer_amd/csrc
    python tests/golden/make_refusal_matrix_records_field.py --lib /tmp/base/fraytracer_amd/libfraytracer_hip.so --commit <commit>

tests/test_refusal_matrix.py replays the same grid (cases() below) against the library in the tree.
"""
import argparse
import ctypes as C
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, "refusal_matrix_records_field.json")

CODES = {0: "O", -1: "I", -2: "N", -3: "H", -4: "U"}       # FT_OK, FT_ERR_INVALID, FT_ERR_NO_DEVICE, FT_ERR_HIP, FT_ERR_UNSUPPORTED

CTXS = ("own", None)                                       # the host-only context, NULL
SCENES = ("own", "lights33", None, "other")                # the context's scene, its scene under 33 lights, NULL, a scene of another context
IN = 0x40000
INPUTS = (None, IN, IN + 8, IN + 2)                        # NULL, 16-byte aligned, 8 off, 2 off
COUNTS = (-1, 0, 5, 0xFFFF0000)
SELECTS = (0, 1, 0xFFFFFFFF)
FLAGS = (0, 1, 2)                                          # none, FT_FIELD_BOUNDED, an unknown bit
LATTICES = (None, (2, 3, 4), (2, 0, 4), (16777217, 1, 1), (65536, 65535, 1), (65535, 65535, 1))     # the fifth has exactly 0xFFFF0000 points


def slot_address(i, k, state):
    """Output (or mask) slot i of k: NULL; 4-byte aligned; 2 off; the input's aligned address; the aligned address of the next slot"""
    own = 0x10004 + 0x1000 * i
    return {"null": None, "ok": own, "off2": own - 2, "input": IN, "other": 0x10004 + 0x1000 * ((i + 1) % k)}[state]


def slot_states(k, has_input=True):
    return ["null", "ok", "off2"] + (["input"] if has_input else []) + (["other"] if k > 1 else [])


# entry point -> (kind, slots, stats?).  slots: the output and mask arguments in the C call's order, after the input.
FORMS = {
    "ft_shade_hits": ("shade", 1, True), "ft_shade_hits_device": ("shade", 1, False),
    "ft_light_visibility": ("vis", 2, True), "ft_light_visibility_device": ("vis", 2, False),           # vis_in, vis_out
    "ft_shade_visible": ("visible", 2, True), "ft_shade_visible_device": ("visible", 2, False),         # visibility, out_rgb
    "ft_sample_points": ("points", 3, False), "ft_sample_points_device": ("points", 3, False),          # distance, normal, material
    "ft_sample_lattice": ("lattice", 3, False), "ft_sample_lattice_device": ("lattice", 3, False),
    "ft_eval_distance": ("eval", 2, False),                                                                # out_distance, out_material
}


def cases():
    """[(entry point, dict(ctx, scene, inp | lat, n, outs, select, flags))].  Two grids per entry point, not their cross product: who is asked
    (context x scene x count x input, every slot absent or every slot sound), and what the buffers are (every state of every slot x count x input,
    on the context's own scenes)."""
    out = []
    for name, (kind, k, _) in FORMS.items():
        lattice = kind == "lattice"
        extra = SELECTS if kind == "vis" else FLAGS if kind in ("points", "lattice") else (0,)
        what = LATTICES if lattice else INPUTS
        counts = (0,) if lattice else COUNTS
        for ctx, scene, n, w, x, state in itertools.product(CTXS, SCENES, counts, what, extra, ("null", "ok")):
            out.append((name, dict(ctx=ctx, scene=scene, n=n, what=w, extra=x, outs=(state,) * k)))
        scenes = ("own", "lights33") if kind in ("vis", "visible", "shade") else ("own",)
        for scene, n, w, outs in itertools.product(scenes, counts, what, itertools.product(slot_states(k, not lattice), repeat=k)):
            out.append((name, dict(ctx="own", scene=scene, n=n, what=w, extra=extra[-1] if kind == "vis" else 0, outs=outs)))
    return out


def run(_lib):
    """(rows, messages): per entry point the status character of every case in cases() order and, beside it, the index of the call's
    ft_last_error text in `messages` (-1: the call was not refused)"""
    import fraytracer_amd as ft
    from fraytracer_amd import synthetic as syn
    L = _lib.lib
    host, stranger = ft.Device(-1), ft.Device(-1)
    own = host.scene(syn.config3(n=8)[0])
    lights = [ft.SdfLight.directional((0.1 * i - 1.0, -1.0, 0.3), (1.0, 1.0, 1.0)) for i in range(33)]
    scenes = {"own": own._scene, "lights33": own.relight((0.0, 0.0, 0.0), lights)._scene, None: None,
              "other": stranger.scene(syn.config3(n=8)[0])._scene}
    st = _lib.Stats()
    rows = {name: {"status": [], "message": []} for name in FORMS}
    messages = []
    try:
        for name, d in cases():
            kind, k, stats = FORMS[name]
            outs = [slot_address(i, k, s) for i, s in enumerate(d["outs"])]
            head = [host._ctx if d["ctx"] else None, scenes[d["scene"]]]
            if kind == "lattice":
                lat = d["what"] and C.byref(_lib.Lattice(_lib.Vec3(0, 0, 0), _lib.Vec3(1, 1, 1), *d["what"]))
                args = head + [lat, 0.01, d["extra"]] + outs
            elif kind == "points":
                args = head + [d["what"], d["n"], 0.01, d["extra"]] + outs
            elif kind == "vis":
                args = head + [d["what"], d["n"], d["extra"]] + outs
            elif kind == "visible":
                args = head + [d["what"], outs[0], d["n"], outs[1]]
            else:                                                      # shade, eval
                args = head + [d["what"], d["n"]] + outs
            rc = getattr(L, name)(*args + ([C.byref(st)] if stats else []))
            rows[name]["status"].append(CODES[rc])
            if rc == 0:
                rows[name]["message"].append(-1)
                continue
            text = _lib.last_error()
            if text not in messages:
                messages.append(text)
            rows[name]["message"].append(messages.index(text))
    finally:
        host.close()
        stranger.close()
    return {n: {"status": "".join(r["status"]), "message": r["message"]} for n, r in rows.items()}, messages


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", required=True, help="libfraytracer_hip.so built from the commit whose behaviour is recorded")
    ap.add_argument("--commit", required=True, help="that commit (noted in the table)")
    a = ap.parse_args()
    os.environ["FRAYTRACER_HIP_LIB"] = os.path.abspath(a.lib)
    sys.path.insert(0, ROOT)
    from fraytracer_amd import _lib
    rows, messages = run(_lib)
    n = sum(len(r["status"]) for r in rows.values())
    with open(TABLE, "w") as f:
        json.dump({"recorded_from_commit": a.commit, "build": _lib.build_info()["src"], "calls": n,
                   "codes": {v: k for k, v in CODES.items()}, "messages": messages, "rows": rows}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{TABLE}: {n} calls, {len(messages)} messages, " + ", ".join(f"{sum(r['status'].count(ch) for r in rows.values())} x {ch}" for ch in "INUOH"))


if __name__ == "__main__":
    main()
