#!/usr/bin/env python3
"""Generates tests/golden/refusal_matrix.json: the status every render and ray-buffer entry point returns for a fixed grid of refused
calls, on a host-only context (ft_ctx_create(-1)) and with a NULL context.  No GPU is needed and no buffer is ever dereferenced: every
call is refused, the scene is NULL throughout and the buffer "addresses" are plain integers.

The table pins the ORDER of the argument checks (which of FT_ERR_INVALID, FT_ERR_NO_DEVICE and FT_ERR_UNSUPPORTED wins), so it is recorded
from the library of the commit whose behaviour is to be kept, not from the code under test:

    git worktree add /tmp/base <commit> && make -C /tmp/base/fraytracer_amd/csrc
    python tests/golden/make_refusal_matrix.py --lib /tmp/base/fraytracer_amd/libfraytracer_hip.so --commit <commit>

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
TABLE = os.path.join(HERE, "refusal_matrix.json")

# one character per call
CODES = {0: "O", -1: "I", -2: "N", -3: "H", -4: "U"}       # FT_OK, FT_ERR_INVALID, FT_ERR_NO_DEVICE, FT_ERR_HIP, FT_ERR_UNSUPPORTED

# Output slots: "w" a buffer of 4-byte words (image, material plane, SdfForm.tryTrace results), "r" 64-byte records (16-byte aligned).
# Addresses by state: absent; aligned (a word buffer only as far as it has to be: 4 but not 16 bytes); misaligned (a record buffer at 8 bytes:
# good enough for words, not for records).
ADDR = {"w": (None, 0x10004, 0x10002), "r": (None, 0x20000, 0x20008)}
RAYS = (None, 0x40000, 0x40008)                                  # NULL, aligned, 8 bytes off (device forms want 16)
VIEWS = (-1, 0, 1, 2, 65)
SPP = (1, 3)                                                     # 3 is not a square: refused by the parameter check
RAY_COUNTS = (-1, 0, 5, 0xFFFF0000)

# entry point -> (kind, views?, output slots, stats?)
FRAMES = {
    "ft_render": (False, "w", True), "ft_render_device": (False, "w", False),
    "ft_render_hits": (False, "wrw", True), "ft_render_hits_device": (False, "wrw", False),
    "ft_render_views": (True, "w", True), "ft_render_views_device": (True, "w", False),
    "ft_render_views_hits": (True, "wrw", True), "ft_render_views_hits_device": (True, "wrw", False),
}
RAY_FORMS = {
    "ft_trace_rays": ("w", True), "ft_trace_rays_device": ("w", False),
    "ft_form_try_trace": ("w", True), "ft_form_try_trace_device": ("w", False),
    "ft_object_try_trace": ("r", True), "ft_object_try_trace_device": ("rw", False),
    "ft_trace_rays_hits": ("wrw", True), "ft_trace_rays_hits_device": ("wrw", False),
}
# the 2^32 job limit: (width = height, spp, views).  4096^2 at spp 64 is 2^30 jobs a view; hits only trace one ray per pixel, whatever spp says
JOB_LIMIT = [(4096, 64, 3), (4096, 64, 4), (4096, 64, 8), (4096, 1, 255), (4096, 1, 256), (64, 64, 16383), (64, 64, 16384),
             (8192, 64, 1), (8192, 16, 1), (8192, 16, 3), (8192, 16, 4), (8192, 1, 63), (8192, 1, 64)]
JOB_LIMIT_OUTPUTS = [(1, 0, 0), (1, 1, 1), (0, 1, 0), (0, 0, 1), (1, 0, 1)]      # states of (image, records, material plane)


def cases():
    """[(entry point, description)]: description = dict(ctx, and for frames cam, params (None or (size, spp)), n, outs; for ray buffers rays, n, outs)"""
    out = []
    for name, (views, slots, _) in FRAMES.items():
        for ctx, cam, par, spp, n, outs in itertools.product((1, 0), (1, 0), (1, 0), SPP, VIEWS if views else (1,), itertools.product(range(3), repeat=len(slots))):
            out.append((name, dict(ctx=ctx, cam=cam, params=(8, spp) if par else None, n=n, outs=outs)))
        for (size, spp, n), outs in itertools.product(JOB_LIMIT, JOB_LIMIT_OUTPUTS):
            if len(slots) == 1 and outs != (1, 0, 0):
                continue
            for ctx in (1, 0):
                out.append((name, dict(ctx=ctx, cam=1, params=(size, spp), n=n, outs=outs[:len(slots)])))
    for name, (slots, _) in RAY_FORMS.items():
        for ctx, rays, n, outs in itertools.product((1, 0), range(3), RAY_COUNTS, itertools.product(range(3), repeat=len(slots))):
            out.append((name, dict(ctx=ctx, rays=rays, n=n, outs=outs)))
    return out


def run(_lib):
    """the status character of every case, in cases() order, per entry point: {name: "INNU..."}"""
    L = _lib.lib
    ctx = C.c_void_p()
    _lib.check(L.ft_ctx_create(-1, C.byref(ctx)))
    cams = (_lib.CameraS * max(max(VIEWS), max(n for _, _, n in JOB_LIMIT)))()
    st = _lib.Stats()
    rows = {}
    try:
        for name, d in cases():
            fn = getattr(L, name)
            c = ctx if d["ctx"] else None
            if name in FRAMES:
                views, slots, stats = FRAMES[name]
                p = None
                if d["params"]:
                    size, spp = d["params"]
                    p = C.byref(_lib.RenderParams(size, size, 0, size, size, 1, 0, spp, 0.01, 100.0, 0, 0.0, 0, 0))
                args = [c, None, cams if d["cam"] else None] + ([d["n"]] if views else []) + [p]
            else:
                slots, stats = RAY_FORMS[name]
                args = [c, None, RAYS[d["rays"]], d["n"]]
            args += [ADDR[k][s] for k, s in zip(slots, d["outs"])] + ([C.byref(st)] if stats else [])
            rows[name] = rows.get(name, "") + CODES[fn(*args)]
    finally:
        L.ft_ctx_destroy(ctx)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", required=True, help="libfraytracer_hip.so built from the commit whose behaviour is recorded")
    ap.add_argument("--commit", required=True, help="that commit (noted in the table)")
    a = ap.parse_args()
    os.environ["FRAYTRACER_HIP_LIB"] = os.path.abspath(a.lib)
    sys.path.insert(0, ROOT)
    from fraytracer_amd import _lib
    rows = run(_lib)
    n = sum(len(r) for r in rows.values())
    with open(TABLE, "w") as f:
        json.dump({"recorded_from_commit": a.commit, "build": _lib.build_info()["src"], "calls": n,
                   "codes": {v: k for k, v in CODES.items()}, "rows": rows}, f, indent=1)
        f.write("\n")
    print(f"{TABLE}: {n} calls, " + ", ".join(f"{sum(r.count(ch) for r in rows.values())} x {ch}" for ch in "INUOH"))


if __name__ == "__main__":
    main()
