#!/usr/bin/env python3
"""Generates tests/golden/flatten_constants.json: what ft::flatten (scene.cpp) decides for a corpus of scenes, as far as the C ABI's getters show
it — ft_scene_info_get, the support sphere, the constants of the miss and the occlusion certificate and the certificate's clusters.  No GPU is
needed: the scenes are built on a host-only context.

The table pins the flattener's constants before flatten() was cut into named steps, so it is recorded from the library of the commit whose
behaviour is to be kept, not from the code under test:

    python tests/golden/make_flatten_constants.py --commit <commit>

Floats are kept as their 32-bit patterns (8 hex digits each, vectors as one string).  The named scenes are kept readable; of each fuzz scene
only one SHA-256 over the same record is kept.  fuzz_scene_edge holds the non-finite constants that take the refusal branches.

tests/test_host_flatten.py replays corpus() against the library in the tree.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "flatten_constants.json")

C3_N = (1, 31, 32, 40, 64, 256)
C3_STRENGTH = (0.05, 0.25, 1.0, 2.0)
FUZZ_SEEDS, EDGE_SEEDS = range(200), range(100)


def named():
    """[(name, thunk of the SdfScene)]"""
    from fraytracer_amd import synthetic as syn
    out = [("config1", lambda: syn.config1()[0]), ("config2", lambda: syn.config2()[0]), ("config2(boxes=True)", lambda: syn.config2(boxes=True)[0])]
    for n in C3_N:
        for s in C3_STRENGTH:
            out.append((f"config3(n={n}, strength={s})", lambda n=n, s=s: syn.config3(n=n, strength=s)[0]))
    out += [("config4", lambda: syn.config4()[0]), ("config5", lambda: syn.config5()[0]), ("console_like(n=300)", lambda: syn.console_like(n=300)[0]),
            ("console_scene", lambda: syn.console_scene()[0]), ("mixed_nested", lambda: syn.mixed_nested()[0]),
            ("combinator_zoo", lambda: syn.combinator_zoo()[0]), ("combinator_crowd(n=50)", lambda: syn.combinator_crowd(n=50)[0])]
    return out


def fuzzed():
    from fraytracer_amd import synthetic as syn
    return ([(f"fuzz_scene({s})", lambda s=s: syn.fuzz_scene(s)[0]) for s in FUZZ_SEEDS] +
            [(f"fuzz_scene_edge({s})", lambda s=s: syn.fuzz_scene_edge(s)[0]) for s in EDGE_SEEDS])


def hexbits(values):
    return "".join("%08x" % w for w in np.asarray(list(values), np.float32).reshape(-1).view(np.uint32))


def record(host, make):
    """everything the getters show of one scene; a scene the library refuses is recorded by its message"""
    import fraytracer_amd as ft
    try:
        ds = host.scene(make())
    except ft.FrayTracerError as e:
        return {"refused": str(e)}
    clusters, members = ds.miss_certificate_clusters()
    out = {"info": ds.info(),
           "support_sphere": hexbits(ds.support_sphere()),
           "miss_certificate": {k: hexbits([v]) for k, v in ds.miss_certificate().items()},
           "occlusion_certificate": {k: hexbits([v]) for k, v in ds.occlusion_certificate().items()},
           "clusters": [hexbits(c) for c in clusters],
           "cluster_members": [hexbits(m) for m in members]}
    ds.close()
    return out


def digest(rec):
    return hashlib.sha256(json.dumps(rec, sort_keys=True).encode()).hexdigest()


def corpus(host):
    """({name: record} of the named scenes, {name: SHA-256 of the record} of the fuzz scenes) on the host-only fraytracer_amd.Device `host`"""
    return ({name: record(host, make) for name, make in named()}, {name: digest(record(host, make)) for name, make in fuzzed()})


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import fraytracer_amd as ft
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    args = ap.parse_args()
    host = ft.Device(-1)
    scenes, fuzz = corpus(host)
    host.close()
    table = {"header": "what ft::flatten decided as recorded from commit %s (tests/golden/make_flatten_constants.py)" % args.commit,
             "recorded_from_commit": args.commit, "scenes": scenes, "fuzz_sha256": fuzz}
    with open(TABLE, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    refused = [k for k, v in scenes.items() if "refused" in v]
    print(f"{len(scenes)} named scenes ({len(refused)} refused), {len(fuzz)} fuzz scenes -> {TABLE}")


if __name__ == "__main__":
    main()
