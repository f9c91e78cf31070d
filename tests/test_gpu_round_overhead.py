"""The fixed part of the lean kernel's round (kernels.hip: the culling pass, the certificates' wave maxima, the sphere regime) on runs of children that the
64-child scenes of the launch-rule table cannot reach: three passes with a ragged last one (130 children), a child behind FT_CULL_MAX (257) and the
benchmark's four whole passes (256, at 160 x 160 where the certificates bite).  A change there may move no decision: every launch counts what the
parent commit counted (tests/golden/round_counters.json, recorded from it by tests/golden/make_round_counters.py) and every frame is the CPU
oracle's bit for bit."""
import json
import os
import sys

import numpy as np
import pytest

from fraytracer_amd import synthetic as syn
import fraytracer_amd as ft
from helpers import COUNTERS, assert_bit_equal, check_counts, options, options_left_at_defaults  # noqa: F401  (options_left_at_defaults: a fixture)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_launch_counters  # noqa: E402
import make_round_counters as pin  # noqa: E402

pytestmark = pytest.mark.gpu

EPS, LEN = syn.EPSILON, syn.RAY_LENGTH
SCENES = {name: (scene, w, h) for name, scene, w, h in pin.scenes()}
_WANT = {}


def wanted(oracle, name):
    """the oracle's (frame, counters) of a scene under the default camera: computed once, shared, never written to"""
    if name not in _WANT:
        scene, w, h = SCENES[name]
        with np.errstate(all="ignore"):
            frame, cnt = oracle.Oracle().scene(scene).render(EPS, LEN, w, h, syn.default_camera().as_array(), nthreads=16)
        frame.setflags(write=False)
        _WANT[name] = (frame, cnt)
    return _WANT[name]


def test_rounds_count_what_the_parent_counted(gpu):
    """every cell of the table — the defaults and one option at a time among cert, occl, the certificate and occlusion schedules (the bundle in every
    round among them), tail_k and cull — on the three scenes: rays, hits, sdf_evals, flags, culled_fraction and tail_fraction as recorded"""
    table = json.load(open(pin.TABLE))
    assert table["recorded_from_commit"] == "dda1776"                  # the parent of the change: not the code under test
    assert table["left_out"] == [] and len(table["cells"]) == 3 * (1 + len(pin.VARIED))
    got = pin.cells(gpu)
    assert list(got) == list(table["cells"])
    for name, want in table["cells"].items():
        print(name, got[name])
        assert got[name] == want, name


@pytest.mark.parametrize("name", list(SCENES))
def test_frames_are_the_oracles(gpu, oracle, name):
    scene, w, h = SCENES[name]
    want, cnt = wanted(oracle, name)
    assert 0 < cnt["hits_primary"] < w * h and 0 < cnt["hits_shadow"] < cnt["rays_shadow"]
    ds = gpu.scene(scene)
    assert ds.info()["fast_path"] == 1                                 # the lean kernel
    got, st = ds.render(EPS, LEN, ft.ImageSize(w, h), syn.default_camera())
    ds.close()
    assert_bit_equal(got, want, name)
    check_counts(st, cnt)
    assert 0.0 < st["culled_fraction"] < 1.0                           # the culling pass ran and dropped some, not all


def test_bundle_every_round_stops_failing_tries_early(gpu, oracle):
    """the bundle certificate tried in every round, on the frame where it bites: most of those tries fail, and the lean kernel leaves a failing
    try after the pass that shows it (tests/test_bundle_early_exit.py: why that moves nothing).  The launch counts what the parent, which ran
    every try to its end, counted under the same word, and the frame is the oracle's"""
    name = "config3(n=256) 160x160"
    scene, w, h = SCENES[name]
    word = make_launch_counters.s32(make_launch_counters.SHIPPED_LANES | (1 << 30))
    want_counters = json.load(open(pin.TABLE))["cells"][f"{name} render cert_policy={word}"]
    want, cnt = wanted(oracle, name)
    ds = gpu.scene(scene)
    with options(gpu, cert_policy=word):
        got, st = ds.render(EPS, LEN, ft.ImageSize(w, h), syn.default_camera())
    ds.close()
    assert make_launch_counters.counters(st) == want_counters
    assert_bit_equal(got, want, "bundle every round")
    check_counts(st, cnt)


def test_one_wave_with_two_epsilons(gpu, oracle):
    """a ray buffer whose waves are hand-made: the 64 rays of an 8 x 8 pixel tile each, epsilon 0.005 and 0.02 in alternating lanes.  The bundle
    certificate holds its sum against the threshold of the strictest member — the wave maximum of epsilon — so a wave whose lanes differ must end
    its rays where the oracle's marches end, ray by ray"""
    scene = SCENES["config3(n=256) 160x160"][0]
    rays = make_launch_counters.pixel_rays(160, 160).reshape(160, 160, 8)
    tiles = [rays[x:x + 8, y:y + 8].reshape(64, 8) for x in range(0, 160, 8) for y in (0, 40, 72, 112, 152)]     # off the blob, at its rim, across it
    buf = np.concatenate(tiles).astype(np.float32)
    buf[0::2, 7] = 0.005
    buf[1::2, 7] = 0.02
    with np.errstate(all="ignore"):
        want, cnt = oracle.Oracle().scene(scene).trace_rays(buf)
    assert cnt["flags"] == 0 and 0 < cnt["hits_primary"] < len(buf)
    ds = gpu.scene(scene)
    got, st = ds.trace_rays(buf)
    ds.close()
    assert_bit_equal(got, want, "two epsilons in one wave")
    for k in COUNTERS[1:]:
        assert st[k] == cnt[k], (k, st[k], cnt[k])
