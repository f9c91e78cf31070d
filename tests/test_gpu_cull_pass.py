"""The culling pass ft_cull_children (kernels.hip "Exact child culling") in both wordings — HELD = false, the general loop of the general trace
kernels and the field kernels, and HELD = true, the lean trace kernel's passes — run by the internal probe ft_selftest_cull on the same points under
the same lane masks: whole, ragged, a single lane.  The wordings must agree bit for bit; idle lanes must not matter; the survivors are the scene's own
records in list order; and the pass's contract holds in float64 with nothing added to the rule's own margins: a dropped child's term is at most half an
ulp of the running sum in front of it at every active point of the wave."""
import ctypes as C

import numpy as np
import pytest

from fraytracer_amd import _lib
from helpers import options_left_at_defaults  # noqa: F401  (fixture)

import cull_cases as cc

pytestmark = pytest.mark.gpu

F = np.float32
L = _lib.lib
NONE, NOCLAMP, ROW = 0xffffffff, 0x10000, 4 * cc.CULL_MAX                                 # kernels.hip FT_CULL_NONE, FT_CULL_NOCLAMP, ft_kernels.h FT_CULL_ROW
FILL = 0xffc0dead                                                                          # ft_kernels.h FT_CULL_PROBE_FILL
FLAG_INIT = 1                                                                              # ft_device.h FT_FLAG_INIT
SCENES = cc.scenes()


def entry_points():
    probe, site = L.ft_selftest_cull, L.ft_scene_cull_site                                 # internal: not in the header
    probe.restype, probe.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    site.restype, site.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    return probe, site


def cull_site(ds):
    """-> (count, flags, si, records (count, 4)) of the scene's cull site as flattened; count 0: none"""
    head = np.zeros(3, np.uint32)
    _lib.check(entry_points()[1](ds._scene, head.ctypes.data_as(C.c_void_p), None, 0))
    rec = np.zeros((int(head[0]), 4), F)
    if len(rec): _lib.check(entry_points()[1](ds._scene, head.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p), len(rec)))
    return int(head[0]), int(head[1]), float(head[2:3].view(F)[0]), rec


def run(gpu, ds, pts, masks):
    """-> words (W, 2) uint32 and rows (W, 2, ROW) uint32: the general wording first"""
    pts, masks = np.ascontiguousarray(pts, F), np.ascontiguousarray(masks, np.uint64)
    assert pts.shape == (len(masks), 64, 3)
    words, rows = np.zeros((len(masks), 2), np.uint32), np.zeros((len(masks), 2, ROW), np.uint32)
    _lib.check(entry_points()[0](gpu._ctx, ds._scene, *(a.ctypes.data_as(C.c_void_p) for a in (pts, masks)), len(masks), *(a.ctypes.data_as(C.c_void_p) for a in (words, rows))))
    return words, rows


def garbage(pts, idle, kind, other):
    p = pts.copy()
    p[idle] = {"huge": F(1e30), "NaN": F(np.nan)}.get(kind, 0)
    if kind == "another wave": p[idle] = other[idle]
    return p


GARBAGE = ("huge", "NaN", "another wave")


@pytest.mark.parametrize("name", list(SCENES))
def test_both_wordings_under_whole_and_ragged_masks(gpu, name):
    scene, start_of = SCENES[name]
    ds = gpu.scene(scene)
    count, flags, si, rec = cull_site(ds)
    looked = min(count, cc.CULL_MAX)
    assert count >= cc.CULL_MIN and si < 0 and (start_of is None) == bool(flags & FLAG_INIT), (name, count, flags, si)
    pts, kinds, on_centre, predicted = cc.waves_for(rec, si, seed=len(name) + count)
    assert len(pts) == 12 and min(predicted) >= 1, (name, predicted)                        # the clusters were put where the restated rule drops children
    # one launch: every wave under every mask, and under every ragged mask three more times with other points in its idle lanes
    jobs, P, M = [], [], []
    for w in range(len(pts)):
        for mname, mask in cc.MASKS.items():
            idle = ~cc.lanes_of(mask)
            variants = [("", pts[w])] + ([(g, garbage(pts[w], idle, g, pts[(w + 5) % len(pts)])) for g in GARBAGE] if idle.any() else [])
            for g, p in variants:
                jobs.append((w, mname, g)); P.append(p); M.append(mask)
    words, rows = run(gpu, ds, np.array(P, F), np.array(M, np.uint64))
    ds.close()
    index_of = {r.tobytes(): i for i, r in enumerate(rec[:looked])}
    assert len(index_of) == looked                                                         # no two children share a record: a survivor names its child
    centres, radii = rec[:looked, :3].astype(np.float64), rec[:looked, 3].astype(np.float64)
    dropped_tight, dropped_later, ran, switched_off = {}, 0, 0, 0
    base = {}
    for k, (w, mname, g) in enumerate(jobs):
        what = (name, kinds[w], w, mname, g)
        # the two wordings: the return word, the survivors and the untouched tail of the row
        assert words[k, 0] == words[k, 1], (what, hex(words[k, 0]), hex(words[k, 1]))
        assert np.array_equal(rows[k, 0], rows[k, 1]), (what, np.flatnonzero(rows[k, 0] != rows[k, 1])[:8])
        if g:                                                                              # other points in the idle lanes: the same output
            assert words[k, 0] == words[base[w, mname], 0] and np.array_equal(rows[k, 0], rows[base[w, mname], 0]), what
            continue
        base[w, mname] = k
        active = cc.lanes_of(cc.MASKS[mname])
        A = pts[w][active].astype(np.float64)
        if cc.restated_pass(rec, si, pts[w], active) is None:                              # a point outside in a lane that evaluates: fast_point_ok fails
            assert kinds[w] == "one point outside" and active[on_centre[w][1]], what
            assert words[k, 0] == NONE and (rows[k] == FILL).all(), (what, hex(words[k, 0]))
            switched_off += 1
            continue
        ran += 1
        assert words[k, 0] != NONE and (words[k, 0] & ~np.uint32(NOCLAMP | 0x1ff)) == 0, (what, hex(words[k, 0]))
        kept_n = int(words[k, 0] & 0xffff)
        assert 1 <= kept_n <= looked and (rows[k, 0, 4 * kept_n:] == FILL).all(), (what, kept_n)
        # survivors: the scene's own records, in list order
        kept = [index_of.get(rows[k, 0, 4 * j:4 * j + 4].tobytes(), -1) for j in range(kept_n)]
        assert min(kept) >= 0 and all(a < b for a, b in zip(kept, kept[1:])) and kept[0] == 0, (what, kept[:8])
        is_kept = np.zeros(looked, bool)
        is_kept[kept] = True
        # the contract, in float64: term_i(p) <= 2^(e - 24), e = floor(log2 S_i(p)), S_i(p) = the accumulator's start + the kept terms in front of child i
        dist = np.linalg.norm(centres[:, None, :] - A[None, :, :], axis=2)                 # (children, active points)
        term = np.exp(si * (dist - radii[:, None]))
        before = np.cumsum(term * is_kept[:, None], axis=0) - term * is_kept[:, None]
        if start_of is not None: before = before + start_of(A, si)[None, :]
        half_ulp = np.ldexp(1.0, np.frexp(before)[1] - 1 - 24)                             # frexp: before = m 2^e', m in [0.5, 1): floor(log2) = e' - 1
        bad = ~is_kept[:, None] & ~(term <= half_ulp)
        assert not bad.any(), (what, np.argwhere(bad)[:4].tolist(), term[bad][:4], half_ulp[bad][:4])
        # FT_CULL_NOCLAMP: no active point within 1e-6 of a centre the pass looked at; a point on a centre takes the flag away
        if words[k, 0] & NOCLAMP: assert dist.min() >= 1e-6, (what, dist.min())
        child, lane = on_centre[w]
        if kinds[w] == "on a centre" and active[lane]: assert not (words[k, 0] & NOCLAMP) and dist.min() == 0.0, what
        n_dropped = looked - kept_n
        if kinds[w] == "tight": dropped_tight[w, mname] = n_dropped
        if kinds[w] == "tight" and (~is_kept[64:]).any(): dropped_later += 1
    # the pass really ran, and really dropped
    assert ran > 50 and switched_off >= 6, (name, ran, switched_off)
    assert len(dropped_tight) == 3 * len(cc.MASKS)
    if count >= 64: assert min(dropped_tight.values()) >= 1, (name, dropped_tight)          # (at least one is always kept: the first child)
    if count in (130, 256): assert dropped_later >= 1, name                                # a child beyond the first 64: `carry` took part in the decision


def test_a_scene_without_a_site_gives_none_twice(gpu):
    ds = gpu.scene(cc.scene_without_a_site())
    assert cull_site(ds)[0] == 0 and ds.info()["cull_pc"] == -1
    pts = np.random.default_rng(3).normal(size=(len(cc.MASKS), 64, 3)).astype(F)
    words, rows = run(gpu, ds, pts, np.array(list(cc.MASKS.values()), np.uint64))
    ds.close()
    assert (words == NONE).all() and (rows == FILL).all()


def test_the_probe_refuses_bad_arguments(gpu):
    probe = entry_points()[0]
    ds = gpu.scene(cc.scene_without_a_site())
    pts, masks, words, rows = np.zeros((1, 64, 3), F), np.array([1], np.uint64), np.zeros((1, 2), np.uint32), np.zeros((1, 2, ROW), np.uint32)
    p = [a.ctypes.data_as(C.c_void_p) for a in (pts, masks, words, rows)]
    zero = np.zeros(1, np.uint64).ctypes.data_as(C.c_void_p)
    for args in ((None, p[0], p[1], 1, p[2], p[3]), (ds._scene, None, p[1], 1, p[2], p[3]), (ds._scene, p[0], None, 1, p[2], p[3]),
                 (ds._scene, p[0], p[1], 0, p[2], p[3]), (ds._scene, p[0], p[1], 4097, p[2], p[3]), (ds._scene, p[0], p[1], 1, None, p[3]),
                 (ds._scene, p[0], p[1], 1, p[2], None), (ds._scene, p[0], zero, 1, p[2], p[3])):              # the last: an empty lane mask
        assert probe(gpu._ctx, *args) == _lib.FT_ERR_INVALID, args
    assert probe(None, ds._scene, p[0], p[1], 1, p[2], p[3]) == _lib.FT_ERR_INVALID
    assert probe(gpu._ctx, ds._scene, p[0], p[1], 1, p[2], p[3]) == 0 and (words == NONE).all()
    ds.close()
