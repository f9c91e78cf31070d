"""The wave primitives of kernels.hip — ft_wave_max_all and its hand-scheduled lean form, ft_wave_scan_incl and its row-masked lean form, the
exclusive prefix by ft_wave_shift_right1 and by the lean culling pass's mov_dpp — run by the internal probe ft_selftest_wave on hand-made waves
and compared bit for bit with the numpy restatement (tests/wave_restatement.py, itself held to the sequential definitions by
tests/test_wave_restatement_host.py), and the lean forms with the general ones.  A few hundred waves, no scene."""
import ctypes as C

import numpy as np
import pytest

from fraytracer_amd import _lib
from helpers import options_left_at_defaults  # noqa: F401  (fixture)

import wave_restatement as wr

pytestmark = pytest.mark.gpu

F = np.float32
L = _lib.lib
PLANES = ("max", "max lean", "scan", "total", "scan lean", "total lean", "exclusive", "exclusive lean")


def probe_fn():
    fn = L.ft_selftest_wave                                                                # internal: not in the header
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_float, C.c_int32, C.c_void_p]
    return fn


def run(gpu, op, waves):
    waves = np.ascontiguousarray(waves, F)
    out = np.full((8 if op == 0 else 4,) + waves.shape, np.nan, F)
    _lib.check(probe_fn()(gpu._ctx, op, waves.ctypes.data_as(C.c_void_p), 1.0, len(waves), out.ctypes.data_as(C.c_void_p)))
    return out


@pytest.fixture(scope="module")
def probed(gpu):
    """every hand-made wave through op 0, in one launch: name -> (waves, {plane: (waves, 64)})"""
    w = wr.waves()
    out = run(gpu, 0, np.concatenate(list(w.values())))
    res, at = {}, 0
    for name, v in w.items():
        res[name] = (v, dict(zip(PLANES, out[:, at:at + len(v)])))
        at += len(v)
    assert at > 200
    return res


def same(got, want, name, by_value=False):
    got, want = np.ascontiguousarray(got, F), np.broadcast_to(np.asarray(want, F), got.shape)
    ok = (got == want) if by_value else (got.view(np.uint32) == np.ascontiguousarray(want).view(np.uint32))
    assert ok.all(), (name, np.argwhere(~ok)[:4].tolist(), got[~ok][:4], want[~ok][:4])


@pytest.mark.parametrize("name", list(wr.waves()))
def test_both_maxima_are_the_restated_maximum_in_every_lane(probed, name):
    """wave-uniform, max(0, v) over the lanes with a quiet NaN dropped; the zeros' signs are compared by value (the contract is v >= 0 and no
    decision reads the sign of a zero), everything else by bits"""
    v, got = probed[name]
    want = wr.wave_max(v)[:, None]
    assert not np.isnan(got["max"]).any() and not np.isnan(got["max lean"]).any(), name
    same(got["max"], want, name + ": general", name in wr.BY_VALUE)
    same(got["max lean"], want, name + ": lean", name in wr.BY_VALUE)
    same(got["max lean"], got["max"], name + ": lean against general", name in wr.BY_VALUE)


@pytest.mark.parametrize("name", [n for n in wr.waves() if n not in wr.NO_SCAN])
def test_both_scans_add_in_the_restated_order(probed, name):
    v, got = probed[name]
    incl, excl, total = wr.wave_scan(v)
    by_value = name in wr.BY_VALUE                                                         # (-0) + (+0): the sums are +0 either way, but the first lane's is its own input
    for form in ("", " lean"):
        same(got["scan" + form], incl, name + ": inclusive" + form, by_value)
        same(got["total" + form], total[:, None], name + ": total" + form, by_value)
        same(got["exclusive" + form], excl, name + ": exclusive" + form, by_value)
    for plane in ("scan", "total", "exclusive"):
        same(got[plane + " lean"], got[plane], name + ": " + plane + ", lean against general")
    assert (got["exclusive"][:, 0].view(np.uint32) == 0).all() and (got["exclusive lean"][:, 0].view(np.uint32) == 0).all(), name   # lane 0 reads +0


def test_four_lean_maxima_back_to_back(gpu):
    """each maximum is taken of a value the VALU formed from the previous maximum's wave-uniform result in the instruction before (as
    ft_bundle_certificate's Wr, epsMax, dLo, dHi): against four maxima restated on their own"""
    w = wr.waves()
    v = np.concatenate([w[n] for n in wr.BACK_TO_BACK])
    got = run(gpu, 1, v)
    want = wr.four_maxima(v)
    for k in range(4):
        same(got[k], want[k][:, None], f"maximum {k}")
    assert len({m.tobytes() for m in want}) == 4                                           # four different answers


def test_the_probe_refuses_bad_arguments(gpu):
    fn = probe_fn()
    x = np.zeros(64, F)
    out = np.zeros((8, 64), F)
    px, po = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for args in ((0, None, 1.0, 1, po), (0, px, 1.0, 1, None), (2, px, 1.0, 1, po), (-1, px, 1.0, 1, po), (0, px, 1.0, 0, po), (0, px, 1.0, 65537, po)):
        assert fn(gpu._ctx, *args) == _lib.FT_ERR_INVALID, args
    assert fn(None, 0, px, 1.0, 1, po) == _lib.FT_ERR_INVALID
    assert fn(gpu._ctx, 0, px, 1.0, 1, po) == 0 and (out == 0).all()
