"""tests/wave_restatement.py against the sequential definitions, on the waves the GPU test hands the kernels: the maximum exactly, the prefix sums
within the seven roundings an element goes through (four steps within its row, p2, p3, the row's offset) of the float64 running sum."""
import numpy as np

import wave_restatement as wr

F = np.float32
SCAN_BOUND = (1.0 + 2.0 ** -24) ** 7 - 1.0         # inputs >= 0: every partial sum is a sum of non-negative terms, each rounded at most seven times


def sequential_max(wave):
    m = F(0.0)
    for x in wave:
        if x > m:                                  # false for a NaN: dropped
            m = x
    return m


def test_the_maximum_is_exact():
    n = 0
    for name, waves in wr.waves().items():
        got = wr.wave_max(waves)
        for k, wave in enumerate(waves):
            want = sequential_max(wave)
            assert got[k] == want and not np.isnan(got[k]), (name, k, got[k], want)
            if name not in wr.BY_VALUE: assert got[k].view(np.uint32) == want.view(np.uint32), (name, k)
            n += 1
    assert n > 200


def test_the_prefix_sums_are_within_seven_roundings_of_the_running_sum():
    n = 0
    for name, waves in wr.waves().items():
        if name in wr.NO_SCAN: continue
        incl, excl, total = wr.wave_scan(waves)
        run = np.cumsum(waves.astype(np.float64), axis=-1)
        finite = np.isfinite(run)
        assert np.array_equal(np.isfinite(incl), finite), name                     # +inf from the lane that holds it on, finite before
        assert (np.abs(incl[finite].astype(np.float64) - run[finite]) <= SCAN_BOUND * run[finite]).all(), name
        assert (incl[~finite] == np.inf).all(), name
        last = run[:, -1]
        ok = np.isfinite(last)
        assert (np.abs(total[ok].astype(np.float64) - last[ok]) <= SCAN_BOUND * last[ok]).all() and (total[~ok] == np.inf).all(), name
        assert np.array_equal(excl[:, 1:].view(np.uint32), incl[:, :-1].view(np.uint32)) and (excl[:, 0].view(np.uint32) == 0).all(), name
        n += len(waves)
    assert n > 200


def test_the_waves_are_what_their_names_say():
    w = wr.waves()
    each = w["maximum in each lane"]
    assert each.shape == (64, 64) and (each.argmax(axis=1) == np.arange(64)).all() and len(set(each.max(axis=1))) == 64
    sub = w["subnormals"]
    assert (sub >= 0).all() and (sub < F(2.0 ** -126)).all() and (sub.max(axis=1) > 0).all()
    nan = w["NaN in one lane"]
    assert {15, 63} <= set(np.argwhere(np.isnan(nan[:8]))[:, 1]) and (np.isnan(nan).sum(axis=1)[:-1] == 1).all() and np.isnan(nan[-1]).sum() == 63
    assert np.signbit(w["-0.0 among +0.0"]).any() and (w["-0.0 among +0.0"] == 0).all()
    rows = w["rows that differ greatly"].reshape(-1, 4, 16)
    assert len(rows) == 28 and (rows[:24].max(axis=2).max(axis=1) / rows[:24].max(axis=2).min(axis=1) > 2.0 ** 55).all()
    for name in wr.BACK_TO_BACK:
        assert np.isfinite(w[name]).all() and (w[name] >= 0).all() and not np.signbit(w[name]).any(), name
    m = wr.four_maxima(w["18 decades"])
    assert all((a > 0).all() for a in m) and not np.array_equal(m[0], m[3])
