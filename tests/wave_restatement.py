"""The wave primitives of the culling pass and the certificates (kernels.hip ft_wave_max_all, ft_wave_scan_incl, ft_wave_shift_right1 and their lean
forms), restated in numpy float32: a wave is the last axis, 64 values in lane order.  tests/test_wave_restatement_host.py holds this file to the
sequential definitions; tests/test_gpu_wave_primitives.py holds the kernels to this file, bit for bit.  The hand-made waves both use are here as well."""
import numpy as np

F = np.float32
LANES, ROW = 64, 16


def wave_max(v):
    """max(0, v) over the lanes, a quiet NaN dropped (fmaxf / v_max_f32 return the other operand); one value per wave"""
    v = np.asarray(v, F)
    with np.errstate(invalid="ignore"):
        return np.fmax(F(0.0), np.fmax.reduce(v, axis=-1)).astype(F)


def wave_scan(v):
    """-> (inclusive, exclusive, total): the kernels' additions in the kernels' order.  Within a row of 16 lanes the value a lane holds is added to
    the lanes 1, 2, 4 and 8 places up (a lane without a source adds 0); r0 .. r3 are the rows' sums, p2 = r0 + r1, p3 = p2 + r2; rows 1, 2, 3 add
    r0, p2, p3 (row 0 adds 0); total = p3 + r3.  The exclusive prefix is the inclusive one a lane down, 0 in lane 0."""
    v = np.asarray(v, F)
    r = v.reshape(v.shape[:-1] + (LANES // ROW, ROW)).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for s in (1, 2, 4, 8):
            up = np.zeros_like(r)
            up[..., s:] = r[..., :-s]
            r = (r + up).astype(F)
        r0, r1, r2, r3 = (r[..., k, ROW - 1] for k in range(4))
        p2 = (r0 + r1).astype(F)
        p3 = (p2 + r2).astype(F)
        off = np.stack([np.zeros_like(r0), r0, p2, p3], axis=-1)
        incl = (r + off[..., None]).astype(F).reshape(v.shape)
        total = (p3 + r3).astype(F)
    excl = np.zeros_like(incl)
    excl[..., 1:] = incl[..., :-1]
    return incl, excl, total


def four_maxima(v, scale=F(1.0)):
    """the probe's back-to-back maxima (kernels.hip ft_selftest_wave_kernel, op 1), each restated on its own: m0 = max(x scale), m1 = max(m0 - x),
    m2 = max(x m1), m3 = max(x + m2); every product, difference and sum is one float32 operation"""
    v = np.asarray(v, F)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        m0 = wave_max((v * F(scale)).astype(F))
        m1 = wave_max((m0[..., None] - v).astype(F))
        m2 = wave_max((v * m1[..., None]).astype(F))
        m3 = wave_max((v + m2[..., None]).astype(F))
    return m0, m1, m2, m3


# ---- the hand-made waves: name -> (waves, 64) float32 ----------------------------------------------------------------------------------------

def decades(rng, n):
    """18 decades of magnitude with some zeros, as tools/experiments/dpp_scan.hip draws them: the rounding order shows in the sums"""
    v = np.exp2(-60.0 * rng.random((n, LANES))).astype(F)
    v[rng.integers(0, 8, (n, LANES)) == 0] = F(0.0)
    return v


def with_lane(base, lanes, value):
    """one wave per lane of `lanes`: `base` with `value` in that lane"""
    out = np.repeat(np.asarray(base, F)[None, :], len(lanes), axis=0)
    out[np.arange(len(lanes)), lanes] = value
    return out


def waves():
    rng = np.random.default_rng(20)
    w = {}
    small = rng.random(LANES).astype(F)                                # all below 1
    w["maximum in each lane"] = with_lane(small, np.arange(LANES), F(1.5))
    w["maximum in each lane"][np.arange(LANES), np.arange(LANES)] += np.arange(LANES, dtype=F)      # 1.5 + lane: another maximum in every wave
    w["all zeros"] = np.zeros((1, LANES), F)
    w["all equal"] = np.stack([np.full(LANES, 0.7, F), np.full(LANES, 1e-3, F), np.full(LANES, 1.0e30, F)])
    sub = rng.integers(0, 0x00800000, (8, LANES), dtype=np.uint32).view(F)                          # [0, 2^-126): the maximum is a subnormal
    sub[0] = np.uint32(1).view(F) * (rng.random(LANES) < 0.1)                                       # nothing but the smallest subnormal and zeros
    sub[0, 40] = np.uint32(1).view(F)
    w["subnormals"] = sub
    special = np.array([0, 15, 16, 31, 37, 47, 48, 63])
    w["+inf in one lane"] = with_lane(small, special, F(np.inf))
    w["NaN in one lane"] = np.concatenate([with_lane(small, special, F(np.nan)), with_lane(np.zeros(LANES, F), special, F(np.nan)),
                                           with_lane(np.full(LANES, np.nan, F), [22], F(0.25))])      # ... and in every lane but one
    # (a wave of nothing but NaN is outside the contract: lane 15 of a row folds its 16 lanes and never meets the 0 that lane 0 read, so the
    # maximum is max(0, v) only where some lane holds a number; every caller hands 0 in its idle lanes and finite values in the others)
    zeros = np.zeros((4, LANES), F)
    zeros[0, :] = F(-0.0)
    zeros[1, ::3] = F(-0.0)
    zeros[2, 15] = zeros[2, 63] = zeros[3, 0] = F(-0.0)
    w["-0.0 among +0.0"] = zeros
    w["18 decades"] = decades(rng, 128)
    rows = []
    for k, order in enumerate([(a, b, c, d) for a in range(4) for b in range(4) for c in range(4) for d in range(4) if len({a, b, c, d}) == 4]):
        v = (F(0.5) + F(0.5) * rng.random(LANES)).astype(F).reshape(4, ROW)
        rows.append((v * np.exp2(np.array(order, F) * F(-20.0) + F(k % 3))[:, None]).astype(F).reshape(LANES))   # the four rows 2^20 apart, in every order
    one_row = np.zeros((4, LANES), F)
    for k in range(4):
        one_row[k, ROW * k:ROW * (k + 1)] = (F(1.0) + rng.random(ROW)).astype(F)                                   # a single row holds everything
    w["rows that differ greatly"] = np.concatenate([np.array(rows, F), one_row])
    return w


NO_SCAN = ("NaN in one lane",)                     # the scans are never given a NaN (their inputs are exponentials of clamped, finite arguments)
BY_VALUE = ("-0.0 among +0.0",)                    # compared with ==, not by bits: the contract is v >= 0, and no decision reads a zero's sign
BACK_TO_BACK = ("maximum in each lane", "all equal", "18 decades", "rows that differ greatly", "all zeros")   # finite, non-negative
