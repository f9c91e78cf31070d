"""The bundle certificate's early exit (kernels.hip ft_bundle_certificate, lean kernel): a try stops after the pass in which some lane's own sum has
reached the threshold, because the total the full try would form cannot be below any lane's partial sum.  Restated here on the CPU in the kernel's
own order of float32 additions — lane k of pass j holds term 64 j + k and adds it to its sum; lane 15 of every row of 16 gathers the row through the
row shifts by 1, 2, 4 and 8; the four rows meet as ((r0 + r1) + r2) + r3 — for 2000 random vectors of 65 to 600 non-negative terms:

  * the float32 total is >= every lane's sum after every pass (the rule the kernel uses: no guard band);
  * a partial sum over whole passes, taken exactly, of thr (1 + 2^-10) or more implies a float32 total >= thr (the guard band a rule on the summed
    passes would need: the tree rounds 6 + passes times per term, far inside 2^-10)."""
import numpy as np

F = np.float32


def kernel_total(terms):
    """-> (float32 total in the kernel's order, [per-lane float32 sums after each pass])"""
    n = len(terms)
    passes = (n + 63) // 64
    padded = np.zeros(passes * 64, F)
    padded[:n] = terms
    lanes = np.zeros(64, F)
    after = []
    for j in range(passes):
        lanes = (lanes + padded[64 * j:64 * j + 64]).astype(F)
        after.append(lanes.copy())
    v = lanes.copy()
    lane = np.arange(64)
    for shift in (1, 2, 4, 8):                                         # row_shr: a lane without a source lane in its row adds 0
        src = np.where(lane % 16 >= shift, np.roll(v, shift), F(0))
        v = (v + src).astype(F)
    r0, r1, r2, r3 = v[15], v[31], v[47], v[63]
    return F(F(F(r0 + r1) + r2) + r3), after


def vectors():
    g = np.random.default_rng(20)
    for _ in range(2000):
        n = int(g.integers(65, 601))
        t = np.exp2(g.uniform(-40.0, 5.0, n)).astype(F)
        t[g.random(n) < 0.1] = 0.0                                     # children far away: terms that flushed to 0
        if g.random() < 0.3:
            t[g.integers(0, n)] = F(np.exp2(g.uniform(5.0, 30.0)))     # one child the bundle passes close to
        yield t


def test_total_is_at_least_every_partial_lane_sum():
    for t in vectors():
        total, after = kernel_total(t)
        for lanes in after:
            assert total >= lanes.max(), (len(t), total, lanes.max())


def test_guard_band_for_whole_passes():
    band = 1.0 + 2.0 ** -10
    for t in vectors():
        total, after = kernel_total(t)
        t64 = t.astype(np.float64)
        for j in range(len(after)):
            exact = t64[:64 * (j + 1)].sum()
            if exact == 0.0:
                continue
            thr = F(exact / band)
            if float(thr) * band > exact:                              # the largest float32 thr with thr (1 + 2^-10) <= the partial sum
                thr = np.nextafter(thr, F(0))
            assert float(thr) * band <= exact and total >= thr, (len(t), j, total, thr)
