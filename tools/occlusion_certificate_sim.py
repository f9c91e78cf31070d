#!/usr/bin/env python3
"""CPU model of the occlusion certificate on the C3 frame (kernels.hip ft_occlusion_certificate; scene.cpp "Occlusion certificate"), on the float64 tiles
and marches of miss_certificate_cluster_sim.py.  A shadow ray is certified as a hit where its line passes hitM = occE (t / eps + 2) + occB inside one
sphere at its closest approach t, or as deep inside the ball of radius -f(y) around a witness y.  Reported:
  * the share of shadow rays that are occluded and the steps they march;
  * the share of the occluded rays certified at birth by their own line against any sphere ("own"), by the sphere that is deepest on the tile's axis
    (the first candidate at or after lane 27, else the first: "axis"), and by the sphere deepest on the line of the candidate whose own depth is greatest
    ("deepest candidate"); with the witness ball: by f at the closest approaches of their own line ("own witness") and by the sphere and the witness
    y of the tile's axis; the same with a margin of 0.05 for comparison with the issue's figures;
  * the evaluation rounds of the lock-step tiles under the candidate schedules (period P: a try every P-th round for the rays born since the last one),
    with the miss certificates at their ideal (a ray that misses ends at the first step from which its own flat certificate holds), and the rounds
    net of the tries priced at TRY VALU against E per round.
Usage: python tools/occlusion_certificate_sim.py [N=64: N*N pixels] [margin=0.0476] [E=4300] [occE=1.63e-5] [occB=3.6e-4] [TRY=220]"""
import os
import sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import miss_certificate_cluster_sim as m

C, R, k, eps, T, E, lanes_D, dirS = m.C, m.R, m.k, m.eps, m.T, m.E, m.D, m.ldir
occE = float(sys.argv[4]) if len(sys.argv) > 4 else 1.63e-5
occB = float(sys.argv[5]) if len(sys.argv) > 5 else 3.6e-4
TRY = float(sys.argv[6]) if len(sys.argv) > 6 else 220.0


def depth_on_line(o, d, L, margin=None):
    """per child: r - closest approach of the line o + t d, 0 <= t <= L, less the margin at that t"""
    t = np.clip(((C - o) @ d) / (d @ d), 0.0, L)
    dist = np.linalg.norm(C - (o + t[:, None] * d), axis=1)
    return R - dist - (occE * (t / eps + 2.0) + occB if margin is None else margin)


def margin_at(t, margin=None):
    return occE * (t / eps + 2.0) + occB if margin is None else margin


def witness(oa, d, La, child):
    """the axis's closest approach to `child` and D = -f there (pass B)"""
    t = float(np.clip(((C[child] - oa) @ d) / (d @ d), 0.0, La))
    y = oa + t * d
    return y, -float(m.sdf(y[None])[0])


def ball_test(o, d, L, y, D, margin=None):
    t = float(np.clip(((y - o) @ d) / (d @ d), 0.0, L))
    return np.linalg.norm(y - (o + t * d)) + margin_at(t, margin) < D


def own_witness(o, d, L, margin=None, near=8):
    """the best the ray's own line could show: f at its closest approaches to its `near` nearest children"""
    t = np.clip(((C - o) @ d) / (d @ d), 0.0, L)
    dist = np.linalg.norm(C - (o + t[:, None] * d), axis=1) - R
    pick = np.argsort(dist)[:near]
    return (-m.sdf(o + t[pick, None] * d) - margin_at(t[pick], margin)).max() > 0.0


def certified(o, d, L, child, y, D, margin=None):
    return depth_on_line(o, d, L, margin)[child] > 0.0 or ball_test(o, d, L, y, D, margin)


def first_clear(trail, d):
    """the first step of a missing march from which the flat miss certificate of its own line holds (ideal: tried every step)"""
    if not trail:
        return 0
    pts = np.array([p for p, _ in trail]); Ls = np.array([l for _, l in trail])
    s = m.terms(pts, np.repeat(d[None], len(pts), 0), Ls, C, R).sum(1)
    ok = np.where(s < m.thr)[0]
    return int(ok[0]) if len(ok) else len(trail)


if __name__ == '__main__':
    nS = len(m.hitS)
    occ = np.where(m.hitS)[0]
    stepsO = np.array([len(m.trailS[i]) for i in occ]); stepsL = np.array([len(m.trailS[i]) for i in np.where(~m.hitS)[0]])
    print(f'N={m.N} tiles={T} shadow rays {nS}, occluded {len(occ)} ({len(occ) / nS:.1%}); steps of an occluded ray: mean {stepsO.mean():.1f} '
          f'p90 {np.percentile(stepsO, 90):.0f}; of a lit ray before any certificate: mean {stepsL.mean():.1f}')
    print(f'margin hitM = {occE:.3g} (t / eps + 2) + {occB:.3g}, eps {eps}')
    # lanes of a tile: ray index -> its shadow ray (or -1)
    for label, margin in (('shipped margin', None), ('margin 0.05', 0.05)):
        own = axis = deep = ownW = axisW = 0
        for t in range(T):
            js = [j for j in range(64) if m.shadowOf[t * 64 + j] >= 0]
            if not js: continue
            sid = [m.shadowOf[t * 64 + j] for j in js]
            born = [m.trailS[s][0] if m.trailS[s] else None for s in sid]
            cand = [i for i in range(len(js)) if born[i] is not None]
            if not cand: continue
            at = [i for i in cand if js[i] >= 27]
            a = at[0] if at else cand[0]
            dA = depth_on_line(born[a][0], dirS, born[a][1], margin)
            childA = int(np.argmax(dA))
            yA, DA = witness(born[a][0], dirS, born[a][1], childA)
            ownD = {i: depth_on_line(born[i][0], dirS, born[i][1], margin) for i in cand}
            b = max(cand, key=lambda i: ownD[i].max())
            childB = int(np.argmax(ownD[b]))
            for i in cand:
                viaA = (dA.max() > 0.0 and ownD[i][childA] > 0.0) or ball_test(born[i][0], dirS, born[i][1], yA, DA, margin)
                if not m.hitS[sid[i]]:
                    assert ownD[i].max() <= 0.0 and not viaA, 'a lit ray certified'
                    continue
                ownW += own_witness(born[i][0], dirS, born[i][1], margin)
                axisW += viaA
                own += ownD[i].max() > 0.0
                axis += dA.max() > 0.0 and ownD[i][childA] > 0.0
                deep += ownD[b].max() > 0.0 and ownD[i][childB] > 0.0
        print(f'{label}: of the occluded rays, certified at birth by their own line {own / len(occ):.1%}, by the tile axis\'s sphere {axis / len(occ):.1%}, '
              f'by the deepest candidate\'s sphere {deep / len(occ):.1%}; with the witness ball: by their own witness {ownW / len(occ):.1%}, by the sphere and the witness of the '
              f'tile\'s axis {axisW / len(occ):.1%}')
    # lock-step rounds per tile: primary march (ideal miss certificate), 4 normal probes, shadow march (first evaluation from the cache)
    clearP = {}
    for period in (0, 1, 2, 3):
        rounds = tries = 0
        for t in range(T):
            end = np.zeros(64, int); birth = np.full(64, -1); sOf = np.full(64, -1)
            for j in range(64):
                r = t * 64 + j
                tp = m.trailP[r]
                if m.hitP[r]:
                    n = len(tp) + 4
                    s = m.shadowOf[r]
                    if s >= 0:
                        birth[j] = n; sOf[j] = s
                        tr = m.trailS[s]
                        if m.hitS[s]: n += max(len(tr) - 1, 0)
                        else:
                            if ('s', s) not in clearP: clearP[('s', s)] = first_clear(tr, dirS)
                            n += max(clearP[('s', s)] - 1, 0)
                else:
                    if r not in clearP: clearP[r] = first_clear(tp, lanes_D[r])
                    n = clearP[r]
                end[j] = n
            if period:
                # try rounds: w % period == 0 with a candidate born in (w - period, w]; axis = first candidate at or after lane 27, else the first
                w = 0
                last = int(end.max())
                while w < last:
                    if w % period == 0:
                        cand = [j for j in range(64) if birth[j] >= 0 and w - period < birth[j] <= w and end[j] > w]
                        if cand:
                            tries += 1
                            at = [j for j in cand if j >= 27]
                            a = at[0] if at else cand[0]

                            def state(j):
                                tr = m.trailS[sOf[j]]
                                return tr[min(1 + w - birth[j], len(tr) - 1)]
                            oa, La = state(a)
                            dA = depth_on_line(oa, dirS, La)
                            if (dA + occE * 2 + occB).max() > -0.25 * np.log(len(C)):      # a child within occNear of the axis
                                ch = int(np.argmax(dA))
                                y, D = witness(oa, dirS, La, ch)
                                for j in cand:
                                    o, L = state(j)
                                    if certified(o, dirS, L, ch, y, D):
                                        assert m.hitS[sOf[j]], 'a lit ray certified'
                                        end[j] = w
                                last = int(end.max())
                    w += 1
            rounds += end.max()
        if period == 0:
            r0 = rounds
            print(f'rounds without the occlusion certificate (ideal miss certificates): {rounds}')
        else:
            net = rounds + tries * TRY / E
            print(f'period {period}: rounds {rounds} ({rounds / r0 - 1:+.2%}), tries {tries}, net of the tries at {TRY:.0f} / {E:.0f} VALU {net:.0f} ({net / r0 - 1:+.2%})', flush=True)
