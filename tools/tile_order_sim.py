#!/usr/bin/env python3
"""CPU model of the hand-out order of a frame's 8x8 tiles (FT_OPT_ORDER; DESIGN.md section 4 "Tile order"): when does the last wave end, for the
order tiles leave the job queue in?  The tiles, marches and lock-step replay are those of miss_certificate_cluster_sim.py / miss_certificate_bundle_sim.py:
N * N / 64 random 8x8 tiles of the 4096^2 C3 frame, each replayed as one wave under the shipped bundle certificate (lane axis, every 2nd round, shadow
rays from their 2nd step, no per-lane tries); a tile's cost is the rounds until its last lane ends.  The tile costs are then bootstrapped (fixed seed)
to the frame's 262 144 tiles and handed to 5120 waves (256 CUs x 5 workgroups x 4 waves), each taking the queue's next tile when it falls idle, at
constant round time.  Printed per order: the end of the last wave over the ideal sum / waves, and the rounds between the queue running dry and that end.
  index order; descending by true cost; descending for the tiles at or above t x mean (t = 1, 1.5, 2) with the rest in index order; descending by
  a cost with lognormal error (a moved camera); and the same for an eighth of the frame (one rank's share at N = 8).
Usage: python tools/tile_order_sim.py [N=128: N*N pixels]"""
import heapq
import os
import sys
import numpy as np
if len(sys.argv) < 2:
    sys.argv.append('128')                  # the tile model reads its size from the command line when it is imported; its own default is 64
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import miss_certificate_bundle_sim as b
m = b.m

WAVES, TILES = 5120, 262144
NEVER = 1 << 30


def tile_costs():
    """rounds of every modelled tile (a tile is replayed as a wave of its own: its first round is round 0 of the bundle's period)"""
    out = []
    b.replay(None, NEVER, NEVER, 64, 0, axis='lane', period=2, shadowFrom=2, B=0.0, per_tile=out)
    return np.array(out, np.int64)


def schedule(costs, waves):
    """every wave takes the next tile of `costs` when it falls idle -> (end of the last wave, the moment the last tile was taken)"""
    free = [0] * waves
    dry = 0
    for c in costs:
        t = heapq.heappop(free)
        dry = t
        heapq.heappush(free, t + int(c))
    return max(free), dry


def by_rule(true, seen, factor):
    """tiles whose seen cost is at least factor x the mean, descending by seen cost clamped to 255 (ties in index order); the others in index order"""
    heavy = np.flatnonzero(seen >= factor * seen.mean())
    heavy = heavy[np.argsort(-np.minimum(seen[heavy], 255), kind='stable')]
    light = np.setdiff1d(np.arange(len(true)), heavy)
    return true[np.concatenate([heavy, light])]


def report(name, costs, waves):
    end, dry = schedule(costs, waves)
    ideal = costs.sum() / waves
    print(f'{name:64s} last wave ends {end / ideal - 1:+7.1%} over ideal, {end - dry:4d} rounds after the queue runs dry', flush=True)


if __name__ == '__main__':
    base = tile_costs()
    print(f'N={m.N} tiles={len(base)}: rounds per tile mean {base.mean():.1f} median {np.median(base):.0f} p90 {np.percentile(base, 90):.0f} '
          f'p99 {np.percentile(base, 99):.0f} max {base.max()}; {np.mean(base <= 2):.0%} of the tiles cost two rounds or fewer')
    rs = np.random.default_rng(7)
    for label, tiles in (('whole frame', TILES), ('an eighth of the frame', TILES // 8)):
        true = base[rs.integers(0, len(base), tiles)]
        print(f'{label}: {tiles} tiles over {WAVES} waves, ideal {true.sum() / WAVES:.1f} rounds a wave')
        report('index order', true, WAVES)
        report('descending by true cost (full sort)', by_rule(true, true, 0.0), WAVES)
        for f in (1.0, 1.5, 2.0):
            report(f'descending for tiles >= {f:g} x mean, the rest in index order', by_rule(true, true, f), WAVES)
        for sigma in (0.2, 0.5):
            seen = true * rs.lognormal(0.0, sigma, tiles)
            report(f'>= mean by a cost with lognormal error sigma {sigma:g}', by_rule(true, seen, 1.0), WAVES)
