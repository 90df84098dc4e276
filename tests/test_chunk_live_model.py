"""Host-only check of the budget split of the exact pruning and of the model's chunk-live rule (tools/prune_model.py: BUDGET1 / BUDGET2
restate kPruneBudget1 / kPruneBudget2 of csrc/glhip_autosort.h; level2_mass's `live`, walk_live and chunk_counts model a chunk level
between the two pruning levels — a column block is staged for a half slab of 128 rows only if some group of it can pass t2 of one of
the half slab's row tiles.  The library does not have that level: on the device it removed tiles but no time, profiles/chunk_skip.txt;
the model keeps the rule so that the tile counts in that file can be reproduced).  On a small law:

* the budgets add up: first level + term rule (2^-26 / e, pinned by tests/test_prune_mass_model.py) + mass rule = 2^-26, and the
  underflow bucket alone stays inside each budget;
* every block the model marks dead for a half slab has, for every row tile of the half slab, all its groups' float64 keys below the
  tile's t2 (recomputed here from the points, not read from the model's buckets): what the rule leaves out is what the mass rule's
  histograms already counted as dropped;
* the home block is never dead, and the rule does take blocks out (the check is not vacuous);
* the walk stages no more tiles than the walk over whole intervals, and every live block of the intervals exactly once;
* the rule is stable under the distance the device's float32 sums may have from the model's float64 ones: with every group's lse moved
  up by one float32 ulp at most HALF_CAP of the half slabs see a t2 move, and on the others at most BIT_CAP of the bits differ.
The model takes finite inputs; special (NaN / inf) blocks are the device's business.
"""

import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import prune_model as pm  # noqa: E402

N = 40000
EPS = 0.01**2
HALF_CAP, BIT_CAP = 0.04, 1e-3


@pytest.fixture(scope="module")
def case():
    x, y, h, _ = pm.bench_problem(N, seed=3)
    px, py = pm.compact_order2(x, 256, 2), pm.compact_order2(y, 256, 2)
    xs, ys, hs = x[px], y[py], h[py]
    keep, mlb, t1, L = pm.plan_mass(xs, ys, hs, EPS)
    slabs = np.array([c for c in np.linspace(0, keep.shape[0] - 1, 12).astype(int) if not keep[c].all()])
    _, _, rec = pm.level2_mass(xs, ys, hs, EPS, keep, L, slabs)
    return xs, ys, hs, keep, L, slabs, rec


def test_dead_blocks_hold_only_keys_below_t2(case):
    xs, ys, hs, keep, L, slabs, rec = case
    glo, ghi = pm.boxes(ys, pm.GROUP)
    glse, _ = pm.group_block_lse(hs, N)
    i2e = pm.inv2eps_of(EPS)
    per = pm.BLOCK // pm.GROUP
    dead = walked = 0
    for c in slabs:
        r = rec[c]
        assert r["live"].shape == (2, r["blocks"].size) and np.array_equal(r["blocks"], np.flatnonzero(keep[c]))
        assert r["live"][:, r["blocks"] == r["home"]].all()              # the home block is never dead
        for hs_ in range(2):
            gone = r["blocks"][~r["live"][hs_]]
            dead += gone.size
            walked += r["blocks"].size
            g = (gone[:, None] * per + np.arange(per)[None]).ravel()
            g = g[g < glo.shape[0]]
            for t in range(hs_ * 4, min(len(r["t2"]), (hs_ + 1) * 4)):
                w0 = c * pm.SLAB + t * pm.TILE
                xr = xs[w0:min(w0 + pm.TILE, N)].astype(np.float64)
                gap = np.maximum(np.maximum(glo[g] - xr.max(0), xr.min(0) - ghi[g]), 0.0)
                key = glse[g] - (gap**2).sum(-1) * i2e
                assert (key < r["t2"][t]).all(), (c, t)
                assert r["skip"][t][np.isin(r["groups"], g)].all()       # ... and the second level's own rule skips them for this tile
    print(f"{dead} of {walked} walked (half slab, block) pairs dead: {dead / walked:.4f}")
    assert dead > 0.02 * walked


def test_budgets_add_up():
    assert abs(pm.BUDGET1 + 2.0**-26 / math.e + pm.BUDGET2 - 2.0**-26) < 1e-22
    assert pm.BUDGET1 > 0 and pm.BUDGET2 > 0 and pm.MARGIN == 1.0
    for M in (1000, 10**6, 2**31 - 1):      # the underflow bucket alone can never exceed its budget (glhip_prune.hip, prune_first_kept)
        eL = math.exp(-(math.log(M) + 26 * math.log(2) + pm.MARGIN))
        assert -(-M // pm.BLOCK) * eL <= pm.BUDGET1 and -(-M // pm.GROUP) * eL <= pm.BUDGET2


def test_cursor_stages_every_live_block_once_and_fewer_tiles(case):
    xs, ys, hs, keep, L, slabs, rec = case
    today = after = 0
    for c in slabs:
        iv = pm.intervals_of(keep[c])
        a, b, walked, dead = pm.chunk_counts(rec[c], iv, N)
        today += a
        after += b
        for hs_ in range(2):
            lv = dict(zip(rec[c]["blocks"].tolist(), rec[c]["live"][hs_].tolist()))
            staged = np.zeros(keep.shape[1], int)
            for j0, cols in pm.walk_live(iv, lambda t: lv.get(t, False), N):
                assert j0 % pm.BLOCK == 0 and cols in (pm.BLOCK, 2 * pm.BLOCK, N - j0)
                staged[j0 // pm.BLOCK:-(-(j0 + cols) // pm.BLOCK)] += 1
            want = np.zeros(keep.shape[1], int)
            want[rec[c]["blocks"][rec[c]["live"][hs_]]] = 1
            assert np.array_equal(staged, want)
    print(f"tiles staged: {after} under the chunk level against {today}")
    assert after <= today


def test_caps_hold_for_the_model_against_itself_one_ulp_up(case, monkeypatch):
    xs, ys, hs, keep, L, slabs, rec = case
    plain = pm.group_block_lse

    def moved(h, M):
        g, b = plain(h, M)
        return np.nextafter(g.astype(np.float32), np.float32(np.inf)).astype(np.float64), b

    monkeypatch.setattr(pm, "group_block_lse", moved)
    _, _, rec2 = pm.level2_mass(xs, ys, hs, EPS, keep, L, slabs)
    halves = off = bits = diff = 0
    for c in slabs:
        for hs_ in range(2):
            rows = slice(hs_ * 4, (hs_ + 1) * 4)
            if rec[c]["fk"][rows].size == 0:
                continue
            halves += 1
            if not np.array_equal(rec[c]["fk"][rows], rec2[c]["fk"][rows]):
                off += 1
                continue
            bits += rec[c]["live"][hs_].size
            diff += int((rec[c]["live"][hs_] != rec2[c]["live"][hs_]).sum())
    print(f"{off} of {halves} half slabs with a moved t2; {diff} of {bits} bits differ on the others")
    assert off <= HALF_CAP * halves and diff <= BIT_CAP * bits
