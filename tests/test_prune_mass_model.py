"""Host-only check of the mass rule of the exact pruning (tools/prune_model.py: plan_mass / level2_mass restate prune_slabs_kernel and
prune_tiles_kernel of csrc/glhip_prune.hip).  On the points themselves, in float64: what the first level drops for a slab plus what
the second level skips for a row's tile holds less than 2^-26 of the row's true sum; and the rule evaluates no more pairs than the
term rule of rounds 7 / 9 on the same order."""

import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import prune_model as pm  # noqa: E402

N = 40000


@pytest.fixture(scope="module")
def clouds():
    x, y, h, _ = pm.bench_problem(N, seed=3)
    px, py = pm.compact_order2(x, 256, 2), pm.compact_order2(y, 256, 2)
    return x[px], y[py], h[py]


@pytest.mark.parametrize("eps", [0.01**2, 0.02**2])
def test_dropped_mass_stays_under_the_budget_and_work_shrinks(clouds, eps):
    xs, ys, hs = clouds
    keep, mlb, t1, L = pm.plan_mass(xs, ys, hs, eps)
    keep_t, mlb_t, L_t = pm.plan(xs, ys, hs, eps)
    assert L == L_t and np.allclose(mlb, mlb_t, rtol=0, atol=1e-6 * np.abs(mlb_t).max())
    slabs = np.linspace(0, keep.shape[0] - 1, 10).astype(int)
    ev, k1, rec = pm.level2_mass(xs, ys, hs, eps, keep, L, slabs)
    ev_t, k1_t, _ = pm.level2(xs, ys, hs, eps, keep_t, L_t, slabs)
    # both levels prune here, and the mass rule does no more work than the term rule
    assert pm.kept_pairs(keep, N, N) < 0.9 * float(N) * N
    assert pm.kept_pairs(keep, N, N) <= pm.kept_pairs(keep_t, N, N)
    assert 0.0 < ev < 0.9 * k1 and k1 <= k1_t
    assert ev <= ev_t
    worst = 0.0
    for c in slabs:
        assert keep[c, rec[c]["home"]]                         # the home block is never dropped
        assert (rec[c]["t2"] >= rec[c]["ms"] - L).all()        # never below the term rule's threshold
        share = pm.dropped_share(xs, ys, hs, eps, keep[c], rec[c], c)
        worst = max(worst, float(share.max()))
    print(f"eps = {eps:.3g}: largest dropped share {worst:.3e} of 2^-26 = {2.0**-26:.3e}; evaluated {ev / k1:.3f} of the first level's pairs "
          f"(term rule {ev_t / k1_t:.3f} of {k1_t / k1:.3f} x as many)")
    assert worst < 2.0**-26


def test_thresholds_sit_on_bucket_edges_and_budgets_add_up(clouds):
    xs, ys, hs = clouds
    keep, mlb, t1, L = pm.plan_mass(xs, ys, hs, 0.01**2)
    q = (t1 - (mlb - L)) / pm.BUCKET_NATS
    assert np.allclose(q, np.round(q), atol=1e-6) and (q >= 0).all() and (q <= pm.BUCKETS).all()
    # first level + term rule + mass rule = 2^-26; the histogram covers ln M + 4 nats for every M an int holds
    assert abs(pm.BUDGET1 + 2.0**-26 / np.e + pm.BUDGET2 - 2.0**-26) < 1e-22
    assert pm.BUCKETS * pm.BUCKET_NATS >= np.log(2.0**31) + 4
    # the underflow bucket alone can never exceed its budget: at most ceil(M / 256) blocks resp. ceil(M / 32) groups, each below e^-L
    for M in (1000, 10**6, 2**31 - 1):
        eL = np.exp(-(np.log(M) + 26 * np.log(2) + pm.MARGIN))
        assert -(-M // pm.BLOCK) * eL <= pm.BUDGET1 and -(-M // pm.GROUP) * eL <= pm.BUDGET2


def test_stored_threshold_rounds_down():
    v = np.array([-1234.5678, 3.3, 1e5 + 0.123, -np.inf])
    f = pm.t2_as_stored(v)
    assert f.dtype == np.float32 and (f.astype(np.float64) <= v * pm.LOG2E).all() and f[3] == -np.inf
    assert (np.nextafter(f[:3], np.float32(np.inf)).astype(np.float64) > v[:3] * pm.LOG2E).all()
