"""Host-only check of the exact block-pruning bound (tools/prune_model.py restates csrc/glhip_prune.hip: prune_slabs_kernel):
no dropped column block holds a term above Mlb(R) - L for any row of its slab, so the dropped mass of a row is below 2^-26 of its sum."""

import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import prune_model as pm  # noqa: E402


@pytest.mark.parametrize("eps", [0.01**2, 0.05**2, 0.2**2])
def test_dropped_blocks_stay_below_the_bound(eps):
    x, y, h, _ = pm.bench_problem(40000, seed=3)
    px, py = pm.compact_order(x, 256), pm.compact_order(y, 512)
    xs, ys, hs = x[px], y[py], h[py]
    keep, mlb, L = pm.plan(xs, ys, hs, eps)
    assert keep.any(1).all()                         # every slab keeps at least its best block
    slabs = np.linspace(0, keep.shape[0] - 1, 24).astype(int)
    assert pm.check_dropped(xs, ys, hs, eps, keep, mlb, L, slabs) < 0.0
    # and Mlb is a lower bound on every row's largest exponent
    for c in slabs[:6]:
        xr = xs[c * pm.SLAB:(c + 1) * pm.SLAB].astype(np.float64)
        e = hs.astype(np.float64)[None] - ((xr[:, None] - ys.astype(np.float64)[None]) ** 2).sum(-1) / (2 * eps)
        assert (e.max(1) >= mlb[c]).all()


def test_clustered_clouds_prune_and_hold():
    rng = np.random.default_rng(0)
    centres = rng.random((8, 3))
    x = (centres[rng.integers(0, 8, 30000)] + 0.02 * rng.standard_normal((30000, 3))).astype(np.float32)
    y = (centres[rng.integers(0, 8, 30000)] + 0.02 * rng.standard_normal((30000, 3))).astype(np.float32)
    h = (0.3 * rng.standard_normal(30000)).astype(np.float32)
    eps = 0.05**2
    px, py = pm.compact_order(x, 256), pm.compact_order(y, 512)
    xs, ys, hs = x[px], y[py], h[py]
    keep, mlb, L = pm.plan(xs, ys, hs, eps)
    assert keep.mean() < 0.5                          # separated clusters: most blocks go
    assert pm.check_dropped(xs, ys, hs, eps, keep, mlb, L, range(keep.shape[0])) < 0.0
