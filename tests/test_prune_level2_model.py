"""Host-only check of the second pruning level (tools/prune_model.py: level2 restates csrc/glhip_softmin_x32.h, P2): inside the kept
blocks a 32-row tile skips a group of 32 columns only if every term of the group lies below (true row maximum - L) for every row of the
tile, checked on the points themselves; and the order of the sorted p = 2 call (compact_order2) is a permutation that keeps the voxel
order of compact_order."""

import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import prune_model as pm  # noqa: E402


def _sorted(x, y, h, sub):
    px, py = pm.compact_order2(x, 256, sub), pm.compact_order2(y, 256, sub)
    return x[px], y[py], h[py]


@pytest.mark.parametrize("eps", [0.01**2, 0.05**2, 0.2**2])
@pytest.mark.parametrize("sub", [1, 2])
def test_uniform_clouds_skipped_pairs_stay_below_the_bound(eps, sub):
    x, y, h, _ = pm.bench_problem(40000, seed=3)
    xs, ys, hs = _sorted(x, y, h, sub)
    keep, mlb, L = pm.plan(xs, ys, hs, eps)
    slabs = np.linspace(0, keep.shape[0] - 1, 12).astype(int)
    ev, k1, worst = pm.level2(xs, ys, hs, eps, keep, L, slabs, check=True)
    assert 0.0 < ev <= k1
    assert worst < 0.0


def test_clustered_clouds_skip_and_hold():
    rng = np.random.default_rng(0)
    centres = rng.random((8, 3))
    x = (centres[rng.integers(0, 8, 30000)] + 0.02 * rng.standard_normal((30000, 3))).astype(np.float32)
    y = (centres[rng.integers(0, 8, 30000)] + 0.02 * rng.standard_normal((30000, 3))).astype(np.float32)
    h = (0.3 * rng.standard_normal(30000)).astype(np.float32)
    h[::997] += 40.0                                  # a few columns far above the rest: their groups stay, the seed is not the maximum
    eps = 0.02**2
    xs, ys, hs = _sorted(x, y, h, 2)
    keep, mlb, L = pm.plan(xs, ys, hs, eps)
    ev, k1, worst = pm.level2(xs, ys, hs, eps, keep, L, range(0, keep.shape[0], 5), check=True)
    assert ev < 0.9 * k1                              # the second level removes work the first keeps
    assert worst < 0.0


def test_second_level_removes_more_with_compact_groups():
    x, y, h, eps = pm.bench_problem(60000, seed=5)
    eps = 0.02**2
    share = {}
    for sub in (1, 2):
        xs, ys, hs = _sorted(x, y, h, sub)
        keep, mlb, L = pm.plan(xs, ys, hs, eps)
        ev, k1, _ = pm.level2(xs, ys, hs, eps, keep, L, np.linspace(0, keep.shape[0] - 1, 16).astype(int))
        share[sub] = ev / k1
    assert share[2] < share[1] < 1.0


@pytest.mark.parametrize("D", [1, 2, 3])
def test_minor_key_refines_the_voxel_order(D):
    rng = np.random.default_rng(D)
    z = rng.random((20000, D)).astype(np.float32)
    p1, p2 = pm.compact_order2(z, 256, 1), pm.compact_order2(z, 256, pm.sort_sub(D))
    assert np.array_equal(np.sort(p2), np.arange(20000))
    assert np.array_equal(p1, pm.compact_order(z, 256))          # sub = 1 is the order of the distance launches
    # same voxels in the same order: the voxel key along p2 is non-decreasing and equals the one along p1
    lo = z.min(0)
    ext = z.max(0) - lo
    voxel = np.float32(np.power(np.float32(np.prod(ext) * np.float32(256) / np.float32(20000)), np.float32(1.0 / D)))
    q = (np.floor(z / voxel) - np.floor(lo / voxel)).astype(np.int64)
    vox = lambda p: [tuple(v) for v in q[p]]
    seq1, seq2 = vox(p1), vox(p2)
    assert [v for i, v in enumerate(seq1) if i == 0 or v != seq1[i - 1]] == [v for i, v in enumerate(seq2) if i == 0 or v != seq2[i - 1]]
