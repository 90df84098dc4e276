"""Host-side checks of tests/dual_patterns.py: each pattern does, on the clouds and temperatures the GPU test uses, what
tests/test_hostile_duals_gpu.py relies on — in float64, without a GPU.  A pattern that cannot tell a kernel with a broken rescale from a
right one fails here, not silently on the GPU."""
import functools

import numpy as np
import pytest

import dual_patterns as dp

CASES = [(N, M, D, p) for (N, M) in dp.SHAPES for (D, p) in dp.CONFIGS]


@functools.lru_cache(maxsize=None)
def _case(N, M, D, p):
    x, y, eps = dp.clouds(D, p, N, M)
    return x, y, eps, dp.patterns(M, np.random.default_rng(M + D))


@functools.lru_cache(maxsize=None)
def _weights(N, M, D, p, name):
    x, y, eps, pats = _case(N, M, D, p)
    E = dp.log_weights(x, y, pats[name], eps, p)
    return E, dp.relative_weights(E)


@pytest.mark.parametrize("N,M,D,p", CASES)
def test_one_hot_patterns_are_one_hot(N, M, D, p):
    for name in dp.ONE_HOT:
        _, W = _weights(N, M, D, p, name)
        second = np.sort(W, axis=1)[:, -2]
        print(f"{name} N={N} M={M} D={D} p={p}: second-largest weight {second.max():.2e} of the largest")
        assert (W.max(1) == 1.0).all() and second.max() <= 2.0 ** -60, name


@pytest.mark.parametrize("N,M,D,p", CASES)
def test_ramp_makes_the_running_maximum_grow(N, M, D, p):
    E, _ = _weights(N, M, D, p, "ramp")
    _, _, grew = dp.plan_model(E, np.zeros((M, 1)))
    R = min(256, M)
    first = (M - R) // dp.GROUP                      # the group that holds the first column of the ramp
    count = grew[:, first:].sum(1)
    print(f"ramp N={N} M={M} D={D} p={p}: the maximum grows at {count.min()} ... {count.max()} of the {grew.shape[1] - first} groups of the ramp")
    assert count.min() >= 7


@pytest.mark.parametrize("N,M,D,p", CASES)
def test_descent_reaches_the_f16_subnormal_band(N, M, D, p):
    """2^13 w is an f16 subnormal for w in (2^-37, 2^-27) of the row maximum."""
    _, W = _weights(N, M, D, p, "descent")
    band = ((W > 2.0 ** -37) & (W < 2.0 ** -27)).sum(1)
    share = (np.where(W < 2.0 ** -27, W, 0.0).sum(1) / W.sum(1)).max()
    print(f"descent N={N} M={M} D={D} p={p}: {band.min()} ... {band.max()} columns in the band, mass share below 2^-27 {share:.2e}")
    assert band.min() >= 4


@pytest.mark.parametrize("N,M,D,p", CASES)
def test_twin_splits_the_mass_somewhere(N, M, D, p):
    _, W = _weights(N, M, D, p, "twin")
    a, b = W[:, 3] / W.sum(1), W[:, M - 2] / W.sum(1)
    both = np.minimum(a, b)
    print(f"twin N={N} M={M} D={D} p={p}: smaller peak holds up to {both.max():.3f} of a row's mass, ratio up to {(both / np.maximum(a, b)).max():.2f}")
    assert both.max() > 0.10


@pytest.mark.parametrize("N,M,D,p", CASES)
def test_teeth(N, M, D, p):
    """The model without the rescale is at least 100 bounds away from float64, in the measure and at the bound of each entry point."""
    x, y, eps, _ = _case(N, M, D, p)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    feat = np.random.default_rng(7).standard_normal((M, 5))

    def unit(j0, j1):      # the directions (x_i - y_j) / |x_i - y_j| of the p = 1 gradient
        diff = x64[:, None, :] - y64[None, j0:j1, :]
        d2 = (diff * diff).sum(-1, keepdims=True)
        return np.where(d2 > 1e-8, diff / np.sqrt(np.maximum(d2, 1e-300)), 0.0)

    for name in ("late", "stairs", "ramp"):
        E, _ = _weights(N, M, D, p, name)
        ref, lse = dp.reference(E, feat)
        good, glse, _ = dp.plan_model(E, feat)
        bad, blse, _ = dp.plan_model(E, feat, rescale=False)
        scale = np.abs(feat).max(0)
        plan = (np.abs(bad - ref) / scale).max() / dp.PLAN_BOUND
        assert (np.abs(good - ref) / scale).max() <= 1e-12 and np.abs(glse - lse).max() <= 1e-9 * max(1.0, np.abs(lse).max())
        gfeat = unit if p == 1 else y64
        gref, _ = dp.reference(E, gfeat)
        gbad, _, _ = dp.plan_model(E, gfeat, rescale=False)
        gref, gbad = (gref, gbad) if p == 1 else (x64 - gref, x64 - gbad)
        grad = np.abs(gbad - gref).max() / np.abs(gref).max() / dp.grad_bound(D, p)
        figures = {"plan": plan, "gradient": grad}
        if p == 1 and name != "stairs":      # (on `stairs` the soft-min is -eps 5000 and its bound grows with it: the weighted sums have the teeth)
            figures["soft-min"] = eps * np.abs(blse - lse).max() / dp.p1_value_bound(-eps * lse, D)
        print(f"teeth {name} N={N} M={M} D={D} p={p}: without the rescale, in bounds: " + ", ".join(f"{k} {v:.3g}" for k, v in figures.items()))
        assert min(figures.values()) >= 100, (name, figures)


def test_patterns_are_valid_inputs():
    for M in (256, 300, 1000, 5000):
        pats = dp.patterns(M, np.random.default_rng(M))
        assert set(pats) == set(dp.ONE_HOT + dp.SPREAD + dp.F64_ONLY)
        for name in dp.VOIDS:
            assert np.isneginf(pats[name]).sum() == (M // 2 if name == "half_void" else 160), name
        feat = dp.feature_patterns(M, 6, np.random.default_rng(1))
        assert feat.dtype == np.float32 and np.isfinite(feat).all() and (feat[:, 3] == 0).all() and (feat[:, 4] == 2.5).all()
        assert 1e-12 * 0.9 <= np.abs(feat[:, 0]).min() and np.abs(feat[:, 0]).max() <= 1e12
