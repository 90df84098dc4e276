"""Host-only check of the sum reference of the exact pruning (csrc/glhip_autosort.h, "Sum reference"; tools/prune_model.py: plan_mass /
level2_mass restate prune_slabs_kernel and prune_tiles_kernel of csrc/glhip_prune.hip): the two mass budgets are shares of e^Slb(R) and
e^ls(W), lower bounds of the row SUM that the block and group records give, where they were shares of one term of it.

On N = M = 20 000 points, D = 1, 2, 3, eps = 0.05^2 and 0.015^2, in the order of the sorted p = 2 call, five laws of the dual vector and
the clouds: the bench law, a uniform dual vector, log-weights spread over 20 nats, two far clusters, and the shells of
tests/test_prune_mass_gpu.py scaled down (many equal small terms around the term rule's threshold).  On each, in float64 on the
points themselves and for EVERY row: Slb(R) <= log S_i, ls(W) <= log S_i, and the share of the row's true sum that both levels drop
stays below 2^-26; and the rule keeps no block and evaluates no group that the old reference (reference="term") dropped.

The records' rounding: lse_dn never exceeds the float64 log sum exp of its columns on 10 000 random groups (spreads up to +-400 nats),
for the model's float64 sums and for sums formed in float32 as the device forms them, nor does a block's value formed from its groups.
"""

import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import prune_model as pm  # noqa: E402

N = 20000
BUDGET = 2.0**-26
LAWS = ["bench", "uniform", "spread", "clusters", "shells"]


def _law(name, D, eps, seed):
    """x (N, D), y (N, D), h (N,) float32"""
    r = np.random.default_rng(seed)
    x = r.random((N, D), dtype=np.float32)
    y = r.random((N, D), dtype=np.float32)
    h = np.full(N, -math.log(N), np.float32)
    if name == "bench":
        h = (h + 0.01 * r.standard_normal(N).astype(np.float32) / np.float32(0.05**2)).astype(np.float32)
    elif name == "spread":
        h = (h + 20.0 * (r.random(N, dtype=np.float32) - 0.5)).astype(np.float32)
    elif name == "clusters":      # two clusters of edge 0.25, 5 apart: the other cluster's terms underflow in float64
        x = (0.25 * x + np.where(r.random(N) < 0.5, 0.0, 5.0)[:, None].astype(np.float32)).astype(np.float32)
        y = (0.25 * y + np.where(r.random(N) < 0.5, 0.0, 5.0)[:, None].astype(np.float32)).astype(np.float32)
    elif name == "shells":
        # rows in a tight cluster; 512 columns inside it set every row's maximum; the others, with equal dual values, on 16 thin
        # shells whose terms run from ln M nats above the term rule's threshold to 3 nats below it; 768 columns in a far clump
        L = math.log(N) + 26 * math.log(2) + 1.0
        c = np.full(D, 0.5, np.float32)
        x = (c + 0.004 * (r.random((N, D), dtype=np.float32) - 0.5)).astype(np.float32)
        inside = c + 0.004 * (r.random((512, D), dtype=np.float32) - 0.5)
        far = c + np.float32(40.0) * np.sqrt(np.float32(2 * eps)) * np.eye(D, dtype=np.float32)[0] + 0.004 * (r.random((768, D), dtype=np.float32) - 0.5)
        per = (N - 512 - 768) // 16
        depth = np.linspace(L - math.log(N), L + 3.0, 16)
        radius = np.repeat(np.sqrt(2 * eps * depth), per)
        u = r.standard_normal((16 * per, D))
        shell = c + (radius[:, None] * u / np.linalg.norm(u, axis=1, keepdims=True))
        y = np.concatenate([inside, far, shell]).astype(np.float32)
        y = np.concatenate([y, y[: N - y.shape[0]]])[r.permutation(N)]
        h = np.zeros(N, np.float32)
    return x, y, h


def _sorted(x, y, h):
    sub = pm.sort_sub(x.shape[1])
    qx, qy = pm.balanced_order(x, pm.compact_order2(x, 256, sub)), pm.balanced_order(y, pm.compact_order2(y, 256, sub))
    return x[qx], y[qy], h[qy]


def _evaluated(rec):
    """per tile: the set of groups whose exponentials run"""
    return [set(rec["groups"][~s].tolist()) for s in rec["skip"]]


@pytest.mark.parametrize("eps", [0.05**2, 0.015**2], ids=["eps0.05", "eps0.015"])
@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("law", LAWS)
def test_bounds_and_dropped_share_on_every_row(law, D, eps):
    xs, ys, hs = _sorted(*_law(law, D, eps, 7 + D))
    got = []
    keep, mlb, t1, L = pm.plan_mass(xs, ys, hs, eps, slb_out=got)
    slb = got[0]
    keep0, mlb0, t10, _ = pm.plan_mass(xs, ys, hs, eps, reference="term")
    C = keep.shape[0]
    assert np.array_equal(mlb, mlb0) and (slb >= mlb).all() and (t1 >= t10).all()
    assert not (keep & ~keep0).any()                                   # no block the old reference dropped
    slabs = np.arange(C)
    ev, k1, rec = pm.level2_mass(xs, ys, hs, eps, keep, L, slabs)
    ev0, k10, rec0 = pm.level2_mass(xs, ys, hs, eps, keep0, L, slabs, reference="term")
    assert ev <= ev0 and k1 <= k10
    i2e = pm.inv2eps_of(eps)
    y64, h64 = torch.from_numpy(ys.astype(np.float64)), torch.from_numpy(hs.astype(np.float64))
    nG = (N + pm.GROUP - 1) // pm.GROUP
    worst_share, worst_slb, worst_ls = 0.0, -np.inf, -np.inf
    buf = torch.empty((2, pm.SLAB, N), dtype=torch.float64)
    for c in slabs:
        r0, r1 = c * pm.SLAB, min(N, (c + 1) * pm.SLAB)
        xr = torch.from_numpy(xs[r0:r1].astype(np.float64))
        e, tmp = buf[0][: r1 - r0].zero_(), buf[1][: r1 - r0]        # (two buffers for every slab: no fresh pages per slab)
        for d in range(D):
            torch.sub(xr[:, d, None], y64[None, :, d], out=tmp)
            e.addcmul_(tmp, tmp)
        e.mul_(-i2e).add_(h64[None])                                  # the exponents h_j - |x_i - y_j|^2 / (2 eps)
        tmax = e.max(1).values
        e.sub_(tmax[:, None]).exp_()
        total = e.sum(1)
        log_s = (tmax + torch.log(total)).numpy()
        worst_slb = max(worst_slb, float((slb[c] - log_s).max()))
        gone1 = np.repeat(~keep[c], pm.BLOCK)[:N]
        new, old = _evaluated(rec[c]), _evaluated(rec0[c])
        for t in range(len(rec[c]["ls"])):
            rows = slice(t * pm.TILE, min((t + 1) * pm.TILE, r1 - r0))
            assert rec[c]["ls"][t] >= rec[c]["ms"][t] and rec[c]["t2"][t] >= rec0[c]["t2"][t]
            worst_ls = max(worst_ls, float((rec[c]["ls"][t] - log_s[rows]).max()))
            assert new[t] <= old[t], (c, t)                           # no group the old reference skipped
            skipped = np.zeros(nG, bool)
            skipped[rec[c]["groups"][rec[c]["skip"][t]]] = True
            gone = torch.from_numpy(gone1 | np.repeat(skipped, pm.GROUP)[:N]).double()
            worst_share = max(worst_share, float(((e[rows] @ gone) / total[rows]).max()))
    print(f"{law} D = {D} eps = {eps:.3g}: first level keeps {keep.mean():.4f} (term reference {keep0.mean():.4f}), evaluated {ev / N / N:.4f} "
          f"({ev0 / N / N:.4f}); Slb - Mlb mean {(slb - mlb).mean():.3f} nats; max(Slb - log S) {worst_slb:.3e}, max(ls - log S) {worst_ls:.3e}, "
          f"largest dropped share {worst_share:.3e} (budget {BUDGET:.3e})")
    assert worst_slb <= 0.0 and worst_ls <= 0.0
    assert worst_share < BUDGET


def _f32_lse(hp):
    """a group's or block's value as the device forms it before rounding up: float32 exponentials around the maximum, a float32 tree sum"""
    hp = hp.astype(np.float32)
    m = hp.max(1)
    with np.errstate(over="ignore", invalid="ignore"):
        se = np.exp((hp - m[:, None]).astype(np.float32)).astype(np.float32)
    while se.shape[1] > 1:
        se = (se[:, 0::2] + se[:, 1::2]).astype(np.float32)
    return (m + np.log(se[:, 0]).astype(np.float32)).astype(np.float32)


def _up(v):
    return (v + pm.LSE_SLACK * (np.abs(v) + np.float32(8.0))).astype(np.float32)


def _lse64(hp):
    m = hp.max(1)
    return m + np.log(np.array([math.fsum(row) for row in np.exp(hp - m[:, None])]))


def test_lse_dn_never_exceeds_the_float64_lse():
    r = np.random.default_rng(5)
    n = 10000
    centre = r.uniform(-400.0, 400.0, n)
    spread = np.concatenate([np.zeros(n // 5), r.uniform(0.0, 1.0, n // 5), r.uniform(0.0, 20.0, n // 5), r.uniform(0.0, 400.0, n - 3 * (n // 5))])
    hp = (centre[:, None] + spread[:, None] * (2 * r.random((n, 32)) - 1)).astype(np.float32)
    hp[: n // 10, 5:] = -np.inf                                       # short groups: the padding of the last one
    true = _lse64(hp.astype(np.float64))
    model, dev = pm.lse_up(hp.astype(np.float64)), _up(_f32_lse(hp)).astype(np.float64)
    for name, v in (("model", model), ("float32 sums", dev)):
        assert (v >= true).all(), name                                 # the record is rounded up
        dn = pm.lse_dn(v, 2)
        print(f"{name}: record - lse in [{(v - true).min():.3e}, {(v - true).max():.3e}], lse - lse_dn in [{(true - dn).min():.3e}, {(true - dn).max():.3e}]")
        assert (dn <= true).all(), name
    # blocks: eight rounded-up group values, summed and rounded up once more, lowered by four slacks
    nb = n // 8
    tb = _lse64(hp[: nb * 8].astype(np.float64).reshape(nb, 256))
    for name, v in (("model", pm.lse_up(model[: nb * 8].reshape(nb, 8))), ("float32 sums", _up(_f32_lse(dev[: nb * 8].reshape(nb, 8))).astype(np.float64))):
        assert (v >= tb).all() and (pm.lse_dn(v, 4) <= tb).all(), name
    assert pm.lse_dn(np.array([-np.inf]))[0] == -np.inf


def test_reference_blocks_rule():
    """whole cells of the score grid from the top while at most K - 1 blocks are in, the home block always, ascending"""
    mlb = 3.0
    score = mlb + pm.REF_TOP - np.array([0.01, 0.02, 0.10, 0.11, 0.12, 5.0, 40.0, np.inf])      # cells 0, 0, 1, 1, 1, 80, past the grid
    assert pm.reference_blocks(score, mlb, home=6, K=3).tolist() == [0, 1, 6]
    assert pm.reference_blocks(score, mlb, home=0, K=3).tolist() == [0, 1]
    assert pm.reference_blocks(score, mlb, home=5, K=6).tolist() == [0, 1, 2, 3, 4, 5]
    assert pm.reference_blocks(score, mlb, home=7, K=2).tolist() == [7]
    assert pm.reference_blocks(score, mlb, home=2, K=32).tolist() == [0, 1, 2, 3, 4, 5]
