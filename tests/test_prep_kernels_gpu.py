"""The preparation kernels of the pruned p = 2 call after their rework (csrc/glhip_prune.hip: prune_slabs_kernel closes gaps from the
bit set, prune_tiles_kernel maps a thread to a (group, tile) pair, balance_kernel partitions its upper levels) at the smallest shapes
that prune (N M >= 1e11, N >= 65536): 65536 x 1525900 (256 slabs, 5961 column blocks), 320000 x 320000 and 317000 x 320037 with D = 2.

* two glhip_prune_inspect calls return identical perm_x, perm_y, home, intervals and t2;
* on the rare-column law of tests/test_prune_thresholds_fast_gpu.py ("many_runs": 0.3 % of the dual values 150 nats up, a fifth of
  the slabs over kPruneRuns runs) the intervals of EVERY slab over the run limit cover exactly the model's kept blocks with the
  smallest gaps closed, and t2 follows tools/prune_model.py: level2_mass on 24 slabs under that file's conditions (exact, or one bucket
  away in at most 1 % of the finite tiles); the same interval check on the wide shape, whose bit set has 94 words;
* bf16 input and D = 1 once each through the pruned forward against the dense launch, within the bound of
  prune_support.close (4e-7 diam^2 + 2e-6 of the output's magnitude).
"""

import math

import numpy as np
import pytest
import torch

import prune_support as ps
from prune_support import RECORDS, pm

pytestmark = pytest.mark.gpu

DEV = ps.DEV


def _input(name):
    """x (n, D), y (m, D), h (m,) on the host, eps.  many_runs is the input of that name of tests/test_prune_thresholds_fast_gpu.py"""
    seed, n, m, D, eps, rare = {"wide": (71, 65536, 1525900, 3, 0.05**2, 0.003), "many_runs": (64, 320000, 320000, 3, 0.05**2, 0.003),
                                "d2_uneven": (72, 317000, 320037, 2, 0.03**2, 0.0)}[name]
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, D, generator=g)
    y = torch.rand(m, D, generator=g)
    h = torch.full((m,), -math.log(m)) + 0.01 * torch.randn(m, generator=g) / 0.05**2
    if rare:
        h[torch.rand(m, generator=g) < rare] += 150.0
    return x, y, h, eps


_CACHE = {}


def _case(name):
    """two sets of device records and the model's first level on the device's order, once per input"""
    if name not in _CACHE:
        x, y, h, eps = _input(name)
        dx, dy, dh = x[None].to(DEV).contiguous(), y[None].to(DEV).contiguous(), h[None].to(DEV).contiguous()
        rec, again = ps.inspect(dx, dy, dh, eps), ps.inspect(dx, dy, dh, eps)
        n, m = x.shape[0], y.shape[0]
        assert np.array_equal(np.sort(rec["perm_x"]), np.arange(n)) and np.array_equal(np.sort(rec["perm_y"]), np.arange(m))
        xs, ys, hs = x.numpy()[rec["perm_x"]], y.numpy()[rec["perm_y"]], h.numpy()[rec["perm_y"]]
        _CACHE[name] = (rec, again, xs, ys, hs, eps, pm.plan_mass(xs, ys, hs, eps))
    return _CACHE[name]


@pytest.mark.parametrize("name", ["wide", "many_runs", "d2_uneven"])
def test_records_repeat(name):
    rec, again = _case(name)[:2]
    for k in RECORDS:
        assert np.array_equal(rec[k], again[k], equal_nan=k in ("mlb", "t1", "t2")), k
    assert (rec["home"] >= 0).any() and np.isfinite(rec["t2"]).any()      # the input prunes: both levels ran


def _closed(keep_row):
    """tests/test_prune_thresholds_fast_gpu.py: the kept blocks with the smallest gaps closed, g one more than the RUNS-th longest gap"""
    idx = np.flatnonzero(keep_row)
    gaps = np.diff(idx) - 1
    gaps = gaps[gaps > 0]
    if len(gaps) + 1 <= pm.RUNS:
        return keep_row
    g = np.sort(gaps)[::-1][pm.RUNS - 1] + 1
    out = keep_row.copy()
    for a, b in zip(idx[:-1], idx[1:]):
        if b - a - 1 < g:
            out[a:b] = True
    return out


def _on_model_bucket(rec, mlb, t1, L):
    q_dev = np.round((rec["t1"] - (rec["mlb"] - L)) / pm.BUCKET_NATS).astype(int)
    q_mod = np.round((t1 - (mlb - L)) / pm.BUCKET_NATS).astype(int)
    return q_dev == q_mod


@pytest.mark.parametrize("name", ["many_runs", "wide"])
def test_closed_gaps_on_every_slab_over_the_limit(name):
    rec, _, xs, ys, hs, eps, (keep, mlb, t1, L) = _case(name)
    C, nT = keep.shape
    M = ys.shape[0]
    same = _on_model_bucket(rec, mlb, t1, L)      # (a threshold within float64 rounding of a bucket edge: that file allows 1 % of the slabs)
    runs = pm.runs_per_slab(keep)
    over = np.flatnonzero((runs > pm.RUNS) & same)
    print(f"{name}: {int((runs > pm.RUNS).sum())} of {C} slabs over {pm.RUNS} runs (most: {runs.max()}), {len(over)} of them on the model's t1 bucket")
    assert int((~same).sum()) <= C // 100 and len(over) > C // 10
    S = rec["intervals"].shape[1]
    pieces = []
    for c in over:
        iv = rec["intervals"][c]
        live = iv[:, 1] > iv[:, 0]
        n = int(live.sum())
        assert live[:n].all() and (iv[n:] == 0).all(), c
        assert (iv[:n, 0] % pm.BLOCK == 0).all() and (np.diff(iv[:n].ravel()) >= 0).all(), c
        assert ((iv[:n, 1] % pm.BLOCK == 0) | (iv[:n, 1] == M)).all(), c
        assert n <= S and (np.diff(iv[:n, 0]) > 0).all(), c
        want = _closed(keep[c])
        assert np.array_equal(ps.covered(rec, c, nT), want), c
        assert pm.runs_per_slab(want[None])[0] <= pm.RUNS, c
        pieces.append(n)
    print(f"{name}: pieces per checked slab {min(pieces)} to {max(pieces)} of {S} slots")


def test_second_level_with_closed_gaps():
    rec, _, xs, ys, hs, eps, (keep, mlb, t1, L) = _case("many_runs")
    same = _on_model_bucket(rec, mlb, t1, L)
    runs = pm.runs_per_slab(keep)
    has = np.flatnonzero((rec["home"] >= 0) & same)
    over = has[runs[has] > pm.RUNS]
    slabs = np.unique(np.concatenate([has[:: max(1, len(has) // 12)][:12], over[:: max(1, len(over) // 12)][:12]]))
    assert 12 <= len(slabs) <= 24 and (runs[slabs] > pm.RUNS).sum() >= 6
    iv = {c: [(int(a), int(b)) for a, b in rec["intervals"][c] if b > a] for c in slabs}
    _, _, l2 = pm.level2_mass(xs, ys, hs, eps, keep, L, slabs, intervals=iv)
    got, want = [], []
    for c in slabs:
        assert l2[c]["home"] == rec["home"][c], c
        k = len(l2[c]["t2"])
        want.append(pm.t2_as_stored(l2[c]["t2"]))
        got.append(rec["t2"][c * 8:c * 8 + k])
    got, want = np.concatenate(got), np.concatenate(want).astype(np.float32)
    fin = np.isfinite(want)
    assert fin.mean() > 0.5 and np.array_equal(np.isinf(got), np.isinf(want))      # the sampled tiles have a finite model t2
    d = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64))
    off = int((d > 0).sum())
    print(f"many_runs: {len(slabs)} slabs, t2 of {off} of {int(fin.sum())} finite tiles off the model's value "
          f"(largest distance {d.max() / (pm.BUCKET_NATS * pm.LOG2E):.3f} buckets)")
    assert d.max() <= pm.BUCKET_NATS * pm.LOG2E + 4 * np.spacing(np.abs(want[fin]).max()) and off <= int(fin.sum()) // 100


# ---- the pruned forward against the dense launch ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,dtype", [(3, torch.bfloat16), (1, torch.float32)], ids=["bf16", "d1"])
def test_pruned_forward_matches_dense(D, dtype):
    n, m, eps = 320000, 320037, 0.05**2
    x, y, h = ps.law(n, m, 80 + D, D=D, dtype=dtype)
    err, bound = ps.close(ps.fwd(x, y, h, eps, ps.F16X2), ps.fwd(x, y, h, eps, ps.F16X2 | ps.NO_SORT), ps.diam2(x, y), require_finite=True)
    print(f"D = {D} {dtype}: pruned against dense, largest difference {err:.3e} (bound {bound:.3e})")
