"""What prune_slabs_kernel and prune_tiles_kernel (csrc/glhip_prune.hip) hand to the sorted p = 2 launch — every slab's Mlb, t1, home
block and column intervals, every tile's t2 — against the NumPy model (tools/prune_model.py) on the device's own order, read through
glhip_prune_inspect.  tests/test_prune_mass_gpu.py does this on the headline law at an even shape; here are the inputs on which the
kept blocks are found from the 64-bit words of a bit set (csrc/glhip_prune_words.h) and on which a cheaper evaluation of the keys could
go wrong: D = 2 at a shape that is no multiple of 64 blocks, 256 columns or 32 rows; dual values of +-400 nats at eps = 0.005^2, where a
float32 key is spaced ~0.01 nat; half of the dual values exactly equal, so that whole families of keys coincide; and rare columns far
above the rest, where a fifth of the slabs have more than kPruneRuns runs and close their smallest gaps (the walk that reads the bit set).

Conditions, those of the existing test: Mlb to float64 rounding; t1 on the model's bucket (one bucket away in at most 1 % of the slabs,
where a key or a running sum lies within rounding of an edge); home and the intervals exact on the other slabs, gap closing included;
t2 exact or one bucket away in at most 1 % of the finite tiles.  Every input was run through the model on the CPU first, in the model's own order: all sampled tiles
get a finite t2 above the term rule's threshold, the first level keeps 17-38 % of the blocks, and the last input has 250 of 1250
slabs over the run limit (the first three: none).  On the large-exponent input the float64 sum of what the device's thresholds drop
is held to 2^-26 of each row's sum on 64 tiles, as tests/test_prune_mass_gpu.py does on its shells.
"""

import math

import numpy as np
import pytest
import torch

import prune_support as ps
from prune_support import pm

pytestmark = pytest.mark.gpu

DEV = ps.DEV
BUDGET = 2.0**-26


def _input(name):
    """x (n, D), y (m, D), h (m,) on the host, eps"""
    seed, n, m, D, eps = {"d2_uneven": (61, 317000, 320037, 2, 0.03**2), "large_exponents": (62, 320000, 320000, 3, 0.005**2),
                          "equal_duals": (63, 320000, 320000, 3, 0.05**2), "many_runs": (64, 320000, 320000, 3, 0.05**2)}[name]
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, D, generator=g)
    y = torch.rand(m, D, generator=g)
    base = torch.full((m,), -math.log(m))
    if name == "d2_uneven":
        h = base + 0.001 * torch.randn(m, generator=g) / 0.05**2
    elif name == "large_exponents":
        h = base + 400.0 * (2 * torch.rand(m, generator=g) - 1)
    else:
        h = base + 0.01 * torch.randn(m, generator=g) / 0.05**2
        if name == "equal_duals":
            h[torch.rand(m, generator=g) < 0.5] = -math.log(m)
        else:
            h[torch.rand(m, generator=g) < 0.003] += 150.0
    return x, y, h, eps


_CACHE = {}


def _case(name):
    """device records and the model's first level on the device's order, once per input"""
    if name not in _CACHE:
        x, y, h, eps = _input(name)
        rec = ps.inspect(x[None].to(DEV).contiguous(), y[None].to(DEV).contiguous(), h[None].to(DEV).contiguous(), eps)
        n, m = x.shape[0], y.shape[0]
        assert np.array_equal(np.sort(rec["perm_x"]), np.arange(n)) and np.array_equal(np.sort(rec["perm_y"]), np.arange(m))
        xs, ys, hs = x.numpy()[rec["perm_x"]], y.numpy()[rec["perm_y"]], h.numpy()[rec["perm_y"]]
        _CACHE[name] = (rec, xs, ys, hs, eps, pm.plan_mass(xs, ys, hs, eps))
    return _CACHE[name]


def _closed(keep_row):
    """the kept blocks with the smallest gaps closed: g = the smallest gap length that leaves at most RUNS runs, gaps shorter than g
    are closed (csrc/glhip_autosort.h)"""
    idx = np.flatnonzero(keep_row)
    gaps = np.diff(idx) - 1
    gaps = gaps[gaps > 0]
    if len(gaps) + 1 <= pm.RUNS:
        return keep_row
    g = np.sort(gaps)[::-1][pm.RUNS - 1] + 1      # RUNS - 1 gaps may stay open: the largest ones; g is one more than the next
    out = keep_row.copy()
    for a, b in zip(idx[:-1], idx[1:]):
        if b - a - 1 < g:
            out[a:b] = True
    return out


@pytest.mark.parametrize("name", ["d2_uneven", "large_exponents", "equal_duals", "many_runs"])
def test_first_level_matches_the_model(name):
    rec, xs, ys, hs, eps, (keep, mlb, t1, L) = _case(name)
    C, nT = keep.shape
    M = ys.shape[0]
    assert np.allclose(rec["mlb"], mlb, rtol=1e-12, atol=1e-9)
    q_dev = np.round((rec["t1"] - (rec["mlb"] - L)) / pm.BUCKET_NATS).astype(int)
    q_mod = np.round((t1 - (mlb - L)) / pm.BUCKET_NATS).astype(int)
    # as tests/test_prune_mass_gpu.py: a threshold sits on the model's bucket, or one bucket away where a key or a running sum lies
    # within float64 rounding of an edge — counted, and capped at 1 % of the slabs; everything else is compared on the other slabs
    off1 = int((q_dev != q_mod).sum())
    print(f"{name}: t1 of {off1} of {C} slabs off the model's bucket")
    assert np.abs(q_dev - q_mod).max() <= 1 and off1 <= C // 100
    same = q_dev == q_mod
    assert np.allclose(rec["t1"][same], t1[same], rtol=1e-12, atol=1e-9)
    assert 0.05 < keep.mean() < 0.9                                   # the input prunes, and keeps something
    runs = pm.runs_per_slab(keep)
    print(f"{name}: first level keeps {keep.mean():.4f} of the blocks; runs per slab mean {runs.mean():.1f} max {runs.max()}, "
          f"{int((runs > pm.RUNS).sum())} of {C} slabs over {pm.RUNS}")
    assert ((runs > pm.RUNS).sum() > C // 10) == (name == "many_runs")
    assert np.array_equal((rec["home"] >= 0)[same], ~keep[same].all(1))
    S = rec["intervals"].shape[1]
    over = np.flatnonzero(runs > pm.RUNS)
    for c in np.unique(np.concatenate([np.arange(0, C, max(1, C // 150)), over[:40], [C - 1]])):
        if not same[c]:
            continue
        iv = rec["intervals"][c]
        live = iv[:, 1] > iv[:, 0]
        n = int(live.sum())
        assert live[:n].all() and (iv[n:] == 0).all(), c              # the pieces first, in order; unused slots empty
        assert (iv[:n, 0] % pm.BLOCK == 0).all() and (np.diff(iv[:n].ravel()) >= 0).all(), c
        assert ((iv[:n, 1] % pm.BLOCK == 0) | (iv[:n, 1] == M)).all(), c
        assert n <= S and (np.diff(iv[:n, 0]) > 0).all(), c
        assert np.array_equal(ps.covered(rec, c, nT), _closed(keep[c])), c


@pytest.mark.parametrize("name", ["d2_uneven", "large_exponents", "equal_duals"])
def test_second_level_matches_the_model(name):
    rec, xs, ys, hs, eps, (keep, mlb, t1, L) = _case(name)
    C = keep.shape[0]
    q_dev = np.round((rec["t1"] - (rec["mlb"] - L)) / pm.BUCKET_NATS).astype(int)
    q_mod = np.round((t1 - (mlb - L)) / pm.BUCKET_NATS).astype(int)
    has = np.flatnonzero((rec["home"] >= 0) & (q_dev == q_mod))
    slabs = has[:: max(1, len(has) // 100)]
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
    assert fin.mean() > 0.5 and np.array_equal(np.isinf(got), np.isinf(want))      # not vacuous: the CPU run of the model said all
    d = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64))
    off = int((d > 0).sum())
    print(f"{name}: t2 of {off} of {int(fin.sum())} tiles off the model's value (largest distance {d.max() / (pm.BUCKET_NATS * pm.LOG2E):.3f} buckets)")
    assert d.max() <= pm.BUCKET_NATS * pm.LOG2E + 4 * np.spacing(np.abs(want[fin]).max()) and off <= int(fin.sum()) // 100


def test_dropped_mass_at_large_exponents():
    """64 tiles of the large-exponent input: the columns outside the slab's intervals and, inside them, every group whose float64 key
    lies below max(t2, smallest true row maximum - L) sum in float64 to less than 2^-26 of each row's sum."""
    rec, xs, ys, hs, eps, (keep, mlb, t1, L) = _case("large_exponents")
    N, M = xs.shape[0], ys.shape[0]
    xs, ys, hs = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV).double() for a in (xs, ys, hs))
    i2e = pm.inv2eps_of(eps)
    nG = (M + 31) // 32
    pad = nG * 32 - M
    yg = torch.cat([ys, ys[-1:].expand(pad, 3)]).view(nG, 32, 3)
    glo, ghi = yg.min(1).values, yg.max(1).values
    glse = torch.logsumexp(torch.cat([hs, hs.new_full((pad,), -math.inf)]).view(nG, 32), 1)
    worst, dropped_cols, tiles = 0.0, 0, 0
    for w in np.linspace(0, N // 32 - 1, 64).astype(int):
        c = w // 8
        if rec["home"][c] < 0:
            continue
        tiles += 1
        xr = xs[w * 32:(w + 1) * 32]
        terms = hs[None] - ((xr[:, None, :] - ys[None]) ** 2).sum(-1) * i2e
        tmax = terms.max(1).values
        total = torch.exp(terms - tmax[:, None]).sum(1)
        inside = torch.zeros(nG, dtype=torch.bool, device=DEV)
        for a, b in rec["intervals"][c]:
            if b > a:
                inside[a // 32:(b + 31) // 32] = True
        gap = torch.clamp(torch.maximum(glo - xr.max(0).values, xr.min(0).values - ghi), min=0.0)
        key = glse - (gap**2).sum(1) * i2e
        t2 = float(rec["t2"][w]) / pm.LOG2E
        assert math.isfinite(t2)
        thr = max(t2 + 1e-9 * abs(t2), float(tmax.min()) - L)
        gone = (~inside | (key < thr)).repeat_interleave(32)[:M]
        share = (torch.exp(terms - tmax[:, None]) * gone[None]).sum(1) / total
        worst = max(worst, float(share.max()))
        dropped_cols += int(gone.sum())
    print(f"largest share a row may lose {worst:.3e} (budget 2^-26 = {BUDGET:.3e}); {dropped_cols / max(tiles, 1) / M:.3f} of the columns "
          f"dropped per sampled tile, {tiles} tiles")
    assert tiles >= 32 and worst < BUDGET and dropped_cols > 0
