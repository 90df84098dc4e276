"""The sum reference of the exact pruning on the device (csrc/glhip_autosort.h, "Sum reference"; prune_slabs_kernel and
prune_tiles_kernel of csrc/glhip_prune.hip): the mass budgets of both levels are shares of a lower bound of the row SUM.

Shapes.  The p = 2 call prunes from 1e11 pairs on (prune_applies); below that glhip_prune_inspect answers GLHIP_EUNSUPPORTED and the
forward call IS the dense launch, so a smaller shape would test nothing here.  The two shapes are the smallest that prune: an even one,
320 000 x 320 000, and one that is no multiple of 256 rows, 256 columns or 32 rows, 320 037 x 313 000.

Against the model (tools/prune_model.py on the device's own order, read through glhip_prune_inspect), under the conditions of
tests/test_prune_thresholds_fast_gpu.py: Mlb to float64 rounding; t1 on the model's bucket, one bucket away in at most 1 % of the slabs;
home and the kept blocks exact on the other slabs; t2 exact or one bucket away in at most 1 % of the finite tiles.  Inputs: D = 3 and
D = 2, float32 and bfloat16 clouds, the bench law and a uniform dual vector, and the half-step (`pot` given).  The model against itself
with every group's and block's lse moved up by one float32 ulp, on each of these inputs on the host (model's own order, 100 slabs for the
second level): t1 of 0 of 1250 slabs and t2 of 0 of 840 tiles move, on every input.

Values: the pruned call against the dense launch (GLHIP_FLAG_NO_SORT) on all rows and against float64 on 2048 rows, both layouts, bound
4e-7 diam^2 + 2e-6 max|value|.  Special values: one slab with a NaN coordinate, a group with h = +inf, all h = -inf — the non-finite
pattern equals the dense launch's and the finite rows stay within the bound.
"""

import math

import numpy as np
import pytest
import torch

import prune_support as ps
from prune_support import pm

pytestmark = pytest.mark.gpu

DEV, NO_SORT, LAYOUTS = ps.DEV, ps.NO_SORT, ps.LAYOUTS
EVEN, UNEVEN = (320000, 320000), (320037, 313000)

# name: (shape, D, cloud dtype, law, eps, half-step)
CASES = {
    "even_d3_f32_bench": (EVEN, 3, torch.float32, "bench", 0.05**2, False),
    "even_d3_f32_uniform": (EVEN, 3, torch.float32, "uniform", 0.05**2, False),
    "uneven_d2_f32_uniform": (UNEVEN, 2, torch.float32, "uniform", 0.03**2, False),
    "uneven_d3_bf16_bench": (UNEVEN, 3, torch.bfloat16, "bench", 0.05**2, False),
    "even_d2_bf16_uniform": (EVEN, 2, torch.bfloat16, "uniform", 0.03**2, False),
    "uneven_d3_f32_bench_pot": (UNEVEN, 3, torch.float32, "bench", 0.05**2, True),
}


def _input(name):
    """x (1, n, D), y (1, m, D) in the cloud dtype, logw (1, m), pot (1, m) or None on the device, and the dual vector h (m,) the
    kernels form, float32 on the host"""
    (n, m), D, dtype, law, eps, half = CASES[name]
    g = torch.Generator().manual_seed(sum(name.encode()))
    x = torch.rand(1, n, D, generator=g).to(dtype)
    y = torch.rand(1, m, D, generator=g).to(dtype)
    logw = torch.full((1, m), -math.log(m))
    noise = 0.01 * torch.randn(1, m, generator=g) / 0.05**2 if law == "bench" else torch.zeros(1, m)
    if half:      # the noise travels in the potential: h = logw + pot / eps, one fused multiply-add in float32
        pot = (noise * eps).float()
        scale = float(np.float32(1.0) / np.float32(eps))
        h = (pot.double() * scale + logw.double()).float()
    else:
        pot, h = None, logw + noise
        logw = h
    dev = lambda t: None if t is None else t.to(DEV).contiguous()      # noqa: E731
    return dev(x), dev(y), dev(logw), dev(pot), h[0].numpy(), eps


@pytest.mark.parametrize("name", list(CASES))
def test_thresholds_match_the_model(name):
    x, y, logw, pot, h, eps = _input(name)
    rec = ps.inspect(x, y, logw, eps, pot)
    n, m = x.shape[1], y.shape[1]
    assert np.array_equal(np.sort(rec["perm_x"]), np.arange(n)) and np.array_equal(np.sort(rec["perm_y"]), np.arange(m))
    xs, ys, hs = x[0].float().cpu().numpy()[rec["perm_x"]], y[0].float().cpu().numpy()[rec["perm_y"]], h[rec["perm_y"]]
    got = []
    keep, mlb, t1, L = pm.plan_mass(xs, ys, hs, eps, slb_out=got)
    C, nT = keep.shape
    assert np.allclose(rec["mlb"], mlb, rtol=1e-12, atol=1e-9)
    q_dev = np.round((rec["t1"] - (rec["mlb"] - L)) / pm.BUCKET_NATS).astype(int)
    q_mod = np.round((t1 - (mlb - L)) / pm.BUCKET_NATS).astype(int)
    off1 = int((q_dev != q_mod).sum())
    print(f"{name}: t1 of {off1} of {C} slabs off the model's bucket; first level keeps {keep.mean():.4f} of the blocks, Slb - Mlb mean "
          f"{(got[0] - mlb).mean():.3f} nats")
    assert np.abs(q_dev - q_mod).max() <= 1 and off1 <= C // 100
    same = q_dev == q_mod
    assert np.allclose(rec["t1"][same], t1[same], rtol=1e-12, atol=1e-9)
    assert 0.05 < keep.mean() < 0.9                                   # the input prunes, and keeps something
    assert (got[0] - mlb).mean() > 0.5                                # and the sum reference is at work
    assert np.array_equal((rec["home"] >= 0)[same], ~keep[same].all(1))
    runs = pm.runs_per_slab(keep)
    for c in np.flatnonzero(same)[:: max(1, C // 150)]:
        want = pm.closed_gaps(keep[c]) if runs[c] > pm.RUNS else keep[c]
        assert np.array_equal(ps.covered(rec, c, nT), want), c
    # second level: 100 slabs, on the device's intervals
    has = np.flatnonzero((rec["home"] >= 0) & same)
    slabs = has[:: max(1, len(has) // 100)]
    iv = {c: [(int(a), int(b)) for a, b in rec["intervals"][c] if b > a] for c in slabs}
    _, _, l2 = pm.level2_mass(xs, ys, hs, eps, keep, L, slabs, intervals=iv)
    dev, want, gain = [], [], []
    for c in slabs:
        assert l2[c]["home"] == rec["home"][c], c
        k = len(l2[c]["t2"])
        want.append(pm.t2_as_stored(l2[c]["t2"]))
        dev.append(rec["t2"][c * 8:c * 8 + k])
        gain.append(l2[c]["ls"] - l2[c]["ms"])
    dev, want, gain = np.concatenate(dev), np.concatenate(want).astype(np.float32), np.concatenate(gain)
    fin = np.isfinite(want)
    assert fin.mean() > 0.5 and np.array_equal(np.isinf(dev), np.isinf(want))
    d = np.abs(dev[fin].astype(np.float64) - want[fin].astype(np.float64))
    off2 = int((d > 0).sum())
    print(f"{name}: t2 of {off2} of {int(fin.sum())} tiles off the model's value (largest distance {d.max() / (pm.BUCKET_NATS * pm.LOG2E):.3f} "
          f"buckets); ls - ms mean {gain.mean():.3f} nats")
    assert d.max() <= pm.BUCKET_NATS * pm.LOG2E + 4 * np.spacing(np.abs(want[fin]).max()) and off2 <= int(fin.sum()) // 100
    assert gain.mean() > 0.5


def _float64_rows(x, y, h, eps, rows):
    """-eps log sum_j exp(h_j - |x_i - y_j|^2 / (2 eps)) for the given rows, float64 on the device"""
    xr, yy, hh = x[0, rows].double(), y[0].double(), h[0].double()
    out = []
    for r0 in range(0, xr.shape[0], 512):
        d2 = ((xr[r0:r0 + 512, None, :] - yy[None]) ** 2).sum(-1)
        out.append(-eps * torch.logsumexp(hh[None] - d2 / (2 * float(np.float32(eps))), 1))
    return torch.cat(out)


@LAYOUTS
@pytest.mark.parametrize("name", ["even_d3_f32_bench", "uneven_d2_f32_uniform", "uneven_d3_bf16_bench"])
def test_values_against_dense_and_float64(name, flags):
    x, y, h, _, _, eps = _input(name)
    diam2 = ps.diam2(x, y)
    pruned = ps.fwd(x, y, h, eps, flags)
    ps.close(pruned, ps.fwd(x, y, h, eps, flags | NO_SORT), diam2, "dense")
    rows = torch.arange(0, x.shape[1], max(1, x.shape[1] // 2048), device=DEV)[:2048]
    ps.close(pruned[0, rows], _float64_rows(x, y, h, eps, rows).float(), diam2, "float64")


@LAYOUTS
@pytest.mark.parametrize("special", ["nan_coordinate", "inf_dual_group", "all_minus_inf"])
def test_special_values_as_the_dense_launch(special, flags):
    x, y, h, _, _, eps = _input("even_d3_f32_bench")
    x, h = x.clone(), h.clone()
    if special == "nan_coordinate":      # one row: its slab keeps everything, its own value is NaN
        x[0, 12345, 1] = float("nan")
    elif special == "inf_dual_group":    # 32 columns: every row's sum is +inf
        h[0, 70000:70032] = float("inf")
    else:
        h[:] = float("-inf")
    pruned, dense = ps.fwd(x, y, h, eps, flags), ps.fwd(x, y, h, eps, flags | NO_SORT)
    assert bool((~torch.isfinite(dense)).any())                       # the input does what it is meant to
    ps.close(pruned, dense, ps.diam2(x, y), "dense")
