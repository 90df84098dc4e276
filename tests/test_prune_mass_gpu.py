"""The mass rule of the exact pruning of big dense p = 2 soft-min launches (csrc/glhip_autosort.h; prune_slabs_kernel and
prune_tiles_kernel in csrc/glhip_prune.hip): both levels drop by the SUM of what they drop, bounded from the block / group records.

What is dropped stays below one ulp of the output by design, so the outputs cannot tell a correct budget from a generous one.  These
tests read the thresholds themselves through glhip_prune_inspect: against the NumPy model (tools/prune_model.py) fed with the device's
own permutations; on an input built against a mass rule (many equal small terms), where the float64 sum of everything the device may
drop is held to 2^-26 of each row's true sum; through the half-step; and on slabs without a second level.  Launches are held to
prune_support.close against the same call under GLHIP_FLAG_NO_SORT.

A tile with a home block but no finite seed cannot be built from outside: a home block attains a finite Mlb, so it holds a finite dual
value and finite points, and a slab with a non-finite row has no home block; the kernel's guard for it (t2 = -inf) is not reachable
here.  Model against itself on the first test's input with every group's lse moved by one float32 ulp (host run, 1250 slabs / 10000
tiles): see test_thresholds_match_the_model's docstring.
"""

import ctypes
import math

import numpy as np
import pytest
import torch

from geomloss_amd import hip

import prune_support as ps
from prune_support import pm

pytestmark = pytest.mark.gpu

DEV, F16X2, NO_SORT, LAYOUTS = ps.DEV, ps.F16X2, ps.NO_SORT, ps.LAYOUTS
N = 320000          # the smallest square shape the p = 2 call prunes (N M >= 1e11)
BUDGET = 2.0**-26


def _device_intervals(rec, c):
    return [(int(a), int(b)) for a, b in rec["intervals"][c] if b > a]


def test_thresholds_match_the_model():
    """Headline law, eps = 0.05^2: t1 of every slab and t2 of every tile against the model on the device's own order.  A threshold
    matches exactly, or lies one bucket away where a key or a running sum sits within float rounding of an edge; those cases are counted
    and capped at 1 % of the slabs / tiles.  (The model against itself with every group's lse moved up by one float32 ulp, this input,
    on the host and in the model's own order: 0 of 1250 slabs and 0 of 10000 tiles move.)"""
    eps = 0.05**2
    x, y, h = ps.law(N, N, 21)
    rec = ps.inspect(x, y, h, eps)
    assert np.array_equal(np.sort(rec["perm_x"]), np.arange(N)) and np.array_equal(np.sort(rec["perm_y"]), np.arange(N))
    xs, ys, hs = x[0].cpu().numpy()[rec["perm_x"]], y[0].cpu().numpy()[rec["perm_y"]], h[0].cpu().numpy()[rec["perm_y"]]
    keep, mlb, t1, L = pm.plan_mass(xs, ys, hs, eps)
    C, nT = keep.shape
    assert np.allclose(rec["mlb"], mlb, rtol=1e-12, atol=1e-9)
    # first level: bucket indices of the thresholds
    q_dev = np.round((rec["t1"] - (rec["mlb"] - L)) / pm.BUCKET_NATS).astype(int)
    q_mod = np.round((t1 - (mlb - L)) / pm.BUCKET_NATS).astype(int)
    off1 = int((q_dev != q_mod).sum())
    print(f"t1: {off1} of {C} slabs off the model's bucket (largest distance {np.abs(q_dev - q_mod).max()} buckets); "
          f"first level keeps {keep.mean():.4f} of the blocks")
    assert np.abs(q_dev - q_mod).max() <= 1 and off1 <= C // 100
    assert keep.mean() < 0.9                                         # the law prunes at this size
    iv = {c: _device_intervals(rec, c) for c in range(C)}
    same = np.flatnonzero(q_dev == q_mod)
    assert (pm.runs_per_slab(keep) <= pm.RUNS).all()                 # no gap closing on this input: intervals = kept blocks
    for c in same[:: max(1, len(same) // 200)]:
        assert np.array_equal(ps.covered(rec, c, nT), keep[c]), c
    # second level: every tile of every slab, on the device's intervals
    has = rec["home"] >= 0
    assert np.array_equal(has[same], ~keep[same].all(1))             # a slab whose blocks all pass has no home block
    _, _, l2 = pm.level2_mass(xs, ys, hs, eps, keep, L, np.flatnonzero(has), intervals=iv)
    want = np.full((N + 31) // 32, -np.inf, np.float32)
    for c in np.flatnonzero(has):
        assert l2[c]["home"] == rec["home"][c], c
        want[c * 8:c * 8 + len(l2[c]["t2"])] = pm.t2_as_stored(l2[c]["t2"])
    got = rec["t2"]
    assert np.array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    d = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64))
    off2 = int((d > 0).sum())
    print(f"t2: {off2} of {int(fin.sum())} tiles off the model's value (largest distance {d.max() / (pm.BUCKET_NATS * pm.LOG2E):.3f} buckets)")
    assert d.max() <= pm.BUCKET_NATS * pm.LOG2E + 4 * np.spacing(np.abs(want[fin]).max()) and off2 <= int(fin.sum()) // 100


def _shells(seed):
    """Rows in a tight cluster; 512 columns inside it set every row's maximum; the other columns, with equal dual values, lie on 16
    thin shells whose terms run from 3 nats below the term rule's threshold (row maximum - L) to ln M nats above it: the band where
    a rule by single terms and a rule by mass differ.  768 columns in a far clump (200 nats down) give every slab a block that any
    rule drops, so that every slab has a home block and a second level.  The cluster and the clump each sit inside one voxel of the
    column sort (edge ~0.09), so each holds whole blocks of 256 sorted columns."""
    eps = 0.05**2
    g = torch.Generator().manual_seed(seed)
    L = math.log(N) + 26 * math.log(2) + 1.0
    x = 0.5 + 0.02 * (torch.rand(N, 3, generator=g) - 0.5)
    inside = 0.5 + 0.02 * (torch.rand(512, 3, generator=g) - 0.5)
    far = torch.tensor([1.5, 0.5, 0.5]) + 0.005 * (torch.rand(768, 3, generator=g) - 0.5)
    per = (N - 512 - 768) // 16
    assert 16 * per == N - 512 - 768
    depth = torch.linspace(L - math.log(N), L + 3.0, 16)             # nats below the maximum
    radius = torch.sqrt(2 * eps * depth).repeat_interleave(per)
    u = torch.randn(16 * per, 3, generator=g)
    shell = 0.5 + radius[:, None] * u / u.norm(dim=1, keepdim=True)
    y = torch.cat([inside, far, shell])[torch.randperm(N, generator=g)]
    h = torch.zeros(N)
    return x[None].to(DEV).contiguous(), y[None].to(DEV).contiguous(), h[None].to(DEV).contiguous(), eps, L


def test_dropped_mass_on_many_equal_small_terms():
    """For a sample of tiles: everything the device may drop — the columns outside the slab's intervals and, inside them, every group
    whose key lse(G) - pen(W, G) (float64, lse not rounded up: a superset of what the kernel's float32 test skips) lies below the
    tile's threshold max(t2, smallest true row maximum - L) — sums in float64 to less than 2^-26 of each row's true sum, while the band
    as a whole holds more than that."""
    x, y, h, eps, L = _shells(31)
    rec = ps.inspect(x, y, h, eps)
    ys = y[0][torch.from_numpy(rec["perm_y"]).to(DEV).long()].double()
    xs = x[0][torch.from_numpy(rec["perm_x"]).to(DEV).long()].double()
    hs = h[0][torch.from_numpy(rec["perm_y"]).to(DEV).long()].double()
    i2e = pm.inv2eps_of(eps)
    nG = (N + 31) // 32
    pad = nG * 32 - N
    yg = torch.cat([ys, ys[-1:].expand(pad, 3)]).view(nG, 32, 3)
    glo, ghi = yg.min(1).values, yg.max(1).values
    glse = torch.logsumexp(torch.cat([hs, hs.new_full((pad,), -math.inf)]).view(nG, 32), 1)
    assert (rec["home"] >= 0).all()
    worst = band_least = None
    dropped_cols = tiles = 0
    for w in range(0, N // 32, N // 32 // 12):
        tiles += 1
        c = w // 8
        xr = xs[w * 32:(w + 1) * 32]
        terms = hs[None] - ((xr[:, None, :] - ys[None]) ** 2).sum(-1) * i2e
        tmax = terms.max(1).values
        total = torch.exp(terms - tmax[:, None]).sum(1)
        inside = torch.zeros(nG, dtype=torch.bool, device=DEV)
        for a, b in _device_intervals(rec, c):
            inside[a // 32:(b + 31) // 32] = True
        gap = torch.clamp(torch.maximum(glo - xr.max(0).values, xr.min(0).values - ghi), min=0.0)
        key = glse - (gap**2).sum(1) * i2e
        t2 = float(rec["t2"][w]) / pm.LOG2E
        assert math.isfinite(t2)
        thr = max(t2 + 1e-9 * abs(t2), float(tmax.min()) - L)
        gone = (~inside | (key < thr)).repeat_interleave(32)[:N]
        share = (torch.exp(terms - tmax[:, None]) * gone[None]).sum(1) / total
        rel = terms - tmax[:, None]
        band = ((rel >= -(L + 3.0)) & (rel <= -L + math.log(N))).double()
        band_share = (torch.exp(rel) * band).sum(1) / total
        worst = max(worst or 0.0, float(share.max()))
        band_least = min(band_least if band_least is not None else math.inf, float(band_share.min()))
        dropped_cols += int(gone.sum())
    print(f"largest share a row may lose {worst:.3e}, smallest share of the band {band_least:.3e}, budget 2^-26 = {BUDGET:.3e}; "
          f"{dropped_cols / tiles / N:.3f} of the columns dropped per sampled tile")
    assert band_least > BUDGET          # dropping the whole band would break the guarantee
    assert worst < BUDGET
    assert dropped_cols > 0             # and the rule does drop something here


@LAYOUTS
def test_many_equal_small_terms_launch(flags):
    x, y, h, eps, _ = _shells(31)
    ps.close(ps.fwd(x, y, h, eps, flags), ps.fwd(x, y, h, eps, flags | NO_SORT), ps.diam2(x, y))


def test_half_step_thresholds_equal_the_forward_call_on_the_formed_duals():
    eps = 0.03**2
    x, y, logw = ps.law(N, N, 22, noise=0.001)
    g = torch.Generator().manual_seed(5)
    pot = (0.002 * torch.randn(1, N, generator=g)).to(DEV)
    scale = np.float32(1.0) / np.float32(eps)
    hcol = (pot.double() * float(scale) + logw.double()).float()      # fma(pot, 1 / eps, logw): one rounding
    a = ps.inspect(x, y, logw, eps, pot)
    b = ps.inspect(x, y, hcol, eps)
    assert (a["home"] >= 0).any() and np.isfinite(a["t2"]).any()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    lib = hip.load_library()
    ws, nbytes = ps.workspace(lib, N, N, 3)
    outs = []
    for fl in (F16X2, F16X2 | NO_SORT):
        out = torch.empty((1, N), dtype=torch.float32, device=DEV)
        rc = lib.glhip_sinkhorn_step(x.data_ptr(), y.data_ptr(), logw.data_ptr(), pot.data_ptr(), None, out.data_ptr(), 1, N, N, 3, float(eps),
                                     1.0, 2, hip._dtype_code(x), None, None, None, 0, ctypes.c_void_p(ws.data_ptr()), nbytes, fl, hip._stream(x))
        assert rc == 0, lib.glhip_last_error()
        outs.append(out)
    ps.close(outs[0], outs[1], ps.diam2(x, y))


@LAYOUTS
def test_slabs_without_a_second_level(flags):
    """home = -1 — a slab with a NaN row; every slab of a cloud with an infinite row (its bounding box, and with it the voxel sort, is
    degenerate: no slab is compact, every block passes); a law whose first level keeps every block — leaves the tile thresholds
    untouched (the inspect entry presets them to -inf), and the launch gives the dense launch's pattern."""
    eps = 0.05**2
    x, y, h = ps.law(N, N, 23)
    x = x.clone()
    x[0, 1000, 1] = math.nan
    x[0, 200000, 0] = math.nan
    rec = ps.inspect(x, y, h, eps)
    pos = np.empty(N, np.int64)
    pos[rec["perm_x"]] = np.arange(N)
    bad = np.unique(pos[[1000, 200000]] // 256)
    assert (rec["home"][bad] == -1).all() and np.isinf(rec["t1"][bad]).all() and (rec["home"] >= 0).sum() > 1000
    t2 = rec["t2"].reshape(-1, 8)
    assert np.array_equal(np.isneginf(t2).all(1), rec["home"] < 0) and np.isfinite(t2[rec["home"] >= 0]).all()
    ps.close(ps.fwd(x, y, h, eps, flags), ps.fwd(x, y, h, eps, flags | NO_SORT), ps.diam2(x, y))
    # an infinite row: no slab has a home block, the slab that holds it has no bound at all
    x[0, 1000, 1] = math.inf
    rec = ps.inspect(x, y, h, eps)
    pos[rec["perm_x"]] = np.arange(N)
    assert (rec["home"] == -1).all() and np.isneginf(rec["t2"]).all() and np.isneginf(rec["t1"][pos[1000] // 256])
    ps.close(ps.fwd(x, y, h, eps, flags), ps.fwd(x, y, h, eps, flags | NO_SORT), ps.diam2(x, y))
    # eps = 1: every block passes, no slab has a home block
    x, y, h = ps.law(N, N, 24)
    rec = ps.inspect(x, y, h, 1.0)
    assert (rec["home"] == -1).all() and np.isneginf(rec["t2"]).all()
    ps.close(ps.fwd(x, y, h, 1.0, flags), ps.fwd(x, y, h, 1.0, flags | NO_SORT), ps.diam2(x, y))


def test_inspect_rejects_shapes_that_are_not_pruned():
    x, y, h = ps.law(70000, 70000, 25)
    rc, _ = ps.inspect_call(x, y, h, 0.0025, records=())
    assert rc == -2
