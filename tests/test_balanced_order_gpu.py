"""The balanced cells of the sorted p = 2 call on the device (csrc/glhip_autosort.h: balanced cells; balance_kernel in
csrc/glhip_compact_sort.hip; the rules: csrc/glhip_balance.h).

After the radix sort, every whole aligned block of 1024 positions of both sorted clouds is split by median cuts along the longest axis
into cells of exactly 512, 256, 128, 64 and 32 points.  The order shows through glhip_prune_inspect (perm_x, perm_y): it must be a
permutation, the same on every call, with the split property at all five levels of every whole block, the axis recomputed from the
points; and it must buy what it is for: the device's intervals cover at most 0.9 of the blocks the CPU model keeps on the path order
of the same input.  The pruning is exact for any order, so launches are held to prune_support.close against the
same call under GLHIP_FLAG_NO_SORT, on inputs that put NaN, infinities and runs of identical points inside whole blocks.
"""

import math

import numpy as np
import pytest
import torch

from geomloss_amd import hip

import prune_support as ps
from prune_support import pm

pytestmark = pytest.mark.gpu

DEV, NO_SORT, LAYOUTS = ps.DEV, ps.NO_SORT, ps.LAYOUTS
BLOCK, LEAF = 1024, 32
EPS = 0.05**2
ORDER = ("perm_x", "perm_y", "intervals")      # the records these tests read


def _check_order(z, perm):
    """perm is a permutation; in every whole block of 1024 the split property holds at all five levels, along the axis the rule picks
    from the segment's own points (keys compared with <=: a bf16 cloud has many ties), and every segment of 64 — the last ones sorted
    — ascends along its axis"""
    n = z.shape[0]
    assert np.array_equal(np.sort(perm), np.arange(n))
    nb = n // BLOCK
    pts = z[perm[:nb * BLOCK]]
    seg = BLOCK
    while seg >= 2 * LEAF:
        p = pts.reshape(-1, seg, z.shape[1])
        axis = pm.balance_axes(p)
        key = pm.order_key(np.take_along_axis(p, axis[:, None, None], 2)[:, :, 0])
        bad = np.flatnonzero(key[:, :seg // 2].max(1) > key[:, seg // 2:].min(1))
        assert bad.size == 0, (seg, bad[:5])
        if seg == 2 * LEAF:
            assert (np.diff(key.astype(np.int64), axis=1) >= 0).all()
        seg //= 2


@pytest.mark.parametrize("n,m,D,dtype", [(320000, 320000, 3, torch.float32), (320000, 320000, 3, torch.bfloat16), (317000, 320037, 2, torch.float32),
                                         (330001, 310000, 1, torch.float32)], ids=["d3", "d3-bf16", "d2-uneven", "d1"])
def test_order_is_balanced_and_repeatable(n, m, D, dtype):
    x, y, h = ps.law(n, m, 40 + D, D=D, dtype=dtype)
    a = ps.inspect(x, y, h, EPS, records=ORDER)
    b = ps.inspect(x, y, h, EPS, records=ORDER)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    _check_order(x[0].float().cpu().numpy(), a["perm_x"])
    _check_order(y[0].float().cpu().numpy(), a["perm_y"])


def test_order_is_in_effect_on_the_mass_law():
    """the law of tests/test_prune_mass_gpu.py (seed 21): the blocks the device's intervals cover against the first-level fraction of
    the model on the path order of the same input (modelled: 0.3183 against 0.3802)"""
    n = 320000
    x, y, h = ps.law(n, n, 21)
    xn, yn, hn = x[0].cpu().numpy(), y[0].cpu().numpy(), h[0].cpu().numpy()
    px, py = pm.compact_order2(xn, 256, 2), pm.compact_order2(yn, 256, 2)
    path = float(pm.plan_mass(xn[px], yn[py], hn[py], EPS)[0].mean())
    rec = ps.inspect(x, y, h, EPS, records=ORDER)
    iv = rec["intervals"].astype(np.int64)
    length = np.maximum(iv[:, :, 1] - iv[:, :, 0], 0)
    covered = float(((length + pm.BLOCK - 1) // pm.BLOCK).sum()) / (iv.shape[0] * ((n + pm.BLOCK - 1) // pm.BLOCK))
    print(f"blocks covered by the device's intervals {covered:.4f}; the model's first level on the path order {path:.4f}")
    assert covered <= 0.9 * path


def _middle(z):
    """caller indices of points in the middle of the sorted order: the first coordinate leads the voxel path"""
    return torch.nonzero((z[0, :, 0] > 0.3) & (z[0, :, 0] < 0.7))[:, 0]


def _positions(perm, idx):
    pos = np.empty(perm.shape[0], np.int64)
    pos[perm] = np.arange(perm.shape[0])
    return pos[idx.cpu().numpy()]


@LAYOUTS
def test_nan_and_infinities_inside_whole_blocks(flags):
    """3000 NaN coordinates in the last axis of points from the middle of the path (the path keeps them between their neighbours of the
    first two axes), first in the rows alone — every other row keeps a finite value to compare — then in the columns too (a NaN column
    makes every row NaN: the pattern is compared); then 50 infinite coordinates on top: an infinite bounding box leaves the path order
    the caller's order, and the marked points sit in the middle of it."""
    n = 320000
    x, y, h = ps.law(n, n, 51)
    g = torch.Generator().manual_seed(52)
    ix, iy = _middle(x), _middle(y)
    ix = ix[torch.randperm(ix.numel(), generator=g)[:3000].to(DEV)]
    iy = iy[torch.randperm(iy.numel(), generator=g)[:3000].to(DEV)]
    whole = (n // BLOCK) * BLOCK

    def check(marked_x, marked_y):
        rec = ps.inspect(x, y, h, EPS, records=ORDER)
        for perm, idx in ((rec["perm_x"], marked_x), (rec["perm_y"], marked_y)):
            if idx is not None:
                pos = _positions(perm, idx)
                assert pos.min() >= BLOCK and pos.max() < whole      # inside whole blocks, away from the ends
        _check_order(x[0].cpu().numpy(), rec["perm_x"])
        _check_order(y[0].cpu().numpy(), rec["perm_y"])
        a, b = ps.fwd(x, y, h, EPS, flags), ps.fwd(x, y, h, EPS, flags | NO_SORT)
        ps.close(a, b, ps.diam2(x, y))
        return a

    x, y = x.clone(), y.clone()
    x[0, ix, 2] = math.nan
    out = check(ix, None)
    assert int(out.isnan().sum()) == 3000 and bool(torch.isfinite(out[~out.isnan()]).all())
    y[0, iy, 2] = math.nan
    check(ix, iy)
    jx = torch.arange(100000, 100050, device=DEV)
    x[0, jx[:25], 0] = math.inf
    x[0, jx[25:], 1] = -math.inf
    y[0, jx[:25] + 7, 1] = math.inf
    y[0, jx[25:] + 7, 2] = -math.inf
    check(jx, jx + 7)


@LAYOUTS
def test_identical_points(flags):
    """5000 identical points in each cloud: they share a voxel, so whole blocks of the path order hold nothing else"""
    n = 320000
    x, y, h = ps.law(n, n, 53)
    x, y = x.clone(), y.clone()
    x[0, 150000:155000] = torch.tensor([0.5, 0.5, 0.5], device=DEV)
    y[0, 70000:75000] = torch.tensor([0.5, 0.25, 0.75], device=DEV)
    rec = ps.inspect(x, y, h, EPS, records=ORDER)
    for perm, lo in ((rec["perm_x"], 150000), (rec["perm_y"], 70000)):
        pos = _positions(perm, torch.arange(lo, lo + 5000))
        full = np.flatnonzero(np.bincount(pos // BLOCK, minlength=n // BLOCK + 1) == BLOCK)
        assert full.size >= 3 and full.max() < n // BLOCK      # one run of the path: at least 3 whole blocks hold nothing else
        for b in full:      # ... and come out in their incoming order: equal path keys, so ascending caller indices
            assert (np.diff(perm[b * BLOCK:(b + 1) * BLOCK]) > 0).all(), b
    _check_order(x[0].cpu().numpy(), rec["perm_x"])
    _check_order(y[0].cpu().numpy(), rec["perm_y"])
    ps.close(ps.fwd(x, y, h, EPS, flags), ps.fwd(x, y, h, EPS, flags | NO_SORT), ps.diam2(x, y))


@LAYOUTS
def test_half_step_at_the_uneven_d2_shape(flags):
    n, m = 317000, 320037
    x, y, h = ps.law(n, m, 54, D=2)
    g = torch.Generator().manual_seed(55)
    logw = torch.full((1, m), -math.log(m)).to(DEV)
    pot = (h - logw) * EPS      # logw + pot / eps = h
    prev = (0.01 * torch.randn(1, n, generator=g)).to(DEV)
    a = hip.sinkhorn_step_raw(x, y, logw, pot, prev, EPS, 0.9, 2, None, flags)
    b = hip.sinkhorn_step_raw(x, y, logw, pot, prev, EPS, 0.9, 2, None, flags | NO_SORT)
    ps.close(a, b, ps.diam2(x, y))
