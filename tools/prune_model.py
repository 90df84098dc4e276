#!/usr/bin/env python
"""CPU model of the exact block pruning of big dense p = 2 soft-min launches (csrc/glhip_autosort.h, glhip_compact_sort.hip, glhip_prune.hip).

Restates in NumPy what the library does on the device: both clouds voxel-sorted along a boustrophedon path (compact_sort), rows cut
into slabs of 256, columns into blocks of 256, the float64 bound

    Mlb(R) = max_T [hmax(T) - dmax(R,T)^2 / (2 eps)],   keep T iff hmax(T) - dmin(R,T)^2 / (2 eps) >= Mlb(R) - (ln M + 26 ln 2 + 1),

and counts the kept pairs and the runs of kept blocks per slab.  ``check_dropped`` verifies on the points themselves that no dropped
block holds a term above Mlb(R) - L for any row of the slab (tests/test_prune_model.py).

The second level (csrc/glhip_softmin_x32.h, P2) is modelled by ``level2``: inside the kept blocks, every 32-row wavefront tile tests
every group of 32 columns against its rows' exact maxima over the slab's home block (the block that attains Mlb) and evaluates only
the groups that pass; ``compact_order2`` is the order of the sorted p = 2 call (voxels of 256 points for both clouds, a minor key of
sub-voxels inside).  ``level2`` also verifies on the points themselves that no skipped pair holds a term above its row's true
maximum - L.  The model's test is exact arithmetic; the kernel's float32 test keeps a little more (its slack is on the keep side).

The mass rule (``plan_mass`` / ``level2_mass``) takes its two budgets relative to a lower bound of the row SUM (glhip_autosort.h, "Sum
reference": Slb per slab from the block records, ls per tile from the group records of the slab's reference blocks);
``reference="term"`` is the rule before library 136, relative to one term of the sum, and ``reference_lines`` prints one beside the other.

    python tools/prune_model.py [--n 1000000] [--eps 0.0025] [--slabs 40]     (the bench problem: bench.make_problem(n, seed=1000))
"""

import argparse
import math

import numpy as np

SLAB, BLOCK, RUNS, MARGIN = 256, 256, 160, 1.0


def compact_order(z, rows_per_voxel):
    """glhip_compact_sort.hip: voxel_kernel + path_keys_kernel + a stable radix sort of the keys"""
    z = np.asarray(z, np.float32)
    n, D = z.shape
    lo, hi = z.min(0), z.max(0)
    ext = (hi - lo).astype(np.float32)
    emax = float(ext.max())
    live = ext > np.float32(1e-6) * np.float32(max(emax, 1e-30))
    vol = np.float32(np.prod(ext[live])) if live.any() else np.float32(1.0)
    voxel = np.float32(np.power(np.float32(vol * np.float32(rows_per_voxel) / np.float32(n)), np.float32(1.0 / max(int(live.sum()), 1))))
    voxel = np.float32(max(voxel, np.float32(emax / 2**20), np.float32(1e-30)))
    qmin = np.floor(lo / voxel).astype(np.int64)
    e = np.floor((lo + ext) / voxel).astype(np.int64) - qmin + 1
    path = np.zeros(n, np.uint64)
    for d in range(D):
        q = np.clip(np.floor(z[:, d] / voxel).astype(np.int64) - qmin[d], 0, e[d] - 1)
        c = np.where(path & np.uint64(1), e[d] - 1 - q, q).astype(np.uint64)
        path = path * np.uint64(e[d]) + c
    return np.argsort(path, kind="stable")


def compact_order2(z, rows_per_voxel, sub):
    """compact_order with the minor key of path_keys_kernel (sub > 1): inside a voxel, sub-voxels of edge voxel / sub along a
    boustrophedon path of their own"""
    z = np.asarray(z, np.float32)
    n, D = z.shape
    lo, hi = z.min(0), z.max(0)
    ext = (hi - lo).astype(np.float32)
    emax = float(ext.max())
    live = ext > np.float32(1e-6) * np.float32(max(emax, 1e-30))
    vol = np.float32(np.prod(ext[live])) if live.any() else np.float32(1.0)
    voxel = np.float32(np.power(np.float32(vol * np.float32(rows_per_voxel) / np.float32(n)), np.float32(1.0 / max(int(live.sum()), 1))))
    voxel = np.float32(max(voxel, np.float32(emax / 2**20), np.float32(1e-30)))
    qmin = np.floor(lo / voxel).astype(np.int64)
    e = np.floor((lo + ext) / voxel).astype(np.int64) - qmin + 1
    path = np.zeros(n, np.uint64)
    minor = np.zeros(n, np.uint64)
    for d in range(D):
        f = (z[:, d] / voxel).astype(np.float32)
        fl = np.floor(f)
        q = np.clip(fl.astype(np.int64) - qmin[d], 0, e[d] - 1)
        c = np.where(path & np.uint64(1), e[d] - 1 - q, q).astype(np.uint64)
        path = path * np.uint64(e[d]) + c
        r = np.clip(((f - fl) * np.float32(sub)).astype(np.int64), 0, sub - 1)
        minor = minor * np.uint64(sub) + np.where(minor & np.uint64(1), sub - 1 - r, r).astype(np.uint64)
    return np.argsort(path * np.uint64(sub**D) + minor, kind="stable")


def sort_sub(D):
    """glhip_autosort.h: prune_sort_sub"""
    return 2 if D >= 3 else (3 if D == 2 else 8)


def order_key(v):
    """glhip_balance.h: balance_key — the order-preserving image of float32 values as uint32: -inf < ... < -0 < +0 < ... < +inf < NaN
    (every NaN, either sign, is one value)"""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32)
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))
    return np.where((b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint32(0xFFFFFFFF), k).astype(np.uint32)


def balance_axes(p):
    """glhip_balance.h: balance_axis for segments p (segments, points, D): the axis of the largest extent over the finite values
    (float32; ties: the lowest axis; an axis without a finite value loses to every other; none at all: axis 0)"""
    fin = np.isfinite(p)
    lo = np.where(fin, p, np.float32(np.inf)).min(1)
    hi = np.where(fin, p, np.float32(-np.inf)).max(1)
    with np.errstate(over="ignore", invalid="ignore"):
        ext = np.where(lo <= hi, (hi - lo).astype(np.float32), np.float32(-1.0))
    return ext.argmax(1)      # (the first of equal maxima)


def balanced_order(z, perm, block=1024, leaf=32):
    """glhip_compact_sort.hip: balance_kernel, on the order `perm` of the cloud z (float32 values; a bf16 cloud: its values as float32).
    Every whole aligned block of `block` positions is split like a k-d tree: levels with segments of block, block / 2, ..., 2 leaf
    points, each segment sorted by (order_key of the coordinate on the segment's own axis, position the point had in the block).
    The last n mod block positions are left as they are.  Returns the new order."""
    z = np.asarray(z, np.float32)
    perm = np.asarray(perm)
    nb = perm.shape[0] // block
    out = perm.copy()
    if nb == 0:
        return out
    head = perm[:nb * block].reshape(nb, block)
    pos = np.broadcast_to(np.arange(block, dtype=np.uint64), (nb, block)).copy()      # incoming position of the point at each place
    seg = block
    while seg >= 2 * leaf:
        ps = pos.reshape(-1, seg)
        first = (np.arange(ps.shape[0]) * seg // block)[:, None]                      # the segment's block
        pts = z[head[first, ps.astype(np.int64)]]                                     # (segments, seg, D)
        axis = balance_axes(pts)
        key = order_key(np.take_along_axis(pts, axis[:, None, None], 2)[:, :, 0])
        word = (key.astype(np.uint64) << np.uint64(32)) | ps
        pos = np.take_along_axis(ps, np.argsort(word, 1), 1).reshape(nb, block)       # (no two words of a segment are equal)
        seg //= 2
    out[:nb * block] = np.take_along_axis(head, pos.astype(np.int64), 1).ravel()
    return out


def closed_gaps(keep_row, runs=None):
    """prune_slabs_kernel's gap closing on the kept blocks of one slab: with more than `runs` runs, the gaps shorter than g — the
    smallest g that leaves at most `runs` runs — are closed.  Returns the row with the closed gaps kept."""
    runs = RUNS if runs is None else runs
    t = np.flatnonzero(keep_row)
    if t.size == 0:
        return keep_row.copy()
    gaps = np.diff(t) - 1
    real = np.sort(gaps[gaps > 0])[::-1]
    if real.size + 1 <= runs:
        return keep_row.copy()
    g = int(real[runs - 1]) + 1       # at most runs - 1 gaps of at least g blocks stay open
    out = keep_row.copy()
    for a, n in zip(t[:-1], gaps):
        if 0 < n < g:
            out[a + 1:a + 1 + n] = True
    return out


def boxes(z, size):
    n = z.shape[0]
    k = (n + size - 1) // size
    pad = np.full((k * size - n, z.shape[1]), np.nan, z.dtype)
    zz = np.concatenate([z, pad]).reshape(k, size, -1)
    return np.nanmin(zz, 1).astype(np.float64), np.nanmax(zz, 1).astype(np.float64)


def plan(xs, ys, h, eps):
    """keep (C, nT) bool, Mlb (C,), L — for finite inputs (the special values are the device's business, tested on the GPU)"""
    M = ys.shape[0]
    rlo, rhi = boxes(xs, SLAB)
    blo, bhi = boxes(ys, BLOCK)
    nT = blo.shape[0]
    hp = np.concatenate([h.astype(np.float64), np.full(nT * BLOCK - M, -np.inf)]).reshape(nT, BLOCK)
    hmax = hp.max(1)
    L = math.log(M) + 26 * math.log(2) + MARGIN
    keep = np.zeros((rlo.shape[0], nT), bool)
    mlb = np.zeros(rlo.shape[0])
    for c0 in range(0, rlo.shape[0], 256):
        a, b = rlo[c0:c0 + 256, None], rhi[c0:c0 + 256, None]
        gap = np.maximum(np.maximum(blo[None] - b, a - bhi[None]), 0.0)
        far = np.maximum(bhi[None] - a, b - blo[None])
        dmin2, dmax2 = (gap**2).sum(-1), (far**2).sum(-1)
        m = (hmax[None] - dmax2 / (2 * eps)).max(1)
        mlb[c0:c0 + 256] = m
        keep[c0:c0 + 256] = hmax[None] - dmin2 / (2 * eps) >= (m - L)[:, None]
    return keep, mlb, L


def runs_per_slab(keep):
    k = keep.astype(np.int8)
    return (np.diff(np.concatenate([np.zeros((k.shape[0], 1), np.int8), k], 1), axis=1) == 1).sum(1)


def kept_pairs(keep, N, M):
    rows = np.full(keep.shape[0], SLAB)
    rows[-1] = N - SLAB * (keep.shape[0] - 1)
    cols = np.full(keep.shape[1], BLOCK)
    cols[-1] = M - BLOCK * (keep.shape[1] - 1)
    return float(rows @ keep.astype(np.float64) @ cols)


def check_dropped(xs, ys, h, eps, keep, mlb, L, slabs):
    """largest (term - (Mlb - L)) over the dropped blocks of the given slabs, exact float64 terms; < 0 means the bound held"""
    worst = -np.inf
    for c in slabs:
        xr = xs[c * SLAB:(c + 1) * SLAB].astype(np.float64)
        cols = np.concatenate([np.arange(t * BLOCK, min((t + 1) * BLOCK, ys.shape[0])) for t in np.flatnonzero(~keep[c])] or [np.zeros(0, int)])
        if cols.size == 0:
            continue
        d2 = ((xr[:, None, :] - ys[cols].astype(np.float64)[None]) ** 2).sum(-1)
        terms = h[cols].astype(np.float64)[None] - d2 / (2 * eps)
        worst = max(worst, float(terms.max() - (mlb[c] - L)))
    return worst


TILE, GROUP = 32, 32


def level2(xs, ys, h, eps, keep, L, slabs, check=False):
    """The second level on the given slabs.  Returns (pairs whose exponential is evaluated, pairs kept by the first level, worst), where
    worst (check=True) is the largest (term - (true row maximum - L)) over the pairs the second level skips, exact float64; < 0 means
    the bound held.  The running maximum of a row is modelled by its seed (the kernel's only rises)."""
    M, D = ys.shape
    x64, y64, h64 = xs.astype(np.float64), ys.astype(np.float64), h.astype(np.float64)
    rlo, rhi = boxes(xs, SLAB)
    blo, bhi = boxes(ys, BLOCK)
    glo, ghi = boxes(ys, GROUP)
    nT, nG = blo.shape[0], glo.shape[0]
    hmax = np.concatenate([h64, np.full(nT * BLOCK - M, -np.inf)]).reshape(nT, BLOCK).max(1)
    ghmax = np.concatenate([h64, np.full(nG * GROUP - M, -np.inf)]).reshape(nG, GROUP).max(1)
    gcols = np.minimum(GROUP, M - GROUP * np.arange(nG))
    evaluated = kept1 = 0.0
    worst = -np.inf
    for c in slabs:
        far = np.maximum(bhi - rlo[c], rhi[c] - blo)
        home = int(np.argmax(hmax - (far**2).sum(-1) / (2 * eps)))
        hc = np.arange(home * BLOCK, min(M, (home + 1) * BLOCK))
        groups = np.concatenate([np.arange(t * (BLOCK // GROUP), min(nG, (t + 1) * (BLOCK // GROUP))) for t in np.flatnonzero(keep[c])])
        r1 = min(xs.shape[0], (c + 1) * SLAB)
        for w0 in range(c * SLAB, r1, TILE):
            xr = x64[w0:min(w0 + TILE, r1)]
            seed = (h64[hc][None] - ((xr[:, None, :] - y64[hc][None]) ** 2).sum(-1) / (2 * eps)).max(1)
            thr = seed.min() - L
            wlo, whi = xr.min(0), xr.max(0)
            gap = np.maximum(np.maximum(glo[groups] - whi, wlo - ghi[groups]), 0.0)
            k2 = ghmax[groups] - (gap**2).sum(-1) / (2 * eps) >= thr
            evaluated += float(gcols[groups][k2].sum()) * xr.shape[0]
            kept1 += float(gcols[groups].sum()) * xr.shape[0]
            if check:
                true_max = np.full(xr.shape[0], -np.inf)
                for j0 in range(0, M, 65536):
                    yy, hh = y64[j0:j0 + 65536], h64[j0:j0 + 65536]
                    true_max = np.maximum(true_max, (hh[None] - ((xr[:, None, :] - yy[None]) ** 2).sum(-1) / (2 * eps)).max(1))
                gone = groups[~k2]
                if gone.size:
                    cols = np.concatenate([np.arange(g * GROUP, min(M, (g + 1) * GROUP)) for g in gone])
                    terms = h64[cols][None] - ((xr[:, None, :] - y64[cols][None]) ** 2).sum(-1) / (2 * eps)
                    worst = max(worst, float((terms - (true_max - L)[:, None]).max()))
    return evaluated, kept1, worst


# ---- the mass rule (glhip_autosort.h, round 10): thresholds by dropped mass, found on histograms of the keys ----------------------------

BUCKETS, BUCKET_NATS = 112, 0.25                 # kPruneBuckets, kPruneBucketNats
MASS_SHARE = 0.5                                 # kPruneMassShare: the mass rule's part of the 2^-26 (the term rule keeps 1 / e)
BUDGET1 = 2.0**-26 * (1.0 - 1.0 / math.e - MASS_SHARE)      # first level, relative to e^Mlb(R)
BUDGET2 = 2.0**-26 * MASS_SHARE                  # second level's mass rule, relative to e^ms(W)
CHUNK = 128                                      # the rows of one f16 x 2 workgroup, half a slab: the chunk-live rule below (model only)
LSE_SLACK = np.float32(2.0**-20)                 # kPruneLseSlack
LOG2E = 1.4426950408889634
REF_BLOCKS = 16                                  # kPruneRefBlocks: reference blocks per slab (the sum reference, glhip_autosort.h)
REF_TOP, REF_CELLS_PER_NAT, REF_CELLS = 5.625, 16, 512      # kPruneRefTop, kPruneRefCellsPerNat, kPruneRefCells: the grid the scores are ranked on
SUM_SLACK = 1e-9                                 # kPruneSumSlack: Slb is lowered by this (float64 sums)
LS_SLACK = 1e-4                                  # kPruneLsSlack: ls_i is lowered by this (the device sums float32 exponentials)


def inv2eps_of(eps):
    """the device's 0.5 / (double)eps of the float32 eps it is handed"""
    return 0.5 / float(np.float32(eps))


def lse_up(hp):
    """prune_blocks_kernel: log sum exp of every row of hp (padding: -inf) as a float32 rounded up by the kernel's slack (the model
    sums in float64; the device's float32 sum differs by far less than the slack)"""
    m = hp.max(1)
    fin = np.isfinite(m)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.exp(hp - np.where(fin, m, 0.0)[:, None]).sum(1)
        v = np.where(fin, m + np.log(np.where(fin, s, 1.0)), m).astype(np.float32)
        up = (v + LSE_SLACK * (np.abs(v) + np.float32(8.0))).astype(np.float32)
    return np.where(fin, up, v).astype(np.float64)


def lse_dn(v, times=2):
    """The record v = lse_up(...) lowered by `times` of its own slack, in float64: never above the true log sum exp.  A group's record
    is rounded up once (times = 2), a block's twice — it is formed from its groups' rounded-up values (times = 4)."""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(v), v - times * float(LSE_SLACK) * (np.abs(v) + 8.0), v)


def logsumexp_rows(a):
    """log sum exp over the last axis, float64; a row without a finite entry gives -inf"""
    m = a.max(-1)
    fin = np.isfinite(m)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = np.exp(a - np.where(fin, m, 0.0)[..., None]).sum(-1)
        return np.where(fin, m + np.log(np.where(fin, s, 1.0)), -np.inf)


def reference_blocks(score, mlb, home, K=None):
    """prune_slabs_kernel's reference list of one slab: the blocks are ranked by their score on a grid of 1 / REF_CELLS_PER_NAT nats
    below Mlb + REF_TOP (no score lies above it), and whole cells are taken from the top while at most K - 1 blocks are in; the home
    block is always in.  Ascending block numbers."""
    K = REF_BLOCKS if K is None else K
    with np.errstate(invalid="ignore"):
        q = np.floor((mlb + REF_TOP - score) * REF_CELLS_PER_NAT)
    ok = np.isfinite(q) & (q < REF_CELLS)
    cell = np.clip(np.where(ok, q, 0), 0, REF_CELLS - 1).astype(np.int64)
    cum = np.cumsum(np.bincount(cell[ok], minlength=REF_CELLS))
    n_cells = int(np.searchsorted(cum, K - 1, side="right"))       # cells 0 .. n_cells - 1 hold at most K - 1 blocks
    take = ok & (cell < n_cells)
    take[home] = True
    return np.flatnonzero(take)


def group_block_lse(h, M):
    """(lse per group of 32, lse per block of 256): the block's value is formed from its groups' rounded-up values, as on the device"""
    nG, nT = (M + GROUP - 1) // GROUP, (M + BLOCK - 1) // BLOCK
    g = lse_up(np.concatenate([h.astype(np.float64), np.full(nG * GROUP - M, -np.inf)]).reshape(nG, GROUP))
    per = BLOCK // GROUP
    b = lse_up(np.concatenate([g, np.full(nT * per - nG, -np.inf)]).reshape(nT, per))
    return g, b


def bucket_of(key, lo):
    """prune_bucket: -1 below the histogram, BUCKETS above its range (never dropped)"""
    d = (key - lo) * (1.0 / BUCKET_NATS)
    with np.errstate(invalid="ignore"):
        return np.where(d < 0.0, -1, np.where(d < BUCKETS, np.floor(np.where(d < BUCKETS, d, 0.0)), BUCKETS)).astype(np.int64)


def first_kept(hist, under, budget):
    """prune_first_kept over the last axis: the first bucket whose mass would take the dropped sum past the budget"""
    over = under[..., None] + np.cumsum(hist, -1) > np.asarray(budget, np.float64)[..., None]
    return np.where(over.any(-1), over.argmax(-1), BUCKETS)


def plan_mass(xs, ys, h, eps, reference="sum", slb_out=None):
    """The first level under the mass rule: keep (C, nT) bool, Mlb (C,), t1 (C,), L — for finite inputs.  A slab that keeps every
    block is what the device calls home = -1.  The budget is a share of e^Slb(R), Slb = log sum_T e^(lse_dn(T) - dmaxpen(R, T)) >= Mlb,
    a lower bound of every row's SUM (reference = "term": of e^Mlb(R), as before library 136).  slb_out: a list that receives Slb (C,)."""
    M = ys.shape[0]
    rlo, rhi = boxes(xs, SLAB)
    blo, bhi = boxes(ys, BLOCK)
    nT = blo.shape[0]
    hmax = np.concatenate([h.astype(np.float64), np.full(nT * BLOCK - M, -np.inf)]).reshape(nT, BLOCK).max(1)
    _, blse = group_block_lse(h, M)
    bdn = lse_dn(blse, 4)
    L = math.log(M) + 26 * math.log(2) + MARGIN
    i2e = inv2eps_of(eps)
    C = rlo.shape[0]
    keep = np.zeros((C, nT), bool)
    mlb, t1, slb = np.zeros(C), np.zeros(C), np.zeros(C)
    for c0 in range(0, C, 256):
        a, b = rlo[c0:c0 + 256, None], rhi[c0:c0 + 256, None]
        gap = np.maximum(np.maximum(blo[None] - b, a - bhi[None]), 0.0)
        far = np.maximum(bhi[None] - a, b - blo[None])
        dmin2, dmax2 = (gap**2).sum(-1), (far**2).sum(-1)
        m = (hmax[None] - dmax2 * i2e).max(1)
        key = blse[None] - dmin2 * i2e
        lo = (m - L)[:, None]
        bk = bucket_of(key, lo)
        with np.errstate(over="ignore"):      # (keys above the range: never dropped, their mass is not used)
            mass = np.exp(key - m[:, None])
        n = m.shape[0]
        flat = (np.arange(n)[:, None] * (BUCKETS + 2) + bk + 1).ravel()
        hist = np.bincount(flat, weights=mass.ravel(), minlength=n * (BUCKETS + 2)).reshape(n, BUCKETS + 2)
        sl = m.copy()
        if reference == "sum":
            sl = logsumexp_rows(bdn[None] - dmax2 * i2e) - SUM_SLACK
            sl = np.where(np.isfinite(sl) & (sl > m), sl, m)
        fk = first_kept(hist[:, 1:BUCKETS + 1], hist[:, 0], BUDGET1 * np.exp(sl - m))
        mlb[c0:c0 + 256] = m
        slb[c0:c0 + 256] = sl
        t1[c0:c0 + 256] = m - L + fk * BUCKET_NATS
        keep[c0:c0 + 256] = bk >= fk[:, None]
    if slb_out is not None:
        slb_out.append(slb)
    return keep, mlb, t1, L


def t2_as_stored(t2_nats):
    """the device's record: log2 units, float32 rounded toward minus infinity"""
    v = np.asarray(t2_nats, np.float64) * LOG2E
    f = v.astype(np.float32)
    return np.where(f.astype(np.float64) > v, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def intervals_of(keep_row):
    """the column intervals of the kept blocks of one slab (without gap closing: at most RUNS runs)"""
    k = np.concatenate([[0], keep_row.astype(np.int8), [0]])
    d = np.diff(k)
    return [(int(a) * BLOCK, int(b) * BLOCK) for a, b in zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1))]


def level2_mass(xs, ys, h, eps, keep, L, slabs, intervals=None, reference="sum", ref_blocks=None):
    """The second level under the mass rule on the given slabs.  intervals: {slab: [(j0, je), ...]} to walk the device's emitted
    intervals instead of the runs of kept blocks.  Returns (pairs evaluated, pairs kept by the first level, per slab a dict with
    home, groups (the groups walked), ms, t2 (nats) per tile and skip (tiles, groups) bool).  A group is evaluated iff its key
    lse(G) - pen(W, G) lies in a bucket from the tile's first kept one on; the kernel's term rule, thr = ms - L against the same key,
    is bucket >= 0.  A chunk level between the two (modelled only — measured on the device and not kept, profiles/chunk_skip.txt):
    blocks (the column blocks walked) and live (2, blocks) bool per half slab of CHUNK rows — some group of the block lies in a bucket
    >= the first kept one of some row tile of the half slab, or the block is the home block; fk and top (tiles, blocks) are the first
    kept bucket and the block's largest bucket per tile.
    The budget is a share of e^ls(W): ls(W) = min_i max(seed_i, ls_i), ls_i = log sum_G e^(lse_dn(G) - dmaxpen(x_i, G)) - LS_SLACK over the
    groups G of the slab's reference blocks (refs in the record; ref_blocks: K) — a lower bound of the row's SUM (reference = "term": of
    e^ms(W), as before library 136).  ls (tiles,) joins the record."""
    N, M = xs.shape[0], ys.shape[0]
    x64, y64, h64 = xs.astype(np.float64), ys.astype(np.float64), h.astype(np.float64)
    rlo, rhi = boxes(xs, SLAB)
    blo, bhi = boxes(ys, BLOCK)
    glo, ghi = boxes(ys, GROUP)
    nT, nG = blo.shape[0], glo.shape[0]
    hmax = np.concatenate([h64, np.full(nT * BLOCK - M, -np.inf)]).reshape(nT, BLOCK).max(1)
    glse, blse = group_block_lse(h, M)
    gdn, bdn = lse_dn(glse, 2), lse_dn(blse, 4)
    gcols = np.minimum(GROUP, M - GROUP * np.arange(nG))
    i2e = inv2eps_of(eps)
    evaluated = kept1 = 0.0
    out = {}
    per_block = BLOCK // GROUP
    for c in slabs:
        far = np.maximum(bhi - rlo[c], rhi[c] - blo)
        dmax2 = (far**2).sum(-1)
        home = int(np.argmax(hmax - dmax2 * i2e))
        refs = reference_blocks(bdn - dmax2 * i2e, float((hmax - dmax2 * i2e)[home]), home, ref_blocks)
        rg = (refs[:, None] * per_block + np.arange(per_block)[None]).ravel()
        rg = rg[rg < nG]
        hc = np.arange(home * BLOCK, min(M, (home + 1) * BLOCK))
        iv = intervals[c] if intervals is not None else intervals_of(keep[c])
        groups = np.concatenate([np.arange(j0 // GROUP, (min(je, M) + GROUP - 1) // GROUP) for j0, je in iv if je > j0])
        r1 = min(N, (c + 1) * SLAB)
        ms, t2, skip, fks, top, lss = [], [], [], [], [], []
        blocks, inv = np.unique(groups // (BLOCK // GROUP), return_inverse=True)
        for w0 in range(c * SLAB, r1, TILE):
            xr = x64[w0:min(w0 + TILE, r1)]
            seed = (h64[hc][None] - ((xr[:, None, :] - y64[hc][None]) ** 2).sum(-1) * i2e).max(1)
            m = seed.min()
            ls = m
            if reference == "sum":
                pfar = np.maximum(np.abs(xr[:, None, :] - glo[rg][None]), np.abs(ghi[rg][None] - xr[:, None, :]))
                ls = float(np.maximum(logsumexp_rows(gdn[rg][None] - (pfar**2).sum(-1) * i2e) - LS_SLACK, seed).min())
                ls = ls if np.isfinite(ls) and ls > m else m
            wlo, whi = xr.min(0), xr.max(0)
            gap = np.maximum(np.maximum(glo[groups] - whi, wlo - ghi[groups]), 0.0)
            key = glse[groups] - (gap**2).sum(-1) * i2e
            bk = bucket_of(key, m - L)
            with np.errstate(over="ignore"):
                hist = np.bincount(bk + 1, weights=np.exp(key - m), minlength=BUCKETS + 2)
            with np.errstate(over="ignore"):      # (rows hundreds of nats apart: an infinite budget drops every bucket, as on the device)
                fk = int(first_kept(hist[1:BUCKETS + 1], hist[0], BUDGET2 * np.exp(np.float64(ls - m))))
            ms.append(m)
            lss.append(ls)
            t2.append(m - L + fk * BUCKET_NATS)
            skip.append(bk < fk)
            fks.append(fk)
            tb = np.full(blocks.size, -1, np.int64)
            np.maximum.at(tb, inv, bk)
            top.append(tb)
            evaluated += float(gcols[groups][bk >= fk].sum()) * xr.shape[0]
            kept1 += float(gcols[groups].sum()) * xr.shape[0]
        fks, top = np.array(fks), np.array(top)
        per = CHUNK // TILE
        live = np.zeros((SLAB // CHUNK, blocks.size), bool)
        for hs in range(live.shape[0]):
            rows = slice(hs * per, (hs + 1) * per)
            live[hs] = blocks == home
            if top[rows].shape[0]:
                live[hs] |= (top[rows] >= fks[rows, None]).any(0)
        out[c] = dict(home=home, groups=groups, ms=np.array(ms), t2=np.array(t2), skip=np.array(skip), blocks=blocks, live=live, fk=fks, top=top,
                      ls=np.array(lss), refs=refs)
    return evaluated, kept1, out


def dropped_share(xs, ys, h, eps, keep_row, rec, c):
    """On the points themselves, float64: for every row of slab c, the share of its true sum held by the columns the first level
    drops (keep_row) plus the columns of the groups the second level skips for the row's tile (rec: level2_mass's record)."""
    N, M = xs.shape[0], ys.shape[0]
    r0, r1 = c * SLAB, min(N, (c + 1) * SLAB)
    xr = xs[r0:r1].astype(np.float64)
    terms = np.empty((r1 - r0, M))
    for j0 in range(0, M, 65536):
        yy = ys[j0:j0 + 65536].astype(np.float64)
        terms[:, j0:j0 + 65536] = h[j0:j0 + 65536].astype(np.float64)[None] - ((xr[:, None, :] - yy[None]) ** 2).sum(-1) / (2 * float(np.float32(eps)))
    e = np.exp(terms - terms.max(1)[:, None])
    gone1 = np.repeat(~keep_row, BLOCK)[:M]
    share = np.zeros(r1 - r0)
    for t in range((r1 - r0 + TILE - 1) // TILE):
        gone = gone1.copy()
        for g in rec["groups"][rec["skip"][t]]:
            gone[g * GROUP:(g + 1) * GROUP] = True
        rows = slice(t * TILE, min((t + 1) * TILE, r1 - r0))
        share[rows] = e[rows][:, gone].sum(1) / e[rows].sum(1)
    return share


def bench_problem(n, seed=1000):
    """bench.make_problem(n, seed) without torch's device copy (same generator calls, same values)"""
    import torch

    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.rand(n, 3, generator=g)
    y = torch.rand(n, 3, generator=g)
    eps = 0.05**2
    h = torch.full((n,), -math.log(n)) + 0.01 * torch.randn(n, generator=g) / eps
    return x.numpy(), y.numpy(), h.numpy(), eps


def tiles_of(keep_row, width=512):
    """column tiles of `width` columns the reducing kernel stages for one slab: every run of kept blocks is walked in whole tiles"""
    k = np.concatenate([[0], keep_row.astype(np.int8), [0]])
    d = np.diff(k)
    return int(sum(-(-(int(b) - int(a)) * BLOCK // width) for a, b in zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1))))


def walk_live(iv, live_of, M, width=2 * BLOCK):
    """The walk a reducing kernel would make under the chunk level: inside the intervals iv = [(j0, je), ...] only the blocks t with
    live_of(t) are staged; a tile is one live block or two adjacent live blocks of one interval.  Returns the tiles as (first
    column, columns)."""
    tiles = []
    for j0, je in iv:
        je = min(je, M)
        t, te = j0 // BLOCK, -(-je // BLOCK)
        while t < te:
            if not live_of(t):
                t += 1
                continue
            two = width >= 2 * BLOCK and t + 1 < te and live_of(t + 1)
            tiles.append((t * BLOCK, min(je, (t + (2 if two else 1)) * BLOCK) - t * BLOCK))
            t += 2 if two else 1
    return tiles


def chunk_counts(rec, iv, M):
    """(512-column tiles staged today, tiles staged under the chunk level, blocks walked, blocks dead) summed over the half slabs of one
    slab's level2_mass record"""
    today = sum(-(-(min(je, M) - j0) // (2 * BLOCK)) for j0, je in iv if je > j0)
    tiles = dead = 0
    for hs in range(rec["live"].shape[0]):
        lv = dict(zip(rec["blocks"].tolist(), rec["live"][hs].tolist()))
        tiles += len(walk_live(iv, lambda t: lv.get(t, False), M))
        dead += int((~rec["live"][hs]).sum())
    return today * rec["live"].shape[0], tiles, rec["blocks"].size * rec["live"].shape[0], dead


def balanced_lines(x, y, h, n, eps_list, n_slabs):
    """The mass rule on today's order of the sorted p = 2 call and on the balanced one (balanced_order): first level, runs, gap closing,
    tiles, and the second level on a sample of slabs scaled to all of them by the first-level fraction."""
    sub = sort_sub(x.shape[1])
    px, py = compact_order2(x, 256, sub), compact_order2(y, 256, sub)
    C = (n + SLAB - 1) // SLAB
    slabs = np.arange(5, C, max(1, (C - 5) // n_slabs)) if n_slabs > 0 and C > 5 else np.zeros(0, int)
    rows = float(sum(min(n, (c + 1) * SLAB) - c * SLAB for c in slabs))
    for eps in eps_list:
        for name, qx, qy in (("path order", px, py), ("balanced 1024", balanced_order(x, px), balanced_order(y, py))):
            xs, ys, hs = x[qx], y[qy], h[qy]
            keep, mlb, t1, L = plan_mass(xs, ys, hs, eps)
            r = runs_per_slab(keep)
            closed = keep.copy()
            for c in np.flatnonzero(r > RUNS):
                closed[c] = closed_gaps(keep[c])
            first = kept_pairs(closed, n, n) / (float(n) * n)
            line = (f"{name}: n = {n}  eps = {eps:.4g}: first level keeps {kept_pairs(keep, n, n) / (float(n) * n):.4f}, runs per slab mean "
                    f"{r.mean():.1f} max {r.max()}, slabs over {RUNS} runs {(r > RUNS).sum()}, kept blocks {int(keep.sum())} + {int(closed.sum() - keep.sum())} "
                    f"by gap closing, 512-column tiles {sum(tiles_of(closed[c]) for c in range(C))}")
            if len(slabs):
                ev, k1, rec = level2_mass(xs, ys, hs, eps, closed, L, slabs)
                line += (f"; on {len(slabs)} slabs: first level {k1 / (rows * n):.4f}, evaluated after the second {ev / (rows * n):.4f}, "
                         f"scaled to all slabs {ev / k1 * first:.4f}")
                cc = np.array([chunk_counts(rec[c], intervals_of(closed[c]), n) for c in slabs if not closed[c].all()]).sum(0)
                if cc.ndim and cc[0]:
                    line += (f"; chunk level (half slabs of {CHUNK} rows): {cc[3] / cc[2]:.4f} of the walked blocks dead, tiles staged "
                             f"{cc[1]} against {cc[0]} ({cc[1] / cc[0]:.4f})")
            print(line, flush=True)


def uniform_problem(n, seed=1000):
    """the bench clouds with a uniform dual vector h = -ln n: smooth potentials, where the row sum exceeds its largest term most"""
    x, y, h, eps = bench_problem(n, seed)
    return x, y, np.full(n, -math.log(n), np.float32), eps


def reference_lines(n, eps_list, n_slabs, ref_blocks=(REF_BLOCKS,)):
    """The old reference of the two mass budgets (one term the row has: e^Mlb, e^ms) beside the new one (a lower bound of the row sum:
    e^Slb, e^ls), balanced order: first level, tiles, evaluated pairs and the gained nats, bench law and a uniform dual vector."""
    for law, (x, y, h, _) in (("bench law", bench_problem(n)), ("uniform h", uniform_problem(n))):
        sub = sort_sub(x.shape[1])
        qx, qy = balanced_order(x, compact_order2(x, 256, sub)), balanced_order(y, compact_order2(y, 256, sub))
        xs, ys, hs = x[qx], y[qy], h[qy]
        C = (n + SLAB - 1) // SLAB
        slabs = np.arange(5, C, max(1, (C - 5) // n_slabs)) if n_slabs > 0 and C > 5 else np.zeros(0, int)
        for eps in eps_list:
            base = None
            for ref, K in [("term", 0)] + [("sum", k) for k in ref_blocks]:
                got = []
                keep, mlb, t1, L = plan_mass(xs, ys, hs, eps, reference=ref, slb_out=got)
                closed = keep.copy()
                for c in np.flatnonzero(runs_per_slab(keep) > RUNS):
                    closed[c] = closed_gaps(keep[c])
                first = kept_pairs(closed, n, n) / (float(n) * n)
                tiles = sum(tiles_of(closed[c]) for c in range(C))
                line = (f"{law}: n = {n}  eps = {eps:.4g}  reference {ref}" + (f" K = {K}" if K else "") + f": first level keeps {first:.4f}, "
                        f"512-column tiles {tiles}, Slb - Mlb mean {(got[0] - mlb).mean():.3f} nats")
                if len(slabs):
                    ev, k1, rec = level2_mass(xs, ys, hs, eps, closed, L, slabs, reference=ref, ref_blocks=K or None)
                    gain = np.concatenate([rec[c]["ls"] - rec[c]["ms"] for c in slabs])
                    frac = ev / k1 * first
                    base = frac if base is None else base
                    line += (f"; on {len(slabs)} slabs: evaluated, scaled to all slabs {frac:.4f} ({frac / base - 1:+.1%}), ls - ms mean {gain.mean():.3f} "
                             f"min {gain.min():.3f} nats, reference blocks mean {np.mean([rec[c]['refs'].size for c in slabs]):.1f}")
                print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--balanced", action="store_true", help="only the lines that compare the path order with the balanced one")
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--eps", type=float, nargs="*", default=[0.01**2, 0.05**2, 0.2**2, 1.0])
    ap.add_argument("--slabs", type=int, default=40, help="slabs sampled for the second level (0: first level only)")
    ap.add_argument("--ref-blocks", type=int, nargs="*", default=[REF_BLOCKS], help="reference blocks per slab (K) for the old-against-new lines")
    a = ap.parse_args()
    x, y, h, _ = bench_problem(a.n)
    if a.balanced:
        balanced_lines(x, y, h, a.n, a.eps, a.slabs)
        return reference_lines(a.n, a.eps, a.slabs, a.ref_blocks)
    px, py = compact_order(x, 256), compact_order(y, 512)
    xs, ys, hs = x[px], y[py], h[py]
    for eps in a.eps:
        keep, mlb, L = plan(xs, ys, hs, eps)
        r = runs_per_slab(keep)
        frac = kept_pairs(keep, a.n, a.n) / (float(a.n) * a.n)
        print(f"n = {a.n}  eps = {eps:.4g}: L = {L:.2f} nats, kept pairs {frac:.4f}, kept blocks per slab {keep.sum(1).mean():.0f} of {keep.shape[1]}, "
              f"runs per slab mean {r.mean():.1f} max {r.max()}, slabs over {RUNS} runs {(r > RUNS).sum()}", flush=True)
    if a.slabs <= 0:
        return
    # the sorted p = 2 call: voxels of 256 points for both clouds; with and without the minor key
    for sub in (1, sort_sub(3)):
        px, py = compact_order2(x, 256, sub), compact_order2(y, 256, sub)
        xs, ys, hs = x[px], y[py], h[py]
        C = (a.n + SLAB - 1) // SLAB
        slabs = np.unique(np.linspace(0, C - 1, a.slabs).astype(int))
        rows = float(sum(min(a.n, (c + 1) * SLAB) - c * SLAB for c in slabs))
        for eps in a.eps:
            keep, mlb, L = plan(xs, ys, hs, eps)
            r = runs_per_slab(keep)
            ev, k1, _ = level2(xs, ys, hs, eps, keep, L, slabs)
            print(f"two levels, voxels 256 / 256, sub {sub}: n = {a.n}  eps = {eps:.4g}: first level keeps {kept_pairs(keep, a.n, a.n) / (float(a.n) * a.n):.4f} "
                  f"(runs per slab mean {r.mean():.1f} max {r.max()}); on {len(slabs)} slabs: first level {k1 / (rows * a.n):.4f}, "
                  f"evaluated after the second {ev / (rows * a.n):.4f}", flush=True)
            if sub == 1:
                continue
            keep, mlb, t1, L = plan_mass(xs, ys, hs, eps)
            r = runs_per_slab(keep)
            ev, k1, _ = level2_mass(xs, ys, hs, eps, keep, L, slabs)
            print(f"mass rule,  voxels 256 / 256, sub {sub}: n = {a.n}  eps = {eps:.4g}: first level keeps {kept_pairs(keep, a.n, a.n) / (float(a.n) * a.n):.4f} "
                  f"(runs per slab mean {r.mean():.1f} max {r.max()}, slabs over {RUNS} runs {(r > RUNS).sum()}); on {len(slabs)} slabs: "
                  f"first level {k1 / (rows * a.n):.4f}, evaluated after the second {ev / (rows * a.n):.4f}", flush=True)
    balanced_lines(x, y, h, a.n, a.eps, a.slabs)
    reference_lines(a.n, a.eps, a.slabs, a.ref_blocks)


if __name__ == "__main__":
    main()
