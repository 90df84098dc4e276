"""What the parity tests on small clouds share: the clouds themselves, their upload, the bound of the expanded p = 2 form, random block-sparse
ranges, and the float64 reference of the p = 2 plan application.  A plain module (NumPy in, NumPy out, but for ``to_dev``); its host-side
checks are in tests/test_support_cpu.py.  Each test file keeps its own temperatures, bounds and cases."""
import numpy as np
import torch

from geomloss_amd import hip
from geomloss_amd.cluster import from_matrix


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def clouds(seed, N, M, D, B=None, offset=0.0):
    """x uniform on the unit cube, y on its middle [0.1, 0.9]^D, both moved by ``offset``; h standard normal.  float32, (n, D) or
    (B, n, D).  The Python float 0.0 added to a float32 array changes neither its dtype nor its bits (the values are >= 0: no -0.0)."""
    rng = np.random.default_rng(seed)
    shp = (lambda n: (n, D)) if B is None else (lambda n: (B, n, D))
    x = rng.random(shp(N)).astype(np.float32) + offset
    y = (rng.random(shp(M)) * 0.8 + 0.1).astype(np.float32) + offset
    h = rng.standard_normal(shp(M)[:-1]).astype(np.float32)
    return x, y, h


def tol(ref, D):
    return 4e-7 * D + 2e-6 * np.abs(ref).max()       # expanded form in fp32: ~2^-22 diam^2 on a potential; diam^2 <= D on the unit cube


def random_ranges(rng, N, M, ci, cj, density, dev):
    """ci x cj ragged clusters, a random ``density`` of the pairs kept -> (ranges, the oracle's (ranges_i, slices_i, redranges_j), the
    same transposed, the kept pairs, the row ranges)"""
    cut_i = np.sort(rng.choice(np.arange(1, N), ci - 1, replace=False))
    cut_j = np.sort(rng.choice(np.arange(1, M), cj - 1, replace=False))
    ri = np.stack([np.r_[0, cut_i], np.r_[cut_i, N]], 1).astype(np.int32)
    rj = np.stack([np.r_[0, cut_j], np.r_[cut_j, M]], 1).astype(np.int32)
    keep = rng.random((ci, cj)) < density
    keep[0, :] = False      # one row block with nothing to reduce over
    keep[1, :] = True
    rg = from_matrix(torch.from_numpy(ri).to(dev), torch.from_numpy(rj).to(dev), torch.from_numpy(keep).to(dev))
    tup = tuple(t.cpu().numpy() for t in (rg.ranges_i, rg.slices_i, rg.redranges_j))
    tup_t = tuple(t.cpu().numpy() for t in (rg.ranges_j, rg.slices_j, rg.redranges_i))
    return rg, tup, tup_t, keep, ri


def plan_ref(x, y, h, eps, feat, rows=64):
    """float64: W @ feat with rows of W = exp(E - lse(E)) summing to 1 (0 for a row without mass), p = 2, row-chunked so that M = 70 001
    stays small."""
    x, y, h, feat = (np.asarray(t, dtype=np.float64) for t in (x, y, h, feat))
    out = np.zeros((x.shape[0], feat.shape[1]))
    for i0 in range(0, x.shape[0], rows):
        xi = x[i0:i0 + rows]
        E = h[None, :] - ((xi * xi).sum(1)[:, None] - 2.0 * xi @ y.T + (y * y).sum(1)[None, :]) / (2.0 * eps)
        m = E.max(1, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)
        W = np.exp(E - m)
        s = W.sum(1, keepdims=True)
        out[i0:i0 + rows] = (W / np.where(s > 0, s, 1.0)) @ np.where(np.isfinite(feat), feat, 0.0)
    return out


def plan_apply(dev, x, y, h, feat, eps, flags=0, *, raw, **kw):
    """Raw launch (``raw``: hip.plan_apply_raw or hip.plan_apply_nd_raw) on (N,D) / (B,N,D) NumPy inputs -> out, mass as NumPy."""
    xb, yb, hb, fb = (to_dev(a, dev) for a in (x, y, h, feat))
    if xb.dim() == 2:
        xb, yb, hb, fb = xb[None], yb[None], hb[None], fb[None]
    fwd = hip.softmin_fwd_raw(xb, yb, hb, eps, 2, None, flags)
    out, mass = raw(xb, yb, hb, fwd, fb, eps, flags, want_mass=True, **kw)
    out, mass = out.cpu().numpy(), mass.cpu().numpy()
    return (out[0], mass[0]) if np.ndim(x) == 2 else (out, mass)


def plan_worst(out, ref, feat):
    """max over columns of max_i |out - ref| / max_j |feat_j|."""
    scale = np.abs(feat).reshape(-1, feat.shape[-1]).max(0) if feat.ndim == 2 else np.abs(feat).max(-2, keepdims=True)
    scale = np.where(scale > 0, scale, 1.0)
    return float((np.abs(out - ref) / scale).max())
