"""The matrix-core row gradients of the distance reductions of 17 <= D <= 4095 (``FLAG_XK_DIST_GRAD``, geomloss_amd/csrc/glhip_dist_grad_xk.h):
the p = 1 soft-min gradient (``glhip_softmin_bwd_x``) and the laplacian / energy kernel gradients (``glhip_kernel_conv_bwd_x``,
``glhip_kernel_conv_fwd_grad``) against float64.

References: ``oracle_c.softmin_grad_x`` / ``kconv_grad_x`` up to D = 64, ``oracle_torch64`` beyond (``_grad64`` of the sweep).  Inputs and
helpers are those of tests/test_dimension_sweep_gpu.py.  Bounds are the project's own for this dimension range: ``relerr <= 5e-6`` at
eps = 0.3 for the soft-min (``_softmin_grad_setups(D, 1)``) and 5e-6 for the products (``_kconv_grad_bound``); for D > 64 the rule of
tests/test_softmin_grad_xk_gpu.py::test_parity: ``max(5e-6, 4 x the error of the same gradient in plain float32 torch)``.  Every launch
carries the flag and is preceded by the predicate assertion.  Each test prints its worst error / bound per kind and, beside it, the
generic kernel's on the same inputs (``pytest -s``; profiles/dist_grad_xk.txt).  The teeth of the near-pair case are checked on the host
in tests/test_dist_grad_xk_cpu.py."""
import math

import numpy as np
import pytest
import torch

from conftest import relerr
from geomloss_amd import SamplesLoss, hip, kernel_samples, sinkhorn_samples
from oracle import oracle_c
from oracle import oracle_torch64 as o64
from test_dimension_sweep_gpu import (CPU, _blur, _case, _finish, _grad64, _host_kconv_grad, _host_softmin_grad, _items, _kconv_grad_bound,
                                      _launches, _Report, _rows, _softmin_grad_setups, _t, _weights)
from test_dist_grad_xk_cpu import NEAR_EPS, NEAR_S, near_clouds

pytestmark = pytest.mark.gpu

XDG, NS = hip.FLAG_XK_DIST_GRAD, hip.FLAG_NO_SPLIT
KINDS = ("laplacian", "energy")
OPS = ("softmin_p1",) + KINDS
SMALL = [17, 31, 32, 33, 47, 63, 64, 65, 96, 97, 127, 130]
LARGE = [257, 1024, 4095]
EPS = 0.3
assert _softmin_grad_setups(17, 1) == [("p1", EPS, (0,), 5e-6)] and _kconv_grad_bound("laplacian", 17) == 5e-6
BOUND = 5e-6
KBOUND_WIDE = 12 * 5e-6      # the product bound of tests/test_dist_xk_gpu.py (_kbound)


def _b3(t):
    """(N, D) | (B, N, D) -> (B, N, D); (M,) | (B, M) -> (B, M) follows with ``_b2``."""
    return (t if t.dim() == 3 else t.unsqueeze(0)).contiguous()


def _b2(t, like):
    return (t if like.dim() == 3 else t.unsqueeze(0)).contiguous()


def _dtype(x):
    return hip.BF16 if x.dtype == torch.bfloat16 else hip.F32


def _uses(op, x, y, flags, want=1):
    xb, yb = _b3(x), _b3(y)
    got = hip.dist_grad_uses_xk(op, xb.shape[0], xb.shape[1], yb.shape[1], xb.shape[2], _dtype(x), flags)
    assert got == want, (op, tuple(xb.shape), tuple(yb.shape), flags, got)


def sm_grad(x, y, h, g, flags, eps=EPS, workspace=True):
    """``glhip_softmin_bwd_x`` with p = 1 on tensors shaped like the sweep's launches; the saved forward value comes from the default
    forward (the matrix-core gradient does not read it)."""
    if flags & XDG:
        _uses("softmin_p1", x, y, flags)
    with torch.no_grad():
        fwd = hip.softmin(eps, x, y, h, p=1)
        out = hip.softmin_bwd_x_raw(_b3(x), _b3(y), _b2(h, x), _b2(fwd, x), _b2(g, x), eps, 1, None, flags, workspace)
    return out.reshape(x.shape)


def kc_grad(kind, x, y, v, g, blur, flags, workspace=True):
    """``glhip_kernel_conv_bwd_x``."""
    if flags & XDG:
        _uses(kind, x, y, flags)
    out = hip.kernel_conv_bwd_x_raw(hip.KERNEL_KINDS[kind], _b3(x), _b3(y), _b2(v, x), _b2(g, x), blur, None, flags, workspace)
    return out.reshape(x.shape)


def grad_of(op, x, y, s, g, scale, flags, workspace=True):
    return sm_grad(x, y, s, g, flags, scale, workspace) if op == "softmin_p1" else kc_grad(op, x, y, s, g, scale, flags, workspace)


def ref_of(op, D, x, y, s, g, scale):
    """float64 reference of one 2-D problem (NumPy inputs)."""
    if op == "softmin_p1":
        return _grad64(oracle_c.softmin_grad_x, o64.softmin_grad_x, D, scale, x, y, s, g, 1)
    return _grad64(oracle_c.kconv_grad_x, o64.kconv_grad_x, D, op, x, y, s, g, scale)


def f32_error(dev, op, x, y, s, g, scale, ref):
    """The same gradient in plain float32 torch (expanded squared distances, the reference's clamp, autograd)."""
    xt = _t(x, dev).requires_grad_(True)
    yt, st, gt = _t(y, dev), _t(s, dev), _t(g, dev)
    d2 = (xt * xt).sum(1)[:, None] - 2.0 * xt @ yt.t() + (yt * yt).sum(1)[None, :]
    if op == "softmin_p1":
        out = -scale * torch.logsumexp(st[None, :] - d2.clamp_min(1e-8).sqrt() / scale, dim=1)
    elif op == "laplacian":
        out = torch.exp(-(d2 / scale**2).clamp_min(1e-8).sqrt()) @ st
    else:
        out = -(d2.clamp_min(1e-8).sqrt() @ st)
    (gx,) = torch.autograd.grad(out, [xt], grad_outputs=gt)
    return relerr(gx.cpu().numpy(), ref)


def _bound(dev, op, D, err, x, y, s, g, scale, ref):
    """5e-6; D > 64: test_parity's rule, evaluated only when the flat bound is missed."""
    if D > 64 and err > BOUND:
        return max(BOUND, 4.0 * f32_error(dev, op, x, y, s, g, scale, ref))
    return BOUND


def _scale(op, D):
    return EPS if op == "softmin_p1" else _blur(D)


def _check(rep, gen, dev, op, D, variant, x, y, s, g, scale=None, flags=XDG, layout=None, ref=None, tensors=None, scale_by=None):
    """One 2-D problem (NumPy inputs, or ``tensors`` = their device copies in another dtype) against float64: the matrix-core gradient
    into ``rep`` (asserted), the generic kernel into ``gen`` (printed).  ``scale_by``: the array whose largest entry the error is relative
    to (default: the reference)."""
    scale = _scale(op, D) if scale is None else scale
    ref = ref_of(op, D, x, y, s, g, scale) if ref is None else ref
    xt, yt, st, gt = tensors if tensors is not None else tuple(_t(a, dev) for a in (x, y, s, g))
    out = grad_of(op, xt, yt, st, gt, scale, flags).cpu().numpy()
    assert np.isfinite(out).all(), (op, D, variant)
    den = max(np.abs(ref if scale_by is None else scale_by).max(), 1e-300)
    err = float(np.abs(out - ref).max() / den)
    rep.add(D, f"{op} {variant} flags={flags}", err, _bound(dev, op, D, err, x, y, s, g, scale, ref), layout or op, strict=False)
    if gen is not None:
        base = grad_of(op, xt, yt, st, gt, scale, flags & ~XDG).cpu().numpy()
        gen.add(D, f"{op} {variant}", float(np.abs(base - ref).max() / den), BOUND, layout or op, strict=False)
    return out


def _done(rep, gen=None):
    if gen is not None:
        gen.failures()      # printed only: the generic kernel is not under test here
    _finish(rep)


def _law(rng, N, M, D):
    """the sweep's input law (per-coordinate scales: coordinates are not exchangeable)"""
    s = 0.5 + 0.5 * rng.random(D)
    x = (rng.random((N, D)) * s).astype(np.float32)
    y = ((rng.random((M, D)) * 0.8 + 0.1) * s).astype(np.float32)
    h = rng.standard_normal(M).astype(np.float32)
    g = rng.standard_normal(N).astype(np.float32)
    return x, y, h, g


# ---- 1. dimensions ---------------------------------------------------------------------------------------------------------------
def test_dimensions(cuda):
    """Pass boundaries at 32 and 64 coordinates and remainders of 1; the sweep's shapes, dense and batched, with and without column
    splits.  Teeth: the float64 reference without the last coordinate moves by >= 100 bounds (D <= 130) resp. >= 1 bound."""
    rep, gen = _Report("dist grad dimensions"), _Report("generic kernel, dimensions")
    for D in SMALL + LARGE:
        big = D in LARGE
        refs = {"softmin_p1": _host_softmin_grad(D, 1)}
        refs.update({kind: _host_kconv_grad(kind, D) for kind in KINDS})
        for op in OPS:
            rep.teeth(D, f"{op} gradient", refs[op][1], 1 if big else 100)
        items = {tag: (x, y, h) for tag, x, y, h in _items(D, big)}
        for flags in (XDG, XDG | NS):
            for tags, (x, y, h) in _launches(D, cuda, big):
                v = h.abs() / h.shape[-1]
                for op in OPS:
                    key = (lambda t: ("p1", t)) if op == "softmin_p1" else (lambda t: t)
                    g = _t(np.stack([refs[op][0][key(t)][1] for t in tags]), cuda).reshape(x.shape[:-1])
                    s, scale = (h if op == "softmin_p1" else v), _scale(op, D)
                    outs = _rows(grad_of(op, x, y, s, g, scale, flags), tags)
                    base = _rows(grad_of(op, x, y, s, g, scale, flags & ~XDG), tags) if flags == XDG else None
                    for k, tag in enumerate(tags):
                        ref, gi = refs[op][0][key(tag)]
                        xi, yi, hi = items[tag]
                        si = hi if op == "softmin_p1" else _weights(hi)
                        err = relerr(outs[k], ref)
                        rep.add(D, f"{op} flags={flags} {tag}", err, _bound(cuda, op, D, err, xi, yi, si, gi, scale, ref), op, strict=False)
                        if base is not None:
                            gen.add(D, f"{op} {tag}", relerr(base[k], ref), BOUND, op, strict=False)
    _done(rep, gen)


# ---- 2. several row blocks and tiles ---------------------------------------------------------------------------------------------
def test_row_blocks_and_tiles(cuda):
    """N = 300, M = 270: two row blocks (the second of 44 rows, centred on its own first row), three column tiles, the last of 14
    columns; float32 and bfloat16 clouds (the reference on the rounded inputs)."""
    rep, gen = _Report("dist grad row blocks"), _Report("generic kernel, row blocks")
    N, M = 300, 270
    for D in (17, 64, 130):
        x, y, h, g = _law(np.random.default_rng(2000 + D), N, M, D)
        v = _weights(h)
        xb, yb = _t(x, cuda).bfloat16(), _t(y, cuda).bfloat16()
        xr, yr = xb.float().cpu().numpy(), yb.float().cpu().numpy()
        for op in OPS:
            s = h if op == "softmin_p1" else v
            _check(rep, gen, cuda, op, D, "f32", x, y, s, g, layout=f"{op} f32")
            _check(rep, gen, cuda, op, D, "bf16", xr, yr, s, g, layout=f"{op} bf16", tensors=(xb, yb, _t(s, cuda), _t(g, cuda)))
    _done(rep, gen)


# ---- 3. column splits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,D", [(130, 70001, 24), (300, 5000, 33)])
def test_column_splits(cuda, N, M, D):
    """(130, 70001, 24): the XCD-aware grid (M >= 65536); (300, 5000, 33): the plain grid with several splits, two row blocks and two
    passes.  Split and unsplit launches against the oracle and each other (2 bounds); no workspace = NO_SPLIT, bit for bit."""
    rep, gen = _Report(f"dist grad column splits {N} x {M}"), _Report("generic kernel, column splits")
    x, y, h, g = _law(np.random.default_rng(3000 + D), N, M, D)
    v = _weights(h)
    lib = hip.load_library()
    per_split = N * (min(D, int(lib.glhip_dist_grad_pass_width())) + 2) * 4
    assert int(lib.glhip_dist_grad_workspace_bytes(1, N, M, D, XDG)) >= 2 * per_split      # the launch does split
    xt, yt, gt = _t(x, cuda), _t(y, cuda), _t(g, cuda)
    for op in OPS:
        s = h if op == "softmin_p1" else v
        scale, st = _scale(op, D), _t(s, cuda)
        ref = ref_of(op, D, x, y, s, g, scale)
        outs = {flags: _check(rep, gen if flags == XDG else None, cuda, op, D, "split" if flags == XDG else "unsplit", x, y, s, g, flags=flags, ref=ref)
                for flags in (XDG, XDG | NS)}
        rep.add(D, f"{op} split vs unsplit", np.abs(outs[XDG] - outs[XDG | NS]).max() / np.abs(ref).max(), 2 * BOUND, f"{op} pair", strict=False)
        bare = grad_of(op, xt, yt, st, gt, scale, XDG, workspace=False)
        assert torch.equal(bare.cpu(), torch.tensor(outs[XDG | NS])), op
    _done(rep, gen)


# ---- 4. near pairs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [17, 64, 130])
def test_near_pairs(cuda, D):
    """What the exact near-pair path is for, N = M = 300.  (a) the self-term y = x: the diagonal sits on the clamp of utils.py:61 and
    contributes no direction; (b) y = x + s noise, s = 3e-5 (around the clamp), 1e-4, 1e-3; (c) as (b) with both clouds shifted by +10 in
    every coordinate (the centring).  On the host, float32 xs W - S without the exact path misses the bound of (b) by 24 ... 3110 x
    (tests/test_dist_grad_xk_cpu.py::test_near_pairs_have_teeth)."""
    rep, gen = _Report(f"dist grad near pairs D={D}"), _Report(f"generic kernel, near pairs D={D}")
    assert NEAR_EPS == EPS
    x, _, h, g = near_clouds(D, 0.0)
    v = _weights(h)
    cases = [("y = x", x, x.copy())]
    for s in NEAR_S:
        cases.append((f"y = x + {s:g} noise",) + near_clouds(D, s)[:2])
        cases.append((f"y = x + {s:g} noise, +10",) + near_clouds(D, s, 10.0)[:2])
    for name, xc, yc in cases:
        layout = "self" if name == "y = x" else "shifted" if name.endswith("+10") else "near"
        for op in OPS:
            _check(rep, gen, cuda, op, D, name, xc, yc, h if op == "softmin_p1" else v, g, layout=f"{op} {layout}")
    _done(rep, gen)


# ---- 5. infinities and padding ---------------------------------------------------------------------------------------------------
def test_infinities_and_padding(cuda):
    """D = 33 (two passes, the second of one coordinate)."""
    rep = _Report("dist grad infinities")
    D = 33
    x, y, h, *_ = _case(D)
    N, M = x.shape[0], y.shape[0]
    g = np.random.default_rng(533).standard_normal(N).astype(np.float32)
    xt, yt, gt = _t(x, cuda), _t(y, cuda), _t(g, cuda)
    # a quarter of the duals at -inf
    hq = np.array(h)
    hq[::4] = -np.inf
    _check(rep, None, cuda, "softmin_p1", D, "a quarter of h at -inf", x, y, hq, g)
    # all duals at -inf, with (150) and without (160) a padded last group of columns, split or not: zeros, never NaN
    for Mi in (M, 160):
        yy = _t(np.concatenate([y, y[: Mi - M] + np.float32(0.01)]) if Mi > M else y, cuda)
        allinf = torch.full((Mi,), -math.inf, device=cuda)
        _uses("softmin_p1", xt, yy, XDG)
        for flags in (XDG, XDG | NS):
            out = hip.softmin_bwd_x_raw(_b3(xt), _b3(yy), _b2(allinf, xt), torch.zeros((1, N), device=cuda), _b2(gt, xt), EPS, 1, None, flags)
            assert bool(torch.isfinite(out).all()) and bool((out == 0).all()), (Mi, flags)
    # product weights of mixed sign: error relative to the gradient under |v|
    v = (np.random.default_rng(534).standard_normal(M) / M).astype(np.float32)
    for kind in KINDS:
        _check(rep, None, cuda, kind, D, "signed weights", x, y, v, g, scale_by=ref_of(kind, D, x, y, np.abs(v), g, _blur(D)))
    # g = 0 rows give exact zeros
    g0 = np.array(g)
    g0[::3] = 0.0
    for op in OPS:
        s = h if op == "softmin_p1" else _weights(h)
        out = _check(rep, None, cuda, op, D, "g = 0 rows", x, y, s, g0)
        assert (out[::3] == 0).all(), op
    # N = 1 and M = 1
    for op in OPS:
        s = h if op == "softmin_p1" else _weights(h) * M      # (weights of order 1: one column carries the whole product)
        _check(rep, None, cuda, op, D, "N = 1", x[:1], y, s, g[:1])
        _check(rep, None, cuda, op, D, "M = 1", x, y[:1], s[:1], g)
        _check(rep, None, cuda, op, D, "N = M = 1", x[:1], y[:1], s[:1], g[:1])
    _done(rep)


# ---- 6. product and gradient in one set of passes --------------------------------------------------------------------------------
def test_fwd_grad(cuda):
    """``glhip_kernel_conv_fwd_grad`` of the laplacian / energy kernels under the flag: the product against ``hip.kernel_conv`` under
    ``FLAG_XK_DIST`` (the product bound of tests/test_dist_xk_gpu.py), g x unit against ``glhip_kernel_conv_bwd_x``, and the gradient through
    autograd with and without the fused product-and-gradient launch."""
    rep = _Report("dist grad fwd_grad")
    fusion = hip.kernel_grad_fusion()
    try:
        for D, N, M in ((33, 70, 150), (64, 300, 270), (130, 70, 2000)):
            x, y, h, g = _law(np.random.default_rng(6000 + D), N, M, D)
            v, blur = _weights(h), _blur(D)
            xt, yt, vt, gt = (_t(a, cuda) for a in (x, y, v, g))
            for kind in KINDS:
                ref = ref_of(kind, D, x, y, v, g, blur)
                for flags in (XDG, XDG | NS):
                    _uses(kind, xt, yt, flags)
                    out, unit = hip.kernel_conv_fwd_grad_raw(hip.KERNEL_KINDS[kind], _b3(xt), _b3(yt), _b2(vt, xt), blur, None, flags)
                    fwd = hip.kernel_conv(kind, xt, yt, vt, blur, flags=hip.FLAG_XK_DIST | (flags & NS))
                    assert hip.kernel_conv_fwd_family(kind, 1, N, M, D, hip.F32, hip.FLAG_XK_DIST) == hip.FAMILY_DIST
                    rep.add(D, f"{kind} product flags={flags}", (out[0] - fwd).abs().max().item(), KBOUND_WIDE * fwd.abs().max().item(), f"{kind} product", strict=False)
                    bwd = kc_grad(kind, xt, yt, vt, gt, blur, flags)
                    rep.add(D, f"{kind} g x unit vs bwd_x flags={flags}", relerr((gt[:, None] * unit[0]).cpu().numpy(), bwd.cpu().numpy()), BOUND, f"{kind} unit", strict=False)
                    err = relerr((gt[:, None] * unit[0]).cpu().numpy(), ref)
                    rep.add(D, f"{kind} g x unit flags={flags}", err, _bound(cuda, kind, D, err, x, y, v, g, blur, ref), f"{kind} unit vs float64", strict=False)
                for fuse in (True, False):
                    hip.set_kernel_grad_fusion(fuse)
                    xg = xt.clone().requires_grad_(True)
                    (gx,) = torch.autograd.grad(hip.kernel_conv(kind, xg, yt, vt, blur, flags=XDG), [xg], grad_outputs=gt)
                    err = relerr(gx.cpu().numpy(), ref)
                    rep.add(D, f"{kind} autograd fuse={fuse}", err, _bound(cuda, kind, D, err, x, y, v, g, blur, ref), f"{kind} autograd", strict=False)
    finally:
        hip.set_kernel_grad_fusion(fusion)
    _done(rep)


# ---- 7. opt-in and reproducibility -----------------------------------------------------------------------------------------------
def test_flag_is_opt_in_and_runs_are_reproducible(cuda):
    D = 33
    x, y, h, *_ = _case(D)
    g = np.random.default_rng(733).standard_normal(x.shape[0]).astype(np.float32)
    xt, yt, ht, gt = (_t(a, cuda) for a in (x, y, h, g))
    vt = ht.abs() / ht.shape[-1]
    # without the flag: the generic kernel, before and after
    for op in OPS:
        s, scale = (ht if op == "softmin_p1" else vt), _scale(op, D)
        _uses(op, xt, yt, 0, want=0)
        plain, generic = grad_of(op, xt, yt, s, gt, scale, 0), grad_of(op, xt, yt, s, gt, scale, hip.FLAG_NO_MFMA)
        assert torch.equal(plain, generic), op
        assert not torch.equal(plain, grad_of(op, xt, yt, s, gt, scale, XDG)), op      # (another kernel: another rounding)
    # p = 2 and the gaussian gradient under FLAG_XK_GRAD do not see the new bit
    XK = hip.FLAG_XK_GRAD
    eps2 = 0.1 * D / 3
    with torch.no_grad():
        fwd = hip.softmin(eps2, xt, yt, ht, p=2)
    p2 = [hip.softmin_bwd_x_raw(_b3(xt), _b3(yt), _b2(ht, xt), _b2(fwd, xt), _b2(gt, xt), eps2, 2, None, f) for f in (XK, XK | XDG)]
    assert hip.softmin_bwd_x_uses_plan(1, x.shape[0], y.shape[0], D, p=2, flags=XK | XDG) == 1 and torch.equal(*p2)
    ga = [hip.kernel_conv_bwd_x_raw(hip.GAUSSIAN, _b3(xt), _b3(yt), _b2(vt, xt), _b2(gt, xt), _blur(D), None, f) for f in (XK, XK | XDG)]
    assert hip.kernel_conv_grad_uses_xk("gaussian", 1, x.shape[0], y.shape[0], D, flags=XK | XDG) == 1 and torch.equal(*ga)
    # two launches on the same inputs: bit-identical — plain, with near pairs, split
    xn, yn, hn, gn = near_clouds(64, 1e-4)
    xs, ys, hs, gs = _law(np.random.default_rng(3033), 300, 5000, 33)
    for name, (xa, ya, ha, ga_), flags in (("plain", (x, y, h, g), XDG), ("near pairs", (xn, yn, hn, gn), XDG), ("split", (xs, ys, hs, gs), XDG),
                                           ("unsplit", (xs, ys, hs, gs), XDG | NS)):
        xa, ya, ha, ga_ = (_t(a, cuda) for a in (xa, ya, ha, ga_))
        va, Da = ha.abs() / ha.shape[-1], xa.shape[-1]
        for op in OPS:
            s, scale = (ha if op == "softmin_p1" else va), _scale(op, Da)
            assert torch.equal(grad_of(op, xa, ya, s, ga_, scale, flags), grad_of(op, xa, ya, s, ga_, scale, flags)), (name, op)
        for kind in KINDS:
            a = hip.kernel_conv_fwd_grad_raw(hip.KERNEL_KINDS[kind], _b3(xa), _b3(ya), _b2(va, xa), _blur(Da), None, flags)
            b = hip.kernel_conv_fwd_grad_raw(hip.KERNEL_KINDS[kind], _b3(xa), _b3(ya), _b2(va, xa), _blur(Da), None, flags)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (name, kind)


# ---- 8. end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["sinkhorn", "laplacian", "energy"])
def test_end_to_end(cuda, monkeypatch, loss):
    """Online SamplesLoss, N = M = 600, D = 40, with the matrix-core gradients (the module defaults) and with them masked out
    (GEOMLOSS_HIP_XK_GRAD=0, latched at import) against the tensorized backend on float64 CPU copies: loss and dL/dx within 1e-4
    relative — the bar of tests/test_dist_xk_gpu.py::test_end_to_end — and the two gradients within the same bar of each other."""
    D = 40
    rng = np.random.default_rng(8040)
    s = 0.5 + 0.5 * rng.random(D)
    x = (rng.random((600, D)) * s).astype(np.float32)
    y = ((rng.random((600, D)) * 0.5 + 0.4) * s).astype(np.float32)
    kw = dict(sinkhorn=dict(p=1, blur=0.3), laplacian=dict(blur=0.5), energy=dict())[loss]
    op = "softmin_p1" if loss == "sinkhorn" else loss
    x64 = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    L64 = SamplesLoss(loss, backend="tensorized", **kw)(x64, torch.tensor(y, dtype=torch.float64))
    (g64,) = torch.autograd.grad(L64, [x64])
    L64, g64 = float(L64.detach()), g64.numpy()
    seen = []
    bwd, cbwd, cfg = hip.softmin_bwd_x_raw, hip.kernel_conv_bwd_x_raw, hip.kernel_conv_fwd_grad_raw

    def spy(fn, iflags, p1_only=False):
        def wrapped(*a, **k):
            flags = k["flags"] if "flags" in k else a[iflags]
            xa, ya = (a[0], a[1]) if fn is bwd else (a[1], a[2])
            if not (p1_only and a[6] != 1):
                seen.append((xa.shape[0], xa.shape[1], ya.shape[1], xa.shape[2], int(flags)))
            return fn(*a, **k)
        return wrapped
    monkeypatch.setattr(hip, "softmin_bwd_x_raw", spy(bwd, 8, True))
    monkeypatch.setattr(hip, "kernel_conv_bwd_x_raw", spy(cbwd, 7))
    monkeypatch.setattr(hip, "kernel_conv_fwd_grad_raw", spy(cfg, 6))
    fn = SamplesLoss(loss, backend="online", **kw)
    default_on = sinkhorn_samples._XK_DIST_GRAD_P1 if loss == "sinkhorn" else loss in kernel_samples._XK_DIST_GRAD_KINDS
    res = {}
    for on in (True, False):
        monkeypatch.setattr(sinkhorn_samples, "_XK_GRAD", on)
        monkeypatch.setattr(kernel_samples, "_XK_GRAD", on)
        del seen[:]
        xt = _t(x, cuda).requires_grad_(True)
        L = fn(xt, _t(y, cuda))
        (gx,) = torch.autograd.grad(L, [xt])
        res[on] = (float(L.detach()), gx.cpu().numpy())
        assert len(seen) > 0, (on, loss)
        for B, N, M, Dd, flags in seen:      # the predicate said 1 for every gradient launch made with the defaults on, 0 with them off
            assert hip.dist_grad_uses_xk(op, B, N, M, Dd, hip.F32, flags) == int(on and default_on), (on, B, N, M, Dd, flags)
        print(f"{loss} D={D} matrix-core gradient {'on' if on else 'off'}: loss rel. err {abs(res[on][0] - L64) / abs(L64):.2e}, gradient {relerr(res[on][1], g64):.2e}")
        assert abs(res[on][0] - L64) <= 1e-4 * abs(L64), (on, res[on][0], L64)
        assert relerr(res[on][1], g64) <= 1e-4, on
    assert relerr(res[True][1], res[False][1]) <= 1e-4
