"""The column-split launches of the plan family through the C-ABI (geomloss_amd/csrc/glhip_launch_plan.h: ONE pass launcher, pass loop,
sizing rule and merge kernel for ``glhip_plan_apply``, ``glhip_plan_apply_nd``, ``glhip_softmin_bwd_x`` / ``glhip_kernel_conv_bwd_x`` /
``glhip_kernel_conv_fwd_grad`` under ``GLHIP_FLAG_XK_GRAD`` and ``glhip_argmin``), each with three workspaces:

    sized   what the entry point's own sizing call asks for
    none    no workspace: the launch runs unsplit
    three   exactly three splits of the widest pass, 3 B N (nv + 2) 4 bytes (argmin: 3 B N 2 4) — at M = 70001 fewer than the 8 the
            XCD-aware grid needs, so the plain-grid rule runs where the sized workspace takes the XCD-aware one

at (N, M) = (130, 70001) (XCD-aware grid) and (300, 5000) (plain 3-D grid, several splits, two row blocks), D = 8 (the resident-operand
plan kernel), 24 (one pass) and 70 (a pass of 64 and a remainder pass).  Every result is held against float64 with the bound the entry
point's own ``test_column_splits`` states (tests/test_plan_apply_gpu.py, test_plan_apply_nd_gpu.py, test_softmin_grad_xk_gpu.py,
test_gauss_grad_xk_gpu.py, whose helpers are used here); argmin indices are compared exactly, on inputs whose float64 runner-up lies
further from the minimum than the kernel's error bound (tests/test_argmin_gpu.py: tol_of).  Figures are printed before they are asserted."""
import ctypes

import numpy as np
import pytest
import torch

import test_argmin_gpu as ta
import test_gauss_grad_xk_gpu as tg
import test_plan_apply_gpu as tp
import test_softmin_grad_xk_gpu as ts
from conftest import relerr
from geomloss_amd import hip

pytestmark = pytest.mark.gpu

XK = hip.FLAG_XK_GRAD
SHAPES = [(130, 70001), (300, 5000)]
DIMS = [24, 70]
MODES = ("sized", "none", "three")
V = 70          # a pass of 64 features and a remainder pass in every dimension used here (5 <= D <= 11, D > 16: 64 per pass)


def _call(entry, t, ws_mode, flags=0, eps=None, blur=None):
    """One call of `entry` on the (1, ., .) device tensors of `t` with the workspace of `ws_mode` -> dict of device outputs."""
    lib = hip.load_library()
    x, y = t["x"], t["y"]
    (B, N, D), M, dev = x.shape, y.shape[1], x.device
    plan = entry in ("glhip_plan_apply", "glhip_plan_apply_nd")
    width = int(lib.glhip_plan_apply_nd_pass_width(D))      # features (the gradients at D > 16: coordinates) per pass
    if plan:
        V = t["feat"].shape[2]
        sized, nv = int(getattr(lib, entry + "_workspace_bytes")(B, N, M, D, V)), min(V, width)
    elif entry == "glhip_argmin":
        sized, nv = int(lib.glhip_argmin_workspace_bytes(B, N, M, D)), 0
    else:
        sizing = lib.glhip_softmin_bwd_x_workspace_bytes if entry == "glhip_softmin_bwd_x" else lib.glhip_kernel_conv_grad_workspace_bytes
        sized, nv = int(sizing(B, N, M, D, int(flags))), min(D, width)
    nbytes = {"sized": sized, "none": 0, "three": 3 * B * N * (nv + 2) * 4}[ws_mode]
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    tail = (*hip._NO_RANGES, ctypes.c_void_p(ws.data_ptr()) if nbytes else None, nbytes, int(flags), hip._stream(x))
    dt, f32 = hip._dtype_code(x), dict(dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        if plan:
            fwd = hip.softmin_fwd_raw(x, y, t["h"], eps, 2, None, flags)
            res = {"out": torch.empty((B, N, V), **f32), "mass": torch.empty((B, N), **f32)}
            rc = getattr(lib, entry)(x.data_ptr(), y.data_ptr(), t["h"].data_ptr(), fwd.data_ptr(), t["feat"].data_ptr(), res["out"].data_ptr(),
                                     res["mass"].data_ptr(), B, N, M, D, V, float(eps), 2, dt, *tail)
        elif entry == "glhip_softmin_bwd_x":
            fwd = hip.softmin_fwd_raw(x, y, t["h"], eps, 2, None, flags & ~XK)
            res = {"gx": torch.empty((B, N, D), **f32)}
            rc = lib.glhip_softmin_bwd_x(x.data_ptr(), y.data_ptr(), t["h"].data_ptr(), fwd.data_ptr(), t["g"].data_ptr(), res["gx"].data_ptr(),
                                         B, N, M, D, float(eps), 2, dt, *tail)
        elif entry == "glhip_kernel_conv_bwd_x":
            res = {"gx": torch.empty((B, N, D), **f32)}
            rc = lib.glhip_kernel_conv_bwd_x(hip.GAUSSIAN, x.data_ptr(), y.data_ptr(), t["v"].data_ptr(), t["g"].data_ptr(), res["gx"].data_ptr(),
                                             B, N, M, D, float(blur), dt, *tail)
        elif entry == "glhip_kernel_conv_fwd_grad":
            res = {"out": torch.empty((B, N), **f32), "unit": torch.empty((B, N, D), **f32)}
            rc = lib.glhip_kernel_conv_fwd_grad(hip.GAUSSIAN, x.data_ptr(), y.data_ptr(), t["v"].data_ptr(), res["out"].data_ptr(),
                                                res["unit"].data_ptr(), B, N, M, D, float(blur), dt, *tail)
        else:
            res = {"index": torch.empty((B, N), dtype=torch.int32, device=dev), "value": torch.empty((B, N), **f32)}
            rc = lib.glhip_argmin(x.data_ptr(), y.data_ptr(), None, res["index"].data_ptr(), res["value"].data_ptr(), B, N, M, D, 2, dt, *tail)
    assert rc == 0, lib.glhip_last_error()
    return res


def _dev(dev, **arrays):
    return {k: tp._t(a, dev)[None].contiguous() for k, a in arrays.items()}


def _np(res):
    return {k: v[0].cpu().numpy() for k, v in res.items()}


def _plan(dev, entry, N, M, D):
    x, y, h = tp._clouds(D, N, M, D)
    feat = np.random.default_rng(V).standard_normal((M, V)).astype(np.float32)
    eps = 0.05**2 * D
    ref = tp._ref(x, y, h, eps, feat)
    t = _dev(dev, x=x, y=y, h=h, feat=feat)
    for mode in MODES:
        r = _np(_call(entry, t, mode, eps=eps))
        err, merr = tp._worst(r["out"], ref, feat), float(np.abs(r["mass"] - 1.0).max())
        print(f"{entry} N={N} M={M} D={D} V={V} workspace {mode}: vs float64 {err:.2e}, |mass - 1| {merr:.2e}")
        assert err <= 1e-4
        assert merr <= 1e-4


@pytest.mark.parametrize("N,M", SHAPES)
def test_plan_apply(cuda, N, M):
    _plan(cuda, "glhip_plan_apply", N, M, 8)


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("N,M", SHAPES)
def test_plan_apply_nd(cuda, N, M, D):
    _plan(cuda, "glhip_plan_apply_nd", N, M, D)


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("N,M", SHAPES)
def test_softmin_gradient(cuda, N, M, D):
    x, y, h = ts._clouds(D, N, M, D)
    g = np.random.default_rng(D).standard_normal(N).astype(np.float32)
    eps = 0.05**2 * D
    ref = ts._ref(cuda, x, y, h, g, eps)
    t = _dev(cuda, x=x, y=y, h=h, g=g)
    for mode in MODES:
        err = relerr(_np(_call("glhip_softmin_bwd_x", t, mode, XK, eps=eps))["gx"], ref)
        print(f"glhip_softmin_bwd_x N={N} M={M} D={D} workspace {mode}: vs float64 {err:.3e}")
        assert err <= 1e-4


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("N,M", SHAPES)
def test_gaussian_gradient(cuda, N, M, D):
    c = tg._Case(cuda, *tg._clouds(D, N, M, D), tg._blur(D))
    t = _dev(cuda, x=c.x, y=c.y, v=c.v, g=c.g)
    for mode in MODES:
        gx = _np(_call("glhip_kernel_conv_bwd_x", t, mode, XK, blur=c.blur))["gx"]
        fg = _np(_call("glhip_kernel_conv_fwd_grad", t, mode, XK, blur=c.blur))
        tg._check(f"gaussian N={N} M={M} D={D} workspace {mode}", c, (gx, fg["out"], fg["unit"]))


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("N,M", SHAPES)
def test_argmin(cuda, N, M, D):
    rng = np.random.default_rng(300 + D)
    x, y = rng.random((N, D)).astype(np.float32), rng.random((M, D)).astype(np.float32)
    C = ta.cost64(x, y)
    two = np.partition(C, 1, axis=1)[:, :2]
    gap, tol = float((two[:, 1] - two[:, 0]).min()), ta.tol_of(D, 0.0)
    print(f"glhip_argmin N={N} M={M} D={D}: smallest gap to the runner-up {gap:.3e}, tol {tol:.3e}")
    assert gap > tol, "the inputs were meant to have no ties within the kernel's error"
    t = _dev(cuda, x=x, y=y)
    for mode in MODES:
        r = _np(_call("glhip_argmin", t, mode))
        wrong = int((r["index"] != C.argmin(1)).sum())
        verr = float(np.abs(r["value"].astype(np.float64) - C.min(1)).max())
        print(f"glhip_argmin N={N} M={M} D={D} workspace {mode}: {wrong} of {N} rows off the float64 argmin, value error {verr:.3e}")
        assert wrong == 0
        assert verr <= tol
