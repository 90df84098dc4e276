"""Host side of the matrix-core distance gradients of 17 <= D <= 4095 (GLHIP_FLAG_XK_DIST_GRAD, geomloss_amd/csrc/glhip_dist_grad_xk.h):
the predicate, the existing predicates under the new bit, the workspace sizing, the flags the Python layers set, and the teeth of the
near-pair case of tests/test_dist_grad_xk_gpu.py.  No device."""
import numpy as np
import pytest
import torch

from conftest import relerr
from geomloss_amd import hip, kernel_samples, sinkhorn_samples
from oracle import oracle_torch64 as o64

XDG, NS = hip.FLAG_XK_DIST_GRAD, hip.FLAG_NO_SPLIT
OPS = ("softmin_p1", "laplacian", "energy")
CPU = torch.device("cpu")


@pytest.fixture(scope="module", autouse=True)
def _library():
    assert hip.library_available(), "libgeomloss_hip.so is not built (python -c 'import __graft_entry__ as g; g.build()')"
    assert hip.load_library().glhip_version() >= 132


def test_flag_value():
    assert XDG == 4096 and XDG & (hip.FLAG_XK_GRAD | hip.FLAG_XK_DIST | hip.FLAG_F16X2 | hip.FLAG_NO_SORT) == 0


@pytest.mark.parametrize("op", OPS)
def test_predicate(op):
    for dtype in (hip.F32, hip.BF16):
        for D in (17, 31, 32, 33, 64, 130, 1024, 4095):
            for B, N, M in ((1, 70, 150), (2, 33, 40), (65535, 1, 1), (1, 1, 1), (1, 100000, 100000), (1, 5, 0)):
                assert hip.dist_grad_uses_xk(op, B, N, M, D, dtype, XDG) == 1, (op, B, N, M, D)
                assert hip.dist_grad_uses_xk(op, B, N, M, D, dtype, XDG | NS | hip.FLAG_F16X2 | hip.FLAG_XK_GRAD | hip.FLAG_XK_DIST) == 1
                assert hip.dist_grad_uses_xk(op, B, N, M, D, dtype, 0) == 0
                assert hip.dist_grad_uses_xk(op, B, N, M, D, dtype, hip.FLAG_XK_GRAD | hip.FLAG_XK_DIST) == 0
                assert hip.dist_grad_uses_xk(op, B, N, M, D, dtype, XDG | hip.FLAG_NO_MFMA) == 0
                assert hip.dist_grad_uses_xk(op, B, N, M, D, dtype, XDG | hip.FLAG_DIRECT) == 0
                assert hip.dist_grad_uses_xk(op, B, N, M, D, dtype, XDG, n_ranges=3) == 0
        for D in (1, 3, 16, 4096, 10000):
            assert hip.dist_grad_uses_xk(op, 1, 70, 150, D, dtype, XDG) == 0, (op, D)
        assert hip.dist_grad_uses_xk(op, 65536, 70, 150, 64, dtype, XDG) == 0
    for bad in (dict(B=-1), dict(N=-1), dict(M=-1), dict(N=2**31), dict(M=2**31), dict(D=0), dict(dtype=2), dict(n_ranges=-1)):
        kw = dict(B=1, N=70, M=150, D=64, dtype=hip.F32, flags=XDG, n_ranges=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            hip.dist_grad_uses_xk(op, **kw)


def test_predicate_rejects_a_bad_op():
    for op in (-1, 3):
        with pytest.raises(ValueError):
            hip.dist_grad_uses_xk(op, 1, 70, 150, 64, hip.F32, XDG)
    assert hip.DIST_GRAD_OPS == {"softmin_p1": 0, "laplacian": hip.LAPLACIAN, "energy": hip.ENERGY}


def test_existing_predicates_do_not_see_the_new_bit():
    for D in (3, 16, 17, 64, 4095, 4096):
        for B, N, M in ((1, 70, 150), (2, 33, 40)):
            for base in (0, hip.FLAG_XK_GRAD, hip.FLAG_XK_GRAD | hip.FLAG_F16X2, hip.FLAG_NO_MFMA):
                for p in (1, 2):
                    assert hip.softmin_bwd_x_uses_plan(B, N, M, D, p=p, flags=base | XDG) == hip.softmin_bwd_x_uses_plan(B, N, M, D, p=p, flags=base)
                    assert hip.softmin_fwd_family(B, N, M, D, p, hip.F32, base | XDG) == hip.softmin_fwd_family(B, N, M, D, p, hip.F32, base)
                for kind in ("gaussian", "laplacian", "energy"):
                    assert hip.kernel_conv_grad_uses_xk(kind, B, N, M, D, flags=base | XDG) == hip.kernel_conv_grad_uses_xk(kind, B, N, M, D, flags=base)
                    assert hip.kernel_conv_fwd_family(kind, B, N, M, D, hip.F32, base | XDG) == hip.kernel_conv_fwd_family(kind, B, N, M, D, hip.F32, base)
            assert hip.softmin_bwd_x_uses_plan(B, N, M, D, p=1, flags=XDG | hip.FLAG_XK_GRAD) == 0
            for kind in ("laplacian", "energy"):
                assert hip.kernel_conv_grad_uses_xk(kind, B, N, M, D, flags=XDG | hip.FLAG_XK_GRAD) == 0


def test_workspace():
    """The sizing call is plan_pass_workspace_bytes (glhip_split_policy.h) at the shipped pass width: glhip_plan_apply_nd_workspace_bytes
    is that function of the same 256-row blocks with V features per pass for V <= 64."""
    lib = hip.load_library()
    width = int(lib.glhip_dist_grad_pass_width())
    assert width in (32, 64)
    for N, M, D, split in ((130, 70001, 24, True), (300, 5000, 33, True), (130, 70001, 130, True), (300, 5000, 4095, True), (70, 150, 64, False)):
        for B in (1, 2):
            got = int(lib.glhip_dist_grad_workspace_bytes(B, N, M, D, XDG))
            assert got == int(lib.glhip_plan_apply_nd_workspace_bytes(B, N, M, D, min(D, width))), (B, N, M, D)
            assert (got > 0) == split, (B, N, M, D, got)
            assert got % (B * N * (min(D, width) + 2) * 4) == 0
            assert int(lib.glhip_dist_grad_workspace_bytes(B, N, M, D, XDG | NS)) == 0
            assert int(lib.glhip_dist_grad_workspace_bytes(B, N, M, D, 0)) == 0
            assert int(lib.glhip_dist_grad_workspace_bytes(B, N, M, D, XDG | hip.FLAG_NO_MFMA)) == 0
    assert int(lib.glhip_dist_grad_workspace_bytes(1, 130, 70001, 16, XDG)) == 0
    assert int(lib.glhip_dist_grad_workspace_bytes(0, 130, 70001, 24, XDG)) == 0


def test_python_flags(monkeypatch):
    lo, hi = torch.zeros(4, 16), torch.zeros(4, 17)
    assert kernel_samples._XK_GRAD is True and sinkhorn_samples._XK_GRAD is True      # the default
    for name in ("laplacian", "energy"):
        assert kernel_samples._grad_flags(name, hi) == (XDG if name in kernel_samples._XK_DIST_GRAD_KINDS else 0)
        assert kernel_samples._grad_flags(name, lo) == 0
        assert kernel_samples._fwd_flags(name, hi) & XDG == 0
    assert kernel_samples._grad_flags("gaussian", hi) == hip.FLAG_XK_GRAD and kernel_samples._grad_flags("gaussian", lo) == 0
    p1, p2 = sinkhorn_samples._HipSoftmin(1, False), sinkhorn_samples._HipSoftmin(2, False)
    assert bool(p1._flags(0.3) & XDG) == sinkhorn_samples._XK_DIST_GRAD_P1 and p2._flags(0.3) & XDG == 0
    assert p2._flags(0.3) & hip.FLAG_XK_GRAD and not p1._flags(0.3) & hip.FLAG_XK_GRAD
    monkeypatch.setattr(kernel_samples, "_XK_GRAD", False)      # GEOMLOSS_HIP_XK_GRAD=0
    monkeypatch.setattr(sinkhorn_samples, "_XK_GRAD", False)
    assert all(kernel_samples._grad_flags(name, hi) == 0 for name in ("gaussian", "laplacian", "energy"))
    assert p1._flags(0.3) & (XDG | hip.FLAG_XK_GRAD) == 0 and p2._flags(0.3) & (XDG | hip.FLAG_XK_GRAD) == 0


# ---- teeth of the near-pair case ---------------------------------------------------------------------------------------------------
NEAR_EPS = 0.3
NEAR_S = (3e-5, 1e-4, 1e-3)


def near_clouds(D, s, shift=0.0):
    """The clouds of tests/test_dist_grad_xk_gpu.py::test_near_pairs, case (b) / (c): the sweep's input law, y = x + s noise."""
    rng = np.random.default_rng(1000 + D)
    sc = 0.5 + 0.5 * rng.random(D)
    x = (rng.random((300, D)) * sc).astype(np.float32)
    h = rng.standard_normal(300).astype(np.float32)
    g = rng.standard_normal(300).astype(np.float32)
    y = (x + s * rng.standard_normal((300, D))).astype(np.float32)
    return (x + np.float32(shift)).astype(np.float32), (y + np.float32(shift)).astype(np.float32), h, g


def _emulated_softmin_grad(x, y, h, g, eps):
    """g_i (xs_i W_i - S_i) / Z_i with float64 weights rounded to float32, float32 coordinates centred on the first row of each block of
    256 rows, and float32 sums — every pair through the difference, none repaired."""
    t = np.float32(1.0 / eps)
    out = np.empty_like(x)
    for r0 in range(0, x.shape[0], 256):
        c = x[r0]
        xs, ys = (x[r0:r0 + 256] - c) * t, (y - c) * t
        d = np.sqrt(np.maximum(((x[r0:r0 + 256, None, :].astype(np.float64) - y[None, :, :].astype(np.float64)) ** 2).sum(-1), 1e-8))
        e = np.exp(h[None, :].astype(np.float64) - d / eps)
        w = np.where(d * d > 1e-8, e / (d / eps), 0.0).astype(np.float32)
        W = w.sum(1, dtype=np.float32)
        S = w @ ys
        out[r0:r0 + 256] = g[r0:r0 + 256, None] * (xs * W[:, None] - S) / e.sum(1).astype(np.float32)[:, None]
    return out


@pytest.mark.parametrize("D", [17, 64, 130])
def test_near_pairs_have_teeth(D):
    """xs W - S in float32 WITHOUT the exact near-pair path, against the float64 gradient of the p = 1 soft-min at eps = 0.3 and the bound
    5e-6 of the GPU test: it misses by 1290 / 251 / 24 x the bound at s = 3e-5 / 1e-4 / 1e-3 for D = 17, 3110 / 954 / 58 for
    D = 64 and 2230 / 1380 / 103 for D = 130 (printed with ``pytest -s``) — at least 10 x for at least one s in every dimension, so
    the near-pair case of the GPU file fails when the exact contributions are dropped or land in the wrong row, column or feature."""
    worst = []
    for s in NEAR_S:
        x, y, h, g = near_clouds(D, s)
        ref = o64.softmin_grad_x(NEAR_EPS, x, y, h, g, 1, device=CPU)
        worst.append(relerr(_emulated_softmin_grad(x, y, h, g, NEAR_EPS), ref) / 5e-6)
    print(f"near pairs D={D}: float32 xs W - S misses the bound by {', '.join(f'{w:.3g}' for w in worst)} x at s = {NEAR_S}")
    assert max(worst) >= 10.0, worst
