"""``glhip_softmin_bwd_x`` under ``GLHIP_FLAG_XK_GRAD``: the p = 2 soft-min gradient of 17 <= D <= 4095 on the matrix cores
(geomloss_amd/csrc/glhip_softmin_grad_xk.h) against ``oracle_torch64.softmin_grad_x`` in float64 on the same float32 (or bf16-rounded)
inputs.  Errors are ``relerr``: relative to the largest entry of the reference.

Bound: the project's rule for this gradient (tests/test_anyd_kernels_gpu.py) — 5e-6, and for D > 64 max(5e-6, 4 e_ref) with e_ref the
error of the same gradient in plain float32 torch on the expanded cost |x|^2 - 2 x.y + |y|^2 with a softmax (the arithmetic of
``_torch_f32_error`` in tests/test_plan_apply_nd_gpu.py), computed here.  ``_clouds`` is cloud_support.clouds, ``_eps`` restates
tests/test_plan_apply_nd_gpu.py.  Every figure is printed before it is asserted."""
import math

import numpy as np
import pytest
import torch

from cloud_support import clouds as _clouds, to_dev as _t
from conftest import relerr
from geomloss_amd import SamplesLoss, hip
from geomloss_amd import sinkhorn_samples
from geomloss_amd.cluster import from_matrix
from oracle import oracle_torch64 as o64

pytestmark = pytest.mark.gpu

XK = hip.FLAG_XK_GRAD
FLAGS = [XK, XK | hip.FLAG_NO_SPLIT, XK | hip.FLAG_F16X2, XK | hip.FLAG_F16X2 | hip.FLAG_NO_SPLIT]


def _eps(D):
    return 0.1 * D / 3


def _ref(dev, x, y, h, g, eps):
    """float64 reference, batched or not."""
    if x.ndim == 2:
        return o64.softmin_grad_x(eps, x, y, h, g, 2, device=dev)
    return np.stack([o64.softmin_grad_x(eps, x[b], y[b], h[b], g[b], 2, device=dev) for b in range(x.shape[0])])


def _grad(dev, x, y, h, g, eps, flags, **kw):
    """Raw forward + gradient launches on (N,D) / (B,N,D) NumPy (or torch) inputs -> grad_x as NumPy."""
    xb, yb, hb, gb = (t if torch.is_tensor(t) else _t(t, dev) for t in (x, y, h, g))
    batched = xb.dim() == 3
    if not batched:
        xb, yb, hb, gb = xb[None], yb[None], hb[None], gb[None]
    fwd = hip.softmin_fwd_raw(xb, yb, hb, eps, 2, None, flags & ~XK)
    gx = hip.softmin_bwd_x_raw(xb, yb, hb, fwd, gb, eps, 2, None, flags, **kw).cpu().numpy()
    return gx if batched else gx[0]


def _f32_error(dev, x, y, h, g, eps, ref):
    """The error of the same gradient in plain float32 torch: expanded cost, softmax, one matrix product."""
    if x.ndim == 3:
        return max(_f32_error(dev, x[b], y[b], h[b], g[b], eps, ref[b]) for b in range(x.shape[0]))
    xt, yt, ht, gt = (_t(a, dev) for a in (x, y, h, g))
    C = (xt * xt).sum(1)[:, None] - 2.0 * xt @ yt.t() + (yt * yt).sum(1)[None, :]
    out = gt[:, None] * (xt - torch.softmax(ht[None, :] - C / (2.0 * eps), dim=1) @ yt)
    return relerr(out.cpu().numpy(), ref)


def _bound(D, e_ref):
    return max(5e-6, 4.0 * e_ref) if D > 64 else 5e-6


# (270, 310, 17): the first dimension            (257, 300, 65): a one-coordinate second pass, a one-row second row block
# (130, 600, 128): two full passes               (130, 600, 300): a long chain, five passes with a remainder
SHAPES = [(270, 310, 17), (300, 257, 31), (97, 513, 32), (257, 300, 65), (130, 600, 128), (64, 8, 64), (1, 1, 100), (130, 600, 300)]
_CASES = {}


def _parity_case(dev, N, M, D):      # inputs, the float64 reference and e_ref, computed once for the four flag settings
    key = (N, M, D)
    if key not in _CASES:
        x, y, h = _clouds(N + M + D, N, M, D)
        g = np.random.default_rng(D).standard_normal(N).astype(np.float32)
        ref = _ref(dev, x, y, h, g, _eps(D))
        _CASES[key] = (x, y, h, g, ref, _f32_error(dev, x, y, h, g, _eps(D), ref))
    return _CASES[key]


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("N,M,D", SHAPES)
def test_parity(cuda, N, M, D, flags):
    x, y, h, g, ref, e_ref = _parity_case(cuda, N, M, D)
    assert hip.softmin_bwd_x_uses_plan(1, N, M, D, flags=flags) == 1
    gx = _grad(cuda, x, y, h, g, _eps(D), flags)
    err, bound = relerr(gx, ref), _bound(D, e_ref)
    print(f"parity N={N} M={M} D={D} flags={flags}: relerr {err:.3e}   float32 torch e_ref {e_ref:.3e}   bound {bound:.3e}")
    assert gx.shape == (N, D) and np.isfinite(gx).all()
    assert err <= bound


@pytest.mark.parametrize("B", [None, 3])
@pytest.mark.parametrize("D", [65, 100, 128, 300])
def test_open_measurement(cuda, D, B):
    """The inputs of tests/test_anyd_kernels_gpu.py::test_softmin_gradient_any_dimension (eps = 0.3): both routes and plain float32
    torch against float64.  Measured on an MI355X (flag on / flag off / e_ref; profiles/softmin_grad_xk.txt): D = 65: 4.6e-7 / 7.1e-7 /
    2.2e-6, 100: 8.1e-7 / 1.3e-6 / 4.0e-6, 128: 1.1e-6 / 1.2e-6 / 7.2e-6, 300: 7.1e-6 / 4.7e-6 / 2.3e-5 unbatched; batched 5.6e-7 / 8.6e-7 /
    2.8e-6, 7.9e-7 / 2.1e-6 / 5.5e-6, 2.2e-6 / 2.0e-6 / 1.1e-5, 6.4e-6 / 5.9e-6 / 3.6e-5.  At D = 300 the new route is above the flat 5e-6:
    the flag stays opt-in for raw calls."""
    N, M, eps = 270, 310, 0.3
    x, y, h = _clouds(51 + D, N, M, D, B=B)
    g = np.random.default_rng(6).standard_normal(x.shape[:-1]).astype(np.float32)
    ref = _ref(cuda, x, y, h, g, eps)
    e_new = relerr(_grad(cuda, x, y, h, g, eps, XK), ref)
    e_old = relerr(_grad(cuda, x, y, h, g, eps, 0), ref)
    e_ref = _f32_error(cuda, x, y, h, g, eps, ref)
    bound = max(5e-6, 4.0 * e_ref)
    print(f"open measurement D={D} B={B}: flag on {e_new:.3e}   flag off {e_old:.3e}   float32 torch e_ref {e_ref:.3e}   bound {bound:.3e}")
    assert e_new <= bound


@pytest.mark.parametrize("D", [40, 100])
def test_exactness_and_operand_order(cuda, D, flags=XK):
    """One-hot plan rows on grid points: x_i - y_perm(i) = e_i with every operation exact in float32.  A wrong K permutation or
    register-to-coordinate map gives another difference, and the position of the first one names the lane.  D = 100: a second pass.
    (bf16 x 3 exponents only: at eps = 1e-4 the exponents are outside the range contract of GLHIP_FLAG_F16X2.)"""
    n = 96
    rng = np.random.default_rng(5)
    y = (rng.integers(0, 1024, (n, D)) / 1024.0).astype(np.float32)
    perm = rng.permutation(n)
    i, d = np.arange(n)[:, None], np.arange(D)[None, :]
    e = (((i + d) % 7 - 3) / 4096.0).astype(np.float32)
    x = y[perm] + e
    assert np.array_equal((x.astype(np.float64) - y[perm]).astype(np.float32), e)      # the construction is exact
    gx = _grad(cuda, x, y, np.zeros(n, np.float32), np.ones(n, np.float32), 1e-4, flags)
    bad = np.argwhere(gx != e)
    print(f"exactness D={D} flags={flags}: {len(bad)} of {gx.size} entries differ, max |grad_x - e| {np.abs(gx - e).max():.3e}")
    assert len(bad) == 0, f"first wrong (row, coordinate) {bad[0]}: got {gx[tuple(bad[0])]!r}, want {e[tuple(bad[0])]!r}"


@pytest.mark.parametrize("flags", [XK, XK | hip.FLAG_F16X2])
def test_clouds_offset_by_1000(cuda, flags):
    """Both clouds far from the origin: the in-kernel centring keeps x_i - ybar_i free of cancellation."""
    N, M, D = 270, 310, 24
    x, y, h = _clouds(7, N, M, D, offset=1000.0)
    assert x.dtype == np.float32 and x.min() >= 1000.0
    g = np.random.default_rng(8).standard_normal(N).astype(np.float32)
    ref = _ref(cuda, x, y, h, g, _eps(D))
    err = relerr(_grad(cuda, x, y, h, g, _eps(D), flags), ref)
    print(f"offset 1000, D={D} flags={flags}: relerr {err:.3e}")
    assert err <= 5e-6


def test_batched_bf16(cuda):
    B, N, M, D = 3, 200, 260, 48
    x, y, h = _clouds(11, N, M, D, B=B)
    g = np.random.default_rng(12).standard_normal((B, N)).astype(np.float32)
    xt, yt = _t(x, cuda).bfloat16(), _t(y, cuda).bfloat16()
    x, y = xt.float().cpu().numpy(), yt.float().cpu().numpy()      # the reference sees the bf16-rounded points
    assert hip.softmin_bwd_x_uses_plan(B, N, M, D, dtype=hip.BF16, flags=XK) == 1
    gx = _grad(cuda, xt, yt, h, g, _eps(D), XK)
    err = relerr(gx, _ref(cuda, x, y, h, g, _eps(D)))
    print(f"batched bf16: relerr {err:.3e}")
    assert gx.shape == (B, N, D) and gx.dtype == np.float32
    assert err <= 5e-6


def test_column_splits(cuda):
    N, M, D = 130, 70001, 72
    lib = hip.load_library()
    nbytes = int(lib.glhip_softmin_bwd_x_workspace_bytes(1, N, M, D, XK))
    print(f"splits: workspace {nbytes} bytes = {nbytes // (N * 66 * 4)} splits of the 64-coordinate pass")
    assert nbytes > 0
    x, y, h = _clouds(D, N, M, D)
    g = np.random.default_rng(D).standard_normal(N).astype(np.float32)
    eps = 0.05**2 * D
    ref = _ref(cuda, x, y, h, g, eps)
    split = _grad(cuda, x, y, h, g, eps, XK)
    unsplit = _grad(cuda, x, y, h, g, eps, XK | hip.FLAG_NO_SPLIT)
    nows = _grad(cuda, x, y, h, g, eps, XK, workspace=False)
    errs = [relerr(o, ref) for o in (split, unsplit, nows)]
    scale = np.abs(ref).max()
    among = [float(np.abs(a - b).max() / scale) for a, b in ((split, unsplit), (split, nows), (unsplit, nows))]
    print(f"splits N={N} M={M} D={D}: vs float64 {errs}, among the runs {among}")
    assert max(errs) <= 1e-4
    assert max(among) <= 2e-5


@pytest.mark.parametrize("flags", [XK, XK | hip.FLAG_F16X2])
def test_massless_columns_and_rows(cuda, flags):
    B, N, M, D = 2, 257, 300, 24
    x, y, h = _clouds(21, N, M, D, B=B)
    g = np.random.default_rng(22).standard_normal((B, N)).astype(np.float32)
    h[0, ::3] = -np.inf                      # a third of the columns carry no mass ...
    y[0, ::3] = 1e4                          # ... whatever (huge, finite) coordinates they hold
    h[1, :] = -np.inf                        # a batch item without any mass
    gx = _grad(cuda, x, y, h, g, _eps(D), flags)
    keep = np.isfinite(h[0])
    ref = _ref(cuda, x[0], y[0][keep], h[0][keep], g[0], _eps(D))
    err = relerr(gx[0], ref)
    print(f"massless columns, flags={flags}: relerr {err:.3e}")
    assert np.isfinite(gx).all()
    assert err <= 5e-6
    assert (gx[1] == 0.0).all()


def test_flag_is_ignored_where_it_does_not_apply(cuda):
    """D <= 16, p = 1 and block-sparse launches are the launches of the flag-less call, bit for bit."""
    def pair(D, p, ranges=None, N=270, M=310):
        x, y, h = (_t(a, cuda)[None] for a in _clouds(D + p, N, M, D))
        g = _t(np.random.default_rng(3).standard_normal(N).astype(np.float32), cuda)[None]
        eps = _eps(D) if p == 2 else 0.3 * math.sqrt(D / 3)
        fwd = hip.softmin_fwd_raw(x, y, h, eps, p, ranges, 0)
        return [hip.softmin_bwd_x_raw(x, y, h, fwd, g, eps, p, ranges, fl) for fl in (0, XK)]

    for D, p in ((16, 2), (40, 1)):
        a, b = pair(D, p)
        assert hip.softmin_bwd_x_uses_plan(1, 270, 310, D, p=p, flags=XK) == 0
        assert torch.equal(a, b), (D, p)
    ri = torch.tensor([[0, 100], [100, 270]], dtype=torch.int32, device=cuda)
    rj = torch.tensor([[0, 150], [150, 310]], dtype=torch.int32, device=cuda)
    keep = torch.tensor([[True, True], [False, True]], device=cuda)
    a, b = pair(40, 2, ranges=from_matrix(ri, rj, keep))
    assert hip.softmin_bwd_x_uses_plan(1, 270, 310, 40, flags=XK, n_ranges=2) == 0
    assert torch.equal(a, b) and torch.isfinite(a).all()


def test_end_to_end_samples_loss(cuda, monkeypatch):
    """The online SamplesLoss backward at D = 32 takes the new kernel by default; GEOMLOSS_HIP_XK_GRAD=0 (latched at import:
    ``sinkhorn_samples._XK_GRAD``) keeps the one-thread-per-row kernel."""
    N = M = 500
    D = 32
    x, y, _ = _clouds(32, N, M, D)
    loss_fn = SamplesLoss("sinkhorn", p=2, blur=0.3 * math.sqrt(D / 3), backend="online")

    def run(on):
        monkeypatch.setattr(sinkhorn_samples, "_XK_GRAD", on)
        xt = _t(x, cuda).requires_grad_(True)
        loss = loss_fn(xt, _t(y, cuda))
        (gx,) = torch.autograd.grad(loss, [xt])
        return float(loss), gx.cpu().numpy()

    assert sinkhorn_samples._XK_GRAD is True      # the default
    soft = sinkhorn_samples._HipSoftmin(2, False)
    assert soft._flags(1.0) & XK and hip.softmin_bwd_x_uses_plan(1, N, M, D, flags=soft._flags(1.0)) == 1
    l_on, g_on = run(True)
    l_off, g_off = run(False)
    assert not (soft._flags(1.0) & XK)
    err = float(np.abs(g_on - g_off).max() / np.abs(g_off).max())
    print(f"end to end D={D}: loss {l_on!r} / {l_off!r}, gradients differ by {err:.3e} of the max-norm")
    assert l_on == l_off
    assert np.abs(g_off).max() > 0 and err <= 1e-4


def test_second_order(cuda):
    """create_graph=True through hip.softmin with the flag at D = 20: ``_plan_moments`` runs the new kernel on its augmented clouds
    (D + 8 = 28).  Against float64 dense autograd at the project's 2e-4."""
    N, M, D = 60, 70, 20
    eps = _eps(D)
    x, y, h = _clouds(20, N, M, D)
    rng = np.random.default_rng(21)
    g, V = rng.standard_normal(N).astype(np.float32), rng.standard_normal((N, D)).astype(np.float32)

    def second(xt, yt, ht, gt, Vt, soft):
        out = soft(xt, yt, ht)
        (gx,) = torch.autograd.grad(out, [xt], grad_outputs=gt, create_graph=True)
        (hv,) = torch.autograd.grad((gx * Vt).sum(), [xt])
        return gx.detach(), hv

    dense = lambda xt, yt, ht: -eps * torch.logsumexp(ht[None, :] - ((xt[:, None, :] - yt[None, :, :]) ** 2).sum(-1) / (2 * eps), dim=1)  # noqa: E731
    g64, hv64 = second(*(torch.from_numpy(a).double().requires_grad_(k == 0) for k, a in enumerate((x, y, h, g, V))), dense)
    args = [_t(a, cuda) for a in (x, y, h, g, V)]
    args[0].requires_grad_(True)
    g32, hv32 = second(*args, lambda xt, yt, ht: hip.softmin(eps, xt, yt, ht, flags=XK))
    e1, e2 = relerr(g32.cpu().numpy(), g64.numpy()), relerr(hv32.cpu().numpy(), hv64.numpy())
    print(f"second order D={D}: gradient {e1:.3e}, Hessian-vector product {e2:.3e}")
    assert e1 <= 5e-6 and e2 <= 2e-4
