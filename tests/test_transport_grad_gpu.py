"""Autograd through ``geomloss_amd.transport`` (p = 2) on the GPU: the gradients of ``apply_plan`` (plain and transposed) and of
``barycentric_map`` against dense float64 autograd, for potentials that come from the solver.

Bound, per gradient: ``max(2e-5, 4 x e32)`` on ``relerr`` (conftest), e32 being the ``relerr`` of the same gradient from dense float32
torch autograd on the same inputs — the rule of tests/test_plan_bilinear_gpu.py.  Every figure is printed (``pytest -s``)."""
import numpy as np
import pytest
import torch

from cloud_support import to_dev
from conftest import relerr
from geomloss_amd import SamplesLoss, apply_plan, barycentric_map
from transport_grad_support import clouds, dense_apply_plan, dense_barycentric_map

pytestmark = pytest.mark.gpu

N, M, V = 300, 257, 7


def _blur(D):
    return 0.1 * (D / 3) ** 0.5


def _bound(e32):
    return max(2e-5, 4 * e32)


def _setup(cuda, D, B=None, offset=0.0, seed=0):
    """Clouds, weights, potentials of the solver (detached) and features, float32 on the device."""
    x, y, _ = clouds(seed, N, M, D, B, offset)
    rng = np.random.default_rng(seed + 50)
    lead = () if B is None else (B,)
    a, b = rng.random(lead + (N,)).astype(np.float32) + 0.1, rng.random(lead + (M,)).astype(np.float32) + 0.1
    a, b = a / a.sum(-1, keepdims=True), b / b.sum(-1, keepdims=True)
    x, y, a, b = (to_dev(t, cuda) for t in (x, y, a, b))
    solver = SamplesLoss("sinkhorn", p=2, blur=_blur(D), potentials=True, debias=False)
    if B is None:
        F, G = solver(a, x, b, y)
    else:
        F, G = (torch.stack(t) for t in zip(*(solver(a[k], x[k], b[k], y[k]) for k in range(B))))
    F, G = F.detach().reshape(lead + (N,)), G.detach().reshape(lead + (M,))
    feat = to_dev(rng.standard_normal(lead + (M, V)).astype(np.float32), cuda)
    featT = to_dev(rng.standard_normal(lead + (N, V)).astype(np.float32), cuda)
    return x, y, F, G, feat, featT, a, b


def _leaves(ts, dtype=None):
    return [t.detach().clone().to(dtype or t.dtype).requires_grad_(True) for t in ts]


def _compare(label, names, got_fn, dense_fn, inputs, seed=9):
    """Gradients of got_fn(*leaves) against dense_fn(*float64 leaves); e32 from dense_fn(*float32 leaves).  Returns the output."""
    got = _leaves(inputs)
    out = got_fn(*got)
    assert out.grad_fn is not None and out.dtype == torch.float32
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed)).to(out.device)
    g_got = torch.autograd.grad(out, got, cot)
    want = _leaves([t.float() for t in inputs], torch.float64)
    g_want = torch.autograd.grad(dense_fn(*want), want, cot.double())
    plain = _leaves([t.float() for t in inputs])
    g_plain = torch.autograd.grad(dense_fn(*plain), plain, cot)
    for name, gg, gw, gp, leaf in zip(names, g_got, g_want, g_plain, got):
        assert gg.dtype == leaf.dtype and gg.shape == leaf.shape and torch.isfinite(gg).all()
        gw = gw.cpu().numpy()
        if leaf.dtype == torch.bfloat16:      # a bf16 gradient: within 2^-7 of its largest entry
            err = float(np.abs(gg.float().cpu().numpy() - gw).max() / np.abs(gw).max())
            print(f"{label} d{name} (bf16): {err:.2e} (bound {2.0**-7:.2e})")
            assert err <= 2.0**-7, (label, name, err)
            continue
        err, e32 = relerr(gg.cpu().numpy(), gw), relerr(gp.cpu().numpy(), gw)
        print(f"{label} d{name}: {err:.2e} (e32 {e32:.2e})")
        assert err <= _bound(e32), (label, name, err, e32)
    return out.detach()


def _all_three(cuda, label, D, B=None, offset=0.0, cloud_dtype=None):
    x, y, F, G, feat, featT, a, b = _setup(cuda, D, B, offset)
    if cloud_dtype is not None:
        x, y = x.to(cloud_dtype), y.to(cloud_dtype)
    blur, eps = _blur(D), _blur(D) ** 2
    a64 = lambda t, like: t.to(like.dtype)  # noqa: E731
    out = _compare(f"{label} apply_plan", "x y F G feat".split(),
                   lambda x_, y_, F_, G_, f_: apply_plan(x_, y_, F_, G_, f_, blur, a=a, b=b),
                   lambda x_, y_, F_, G_, f_: dense_apply_plan(x_, y_, F_, G_, f_, eps, a64(a, x_), a64(b, x_)), (x, y, F, G, feat))
    assert torch.equal(out, apply_plan(x, y, F, G, feat, blur, a=a, b=b))             # the forward value of the no-grad call, bit for bit
    _compare(f"{label} apply_plan^T", "x y F G feat".split(),
             lambda x_, y_, F_, G_, f_: apply_plan(x_, y_, F_, G_, f_, blur, a=a, b=b, transpose=True),
             lambda x_, y_, F_, G_, f_: dense_apply_plan(x_, y_, F_, G_, f_, eps, a64(a, x_), a64(b, x_), transpose=True), (x, y, F, G, featT))
    T = _compare(f"{label} barycentric_map", "x y G".split(),
                 lambda x_, y_, G_: barycentric_map(x_, y_, F, G_, blur, b=b),
                 lambda x_, y_, G_: dense_barycentric_map(x_, y_, G_, eps, a64(b, x_)), (x, y, G))
    assert torch.equal(T, barycentric_map(x, y, F, G, blur, b=b))


@pytest.mark.parametrize("D", (3, 24, 100))
def test_gradients(cuda, D):
    _all_three(cuda, f"D={D}", D)


def test_gradients_batched(cuda):
    _all_three(cuda, "B=2 D=24", 24, B=2)


def test_gradients_offset_clouds(cuda):
    _all_three(cuda, "offset 10 D=24", 24, offset=10.0)


def test_gradients_bf16_clouds(cuda):
    _all_three(cuda, "bf16 D=24", 24, cloud_dtype=torch.bfloat16)


def test_grad_fn_exactly_when_requested(cuda):
    x, y, F, G, feat, _, a, b = _setup(cuda, 3)
    blur = _blur(3)
    assert apply_plan(x, y, F, G, feat, blur, a=a, b=b).grad_fn is None
    assert barycentric_map(x, y, F, G, blur, b=b).grad_fn is None
    for k in range(5):
        args = [x, y, F, G, feat]
        args[k] = args[k].clone().requires_grad_(True)
        assert apply_plan(*args, blur, a=a, b=b).grad_fn is not None
        with torch.no_grad():
            assert apply_plan(*args, blur, a=a, b=b).grad_fn is None
    for k in (0, 1, 3):
        args = [x, y, F, G]
        args[k] = args[k].clone().requires_grad_(True)
        assert barycentric_map(*args, blur, b=b).grad_fn is not None
    xg = x.clone().requires_grad_(True)
    assert apply_plan(xg, y, F, G, feat, _blur(3), p=1).grad_fn is None                  # p = 1 stays as it is
    # the loss users write: it fills x.grad and y.grad
    yg = y.clone().requires_grad_(True)
    (barycentric_map(xg, yg, F, G, blur) - 0.5).pow(2).sum().backward()
    assert torch.isfinite(xg.grad).all() and torch.isfinite(yg.grad).all() and xg.grad.abs().max() > 0 and yg.grad.abs().max() > 0
