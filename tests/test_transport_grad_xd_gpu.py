"""Autograd through ``geomloss_amd.transport`` with ``resident=True`` (the resident-operand bilinear kernel, glhip_plan_bilinear_xd.h): the
gradients of ``apply_plan`` (plain and transposed) and of ``barycentric_map`` against dense float64 autograd, for potentials that come
from the solver.  Bound, per gradient: ``max(2e-5, 4 x e32)`` on ``relerr``, e32 from dense float32 autograd on the same inputs —
exactly the rule of tests/test_transport_grad_gpu.py.  Every figure is printed (``pytest -s``)."""
import numpy as np
import pytest
import torch

from cloud_support import to_dev
from conftest import relerr
from geomloss_amd import SamplesLoss, apply_plan, barycentric_map
from transport_grad_support import clouds, dense_apply_plan, dense_barycentric_map

pytestmark = pytest.mark.gpu

N, M, V = 300, 257, 7


@pytest.mark.parametrize("D", (3, 16))
def test_gradients(cuda, D):
    blur = 0.1 * (D / 3) ** 0.5
    eps = blur ** 2
    x, y, _ = clouds(0, N, M, D)
    rng = np.random.default_rng(50)
    a, b = rng.random(N).astype(np.float32) + 0.1, rng.random(M).astype(np.float32) + 0.1
    x, y, a, b = (to_dev(t, cuda) for t in (x, y, a / a.sum(), b / b.sum()))
    F, G = (t.detach().reshape(-1) for t in SamplesLoss("sinkhorn", p=2, blur=blur, potentials=True, debias=False)(a, x, b, y))
    feat = to_dev(rng.standard_normal((M, V)).astype(np.float32), cuda)
    featT = to_dev(rng.standard_normal((N, V)).astype(np.float32), cuda)
    cases = (
        ("apply_plan", "x y F G feat", (x, y, F, G, feat),
         lambda x_, y_, F_, G_, f_: apply_plan(x_, y_, F_, G_, f_, blur, a=a, b=b, resident=True),
         lambda x_, y_, F_, G_, f_: dense_apply_plan(x_, y_, F_, G_, f_, eps, a.to(x_.dtype), b.to(x_.dtype))),
        ("apply_plan^T", "x y F G feat", (x, y, F, G, featT),
         lambda x_, y_, F_, G_, f_: apply_plan(x_, y_, F_, G_, f_, blur, a=a, b=b, transpose=True, resident=True),
         lambda x_, y_, F_, G_, f_: dense_apply_plan(x_, y_, F_, G_, f_, eps, a.to(x_.dtype), b.to(x_.dtype), transpose=True)),
        ("barycentric_map", "x y G", (x, y, G),
         lambda x_, y_, G_: barycentric_map(x_, y_, F, G_, blur, b=b, resident=True),
         lambda x_, y_, G_: dense_barycentric_map(x_, y_, G_, eps, b.to(x_.dtype))),
    )
    for label, names, inputs, got_fn, dense_fn in cases:
        leaves = lambda dtype: [t.detach().clone().to(dtype).requires_grad_(True) for t in inputs]  # noqa: E731
        got, want, plain = leaves(torch.float32), leaves(torch.float64), leaves(torch.float32)
        out = got_fn(*got)
        assert out.grad_fn is not None and out.dtype == torch.float32
        cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(9)).to(out.device)
        g_got = torch.autograd.grad(out, got, cot)
        g_want = torch.autograd.grad(dense_fn(*want), want, cot.double())
        g_plain = torch.autograd.grad(dense_fn(*plain), plain, cot)
        for name, gg, gw, gp in zip(names.split(), g_got, g_want, g_plain):
            assert torch.isfinite(gg).all()
            err, e32 = relerr(gg.cpu().numpy(), gw.cpu().numpy()), relerr(gp.cpu().numpy(), gw.cpu().numpy())
            print(f"D={D} resident {label} d{name}: {err:.2e} (e32 {e32:.2e})")
            assert err <= max(2e-5, 4 * e32), (label, name, err, e32)
