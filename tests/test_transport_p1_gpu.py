"""The plan of the p = 1 potentials applied to features end to end: ``geomloss_amd.transport`` with ``p=1`` through ONE
``hip.plan_apply_p1`` launch (geomloss_amd/csrc/glhip_dist_plan_xk.h), against the dense float64 plan built from the same potentials.
Bound: 1e-4 relative, that of tests/test_transport_nd_gpu.py::test_legacy_potentials_in_24_dimensions for the same quantities."""
import numpy as np
import pytest
import torch

from conftest import relerr
from geomloss_amd import SamplesLoss, apply_plan, barycentric_map, hip

pytestmark = pytest.mark.gpu


def _f64(t):
    return t.detach().double().cpu().numpy().squeeze()


@pytest.mark.parametrize("D", [3, 24])
def test_p1_potentials(cuda, D):
    N, M = 500, 600
    blur = 0.1 * float(np.sqrt(D / 3))
    rng = np.random.default_rng(D)
    x, y = rng.random((N, D)).astype(np.float32), (rng.random((M, D)) * 0.8 + 0.1).astype(np.float32)
    a, b = rng.random(N).astype(np.float32) + 0.1, rng.random(M).astype(np.float32) + 0.1
    a, b = a / a.sum(), b / b.sum()
    xt, yt, at, bt = (torch.from_numpy(v).to(cuda) for v in (x, y, a, b))
    F, G = SamplesLoss("sinkhorn", p=1, blur=blur, potentials=True, debias=False)(at, xt, bt, yt)
    C = np.sqrt(np.maximum(((x.astype(np.float64)[:, None, :] - y.astype(np.float64)[None, :, :]) ** 2).sum(-1), 1e-8))
    P = a.astype(np.float64)[:, None] * b.astype(np.float64)[None, :] * np.exp((_f64(F)[:, None] + _f64(G)[None, :] - C) / blur)
    feat = rng.standard_normal((M, 7)).astype(np.float32)
    featT = rng.standard_normal((N, 5)).astype(np.float32)
    got = apply_plan(xt, yt, F, G, torch.from_numpy(feat).to(cuda), blur, a=at, b=bt, p=1)
    gotT = apply_plan(xt, yt, F, G, torch.from_numpy(featT).to(cuda), blur, a=at, b=bt, transpose=True, p=1)
    T = barycentric_map(xt, yt, F, G, blur, b=bt, p=1)
    marg = apply_plan(xt, yt, F, G, torch.ones(M, device=cuda), blur, a=at, b=bt, p=1)
    errs = (relerr(_f64(got), P @ feat), relerr(_f64(gotT), P.T @ featT),
            relerr(_f64(T), (P @ y.astype(np.float64)) / P.sum(1, keepdims=True)), relerr(_f64(marg), P.sum(1)))
    print(f"p = 1 potentials, D = {D}: apply {errs[0]:.2e}, transposed {errs[1]:.2e}, barycentric map {errs[2]:.2e}, marginal {errs[3]:.2e}"
          f" (bound 1e-4)")
    assert got.shape == (N, 7) and gotT.shape == (M, 5) and T.shape == (N, D) and marg.shape == (N,)
    assert got.grad_fn is None and T.grad_fn is None
    assert max(errs) <= 1e-4
    # uniform weights given as None
    Fu, Gu = SamplesLoss("sinkhorn", p=1, blur=blur, potentials=True, debias=False)(xt, yt)
    Pu = np.exp((_f64(Fu)[:, None] + _f64(Gu)[None, :] - C) / blur) / (N * M)
    errs_u = (relerr(_f64(apply_plan(xt, yt, Fu, Gu, torch.from_numpy(feat).to(cuda), blur, p=1)), Pu @ feat),
              relerr(_f64(apply_plan(xt, yt, Fu, Gu, torch.from_numpy(featT).to(cuda), blur, transpose=True, p=1)), Pu.T @ featT),
              relerr(_f64(barycentric_map(xt, yt, Fu, Gu, blur, p=1)), (Pu @ y.astype(np.float64)) / Pu.sum(1, keepdims=True)),
              relerr(_f64(apply_plan(xt, yt, Fu, Gu, torch.ones(M, device=cuda), blur, p=1)), Pu.sum(1)))
    print(f"  uniform weights: apply {errs_u[0]:.2e}, transposed {errs_u[1]:.2e}, barycentric map {errs_u[2]:.2e}, marginal {errs_u[3]:.2e}")
    assert max(errs_u) <= 1e-4


def _counting(monkeypatch):
    calls = {"softmin": 0, "plan_apply_nd": 0, "plan_apply_p1": 0}

    def count(name, fn):
        def wrapper(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapper
    for name in calls:
        monkeypatch.setattr(hip, name, count(name, getattr(hip, name)))
    return calls


def test_one_launch_per_application(cuda, monkeypatch):
    N, M, D, blur = 120, 150, 24, 0.3
    g = torch.Generator().manual_seed(0)
    x, y = torch.rand(N, D, generator=g).to(cuda), (torch.rand(M, D, generator=g) * 0.8 + 0.1).to(cuda)
    F, G = torch.randn(N, generator=g).to(cuda) * 0.1, torch.randn(M, generator=g).to(cuda) * 0.1
    feat, featT = torch.randn(M, 7, generator=g).to(cuda), torch.randn(N, 5, generator=g).to(cuda)
    calls = _counting(monkeypatch)
    for run in (lambda: apply_plan(x, y, F, G, feat, blur, p=1), lambda: apply_plan(x, y, F, G, featT, blur, transpose=True, p=1),
                lambda: barycentric_map(x, y, F, G, blur, p=1)):
        calls.update(softmin=0, plan_apply_nd=0, plan_apply_p1=0)
        run()
        assert calls == {"softmin": 0, "plan_apply_nd": 0, "plan_apply_p1": 1}
    # the p = 2 path makes exactly the calls it made before
    for kw in ({}, {"p": 2}):
        calls.update(softmin=0, plan_apply_nd=0, plan_apply_p1=0)
        apply_plan(x, y, F, G, feat, blur, **kw)
        assert calls == {"softmin": 1, "plan_apply_nd": 1, "plan_apply_p1": 0}
    calls.update(softmin=0, plan_apply_nd=0, plan_apply_p1=0)
    barycentric_map(x, y, F, G, blur)
    assert calls == {"softmin": 0, "plan_apply_nd": 1, "plan_apply_p1": 0}


def test_other_costs_are_refused(cuda):
    x, y = torch.rand(40, 3, device=cuda), torch.rand(50, 3, device=cuda)
    F, G, feat = torch.zeros(40, device=cuda), torch.zeros(50, device=cuda), torch.ones(50, 2, device=cuda)
    with pytest.raises(ValueError):
        apply_plan(x, y, F, G, feat, 0.1, p=3)
    with pytest.raises(ValueError):
        apply_plan(x, y, F, G, torch.ones(40, 2, device=cuda), 0.1, transpose=True, p=3)
    with pytest.raises(ValueError):
        barycentric_map(x, y, F, G, 0.1, p=0)
