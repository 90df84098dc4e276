"""The plan applied to features end to end for clouds of D > 16: ``geomloss_amd.transport`` and ``ot.solve_sample(...).plan_operator @ S``
through one forward reduction and one ``hip.plan_apply_nd`` (geomloss_amd/csrc/glhip_plan_apply_xk.h).  Bounds: those of
tests/test_transport_gpu.py for the same quantities at D <= 16."""
import numpy as np
import pytest
import torch

from conftest import relerr
from geomloss_amd import SamplesLoss, apply_plan, barycentric_map, hip, ot

pytestmark = pytest.mark.gpu


def test_legacy_potentials_in_24_dimensions(cuda):
    N, M, D, blur = 200, 260, 24, 0.7
    rng = np.random.default_rng(0)
    x, y = rng.random((N, D)).astype(np.float32), (rng.random((M, D)) * 0.8 + 0.1).astype(np.float32)
    a, b = rng.random(N).astype(np.float32) + 0.1, rng.random(M).astype(np.float32) + 0.1
    a, b = a / a.sum(), b / b.sum()
    xt, yt, at, bt = (torch.from_numpy(v).to(cuda) for v in (x, y, a, b))
    F, G = SamplesLoss("sinkhorn", p=2, blur=blur, potentials=True, debias=False)(at, xt, bt, yt)
    f64 = lambda t: t.detach().double().cpu().numpy().squeeze()  # noqa: E731
    C = ((x.astype(np.float64)[:, None, :] - y.astype(np.float64)[None, :, :]) ** 2).sum(-1) / 2.0
    P = a.astype(np.float64)[:, None] * b.astype(np.float64)[None, :] * np.exp((f64(F)[:, None] + f64(G)[None, :] - C) / blur**2)
    feat = rng.standard_normal((M, 7)).astype(np.float32)
    featT = rng.standard_normal((N, 5)).astype(np.float32)
    got = apply_plan(xt, yt, F, G, torch.from_numpy(feat).to(cuda), blur, a=at, b=bt)
    gotT = apply_plan(xt, yt, F, G, torch.from_numpy(featT).to(cuda), blur, a=at, b=bt, transpose=True)
    T = barycentric_map(xt, yt, F, G, blur, b=bt)
    errs = (relerr(f64(got), P @ feat), relerr(f64(gotT), P.T @ featT),
            relerr(f64(T), (P @ y.astype(np.float64)) / P.sum(1, keepdims=True)))
    print(f"legacy potentials, D = {D}: apply {errs[0]:.2e}, transposed {errs[1]:.2e}, barycentric map {errs[2]:.2e}")
    assert got.shape == (N, 7) and gotT.shape == (M, 5) and T.shape == (N, D)
    assert max(errs) <= 1e-4
    # uniform weights by default
    Fu, Gu = SamplesLoss("sinkhorn", p=2, blur=blur, potentials=True, debias=False)(xt, yt)
    Pu = np.exp((f64(Fu)[:, None] + f64(Gu)[None, :] - C) / blur**2) / (N * M)
    assert relerr(f64(apply_plan(xt, yt, Fu, Gu, torch.from_numpy(feat).to(cuda), blur)), Pu @ feat) <= 1e-4


def _counting(monkeypatch):
    calls = {"softmin": 0, "plan_apply_nd": 0}
    softmin, plan = hip.softmin, hip.plan_apply_nd

    def count(name, fn):
        def wrapper(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapper
    monkeypatch.setattr(hip, "softmin", count("softmin", softmin))
    monkeypatch.setattr(hip, "plan_apply_nd", count("plan_apply_nd", plan))
    return calls


def test_solve_sample_operators_in_20_dimensions(cuda, monkeypatch):
    N, M, D = 150, 170, 20
    g = torch.Generator().manual_seed(0)
    x, y = torch.rand(N, D, generator=g).to(cuda), (torch.rand(M, D, generator=g) * 0.8 + 0.1).to(cuda)
    res = ot.solve_sample(x, y, reg=2.0, max_iter=40)
    P = res.plan
    S, U = torch.randn(M, 8, generator=g).to(cuda), torch.randn(N, 8, generator=g).to(cuda)
    calls = _counting(monkeypatch)
    for got, want in ((lambda: res.plan_operator @ S, P @ S), (lambda: res.plan_operator.T @ U, P.t() @ U)):
        calls.update(softmin=0, plan_apply_nd=0)
        out = got()
        err = relerr(out.cpu().numpy(), want.cpu().numpy())
        print(f"solve_sample D = {D}, V = 8: {err:.2e} with {calls}")
        assert err < 1e-4
        assert calls == {"softmin": 1, "plan_apply_nd": 1}
    # a single column stays on the log-domain loop
    calls.update(softmin=0, plan_apply_nd=0)
    v = torch.randn(M, generator=g).to(cuda)
    assert relerr((res.lazy_plan @ v).cpu().numpy(), (P @ v).cpu().numpy()) < 1e-4
    assert calls["plan_apply_nd"] == 0
