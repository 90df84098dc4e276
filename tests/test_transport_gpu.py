"""The plan applied to features end to end: ``ot.solve_sample(...).plan_operator @ S`` through one forward reduction and one
``hip.plan_apply`` (geomloss_amd/ot/sample.py), and ``geomloss_amd.transport`` for the potentials of the legacy API."""
import numpy as np
import pytest
import torch

from conftest import load_golden, relerr
from geomloss_amd import SamplesLoss, apply_plan, barycentric_map, hip, ot

pytestmark = pytest.mark.gpu


def _solve(cuda, name):
    rec = load_golden(name)
    x, y = (torch.from_numpy(rec[k]).float().to(cuda) for k in ("x", "y"))
    a, b = (torch.from_numpy(rec[k]).float().to(cuda) if k in rec else None for k in ("a", "b"))
    return ot.solve_sample(x, y, a=a, b=b, **rec["kwargs"])


@pytest.mark.parametrize("name", ["ot_unbalanced_d2", "ot_balanced_d3_uniform"])
def test_operators_on_golden_solves_take_one_forward_reduction(cuda, name, monkeypatch):
    res = _solve(cuda, name)
    P, dens = res.plan, res.density
    N, M = P.shape
    g = torch.Generator().manual_seed(0)
    S, U = torch.randn(M, 40, generator=g).to(cuda), torch.randn(N, 40, generator=g).to(cuda)
    calls = []
    raw = hip.softmin_fwd_raw
    monkeypatch.setattr(hip, "softmin_fwd_raw", lambda *a, **k: (calls.append(1), raw(*a, **k))[1])
    for op, dense in ((res.plan_operator, P), (res.density_operator, dens)):
        for got, want in ((lambda: op @ S, dense @ S), (lambda: op.T @ U, dense.t() @ U)):
            calls.clear()
            out = got()
            err = relerr(out.cpu().numpy(), want.cpu().numpy())
            print(f"{name}: {err:.2e} with {len(calls)} forward reduction(s)")
            assert err < 1e-4
            assert len(calls) <= 1


def test_marginals_stay_on_the_log_domain_path(cuda, monkeypatch):
    res = _solve(cuda, "ot_unbalanced_d2")
    ma, mb = res.marginal_a.clone(), res.marginal_b.clone()

    def refuse(*a, **k):
        raise AssertionError("the marginals must not go through hip.plan_apply")
    monkeypatch.setattr(hip, "plan_apply", refuse)
    again = _solve(cuda, "ot_unbalanced_d2")
    assert torch.equal(again.marginal_a, ma) and torch.equal(again.marginal_b, mb)


def test_one_or_two_columns_stay_on_the_log_domain_path(cuda, monkeypatch):
    """2 V forward reductions are cheaper than a forward reduction and an application up to V = 2: `lazy_plan @ v` is what it was."""
    res = _solve(cuda, "ot_unbalanced_d2")
    P = res.plan
    g = torch.Generator().manual_seed(1)
    v, S2 = torch.randn(P.shape[1], generator=g).to(cuda), torch.randn(P.shape[1], 2, generator=g).to(cuda)

    def refuse(*a, **k):
        raise AssertionError("one or two columns must not go through hip.plan_apply")
    monkeypatch.setattr(hip, "plan_apply", refuse)
    assert relerr((res.lazy_plan @ v).cpu().numpy(), (P @ v).cpu().numpy()) < 1e-4
    assert relerr((res.plan_operator @ S2).cpu().numpy(), (P @ S2).cpu().numpy()) < 1e-4


def test_legacy_potentials(cuda):
    N, M, D, blur = 400, 500, 3, 0.1
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
    ones = apply_plan(xt, yt, F, G, torch.ones(M, device=cuda), blur, a=at, b=bt)
    T = barycentric_map(xt, yt, F, G, blur, b=bt)
    errs = (relerr(f64(got), P @ feat), relerr(f64(gotT), P.T @ featT), relerr(f64(ones), P.sum(1)),
            relerr(f64(T), (P @ y.astype(np.float64)) / P.sum(1, keepdims=True)))
    print(f"legacy potentials: apply {errs[0]:.2e}, transposed {errs[1]:.2e}, ones {errs[2]:.2e}, barycentric map {errs[3]:.2e}")
    assert got.shape == (N, 7) and gotT.shape == (M, 5) and ones.shape == (N,) and T.shape == (N, D)
    assert max(errs) <= 1e-4
    # uniform weights by default
    Fu, Gu = SamplesLoss("sinkhorn", p=2, blur=blur, potentials=True, debias=False)(xt, yt)
    Pu = np.exp((f64(Fu)[:, None] + f64(Gu)[None, :] - C) / blur**2) / (N * M)
    assert relerr(f64(apply_plan(xt, yt, Fu, Gu, torch.from_numpy(feat).to(cuda), blur)), Pu @ feat) <= 1e-4
