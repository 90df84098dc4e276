"""The autograd functions of ``geomloss_amd.transport`` (p = 2) on the CPU: ``hip.softmin``, ``hip.plan_apply_nd`` and ``hip.plan_bilinear``
are replaced by dense float32 stand-ins (tests/transport_grad_support.py), and every gradient of ``apply_plan`` (plain and transposed) and
of ``barycentric_map`` is compared with dense float64 autograd.  Checks the formulas and the plumbing, not the kernels."""
import pytest
import torch

from conftest import relerr
from geomloss_amd import transport
from transport_grad_support import DenseHip, clouds, dense_apply_plan, dense_barycentric_map

N, M, D, V = 40, 50, 5, 7
BLUR = 0.4
EPS = BLUR**2
TOL = 1e-4


def _inputs(B, vector=False, transpose=False, seed=0):
    """float32 leaves x, y, F, G, feat and weights a, b; feat lives on the columns (on the rows for the transposed product)."""
    x, y, _ = clouds(seed, N, M, D, B)
    g = torch.Generator().manual_seed(seed + 1)
    lead = () if B is None else (B,)
    x, y = torch.from_numpy(x), torch.from_numpy(y)
    F = 0.1 * torch.randn(lead + (N,), generator=g)
    G = 0.1 * torch.randn(lead + (M,), generator=g)
    feat = torch.randn(lead + ((N if transpose else M),) + (() if vector else (V,)), generator=g)
    a = torch.rand(lead + (N,), generator=g) + 0.5
    b = torch.rand(lead + (M,), generator=g) + 0.5
    return x, y, F, G, feat, a / a.sum(-1, keepdim=True), b / b.sum(-1, keepdim=True)


def _leaves(ts, dtype=None):
    return [t.detach().clone().to(dtype or t.dtype).requires_grad_(True) for t in ts]


@pytest.fixture
def dense(monkeypatch):
    return DenseHip().install(monkeypatch)


@pytest.mark.parametrize("transpose", (False, True))
@pytest.mark.parametrize("B,vector", ((None, False), (2, False), (None, True)))
def test_apply_plan_gradients(dense, B, vector, transpose):
    *diff, a, b = _inputs(B, vector, transpose)
    got = _leaves(diff)
    out = transport.apply_plan(*got, BLUR, a=a, b=b, transpose=transpose)
    assert out.grad_fn is not None and out.dtype == torch.float32
    want = _leaves(diff, torch.float64)
    ref = dense_apply_plan(*want, EPS, a.double(), b.double(), transpose=transpose)
    assert relerr(out.detach().numpy(), ref.detach().numpy()) < TOL
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(7))
    g_got = torch.autograd.grad(out, got, cot)
    g_want = torch.autograd.grad(ref, want, cot.double())
    for name, gg, gw, leaf in zip("x y F G feat".split(), g_got, g_want, got):
        assert gg.dtype == leaf.dtype and gg.shape == leaf.shape
        err = relerr(gg.numpy(), gw.numpy())
        print(f"apply_plan B={B} vector={vector} transpose={transpose} d{name}: {err:.2e}")
        assert err < TOL, (name, err)


@pytest.mark.parametrize("B", (None, 2))
def test_barycentric_map_gradients(dense, B):
    x, y, F, G, _, _, b = _inputs(B)
    got = _leaves((x, y, G))
    T = transport.barycentric_map(got[0], got[1], F, got[2], BLUR, b=b)
    assert T.grad_fn is not None
    want = _leaves((x, y, G), torch.float64)
    ref = dense_barycentric_map(*want, EPS, b.double())
    assert relerr(T.detach().numpy(), ref.detach().numpy()) < TOL
    cot = torch.randn(T.shape, generator=torch.Generator().manual_seed(7))
    g_got = torch.autograd.grad(T, got, cot)
    g_want = torch.autograd.grad(ref, want, cot.double())
    for name, gg, gw, leaf in zip("x y G".split(), g_got, g_want, got):
        assert gg.dtype == leaf.dtype and gg.shape == leaf.shape
        err = relerr(gg.numpy(), gw.numpy())
        print(f"barycentric_map B={B} d{name}: {err:.2e}")
        assert err < TOL, (name, err)
    # the usual loss: |T(x) - target|^2 fills x.grad and y.grad
    xg, yg = _leaves((x, y))
    (transport.barycentric_map(xg, yg, F, G, BLUR) - 0.5).pow(2).sum().backward()
    assert xg.grad is not None and yg.grad is not None and torch.isfinite(xg.grad).all() and torch.isfinite(yg.grad).all()


def test_only_the_needed_reductions_run(dense):
    x, y, F, G, feat, a, b = _inputs(None)

    def bilinear_calls(which):
        args = [x, y, F, G, feat]
        args[which] = args[which].clone().requires_grad_(True)
        out = transport.apply_plan(*args, BLUR, a=a, b=b)
        before = dict(dense.calls)
        out.sum().backward()
        assert args[which].grad is not None
        return {k: dense.calls[k] - before[k] for k in before}

    assert bilinear_calls(4) == {"softmin": 1, "plan_apply_nd": 1, "plan_bilinear": 0}      # feat alone: the transposed application
    assert bilinear_calls(0) == {"softmin": 0, "plan_apply_nd": 0, "plan_bilinear": 1}      # x alone: one reduction, the saved soft-min
    assert bilinear_calls(2) == {"softmin": 0, "plan_apply_nd": 0, "plan_bilinear": 0}      # F alone: <Gb, out> / eps
    assert bilinear_calls(1) == {"softmin": 1, "plan_apply_nd": 0, "plan_bilinear": 1}
    assert bilinear_calls(3) == {"softmin": 1, "plan_apply_nd": 0, "plan_bilinear": 1}


def test_no_graph_without_a_request(dense):
    x, y, F, G, feat, a, b = _inputs(None)
    plain = transport.apply_plan(x, y, F, G, feat, BLUR, a=a, b=b)
    plain_t = transport.barycentric_map(x, y, F, G, BLUR, b=b)
    assert plain.grad_fn is None and plain_t.grad_fn is None and not plain.requires_grad
    calls = dict(dense.calls)
    assert calls == {"softmin": 1, "plan_apply_nd": 2, "plan_bilinear": 0}      # the launches of the present functions
    xg = x.clone().requires_grad_(True)
    with torch.no_grad():
        quiet = transport.apply_plan(xg, y, F, G, feat, BLUR, a=a, b=b)
        quiet_t = transport.barycentric_map(xg, y, F, G, BLUR, b=b)
    assert quiet.grad_fn is None and quiet_t.grad_fn is None
    assert torch.equal(quiet, plain) and torch.equal(quiet_t, plain_t)
    # the recorded call returns the same values
    assert torch.equal(transport.apply_plan(xg, y, F, G, feat, BLUR, a=a, b=b).detach(), plain)
    assert torch.equal(transport.barycentric_map(xg, y, F, G, BLUR, b=b).detach(), plain_t)
    # the weights are constants: they alone do not start a graph
    assert transport.apply_plan(x, y, F, G, feat, BLUR, a=a.clone().requires_grad_(True), b=b).grad_fn is None


def test_p1_stays_without_graph(monkeypatch):
    from geomloss_amd import hip

    def fake_p1(eps, x, y, h, feat, flags=0, want_softmin=False, ranges=None):
        avg = torch.zeros(x.shape[:-1] + feat.shape[-1:])
        return (avg, torch.zeros(x.shape[:-1])) if want_softmin else avg

    monkeypatch.setattr(hip, "plan_apply_p1", fake_p1)
    x, y, F, G, feat, a, b = _inputs(None)
    xg = x.clone().requires_grad_(True)
    assert transport.apply_plan(xg, y, F, G, feat, BLUR, p=1).grad_fn is None
    assert transport.barycentric_map(xg, y, F, G, BLUR, p=1).grad_fn is None
