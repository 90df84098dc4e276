"""``hip.argmin`` (glhip_argmin, geomloss_amd/csrc/glhip_argmin_xk.h) and ``transport.plan_argmax`` against a float64 NumPy oracle:
``C = |x - y|^2 / 2 - g``, ``C.argmin(1)``.

Criterion of every case: the float64 cost of the returned column exceeds the true row minimum by at most

    tol = 2 (NM + 5) 2^-24 (D + max |g|),    NM = (6 + 6 D + 15) // 16,

twice the worst-case exponent error stated in the header of glhip_softmin_xk.h (two exponents are compared) with diam^2 <= D and
|H_j| <= D / 2 + max |g| for clouds in the unit cube; the returned float32 value is within tol of the float64 minimum."""
import functools

import numpy as np
import pytest
import torch

from geomloss_amd import SamplesLoss, hip, plan_argmax

pytestmark = pytest.mark.gpu

# (N, M, D, gs): partial row blocks of 256, partial tiles of 128, a single column, both sides of D = 16 | 17, a long K loop
SHAPES = [(300, 129, 1, 0.0), (257, 1, 3, 0.0), (3000, 200, 4, 0.0), (3000, 200, 4, 0.05), (1000, 700, 16, 0.0), (1000, 700, 17, 0.1),
          (600, 500, 100, 0.0), (40, 5000, 24, 0.0)]


def tol_of(D, gmax):
    return 2.0 * ((6 + 6 * D + 15) // 16 + 5) * 2.0**-24 * (D + gmax)


def cost64(x, y, g=None):
    """|x_i - y_j|^2 / 2 - g_j in float64 from explicit differences, one coordinate at a time."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    C = np.zeros((x.shape[0], y.shape[0]))
    for d in range(x.shape[1]):
        C += (x[:, d, None] - y[None, :, d]) ** 2
    C *= 0.5
    return C if g is None else C - np.asarray(g, np.float64)[None, :]


@functools.lru_cache(maxsize=None)
def case(N, M, D, gs):
    """Clouds uniform in the unit cube, g = gs * standard_normal, seed default_rng(100 + D); the float64 costs, computed once."""
    rng = np.random.default_rng(100 + D)
    x, y = rng.random((N, D)).astype(np.float32), rng.random((M, D)).astype(np.float32)
    g = (gs * rng.standard_normal(M)).astype(np.float32)
    C = cost64(x, y, g)
    for a in (x, y, g, C):
        a.setflags(write=False)
    return x, y, g, C


def judge(idx, val, C, tol, what):
    """The criterion above; returns the number of rows whose index differs from the float64 argmin."""
    idx, val = np.asarray(idx, np.int64), np.asarray(val, np.float64)
    rows = np.arange(C.shape[0])
    assert idx.min() >= 0 and idx.max() < C.shape[1], what
    cmin = C.min(1)
    excess, verr = (C[rows, idx] - cmin).max(), np.abs(val - cmin).max()
    wrong = int((idx != C.argmin(1)).sum())
    print(f"{what}: cost excess {excess:.3e}, value error {verr:.3e}, tol {tol:.3e}, {wrong} of {len(rows)} rows off the float64 argmin")
    assert excess <= tol, what
    assert verr <= tol, what
    return wrong


@pytest.mark.parametrize("N,M,D,gs", SHAPES)
def test_argmin_against_float64(cuda, N, M, D, gs):
    x, y, g, C = case(N, M, D, gs)
    xt, yt, gt = (torch.tensor(v).to(cuda) for v in (x, y, g))
    idx, val = hip.argmin(xt, yt, gt if gs else None, return_value=True)
    assert idx.dtype == torch.int32 and idx.shape == (N,) and val.dtype == torch.float32 and val.shape == (N,)
    wrong = judge(idx.cpu().numpy(), val.cpu().numpy(), C, tol_of(D, float(np.abs(g).max())), f"argmin {(N, M, D, gs)}")
    if D > 1:      # (D = 1: neighbouring columns are 2e-5 apart, ~10 % of the rows have a runner-up inside tol: the cost criterion alone)
        assert wrong == 0
    # g = zeros is g = None, and the index alone is the same launch without the value
    if not gs:
        assert torch.equal(hip.argmin(xt, yt, gt), idx)
    assert torch.equal(hip.argmin(xt, yt, gt if gs else None), idx)


def test_argmin_d2(cuda):
    """D = 2, the dimension the table above leaves out of 1, 2, 3, 4, 16, 17: two MFMAs, the second 24-slot group all zeros.
    (No row of these inputs has a runner-up inside tol: checked with NumPy.)"""
    N, M, D = 500, 300, 2
    rng = np.random.default_rng(100 + D)
    x, y = rng.random((N, D)).astype(np.float32), rng.random((M, D)).astype(np.float32)
    idx, val = hip.argmin(torch.tensor(x).to(cuda), torch.tensor(y).to(cuda), return_value=True)
    assert judge(idx.cpu().numpy(), val.cpu().numpy(), cost64(x, y), tol_of(D, 0.0), "D = 2") == 0


def test_argmin_batched(cuda):
    B, N, M, D = 3, 257, 300, 5
    rng = np.random.default_rng(100 + D)
    x, y = rng.random((B, N, D)).astype(np.float32), rng.random((B, M, D)).astype(np.float32)
    g = (0.05 * rng.standard_normal((B, M))).astype(np.float32)
    idx, val = hip.argmin(*(torch.tensor(v).to(cuda) for v in (x, y, g)), return_value=True)
    assert idx.shape == (B, N) and val.shape == (B, N)
    for b in range(B):
        wrong = judge(idx[b].cpu().numpy(), val[b].cpu().numpy(), cost64(x[b], y[b], g[b]), tol_of(D, float(np.abs(g).max())), f"batch item {b}")
        assert wrong == 0


def test_argmin_bf16(cuda):
    N, M, D = 500, 300, 8
    rng = np.random.default_rng(100 + D)
    xt = torch.tensor(rng.random((N, D)).astype(np.float32)).to(cuda).bfloat16()
    yt = torch.tensor(rng.random((M, D)).astype(np.float32)).to(cuda).bfloat16()
    g = (0.05 * rng.standard_normal(M)).astype(np.float32)
    idx, val = hip.argmin(xt, yt, torch.tensor(g).to(cuda), return_value=True)
    C = cost64(xt.float().cpu().numpy(), yt.float().cpu().numpy(), g)      # the oracle on the bf16-rounded points
    judge(idx.cpu().numpy(), val.cpu().numpy(), C, tol_of(D, float(np.abs(g).max())), "bf16 clouds")


def test_column_splits_do_not_change_the_result(cuda):
    N, M, D, gs = 40, 5000, 24, 0.0
    x, y, _, C = case(N, M, D, gs)
    assert hip.load_library().glhip_argmin_workspace_bytes(1, N, M, D) > 0      # the default launch splits its columns
    xt, yt = torch.tensor(x).to(cuda), torch.tensor(y).to(cuda)
    i1, v1 = hip.argmin(xt, yt, return_value=True)
    i2, v2 = hip.argmin(xt, yt, return_value=True, flags=hip.FLAG_NO_SPLIT)
    assert torch.equal(i1, i2) and torch.equal(v1, v2)
    assert np.array_equal(i1.cpu().numpy(), C.argmin(1))
    # ... with duplicates spread over the splits too: the first copy, whatever the launch
    y4 = torch.cat((yt, yt, yt, yt))
    assert torch.equal(hip.argmin(xt, y4), i1) and torch.equal(hip.argmin(xt, y4, flags=hip.FLAG_NO_SPLIT), i1)


def test_ties_and_masks(cuda):
    N, M, D, gs = 3000, 200, 4, 0.05
    x, y, g, C = case(N, M, D, gs)
    xt, yt, gt = (torch.tensor(v).to(cuda) for v in (x, y, g))
    idx, val = hip.argmin(xt, yt, gt, return_value=True)
    # exact duplicates: the first copy wins
    i2, v2 = hip.argmin(xt, torch.cat((yt, yt)), torch.cat((gt, gt)), return_value=True)
    assert int(i2.max()) < M and torch.equal(i2, idx) and torch.equal(v2, val)
    # g = -inf on a random half of the columns: only the other half is ever returned
    rng = np.random.default_rng(5)
    off = np.zeros(M, bool)
    off[rng.permutation(M)[: M // 2]] = True
    gm = g.copy()
    gm[off] = -np.inf
    im, vm = hip.argmin(xt, yt, torch.tensor(gm).to(cuda), return_value=True)
    assert not off[im.cpu().numpy()].any()
    Cm = np.where(off[None, :], np.inf, C)
    judge(im.cpu().numpy(), vm.cpu().numpy(), Cm, tol_of(D, float(np.abs(g).max())), "masked columns")      # (one row has a runner-up inside tol)
    # no admissible column: index -1, value +inf
    for ie, ve in (hip.argmin(xt, yt, torch.full((M,), -float("inf"), device=cuda), return_value=True),
                   hip.argmin(xt, yt[:0], return_value=True)):
        assert ie.shape == (N,) and bool((ie == -1).all()) and bool((ve == float("inf")).all())
    # two runs are bit-identical
    i3, v3 = hip.argmin(xt, yt, gt, return_value=True)
    assert torch.equal(i3, idx) and torch.equal(v3, val)


def test_errors(cuda):
    x, y = torch.rand(50, 3, device=cuda), torch.rand(60, 3, device=cuda)
    with pytest.raises(NotImplementedError):
        hip.argmin(x, y, p=1)
    with pytest.raises(NotImplementedError):
        hip.argmin(x.double(), y.double())
    with pytest.raises(NotImplementedError):
        hip.argmin(torch.rand(4, 4096, device=cuda), torch.rand(5, 4096, device=cuda))
    with pytest.raises(ValueError):
        hip.argmin(x, y, torch.zeros(59, device=cuda))
    assert hip.argmin(x, y, flags=hip.FLAG_F16X2).shape == (50,)      # accepted and ignored


def test_plan_argmax(cuda):
    """On the potentials of tests/test_transport_gpu.py::test_legacy_potentials: the returned column's entry of the float64 dense
    plan is within a factor exp(-tol / eps) of the row maximum, and it is the row maximum itself on all but at most 1 % of the rows
    (the cap is there so that near-ties cannot hide a wrong kernel)."""
    N, M, D, blur = 400, 500, 3, 0.1
    eps = blur**2
    rng = np.random.default_rng(0)
    x, y = rng.random((N, D)).astype(np.float32), (rng.random((M, D)) * 0.8 + 0.1).astype(np.float32)
    a, b = rng.random(N).astype(np.float32) + 0.1, rng.random(M).astype(np.float32) + 0.1
    a, b = a / a.sum(), b / b.sum()
    xt, yt, at, bt = (torch.tensor(v).to(cuda) for v in (x, y, a, b))
    F, G = SamplesLoss("sinkhorn", p=2, blur=blur, potentials=True, debias=False)(at, xt, bt, yt)
    f64 = lambda t: t.detach().double().cpu().numpy().squeeze()  # noqa: E731
    P = a.astype(np.float64)[:, None] * b.astype(np.float64)[None, :] * np.exp((f64(F)[:, None] + f64(G)[None, :] - cost64(x, y)) / eps)
    idx = plan_argmax(xt, yt, F, G, blur, b=bt)
    assert idx.dtype == torch.int32 and idx.shape == (N,)
    idx = idx.cpu().numpy().astype(np.int64)
    gmax = float(np.abs(f64(G) + eps * np.log(b.astype(np.float64))).max())
    tol = tol_of(D, gmax)
    ratio = (P[np.arange(N), idx] / P.max(1)).min()
    wrong = int((idx != P.argmax(1)).sum())
    print(f"plan_argmax: smallest P[i, idx] / max_j P_ij = {ratio:.9f} (bound {np.exp(-tol / eps):.9f}), {wrong} of {N} rows off the float64 argmax")
    assert ratio >= np.exp(-tol / eps)
    assert wrong <= N // 100
    # a column of zero weight is never returned
    b0 = bt.clone()
    b0[idx[:50]] = 0.0
    assert not np.isin(plan_argmax(xt, yt, F, G, blur, b=b0).cpu().numpy(), idx[:50]).any()
