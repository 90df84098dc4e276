"""``hip.argkmin`` (glhip_argkmin, geomloss_amd/csrc/glhip_argkmin_xk.h), ``geomloss_amd.knn``, ``transport.plan_topk`` and
``OTResultSample.sparse_plan`` against a float64 NumPy oracle: ``C = |x - y|^2 / 2 - g``, ``argsort(C, 1)[:, :k]``.

Inputs are those of tests/test_argmin_gpu.py (its generator ``case`` and its oracle ``cost64``), and so is the tolerance

    tol = 2 (NM + 5) 2^-24 (D + max |g|),    NM = (6 + 6 D + 15) // 16:

the worst-case exponent error of glhip_softmin_xk.h, doubled because two exponents are compared.  Criteria, for every row i and rank r
(``judge``):
  (a) indices are valid and distinct within a row; ranks beyond the admissible columns of a row are (-1, +inf);
  (b) |C[i, index[i, r]] - sorted(C[i])[r]| <= tol — order statistics are 1-Lipschitz in the sup norm, so this holds for any kernel
      whose exponents are within tol / 2, whatever it does among near-ties — and the returned value is within tol of the same number;
  (c) on every row whose first min(k + 1, M) float64 order statistics are pairwise more than tol apart, index equals the float64
      argsort[:k] exactly.  The share of rows (c) leaves out is capped per test (5 % for the generator's cases with D >= 2).
Everything that must be bit-identical — against ``hip.argmin``, across k, across launch forms, on duplicates — is compared with
``torch.equal``."""
import numpy as np
import pytest
import torch

import geomloss_amd
from geomloss_amd import hip, ot, plan_topk
from test_argmin_gpu import case, cost64, tol_of

pytestmark = pytest.mark.gpu

# (N, M, D, gs, k): partial row blocks of 256, partial tiles of 128, M < k, both sides of D = 16 | 17, a long K loop, column splits,
# every list capacity (4, 8, 16) and a k that fills none
CASES = [(300, 129, 1, 0.0, 4), (257, 1, 3, 0.0, 4), (257, 7, 3, 0.0, 8), (500, 300, 2, 0.0, 16), (3000, 200, 4, 0.05, 16),
         (1000, 700, 16, 0.0, 8), (1000, 700, 17, 0.1, 16), (600, 500, 100, 0.0, 5), (40, 5000, 24, 0.0, 16)]
INF = float("inf")


def judge(idx, val, C, k, tol, what, exact=True):
    """Criteria (a), (b), (c) of the module docstring on one problem; columns with C = +inf are inadmissible.  Returns the share of
    rows that (c) leaves out."""
    idx, val = np.asarray(idx, np.int64), np.asarray(val, np.float64)
    N, M = C.shape
    assert idx.shape == (N, k) and val.shape == (N, k), what
    order = np.argsort(C, axis=1, kind="stable")[:, :k] if M else np.zeros((N, 0), np.int64)
    stat = np.take_along_axis(C, order, 1) if M else np.zeros((N, 0))
    order = np.concatenate((order, np.full((N, k - order.shape[1]), -1)), 1)
    stat = np.concatenate((stat, np.full((N, k - stat.shape[1]), np.inf)), 1)
    filled = np.isfinite(stat)
    order = np.where(filled, order, -1)
    # (a)
    assert np.array_equal(idx >= 0, filled), what
    assert (idx < max(M, 1)).all() and (val[~filled] == np.inf).all(), what
    srt = np.sort(np.where(filled, idx, -1 - np.arange(k)[None, :]), axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), f"{what}: an index twice in a row"
    # (b)
    got = np.where(filled, C[np.arange(N)[:, None], np.where(filled, idx, 0)], np.inf) if M else stat
    with np.errstate(invalid="ignore"):
        excess = np.where(filled, np.abs(got - stat), 0.0).max(initial=0.0)
        verr = np.where(filled, np.abs(val - stat), 0.0).max(initial=0.0)
    # (c)
    first = np.sort(C, axis=1)[:, :min(k + 1, M)] if M else np.zeros((N, 0))
    with np.errstate(invalid="ignore"):
        gaps = np.diff(first, axis=1)
        clear = ~((gaps <= tol) & np.isfinite(first[:, 1:])).any(1) if gaps.size else np.ones(N, bool)
    left_out = 1.0 - clear.mean() if N else 0.0
    wrong = int((idx[clear] != order[clear]).any(1).sum())
    print(f"{what}: worst excess {excess:.3e}, worst value error {verr:.3e}, tol {tol:.3e}, (c) leaves out {100 * left_out:.1f} % of "
          f"{N} rows, {wrong} of the others off the float64 argsort")
    assert excess <= tol, what
    assert verr <= tol, what
    if exact:
        assert wrong == 0, what
    return left_out


def gpu(cuda, *arrays):
    return tuple(torch.tensor(np.asarray(v)).to(cuda) for v in arrays)


@pytest.mark.parametrize("N,M,D,gs,k", CASES)
def test_argkmin_against_float64(cuda, N, M, D, gs, k):
    x, y, g, C = case(N, M, D, gs)
    xt, yt, gt = gpu(cuda, x, y, g)
    idx, val = hip.argkmin(xt, yt, k, gt if gs else None, return_value=True)
    assert idx.dtype == torch.int32 and idx.shape == (N, k) and val.dtype == torch.float32 and val.shape == (N, k)
    left_out = judge(idx.cpu().numpy(), val.cpu().numpy(), C, k, tol_of(D, float(np.abs(g).max())), f"argkmin {(N, M, D, gs, k)}", exact=D > 1)
    if D > 1:      # (D = 1: neighbouring columns are 2e-5 apart, 15.7 % of the rows have a near-tie among their first k + 1: (a) and (b) alone)
        assert left_out <= 0.05
    # the index alone is the same launch without the value
    assert torch.equal(hip.argkmin(xt, yt, k, gt if gs else None), idx)


@pytest.mark.parametrize("N,M,D,gs", [(3000, 200, 4, 0.05), (600, 500, 100, 0.0), (40, 5000, 24, 0.0)])
def test_k1_is_argmin_and_k_is_a_prefix(cuda, N, M, D, gs):
    x, y, g, _ = case(N, M, D, gs)
    xt, yt, gt = gpu(cuda, x, y, g)
    gt = gt if gs else None
    i1, v1 = hip.argkmin(xt, yt, 1, gt, return_value=True)
    ia, va = hip.argmin(xt, yt, gt, return_value=True)
    assert torch.equal(i1[:, 0], ia) and torch.equal(v1[:, 0], va)
    i16, v16 = hip.argkmin(xt, yt, 16, gt, return_value=True)
    i5, v5 = hip.argkmin(xt, yt, 5, gt, return_value=True)
    assert torch.equal(i5, i16[:, :5]) and torch.equal(v5, v16[:, :5])
    assert torch.equal(i1, i16[:, :1]) and torch.equal(v1, v16[:, :1])


def test_splits_and_duplicates(cuda):
    N, M, D, k = 40, 5000, 24, 16
    x, y, _, _ = case(N, M, D, 0.0)
    assert hip.load_library().glhip_argkmin_workspace_bytes(1, N, M, D, k) > 0      # the default launch splits its columns
    xt, yt = gpu(cuda, x, y)
    i1, v1 = hip.argkmin(xt, yt, k, return_value=True)
    i2, v2 = hip.argkmin(xt, yt, k, return_value=True, flags=hip.FLAG_NO_SPLIT)
    assert torch.equal(i1, i2) and torch.equal(v1, v2)
    # four copies of every column, spread over the splits: the copies of a column share its rank, in ascending index order
    y4 = torch.cat((yt, yt, yt, yt))
    for flags in (0, hip.FLAG_NO_SPLIT):
        i4, v4 = hip.argkmin(xt, y4, k, return_value=True, flags=flags)
        for r in range(4):
            for c in range(4):
                assert torch.equal(i4[:, 4 * r + c], i1[:, r] + c * M), (flags, r, c)
                assert torch.equal(v4[:, 4 * r + c], v1[:, r]), (flags, r, c)


def test_masks_and_empty_problems(cuda):
    N, M, D, gs, k = 3000, 200, 4, 0.05, 8
    x, y, g, C = case(N, M, D, gs)
    xt, yt = gpu(cuda, x, y)
    rng = np.random.default_rng(5)
    off = np.zeros(M, bool)
    off[rng.permutation(M)[: M // 2]] = True
    gm = g.copy()
    gm[off] = -np.inf
    im, vm = hip.argkmin(xt, yt, k, torch.tensor(gm).to(cuda), return_value=True)
    assert not off[im.cpu().numpy()].any()
    left_out = judge(im.cpu().numpy(), vm.cpu().numpy(), np.where(off[None, :], np.inf, C), k, tol_of(D, float(np.abs(g).max())), "masked columns")
    assert left_out <= 0.05
    # fewer admissible columns than k: the last ranks are (-1, +inf)
    g3 = np.full(M, -np.inf, np.float32)
    g3[[7, 50, 199]] = g[[7, 50, 199]]
    i3, v3 = hip.argkmin(xt, yt, k, torch.tensor(g3).to(cuda), return_value=True)
    judge(i3.cpu().numpy(), v3.cpu().numpy(), np.where(np.isinf(g3)[None, :], np.inf, C), k, tol_of(D, float(np.abs(g).max())), "three admissible columns")
    # none at all
    for ie, ve in (hip.argkmin(xt, yt, k, torch.full((M,), -INF, device=cuda), return_value=True), hip.argkmin(xt, yt[:0], k, return_value=True)):
        assert ie.shape == (N, k) and bool((ie == -1).all()) and bool((ve == INF).all())
    # no rows
    i0, v0 = hip.argkmin(xt[:0], yt, k, return_value=True)
    assert i0.shape == (0, k) and v0.shape == (0, k) and i0.dtype == torch.int32


@pytest.mark.parametrize("falling", [True, False])
def test_insertion_under_load(cuda, falling):
    """Columns on a ray that runs towards the rows (falling: every row's cost falls strictly with j, every column enters its lane's
    list) or away from them (no column enters after a list has filled).  Consecutive costs of a row differ by >= 0.1 * 4e-4 = 4e-5,
    24 tol: no row is left out of (c) — asserted."""
    N, M, D, k = 300, 2000, 2, 16
    rng = np.random.default_rng(100 + D)
    x = (0.1 * rng.random((N, D))).astype(np.float32)
    t = np.linspace(1.0, 0.2, M) if falling else np.linspace(0.2, 1.0, M)
    y = np.stack((t, np.zeros(M)), 1).astype(np.float32)
    C = cost64(x, y)
    assert (np.diff(C, axis=1) < 0).all() if falling else (np.diff(C, axis=1) > 0).all()
    idx, val = hip.argkmin(*gpu(cuda, x, y), k, return_value=True)
    assert judge(idx.cpu().numpy(), val.cpu().numpy(), C, k, tol_of(D, 0.0), f"falling = {falling}") == 0.0
    want = np.arange(M - 1, M - 1 - k, -1) if falling else np.arange(k)
    assert np.array_equal(idx.cpu().numpy(), np.broadcast_to(want, (N, k)))


def test_batched(cuda):
    B, N, M, D, k = 3, 257, 300, 5, 8
    rng = np.random.default_rng(100 + D)
    x, y = rng.random((B, N, D)).astype(np.float32), rng.random((B, M, D)).astype(np.float32)
    g = (0.05 * rng.standard_normal((B, M))).astype(np.float32)
    idx, val = hip.argkmin(*gpu(cuda, x, y), k, gpu(cuda, g)[0], return_value=True)
    assert idx.shape == (B, N, k) and val.shape == (B, N, k)
    for b in range(B):
        assert judge(idx[b].cpu().numpy(), val[b].cpu().numpy(), cost64(x[b], y[b], g[b]), k, tol_of(D, float(np.abs(g).max())), f"batch item {b}") <= 0.05


def test_bf16(cuda):
    N, M, D, k = 500, 300, 8, 8
    rng = np.random.default_rng(100 + D)
    xt = torch.tensor(rng.random((N, D)).astype(np.float32)).to(cuda).bfloat16()
    yt = torch.tensor(rng.random((M, D)).astype(np.float32)).to(cuda).bfloat16()
    g = (0.05 * rng.standard_normal(M)).astype(np.float32)
    idx, val = hip.argkmin(xt, yt, k, torch.tensor(g).to(cuda), return_value=True)
    C = cost64(xt.float().cpu().numpy(), yt.float().cpu().numpy(), g)      # the oracle on the bf16-rounded points
    # (bf16 points lie on a coarse grid: exact ties and near-ties are common, so (c) may leave out more rows; (a) and (b) hold for all)
    judge(idx.cpu().numpy(), val.cpu().numpy(), C, k, tol_of(D, float(np.abs(g).max())), "bf16 clouds")


def test_errors(cuda):
    x, y = torch.rand(50, 3, device=cuda), torch.rand(60, 3, device=cuda)
    with pytest.raises(ValueError):
        hip.argkmin(x, y, 4, torch.zeros(59, device=cuda))
    with pytest.raises(ValueError):
        hip.argkmin(x, y, 0)
    with pytest.raises(NotImplementedError):
        hip.argkmin(x, y, hip.ARGKMIN_MAX_K + 1)
    with pytest.raises(NotImplementedError):
        hip.argkmin(x, y, 4, p=1)
    assert hip.argkmin(x, y, 4, flags=hip.FLAG_F16X2).shape == (50, 4)      # accepted and ignored


def test_knn(cuda):
    N, M, D, k = 1000, 700, 16, 8
    x, y, _, C = case(N, M, D, 0.0)
    idx, sq = geomloss_amd.knn(*gpu(cuda, x, y), k)
    assert idx.dtype == torch.int32 and sq.dtype == torch.float32
    assert judge(idx.cpu().numpy(), 0.5 * sq.double().cpu().numpy(), C, k, tol_of(D, 0.0), "knn") <= 0.05
    iv, vv = hip.argkmin(*gpu(cuda, x, y), k, return_value=True)
    assert torch.equal(idx, iv) and torch.equal(sq, 2.0 * vv)


def judge_plan(idx, w, P, eps, D, gmax, k, what):
    """A sparse plan against the dense float64 one: the indices by (b) and (c) on -eps log P, the weights within
    (expm1(tol / eps) + 1e-5) P — the exponent's error in units of eps, and three float32 ulps of an exponent argument of size <= 50
    (asserted by the callers) for the float32 evaluation of the weight."""
    tol = tol_of(D, gmax)
    with np.errstate(divide="ignore"):
        Cp = -eps * np.log(P)
    idx = np.asarray(idx, np.int64)
    left_out = judge(idx, np.take_along_axis(Cp, idx, 1), Cp, k, tol, what)      # (the value criterion is vacuous here: the weights follow)
    assert left_out <= 0.05
    Pk = np.take_along_axis(P, idx, 1)
    rel = (np.abs(np.asarray(w, np.float64) - Pk) / Pk).max()
    bound = np.expm1(tol / eps) + 1e-5
    print(f"{what}: worst relative weight error {rel:.3e}, bound {bound:.3e}")
    assert rel <= bound, what


def test_plan_topk(cuda):
    N, M, D, blur, k = 300, 400, 3, 0.1, 8
    eps = blur**2
    rng = np.random.default_rng(0)
    x, y = rng.random((N, D)).astype(np.float32), rng.random((M, D)).astype(np.float32)
    a, b = rng.random(N).astype(np.float32) + 0.1, rng.random(M).astype(np.float32) + 0.1
    b[17] = 0.0
    a, b = a / a.sum(), b / b.sum()
    F, G = (0.05 * rng.standard_normal(N)).astype(np.float32), (0.05 * rng.standard_normal(M)).astype(np.float32)
    d = lambda v: v.astype(np.float64)  # noqa: E731
    with np.errstate(divide="ignore"):
        P = d(a)[:, None] * d(b)[None, :] * np.exp((d(F)[:, None] + d(G)[None, :] - cost64(x, y)) / eps)
        gmax = float(np.abs(d(G) + eps * np.log(d(b)))[b > 0].max())
    xt, yt, at, bt, Ft, Gt = gpu(cuda, x, y, a, b, F, G)
    idx, w = plan_topk(xt, yt, Ft, Gt, blur, k, a=at, b=bt)
    assert idx.dtype == torch.int32 and idx.shape == (N, k) and w.dtype == torch.float32 and w.shape == (N, k)
    idx, w = idx.cpu().numpy(), w.cpu().numpy()
    assert not (idx == 17).any()                                        # the column of zero weight is never returned
    assert np.abs(np.log(np.take_along_axis(P, idx.astype(np.int64), 1))).max() <= 50.0
    judge_plan(idx, w, P, eps, D, gmax, k, "plan_topk")
    with pytest.raises(NotImplementedError):
        plan_topk(xt, yt, Ft, Gt, blur, k, p=1)


def test_sparse_plan(cuda):
    N, M, D, k = 200, 250, 2, 8
    rng = np.random.default_rng(1)
    x, y = rng.random((N, D)).astype(np.float32), rng.random((M, D)).astype(np.float32)
    a, b = rng.random(N).astype(np.float32) + 0.1, rng.random(M).astype(np.float32) + 0.1
    a, b = a / a.sum(), b / b.sum()
    reg = 0.02
    res = ot.solve_sample(torch.tensor(x).to(cuda), torch.tensor(y).to(cuda), a=torch.tensor(a).to(cuda), b=torch.tensor(b).to(cuda), reg=reg, max_iter=20)
    idx, w = res.sparse_plan(k)
    assert idx.shape == (N, k) and w.shape == (N, k) and idx.dtype == torch.int32 and w.dtype == torch.float32
    f64 = lambda t: t.detach().double().cpu().numpy()  # noqa: E731
    # its own dense plan, in float64 from the same float32 potentials
    f, g = f64(res.potential_a), f64(res.potential_b)
    P = a.astype(np.float64)[:, None] * b.astype(np.float64)[None, :] * np.exp((f[:, None] + g[None, :] - 2.0 * cost64(x, y)) / reg)
    assert np.abs(f64(res.plan) - P).max() <= 1e-4 * P.max()            # (the float32 property is that matrix)
    idx, w = idx.cpu().numpy(), w.cpu().numpy()
    assert np.abs(np.log(np.take_along_axis(P, idx.astype(np.int64), 1))).max() <= 50.0
    gmax = float(np.abs(g / 2.0 + (reg / 2.0) * np.log(b.astype(np.float64))).max())
    judge_plan(idx, w, P, reg / 2.0, D, gmax, k, "sparse_plan")
