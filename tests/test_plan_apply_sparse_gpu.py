"""``hip.plan_apply_sparse`` / ``glhip_plan_apply_sparse`` (geomloss_amd/csrc/glhip_plan_apply_sparse.h): the plan of a p = 2 soft-min
applied to features on block-sparse ranges, against float64 NumPy on the ranges expanded to a boolean mask: W = exp(E - lse_masked(E)),
ref = W @ feat.  Bound per feature column, the bar of tests/test_plan_apply_gpu.py::test_parity: |out - ref|[:, v] <= 2e-5 max_j
|feat[j, v]| at eps = 0.01 (D <= 3) / 0.1 D / 3 (D >= 4), |mass - 1| <= 1e-4."""
import numpy as np
import pytest
import torch

from cloud_support import clouds as _clouds, to_dev as _t
from geomloss_amd import SamplesLoss, hip, transport

pytestmark = pytest.mark.gpu

N, M = 700, 900
# row block -> its column intervals.  300 rows: two chunks; 20 rows: under one wavefront; 100: no multiple of 32; [420, 500): an empty
# slice; rows [500, 530) lie in no block.  Block 0 gathers 10 + 25 + 10 + 120 + 5 columns across the 128-column tile boundary (and the
# 64-column one of four-chunk passes); blocks 1 and 2 hold long intervals.
BLOCKS = [((0, 300), [(0, 10), (15, 40), (50, 60), (100, 220), (300, 305)]), ((300, 320), [(0, 900)]),
          ((320, 420), [(0, 31), (400, 900)]), ((420, 500), []), ((530, 700), [(600, 631), (640, 651), (700, 900)])]
VOID = [20, 650]      # columns with h = -inf and a feature of 1e30, inside kept intervals


def _eps(D):
    return 0.01 if D <= 3 else 0.1 * D / 3


def _ranges(blocks, dev):
    ri = np.array([b for b, _ in blocks], dtype=np.int32).reshape(-1, 2)
    red = np.array([iv for _, ivs in blocks for iv in ivs], dtype=np.int32).reshape(-1, 2)
    sl = np.cumsum([len(ivs) for _, ivs in blocks]).astype(np.int32)
    t = [_t(a, dev) for a in (ri, sl, red)]
    return hip.BlockRanges(*t, *t)      # (the transposed half is not read here)


def _mask(blocks, n, m):
    K = np.zeros((n, m), dtype=bool)
    for (r0, r1), ivs in blocks:
        for j0, j1 in ivs:
            K[r0:r1, j0:j1] = True
    return K


def _ref(x, y, h, eps, feat, K):
    x, y, h, feat = (np.asarray(t, dtype=np.float64) for t in (x, y, h, feat))
    E = np.where(K, h[None, :] - ((x * x).sum(1)[:, None] - 2.0 * x @ y.T + (y * y).sum(1)[None, :]) / (2.0 * eps), -np.inf)
    m = E.max(1, keepdims=True)
    W = np.exp(E - np.where(np.isfinite(m), m, 0.0))
    s = W.sum(1, keepdims=True)
    return (W / np.where(s > 0, s, 1.0)) @ feat, s[:, 0] > 0


_CASES = {}


def _case(D, V):      # inputs and the float64 reference, computed once for every flag setting
    if (D, V) not in _CASES:
        x, y, h = _clouds(D + V, N, M, D)
        feat = np.random.default_rng(V).standard_normal((M, V)).astype(np.float32)
        h[VOID], feat[VOID] = -np.inf, 1e30
        _CASES[(D, V)] = (x, y, h, feat)
    return _CASES[(D, V)]


def _run(cuda, x, y, h, feat, eps, blocks, flags=0, bf16=False):
    xt, yt = _t(x, cuda), _t(y, cuda)
    if bf16:
        xt, yt = xt.bfloat16(), yt.bfloat16()
    out, mass = hip.plan_apply_sparse(eps, xt, yt, _t(h, cuda), _t(feat, cuda), _ranges(blocks, cuda), flags=flags, want_mass=True)
    ref, live = _ref(xt.float().cpu().numpy(), yt.float().cpu().numpy(), h, eps, feat, _mask(blocks, len(x), len(y)))
    return out.cpu().numpy(), mass.cpu().numpy(), ref, live


PARITY = [(D, V, flags, False) for D, V in [(1, 1), (3, 33), (3, 129), (8, 40), (16, 31)] for flags in (0, hip.FLAG_F16X2, hip.FLAG_NO_SPLIT)]


@pytest.mark.parametrize("D,V,flags,bf16", PARITY + [(3, 33, 0, True)])
def test_parity(cuda, D, V, flags, bf16):
    x, y, h, feat = _case(D, V)
    out, mass, ref, live = _run(cuda, x, y, h, feat, _eps(D), BLOCKS, flags, bf16)
    err = (np.abs(out - ref) / np.abs(feat[np.isfinite(h)]).max(0)).max()
    print(f"sparse parity D={D} V={V} flags={flags} bf16={bf16}: {err:.2e}, |mass - 1| {np.abs(mass[live] - 1).max():.2e}")
    assert out.shape == (N, V) and np.isfinite(out).all()
    assert err <= 2e-5
    assert np.abs(mass[live] - 1.0).max() <= 1e-4
    # the empty slice and the rows of no block: exactly 0, written by the launch
    assert live.sum() == N - 80 - 30 and (out[~live] == 0.0).all() and (mass[~live] == 0.0).all()


def test_one_hot_rows_are_exact(cuda):
    """tests/test_plan_apply_gpu.py::test_operand_order on ranges: integer features of one-hot rows come back bit for bit."""
    n = 96
    rng = np.random.default_rng(5)
    gx, gy = np.meshgrid(np.arange(12), np.arange(8), indexing="ij")
    y = (np.stack([gx.ravel(), gy.ravel()], 1) / 12.0 + rng.random((n, 2)) * 0.01).astype(np.float32)
    perm = rng.permutation(n)
    feat = (1000.0 * np.arange(n)[:, None] + np.arange(64)[None, :]).astype(np.float32)
    rg = _ranges([((0, 50), [(0, 96)]), ((50, 96), [(0, 40), (40, 96)])], cuda)
    out = hip.plan_apply_sparse(1e-5, _t(y[perm], cuda), _t(y, cuda), torch.zeros(n, device=cuda), _t(feat, cuda), rg).cpu().numpy()
    assert (out == feat[perm]).all(), np.argwhere(out != feat[perm])[:1]


def test_one_range_is_the_dense_plan(cuda):
    x, y, h, feat = _case(3, 33)
    args = (0.01, _t(x, cuda), _t(y, cuda), _t(h, cuda), _t(feat, cuda))
    rg = _ranges([((0, N), [(0, M)])], cuda)
    one, again, dense = hip.plan_apply_sparse(*args, rg), hip.plan_apply_sparse(*args, rg), hip.plan_apply(*args)
    err = float(((one - dense).abs().max(0).values / _t(np.abs(feat[np.isfinite(h)]).max(0), cuda)).max())
    print(f"one range against the dense kernel: {err:.2e}")
    assert err <= 2e-5 and torch.equal(one, again)


def test_barycentric_map_through_the_helper(cuda):
    """N = M = 6000, D = 3, blur 0.05 (eps = 0.0025, a quarter of the parity tests'; the offsets from a chunk's first row are cluster
    diameters, more than four times shorter than the unit cube's, so the exponents are no worse and the bound stays 2e-5 max |y|).
    The masked float64 reference is computed in the CALLER's order: it checks the un-permutation too."""
    n, blur = 6000, 0.05
    x, y, _ = _clouds(7, n, n, 3)
    xt, yt = _t(x, cuda), _t(y, cuda)
    F, G = (t.reshape(-1) for t in SamplesLoss("sinkhorn", p=2, blur=blur, debias=False, potentials=True, backend="online")(xt, yt))
    px, py, rg = transport.plan_ranges(xt, yt, F, G, blur)
    T = torch.empty_like(xt)
    T[px] = transport.barycentric_map(xt[px], yt[py], F[px], G[py], blur, ranges=rg)
    blocks, q0 = [], 0
    for (r0, r1), q1 in zip(rg.ranges_i.tolist(), rg.slices_i.tolist()):
        blocks.append(((r0, r1), rg.redranges_j[q0:q1].tolist()))
        q0 = q1
    K = np.zeros((n, n), dtype=bool)
    K[np.ix_(px.cpu().numpy(), py.cpu().numpy())] = _mask(blocks, n, n)
    ref, live = _ref(x, y, G.cpu().numpy() / blur**2, blur**2, y, K)
    err = np.abs(T.cpu().numpy() - ref).max() / np.abs(y).max()
    print(f"helper: {len(blocks)} row blocks, kept {K.mean():.3f} of the pairs, error {err:.2e}")
    assert live.all() and 0.0 < K.mean() < 0.5 and err <= 2e-5


def test_refusals(cuda):
    x, y, h = (_t(a, cuda) for a in _clouds(1, 40, 50, 3))
    feat, rg = torch.ones(50, 2, device=cuda), _ranges([((0, 40), [(0, 50)])], cuda)
    assert hip.plan_apply_sparse_applies(x, rg) and not hip.plan_apply_sparse_applies(x, None)
    x17, y17 = torch.rand(40, 17, device=cuda), torch.rand(50, 17, device=cuda)
    for bad in (lambda: hip.plan_apply_sparse(0.01, x, y, h, feat, rg, p=1),
                lambda: hip.plan_apply_sparse(0.01, x17, y17, h, feat, rg),
                lambda: hip.plan_apply_sparse(0.01, x.double(), y.double(), h, feat, rg),
                lambda: hip.plan_apply_sparse(0.01, x[None], y[None], h[None], feat[None], rg),
                lambda: hip.plan_apply_sparse_raw(x17[None], y17[None], h[None], torch.zeros(1, 40, device=cuda), feat[None], 0.01, rg),
                lambda: transport.barycentric_map(x.clone().requires_grad_(), y, h, h, 0.1, ranges=rg),
                lambda: transport.apply_plan(x, y, torch.zeros(40, device=cuda), h, feat.requires_grad_(), 0.1, ranges=rg)):
        with pytest.raises(NotImplementedError):
            bad()
