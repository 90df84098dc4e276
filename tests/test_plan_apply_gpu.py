"""``hip.plan_apply`` / ``glhip_plan_apply`` (geomloss_amd/csrc/glhip_plan_apply.h): the plan of a p = 2 soft-min applied to a feature
matrix on the matrix cores, against a float64 NumPy reference W = exp(E - lse(E)), ref = W @ feat.

Acceptance bound, per feature column: |out - ref|[:, v] <= tol * max_j |feat[j, v]|, with tol from the project's own bars for these plan
weights (tests/test_xd_kernels_gpu.py::test_softmin_gradient_transposed_kernel): 2e-5 at eps = 0.01 (D <= 3) / eps = 0.1 D / 3 (D >= 4),
1e-4 for the many-column launches at eps = 0.05^2 D."""
import numpy as np
import pytest
import torch

from cloud_support import clouds as _clouds, plan_apply as _apply, plan_ref as _ref, plan_worst as _worst, to_dev as _t
from geomloss_amd import hip

pytestmark = pytest.mark.gpu


def _eps(D):
    return 0.01 if D <= 3 else 0.1 * D / 3


SHAPES = [(300, 257, 3, 1), (1030, 1100, 2, 33), (200, 300, 1, 32), (64, 8, 3, 5), (1, 1, 3, 3), (5, 3000, 2, 70), (130, 600, 8, 40),
          (97, 513, 16, 31), (257, 300, 5, 129)]
_REFS = {}


def _parity_case(N, M, D, V):      # inputs and the float64 reference, computed once for the four flag settings
    key = (N, M, D, V)
    if key not in _REFS:
        x, y, h = _clouds(N + M + D, N, M, D)
        feat = np.random.default_rng(V).standard_normal((M, V)).astype(np.float32)
        _REFS[key] = (x, y, h, feat, _ref(x, y, h, _eps(D), feat))
    return _REFS[key]


@pytest.mark.parametrize("flags", [0, hip.FLAG_NO_SPLIT, hip.FLAG_F16X2, hip.FLAG_F16X2 | hip.FLAG_NO_SPLIT])
@pytest.mark.parametrize("N,M,D,V", SHAPES)
def test_parity(cuda, N, M, D, V, flags):
    """Measured worst case over all shapes and flags on an MI355X: see DESIGN §4."""
    x, y, h, feat, ref = _parity_case(N, M, D, V)
    out, mass = _apply(cuda, x, y, h, feat, _eps(D), flags, raw=hip.plan_apply_raw)
    err = _worst(out, ref, feat)
    print(f"parity N={N} M={M} D={D} V={V} flags={flags}: {err:.2e}, |mass - 1| {np.abs(mass - 1).max():.2e}")
    assert out.shape == (N, V) and np.isfinite(out).all()
    assert err <= 2e-5
    assert np.abs(mass - 1.0).max() <= 1e-4


def test_operand_order(cuda):
    """One-hot plan rows and integer features: a wrong K permutation or register-to-feature map gives wrong integers, and the
    position of the first one names the lane.  Exact because the kernel takes its weights relative to the running maximum of the row:
    the one weight of a row is 2^13 bit for bit, whatever the float32 error of the exponent it came from."""
    n = 96
    rng = np.random.default_rng(5)
    gx, gy = np.meshgrid(np.arange(12), np.arange(8), indexing="ij")
    y = (np.stack([gx.ravel(), gy.ravel()], 1) / 12.0 + rng.random((n, 2)) * 0.01).astype(np.float32)
    perm = rng.permutation(n)
    x = y[perm]
    feat = (1000.0 * np.arange(n)[:, None] + np.arange(64)[None, :]).astype(np.float32)
    out = hip.plan_apply(1e-5, _t(x, cuda), _t(y, cuda), torch.zeros(n, device=cuda), _t(feat, cuda)).cpu().numpy()
    want = feat[perm]
    bad = np.argwhere(out != want)
    print(f"operand order: {len(bad)} of {out.size} entries differ, max |out - want| {np.abs(out - want).max():.3e}, "
          f"rounded map equal: {bool((np.rint(out) == want).all())}")
    assert (np.rint(out) == want).all(), f"wrong feature at (row, feature) {bad[0]}: got {out[tuple(bad[0])]}, want {want[tuple(bad[0])]}"
    assert len(bad) == 0, f"first inexact entry (row, feature) {bad[0]}: got {out[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}"


@pytest.mark.parametrize("N,M,D,V", [(300, 70001, 3, 33), (130, 70001, 8, 16)])
def test_column_splits_and_long_reductions(cuda, N, M, D, V):
    x, y, h = _clouds(D, N, M, D)
    feat = np.random.default_rng(V).standard_normal((M, V)).astype(np.float32)
    eps = 0.05**2 * D
    ref = _ref(x, y, h, eps, feat)
    split, m0 = _apply(cuda, x, y, h, feat, eps, 0, raw=hip.plan_apply_raw)
    unsplit, m1 = _apply(cuda, x, y, h, feat, eps, hip.FLAG_NO_SPLIT, raw=hip.plan_apply_raw)
    nows, m2 = _apply(cuda, x, y, h, feat, eps, 0, workspace=False, raw=hip.plan_apply_raw)
    errs = [_worst(o, ref, feat) for o in (split, unsplit, nows)]
    agree = max(_worst(split, unsplit, feat), _worst(split, nows, feat))
    print(f"splits N={N} M={M} D={D} V={V}: vs reference {errs}, split vs unsplit {agree:.2e}")
    assert max(errs) <= 1e-4
    assert agree <= 2e-6
    assert max(np.abs(m - 1.0).max() for m in (m0, m1, m2)) <= 1e-4


def test_feature_range(cuda):
    N, M, D = 300, 257, 3
    x, y, h = _clouds(0, N, M, D)
    feat = np.random.default_rng(1).standard_normal((M, 6)).astype(np.float32)
    feat[:, 0] *= 1e12
    feat[:, 1] *= 1e-12
    feat[:, 3] = 0.0
    feat[:, 4] = 2.5
    feat[:, 5] = np.abs(feat[:, 5])
    ref = _ref(x, y, h, 0.01, feat)
    out, _ = _apply(cuda, x, y, h, feat, 0.01, raw=hip.plan_apply_raw)
    per_col = np.abs(out - ref).max(0) / np.where(np.abs(feat).max(0) > 0, np.abs(feat).max(0), 1.0)
    print(f"feature range: per column {per_col}, constant column {np.abs(out[:, 4] / 2.5 - 1).max():.2e}")
    assert (per_col <= 2e-5).all()
    assert (out[:, 3] == 0.0).all()
    assert np.abs(out[:, 4] / 2.5 - 1.0).max() <= 2e-6
    assert (out[:, 5] >= 0.0).all()


@pytest.mark.parametrize("bf16", [False, True])
def test_batched_and_bf16(cuda, bf16):
    B, N, M, D, V = 3, 257, 300, 3, 10
    x, y, h = _clouds(11, N, M, D, B=B)
    feat = np.random.default_rng(2).standard_normal((B, M, V)).astype(np.float32)
    xt, yt = _t(x, cuda), _t(y, cuda)
    if bf16:
        xt, yt = xt.bfloat16(), yt.bfloat16()
        x, y = xt.float().cpu().numpy(), yt.float().cpu().numpy()      # the reference sees the bf16-rounded points
    out = hip.plan_apply(0.01, xt, yt, _t(h, cuda), _t(feat, cuda))
    assert out.shape == (B, N, V) and out.dtype == torch.float32 and out.grad_fn is None
    out = out.cpu().numpy()
    errs = [_worst(out[b], _ref(x[b], y[b], h[b], 0.01, feat[b]), feat[b]) for b in range(B)]
    print(f"batched bf16={bf16}: {errs}")
    assert max(errs) <= 2e-5


def test_public_shapes(cuda):
    N, M, D = 70, 90, 3
    x, y, h = _clouds(4, N, M, D)
    feat = np.random.default_rng(3).standard_normal((M, 4)).astype(np.float32)
    xt, yt, ht, ft = (_t(a, cuda) for a in (x, y, h, feat))
    ref = _ref(x, y, h, 0.01, feat)
    mat = hip.plan_apply(0.01, xt.requires_grad_(), yt, ht, ft)
    vec = hip.plan_apply(0.01, xt, yt, ht, ft[:, 0])
    fwd = hip.softmin(0.01, xt.detach(), yt, ht)
    again = hip.plan_apply(0.01, xt, yt, ht, ft, fwd=fwd)
    assert mat.shape == (N, 4) and vec.shape == (N,) and mat.grad_fn is None and not mat.requires_grad
    assert _worst(mat.cpu().numpy(), ref, feat) <= 2e-5
    assert torch.equal(vec, mat[:, 0]) and torch.equal(again, mat)


@pytest.mark.parametrize("flags", [0, hip.FLAG_F16X2])
def test_special_values(cuda, flags):
    B, N, M, D, V = 2, 257, 300, 3, 10
    x, y, h = _clouds(21, N, M, D, B=B)
    feat = np.random.default_rng(6).standard_normal((B, M, V)).astype(np.float32)
    h[0, ::3] = -np.inf                      # a third of the columns carry no mass ...
    feat[0, ::3] = 1e4                       # ... whatever (finite) features they hold
    h[1, :] = -np.inf                        # a batch item without any mass
    out, mass = _apply(cuda, x, y, h, feat, 0.01, flags, raw=hip.plan_apply_raw)
    assert np.isfinite(out).all() and np.isfinite(mass).all()
    err = _worst(out[0], _ref(x[0], y[0], h[0], 0.01, np.where(np.isfinite(h[0])[:, None], feat[0], 0.0)), feat[0, 1::3])
    print(f"special values: masked columns {err:.2e}")
    assert err <= 2e-5 and np.abs(mass[0] - 1.0).max() <= 1e-4
    assert (out[1] == 0.0).all() and (mass[1] == 0.0).all()


def test_offset_clouds(cuda):
    N, M, D, V = 300, 257, 3, 10
    x, y, h = _clouds(8, N, M, D, offset=1000.0)
    feat = np.random.default_rng(7).standard_normal((M, V)).astype(np.float32)
    eps = 0.05**2
    out, mass = _apply(cuda, x, y, h, feat, eps, raw=hip.plan_apply_raw)
    err = _worst(out, _ref(x, y, h, eps, feat), feat)
    print(f"offset clouds: {err:.2e}")
    assert err <= 1e-4


@pytest.mark.parametrize("D", [3, 8])
def test_cross_check_against_the_gradient_kernels(cuda, D):
    """d softmin_i / d x_i = x_i - sum_j P_ij y_j comes from wsum_mfma_kernel (D = 3) / wsum_t32_kernel (D = 8)."""
    N, M = 300, 517
    x, y, h = _clouds(D, N, M, D)
    eps = _eps(D)
    xt, yt, ht = _t(x, cuda).requires_grad_(), _t(y, cuda), _t(h, cuda)
    out = hip.softmin(eps, xt, yt, ht)
    (g,) = torch.autograd.grad(out, [xt], grad_outputs=torch.ones_like(out))
    mine = xt.detach() - hip.plan_apply(eps, xt.detach(), yt, ht, yt)
    bound = 2e-5 * (float(yt.abs().max()) + float(g.abs().max()))
    err = float((mine - g).abs().max())
    print(f"cross-check D={D}: {err:.2e} (bound {bound:.2e})")
    assert err <= bound


def test_refusals(cuda):
    x, y, h = (_t(a, cuda) for a in _clouds(1, 40, 50, 3))
    feat = torch.ones(50, 2, device=cuda)
    with pytest.raises(NotImplementedError):
        hip.plan_apply(0.01, x, y, h, feat, p=1)
    with pytest.raises(NotImplementedError):
        hip.plan_apply(0.01, torch.rand(40, 17, device=cuda), torch.rand(50, 17, device=cuda), h, feat)
    with pytest.raises(NotImplementedError):
        hip.plan_apply(0.01, x.double(), y.double(), h, feat)
    rng = hip.BlockRanges(*[torch.zeros(2, dtype=torch.int32, device=cuda)] * 6)
    with pytest.raises(NotImplementedError):
        hip.plan_apply(0.01, x, y, h, feat, ranges=rng)
    with pytest.raises(ValueError):
        hip.plan_apply(0.01, x, y, h, torch.ones(49, 2, device=cuda))
    # the library itself refuses the same through its return codes
    fwd = torch.zeros(1, 40, device=cuda)
    with pytest.raises(NotImplementedError):
        hip.plan_apply_raw(x[None], y[None], h[None], fwd, feat[None], 0.01, p=1)
    x17, y17 = torch.rand(1, 40, 17, device=cuda), torch.rand(1, 50, 17, device=cuda)
    with pytest.raises(NotImplementedError):
        hip.plan_apply_raw(x17, y17, h[None], fwd, feat[None], 0.01)
