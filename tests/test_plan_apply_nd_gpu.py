"""``hip.plan_apply_nd`` / ``glhip_plan_apply_nd`` for clouds of 17 <= D <= 4095 (geomloss_amd/csrc/glhip_plan_apply_xk.h): the plan of a
p = 2 soft-min applied to a feature matrix on the matrix cores, against a float64 NumPy reference W = exp(E - lse(E)), ref = W @ feat.

The float64 reference ``_ref``, ``_clouds`` and the ``_worst`` measure are those of tests/test_plan_apply_gpu.py (tests/cloud_support.py);
``_eps`` restates it for D >= 17.  Acceptance bound, per feature column: |out - ref|[:, v] <= 2e-5 max_j |feat[j, v]| and
|mass - 1| <= 1e-4, the project's bars for these plan weights at
eps = 0.1 D / 3 (diam^2 / eps <= 30: the f16 range contract holds); 1e-4 for the many-column launch at eps = 0.05^2 D."""
import numpy as np
import pytest
import torch

from cloud_support import clouds as _clouds, plan_apply as _apply, plan_ref as _ref, plan_worst as _worst, to_dev as _t
from geomloss_amd import hip

pytestmark = pytest.mark.gpu


def _eps(D):
    return 0.1 * D / 3


def _torch_f32_error(dev, x, y, h, eps, feat, ref):
    """The error of the same product in plain float32 torch (dense cost, softmax @ feat) against the float64 reference."""
    xt, yt, ht, ft = (_t(a, dev) for a in (x, y, h, feat))
    C = (xt * xt).sum(1)[:, None] - 2.0 * xt @ yt.t() + (yt * yt).sum(1)[None, :]
    out = torch.softmax(ht[None, :] - C / (2.0 * eps), dim=1) @ ft
    return _worst(out.cpu().numpy(), ref, feat)


FLAGS = [0, hip.FLAG_NO_SPLIT, hip.FLAG_F16X2, hip.FLAG_F16X2 | hip.FLAG_NO_SPLIT]
# (270, 310, 17, 5): the first dimension — f16 x 2 needs 4 MFMAs, less than one stage; bf16 x 3 needs 7, two stages
# (300, 257, 31, 33): bf16 x 3: exactly two full stages; a one-column tile; a one-feature remainder pass
# (97, 513, 32, 31): a third stage of one chunk          (257, 300, 40, 129): a one-row second row block; several passes
# (64, 8, 64, 1): M below one column group               (1, 1, 100, 3): single row, single column          (130, 600, 300, 40): long chain
SHAPES = [(270, 310, 17, 5), (300, 257, 31, 33), (97, 513, 32, 31), (257, 300, 40, 129), (64, 8, 64, 1), (1, 1, 100, 3), (130, 600, 300, 40)]
_REFS = {}


def _parity_case(N, M, D, V):      # inputs and the float64 reference, computed once for the four flag settings
    key = (N, M, D, V)
    if key not in _REFS:
        x, y, h = _clouds(N + M + D, N, M, D)
        feat = np.random.default_rng(V).standard_normal((M, V)).astype(np.float32)
        _REFS[key] = (x, y, h, feat, _ref(x, y, h, _eps(D), feat))
    return _REFS[key]


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("N,M,D,V", SHAPES)
def test_parity(cuda, N, M, D, V, flags):
    """Measured worst case per dimension on an MI355X: see DESIGN §4."""
    x, y, h, feat, ref = _parity_case(N, M, D, V)
    out, mass = _apply(cuda, x, y, h, feat, _eps(D), flags, raw=hip.plan_apply_nd_raw)
    err = _worst(out, ref, feat)
    print(f"parity N={N} M={M} D={D} V={V} flags={flags}: {err:.2e}, |mass - 1| {np.abs(mass - 1).max():.2e}")
    assert out.shape == (N, V) and np.isfinite(out).all()
    bound = 2e-5
    if err > bound and D > 64:      # the rule of test_softmin_gradient_any_dimension: four times what plain float32 makes of the same product
        e_ref = _torch_f32_error(cuda, x, y, h, _eps(D), feat, ref)
        bound = max(2e-5, 4.0 * e_ref)
        print(f"  float32 torch on the same inputs: {e_ref:.2e} -> bound {bound:.2e}")
    assert err <= bound
    assert np.abs(mass - 1.0).max() <= 1e-4


def test_batched_bf16(cuda):
    B, N, M, D, V = 3, 200, 260, 48, 20
    x, y, h = _clouds(11, N, M, D, B=B)
    feat = np.random.default_rng(2).standard_normal((B, M, V)).astype(np.float32)
    xt, yt = _t(x, cuda).bfloat16(), _t(y, cuda).bfloat16()
    x, y = xt.float().cpu().numpy(), yt.float().cpu().numpy()      # the reference sees the bf16-rounded points
    out = hip.plan_apply_nd(_eps(D), xt, yt, _t(h, cuda), _t(feat, cuda))
    assert out.shape == (B, N, V) and out.dtype == torch.float32 and out.grad_fn is None
    out = out.cpu().numpy()
    errs = [_worst(out[b], _ref(x[b], y[b], h[b], _eps(D), feat[b]), feat[b]) for b in range(B)]
    print(f"batched bf16: {errs}")
    assert max(errs) <= 2e-5


def test_operand_order(cuda):
    """One-hot plan rows and integer features: a wrong K permutation or register-to-feature map gives wrong integers, and the
    position of the first one names the lane.  Exact because the kernel takes its weights relative to the running maximum of the row."""
    n, D = 96, 40
    rng = np.random.default_rng(5)
    y = rng.random((n, D)).astype(np.float32)
    perm = rng.permutation(n)
    x = y[perm]
    feat = (1000.0 * np.arange(n)[:, None] + np.arange(64)[None, :]).astype(np.float32)
    out = hip.plan_apply_nd(1e-3, _t(x, cuda), _t(y, cuda), torch.zeros(n, device=cuda), _t(feat, cuda)).cpu().numpy()
    want = feat[perm]
    bad = np.argwhere(out != want)
    print(f"operand order: {len(bad)} of {out.size} entries differ, max |out - want| {np.abs(out - want).max():.3e}")
    assert len(bad) == 0, f"first wrong (row, feature) {bad[0]}: got {out[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}"


@pytest.mark.parametrize("flags", [0, hip.FLAG_F16X2])
def test_massless_rows_and_columns(cuda, flags):
    B, N, M, D, V = 2, 257, 300, 24, 10
    x, y, h = _clouds(21, N, M, D, B=B)
    feat = np.random.default_rng(6).standard_normal((B, M, V)).astype(np.float32)
    h[0, ::3] = -np.inf                      # a third of the columns carry no mass ...
    feat[0, ::3] = 1e4                       # ... whatever (finite) features they hold
    h[1, :] = -np.inf                        # a batch item without any mass
    out, mass = _apply(cuda, x, y, h, feat, _eps(D), flags, raw=hip.plan_apply_nd_raw)
    assert np.isfinite(out).all() and np.isfinite(mass).all()
    err = _worst(out[0], _ref(x[0], y[0], h[0], _eps(D), np.where(np.isfinite(h[0])[:, None], feat[0], 0.0)), feat[0, 1::3])
    print(f"massless columns, flags={flags}: {err:.2e}")
    assert err <= 2e-5 and np.abs(mass[0] - 1.0).max() <= 1e-4
    assert (out[1] == 0.0).all() and (mass[1] == 0.0).all()


def test_column_splits(cuda):
    N, M, D, V = 130, 70001, 24, 16
    x, y, h = _clouds(D, N, M, D)
    feat = np.random.default_rng(V).standard_normal((M, V)).astype(np.float32)
    eps = 0.05**2 * D
    ref = _ref(x, y, h, eps, feat)
    split, m0 = _apply(cuda, x, y, h, feat, eps, 0, raw=hip.plan_apply_nd_raw)
    unsplit, m1 = _apply(cuda, x, y, h, feat, eps, hip.FLAG_NO_SPLIT, raw=hip.plan_apply_nd_raw)
    nows, m2 = _apply(cuda, x, y, h, feat, eps, 0, workspace=False, raw=hip.plan_apply_nd_raw)
    errs = [_worst(o, ref, feat) for o in (split, unsplit, nows)]
    print(f"splits N={N} M={M} D={D} V={V}: vs reference {errs}, split vs unsplit {_worst(split, unsplit, feat):.2e}")
    assert max(errs) <= 1e-4
    assert max(np.abs(m - 1.0).max() for m in (m0, m1, m2)) <= 1e-4


def test_continuity_with_the_resident_operand_kernel(cuda):
    N, M, D, V = 97, 513, 16, 31
    x, y, h = _clouds(N + M + D, N, M, D)
    feat = np.random.default_rng(V).standard_normal((M, V)).astype(np.float32)
    eps = _eps(D)
    nd, mnd = _apply(cuda, x, y, h, feat, eps, raw=hip.plan_apply_nd_raw)
    xd, mxd = _apply(cuda, x, y, h, feat, eps, raw=hip.plan_apply_raw)
    assert np.array_equal(nd, xd) and np.array_equal(mnd, mxd)      # the very same launch
    pad = lambda a: np.concatenate([a, np.zeros((a.shape[0], 1), np.float32)], 1)  # noqa: E731
    xk, _ = _apply(cuda, pad(x), pad(y), h, feat, eps, raw=hip.plan_apply_nd_raw)
    err = _worst(xk, xd, feat)
    print(f"continuity D=16 -> 17: {err:.2e}")
    assert err <= 4e-5


@pytest.mark.parametrize("D", [40, 100])
def test_cross_check_against_the_gradient_kernel(cuda, D):
    """d softmin_i / d x_i = x_i - sum_j P_ij y_j comes from the one-thread-per-row kernel of glhip_generic.h.  The two errors against
    float64 printed here are what routing that gradient through the plan application would trade."""
    N, M = 300, 517
    x, y, h = _clouds(D, N, M, D)
    eps = _eps(D)
    xt, yt, ht = _t(x, cuda).requires_grad_(), _t(y, cuda), _t(h, cuda)
    out = hip.softmin(eps, xt, yt, ht)
    (g,) = torch.autograd.grad(out, [xt], grad_outputs=torch.ones_like(out))
    mine = xt.detach() - hip.plan_apply_nd(eps, xt.detach(), yt, ht, yt)
    g64 = x.astype(np.float64) - _ref(x, y, h, eps, y)
    e_plan, e_grad = np.abs(mine.cpu().numpy() - g64).max(), np.abs(g.cpu().numpy() - g64).max()
    bound = 2e-5 * (float(yt.abs().max()) + float(g.abs().max()))
    err = float((mine - g).abs().max())
    print(f"cross-check D={D}: {err:.2e} (bound {bound:.2e}); against float64: plan application {e_plan:.2e}, gradient kernel {e_grad:.2e}")
    assert err <= bound


def test_refusals(cuda):
    x, y, h = (_t(a, cuda) for a in _clouds(1, 40, 50, 24))
    feat = torch.ones(50, 2, device=cuda)
    with pytest.raises(NotImplementedError):
        hip.plan_apply_nd(0.8, x, y, h, feat, p=1)
    with pytest.raises(NotImplementedError):
        hip.plan_apply_nd(0.8, x.double(), y.double(), h, feat)
    rng = hip.BlockRanges(*[torch.zeros(2, dtype=torch.int32, device=cuda)] * 6)
    with pytest.raises(NotImplementedError):
        hip.plan_apply_nd(0.8, x, y, h, feat, ranges=rng)
    with pytest.raises(NotImplementedError):
        hip.plan_apply_nd(100.0, torch.rand(40, 4096, device=cuda), torch.rand(50, 4096, device=cuda), h, feat)
    with pytest.raises(ValueError):
        hip.plan_apply_nd(0.8, x, y, h, torch.ones(49, 2, device=cuda))
    # the library itself refuses the same through its return codes
    fwd = torch.zeros(1, 40, device=cuda)
    with pytest.raises(NotImplementedError):
        hip.plan_apply_nd_raw(x[None], y[None], h[None], fwd, feat[None], 0.8, p=1)
    x4096, y4096 = torch.rand(1, 40, 4096, device=cuda), torch.rand(1, 50, 4096, device=cuda)
    with pytest.raises(NotImplementedError):
        hip.plan_apply_nd_raw(x4096, y4096, h[None], fwd, feat[None], 100.0)
    assert not hip.plan_apply_nd_applies(x4096[0]) and hip.plan_apply_nd_applies(x) and not hip.plan_apply_nd_applies(x, p=1)


@pytest.mark.parametrize("D", [8, 24])
def test_empty_plans_and_features(cuda, D):
    """M == 0 or V == 0 with N > 0: out and mass are zeroed; N == 0: nothing to write."""
    N = 40
    x = torch.rand(1, N, D, device=cuda)
    fwd = torch.zeros(1, N, device=cuda)
    out, mass = hip.plan_apply_nd_raw(x, torch.rand(1, 50, D, device=cuda), torch.zeros(1, 50, device=cuda), fwd,
                                      torch.ones(1, 50, 0, device=cuda), _eps(D), want_mass=True)
    assert out.shape == (1, N, 0) and (mass == 0).all()
    out, mass = hip.plan_apply_nd_raw(x, torch.rand(1, 0, D, device=cuda), torch.zeros(1, 0, device=cuda), fwd,
                                      torch.ones(1, 0, 3, device=cuda), _eps(D), want_mass=True)
    assert (out == 0).all() and (mass == 0).all()
    out = hip.plan_apply_nd_raw(x[:, :0], torch.rand(1, 50, D, device=cuda), torch.zeros(1, 50, device=cuda), fwd[:, :0],
                                torch.ones(1, 50, 3, device=cuda), _eps(D))
    assert out.shape == (1, 0, 3)
