"""``hip.plan_apply_p1`` / ``glhip_plan_apply_p1`` for clouds of 1 <= D <= 4095 (geomloss_amd/csrc/glhip_dist_plan_xk.h): the plan of a
p = 1 soft-min applied to a feature matrix on the matrix cores, against a float64 NumPy reference on explicit differences,

    d = sqrt(max(sum((x_i - y_j)^2), 1e-8)),   W = exp(h - d / eps - rowmax),   ref = (W / W.sum) @ feat,   softmin = -eps log sum exp(h - d / eps).

Measure (tests/test_plan_apply_nd_gpu.py): per feature column max_i |out - ref| / max_j |feat[j, v]|.  Input law: that of
tests/test_dist_xk_gpu.py::_law (per-coordinate scales), eps = 0.05 sqrt(D) unless said otherwise.  Bounds: 2e-5 on ``out``, the
project's bar for plan weights — for D > 64 only, max(2e-5, 4 x the error of plain float32 torch on the same inputs: torch.cdist in its
matrix-multiply mode, clamped at 1e-4, softmax @ feat); 12 x 2e-6 max(1, |ref|max) on ``softmin``, the bound test_dist_xk_gpu.py holds
this chain's soft-min to.  Every test prints its worst error over the bound (``pytest -s``); the values are in profiles/dist_plan_xk.txt."""
import numpy as np
import pytest
import torch

from cloud_support import to_dev as _t
from geomloss_amd import hip

pytestmark = pytest.mark.gpu

BOUND = 2e-5


def _law(rng, N, M, D):
    """the input law of tests/test_dist_xk_gpu.py (per-coordinate scales: coordinates are not exchangeable)"""
    s = 0.5 + 0.5 * rng.random(D)
    x = (rng.random((N, D)) * s).astype(np.float32)
    y = ((rng.random((M, D)) * 0.8 + 0.1) * s).astype(np.float32)
    h = rng.standard_normal(M).astype(np.float32)
    return x, y, h


def _eps(D):
    return 0.05 * float(np.sqrt(D))


def _ref(x, y, h, eps, feat):
    """float64 on explicit differences, row-chunked: (W / W.sum) @ feat (0 for a row without mass) and the soft-min (+inf there)."""
    x, y, h, feat = (np.asarray(t, dtype=np.float64) for t in (x, y, h, feat))
    N, (M, D) = x.shape[0], y.shape
    out, soft = np.zeros((N, feat.shape[1])), np.full(N, np.inf)
    if M == 0:
        return out, soft
    rows = max(1, int(4e6 // (M * D)))
    for i0 in range(0, N, rows):
        diff = x[i0:i0 + rows, None, :] - y[None, :, :]
        d = np.sqrt(np.maximum((diff * diff).sum(-1), 1e-8))
        E = h[None, :] - d / eps
        m = E.max(1, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)
        W = np.exp(E - m)
        s = W.sum(1, keepdims=True)
        out[i0:i0 + rows] = (W / np.where(s > 0, s, 1.0)) @ np.where(np.isfinite(feat), feat, 0.0)
        with np.errstate(divide="ignore"):
            soft[i0:i0 + rows] = -eps * (np.log(s[:, 0]) + m[:, 0])
    return out, soft


def _apply(dev, x, y, h, feat, eps, flags=0, **kw):
    """Raw launch on (N,D) / (B,N,D) NumPy inputs -> out, softmin as NumPy."""
    xb, yb, hb, fb = (_t(a, dev) for a in (x, y, h, feat))
    if xb.dim() == 2:
        xb, yb, hb, fb = xb[None], yb[None], hb[None], fb[None]
    out, soft = hip.plan_apply_p1_raw(xb, yb, hb, fb, eps, flags, want_softmin=True, **kw)
    out, soft = out.cpu().numpy(), soft.cpu().numpy()
    return (out[0], soft[0]) if np.ndim(x) == 2 else (out, soft)


def _worst(out, ref, feat):
    """max over columns of max_i |out - ref| / max_j |feat_j|."""
    scale = np.abs(feat).reshape(-1, feat.shape[-1]).max(0)
    scale = np.where(scale > 0, scale, 1.0)
    return float((np.abs(out - ref) / scale).max())


def _sbound(ref):
    fin = ref[np.isfinite(ref)]
    return 12 * 2e-6 * max(1.0, float(np.abs(fin).max()) if fin.size else 1.0)


def _torch_f32_error(dev, x, y, h, eps, feat, ref):
    """The error of the same product in plain float32 torch (cdist in its matrix-multiply mode, clamped at 1e-4, softmax @ feat)."""
    xt, yt, ht, ft = (_t(a, dev) for a in (x, y, h, feat))
    d = torch.cdist(xt, yt).clamp_min(1e-4)
    out = torch.softmax(ht[None, :] - d / eps, dim=1) @ ft
    return _worst(out.cpu().numpy(), ref, feat)


def _check(tag, dev, x, y, h, feat, eps, out, soft, ref, sref, D, escape=True, bound=BOUND):
    """Prints the worst errors over their bounds, then asserts them."""
    err, serr = _worst(out, ref, feat), float(np.abs(soft - sref).max())
    if escape and err > bound and D > 64:
        e_ref = _torch_f32_error(dev, x, y, h, eps, feat, ref)
        bound = max(bound, 4.0 * e_ref)
        print(f"  float32 torch on the same inputs: {e_ref:.2e} -> bound {bound:.2e}")
    sb = _sbound(sref)
    print(f"{tag}: out {err:.2e} = {err / bound:.3f} x bound, softmin {serr:.2e} = {serr / sb:.3f} x bound")
    assert np.isfinite(out).all() and np.isfinite(soft).all()
    assert err <= bound
    assert serr <= sb


# the stage, tile, row-block and remainder-pass edges tests/test_plan_apply_nd_gpu.py names, plus the small dimensions (one MFMA at
# D = 1; exactly one stage at D = 15; D = 16, 17 around the forward kernel's first dimension) and the longest chain, D = 4095
SHAPES = [(270, 310, 17, 5), (300, 257, 31, 33), (97, 513, 32, 31), (257, 300, 40, 129), (64, 8, 64, 1), (1, 1, 100, 3), (130, 600, 300, 40),
          (150, 200, 1, 3), (200, 260, 3, 7), (260, 300, 15, 9), (260, 300, 16, 9), (70, 90, 4095, 2)]
_REFS = {}


def _parity_case(N, M, D, V, eps):      # inputs and the float64 reference, computed once for both flag settings
    key = (N, M, D, V, eps)
    if key not in _REFS:
        x, y, h = _law(np.random.default_rng(N + M + D), N, M, D)
        feat = np.random.default_rng(V).standard_normal((M, V)).astype(np.float32)
        _REFS[key] = (x, y, h, feat) + _ref(x, y, h, eps, feat)
    return _REFS[key]


@pytest.mark.parametrize("flags", [0, hip.FLAG_NO_SPLIT])
@pytest.mark.parametrize("N,M,D,V", SHAPES)
def test_parity(cuda, N, M, D, V, flags):
    eps = _eps(D)
    x, y, h, feat, ref, sref = _parity_case(N, M, D, V, eps)
    out, soft = _apply(cuda, x, y, h, feat, eps, flags)
    assert out.shape == (N, V) and soft.shape == (N,)
    _check(f"parity N={N} M={M} D={D} V={V} flags={flags}", cuda, x, y, h, feat, eps, out, soft, ref, sref, D)


@pytest.mark.parametrize("flags", [0, hip.FLAG_NO_SPLIT])
@pytest.mark.parametrize("N,M,D,V", SHAPES[:4])
def test_small_blur(cuda, N, M, D, V, flags):
    eps = 0.05
    x, y, h, feat, ref, sref = _parity_case(N, M, D, V, eps)
    out, soft = _apply(cuda, x, y, h, feat, eps, flags)
    _check(f"small blur N={N} M={M} D={D} V={V} flags={flags}", cuda, x, y, h, feat, eps, out, soft, ref, sref, D)


@pytest.mark.parametrize("D", [40, 3])
def test_operand_order(cuda, D):
    """One-hot plan rows and integer features: a wrong K permutation or register-to-feature map gives wrong integers, and the
    position of the first one names the lane.  Exact because the kernel takes its weights relative to the running maximum of the row.
    D = 3: points on a grid of spacing 0.1, so that no two are closer than 100 eps."""
    n = 96
    rng = np.random.default_rng(5)
    if D == 40:
        y = rng.random((n, D)).astype(np.float32)
    else:
        cells = rng.permutation(1000)[:n]
        y = (0.1 * np.stack([cells // 100, (cells // 10) % 10, cells % 10], 1)).astype(np.float32)
    perm = rng.permutation(n)
    x = y[perm]
    feat = (1000.0 * np.arange(n)[:, None] + np.arange(64)[None, :]).astype(np.float32)
    out = hip.plan_apply_p1(1e-3, _t(x, cuda), _t(y, cuda), torch.zeros(n, device=cuda), _t(feat, cuda)).cpu().numpy()
    want = feat[perm]
    bad = np.argwhere(out != want)
    print(f"operand order D={D}: {len(bad)} of {out.size} entries differ, max |out - want| {np.abs(out - want).max():.3e}")
    assert len(bad) == 0, f"first wrong (row, feature) {bad[0]}: got {out[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}"


@pytest.mark.parametrize("D", [3, 17, 40, 130])
def test_near_pairs_carry_the_mass(cuda, D):
    """Every row's mass sits on four columns 1e-3 away: the expanded form has lost its bits there.  Fails whenever the guard, the exact
    re-evaluation or its row / column index map is wrong (a float32 model of the kernel: 8e-8 ... 2.4e-7 with the repair, 5e-3 ... 1e-2
    without).  No float32-torch escape here."""
    N, V = 300, 6
    rng = np.random.default_rng(D)
    x, _, _ = _law(rng, N, 1, D)
    y = (np.repeat(x, 4, axis=0) + 1e-3 * rng.standard_normal((4 * N, D))).astype(np.float32)
    h = rng.standard_normal(4 * N).astype(np.float32)
    feat = rng.standard_normal((4 * N, V)).astype(np.float32)
    eps = 1e-3 * float(np.sqrt(D))
    ref, sref = _ref(x, y, h, eps, feat)
    out, soft = _apply(cuda, x, y, h, feat, eps)
    _check(f"near pairs D={D}", cuda, x, y, h, feat, eps, out, soft, ref, sref, D, escape=False)


def test_self_plan(cuda):
    """y = x: the diagonal sits on the clamp."""
    N, D, V = 300, 17, 6
    rng = np.random.default_rng(17)
    x, _, _ = _law(rng, N, 1, D)
    h = rng.standard_normal(N).astype(np.float32)
    feat = rng.standard_normal((N, V)).astype(np.float32)
    ref, sref = _ref(x, x, h, 0.05, feat)
    out, soft = _apply(cuda, x, x, h, feat, 0.05)
    _check("self-plan D=17", cuda, x, x, h, feat, 0.05, out, soft, ref, sref, D, escape=False)


def test_batched_bf16(cuda):
    B, N, M, D, V = 3, 200, 260, 48, 20
    rng = np.random.default_rng(11)
    items = [_law(rng, N, M, D) for _ in range(B)]
    x, y, h = (np.stack([it[k] for it in items]) for k in range(3))
    feat = np.random.default_rng(2).standard_normal((B, M, V)).astype(np.float32)
    xt, yt = _t(x, cuda).bfloat16(), _t(y, cuda).bfloat16()
    x, y = xt.float().cpu().numpy(), yt.float().cpu().numpy()      # the reference sees the bf16-rounded points
    out, soft = hip.plan_apply_p1(_eps(D), xt, yt, _t(h, cuda), _t(feat, cuda), want_softmin=True)
    assert out.shape == (B, N, V) and out.dtype == torch.float32 and out.grad_fn is None
    assert soft.shape == (B, N) and soft.dtype == torch.float32 and soft.grad_fn is None
    out, soft = out.cpu().numpy(), soft.cpu().numpy()
    for b in range(B):
        ref, sref = _ref(x[b], y[b], h[b], _eps(D), feat[b])
        _check(f"batched bf16 item {b}", cuda, x[b], y[b], h[b], feat[b], _eps(D), out[b], soft[b], ref, sref, D)


def test_massless_columns_and_items(cuda):
    B, N, M, D, V = 2, 257, 300, 24, 10
    rng = np.random.default_rng(21)
    items = [_law(rng, N, M, D) for _ in range(B)]
    x, y, h = (np.stack([it[k] for it in items]) for k in range(3))
    feat = np.random.default_rng(6).standard_normal((B, M, V)).astype(np.float32)
    h[0, ::3] = -np.inf                      # a third of the columns carry no mass ...
    feat[0, ::3] = 1e4                       # ... whatever (finite) features they hold
    h[1, :] = -np.inf                        # a batch item without any mass
    out, soft = _apply(cuda, x, y, h, feat, _eps(D))
    keep = np.isfinite(h[0])
    ref, sref = _ref(x[0][:, :], y[0][keep], h[0][keep], _eps(D), feat[0][keep])      # the reference without those columns
    err, serr = _worst(out[0], ref, feat[0][keep]), float(np.abs(soft[0] - sref).max())
    print(f"massless columns: out {err:.2e} = {err / BOUND:.3f} x bound, softmin {serr:.2e} = {serr / _sbound(sref):.3f} x bound")
    assert np.isfinite(out).all() and np.isfinite(soft[0]).all()
    assert err <= BOUND and serr <= _sbound(sref)
    assert (out[1] == 0.0).all() and not np.isnan(soft[1]).any()
    assert (soft[1] > 1e30).all()            # +inf or a huge finite value


def test_column_splits(cuda):
    N, M, D, V = 130, 70001, 24, 16
    x, y, h = _law(np.random.default_rng(D), N, M, D)
    feat = np.random.default_rng(V).standard_normal((M, V)).astype(np.float32)
    eps = 0.05
    ref, sref = _ref(x, y, h, eps, feat)
    split, s0 = _apply(cuda, x, y, h, feat, eps, 0)
    unsplit, s1 = _apply(cuda, x, y, h, feat, eps, hip.FLAG_NO_SPLIT)
    nows, s2 = _apply(cuda, x, y, h, feat, eps, 0, workspace=False)
    errs = [_worst(o, ref, feat) for o in (split, unsplit, nows)]
    serrs = [float(np.abs(s - sref).max()) for s in (s0, s1, s2)]
    between = _worst(split, unsplit, feat)
    print(f"splits N={N} M={M} D={D} V={V}: vs reference {errs} (bound 1e-4), split vs unsplit {between:.2e} = {between / BOUND:.3f} x bound, "
          f"softmin {serrs} (bound {_sbound(sref):.2e})")
    assert max(errs) <= 1e-4
    assert between <= BOUND
    assert max(serrs) <= _sbound(sref)


def test_passes(cuda):
    """A pass does not depend on the passes next to it: the leading `width` columns alone give the bits they give inside a wider call."""
    width = hip.load_library().glhip_plan_apply_p1_pass_width()
    N, M, D = 257, 300, 40
    V = 2 * width + 1
    x, y, h = _law(np.random.default_rng(8), N, M, D)
    feat = np.random.default_rng(V).standard_normal((M, V)).astype(np.float32)
    full, sfull = _apply(cuda, x, y, h, feat, _eps(D))
    alone, salone = _apply(cuda, x, y, h, feat[:, :width], _eps(D))
    ref, sref = _ref(x, y, h, _eps(D), feat)
    _check(f"passes V={V}", cuda, x, y, h, feat, _eps(D), full, sfull, ref, sref, D)
    assert np.array_equal(alone, full[:, :width])
    assert np.array_equal(salone, sfull)


def test_run_to_run(cuda):
    N, M, D, V = 300, 70001, 24, 16          # column splits and their merge included
    x, y, h = _law(np.random.default_rng(9), N, M, D)
    feat = np.random.default_rng(V).standard_normal((M, V)).astype(np.float32)
    a, sa = _apply(cuda, x, y, h, feat, _eps(D))
    b, sb = _apply(cuda, x, y, h, feat, _eps(D))
    assert np.array_equal(a, b) and np.array_equal(sa, sb)


def test_agreement_with_the_forward(cuda):
    N, M, D, V = 300, 517, 33, 4
    x, y, h = _law(np.random.default_rng(33), N, M, D)
    feat = np.random.default_rng(V).standard_normal((M, V)).astype(np.float32)
    eps = _eps(D)
    _, soft = _apply(cuda, x, y, h, feat, eps)
    fwd = hip.softmin(eps, _t(x, cuda), _t(y, cuda), _t(h, cuda), p=1, flags=hip.FLAG_XK_DIST).cpu().numpy()
    diff, bound = float(np.abs(soft - fwd).max()), 2 * _sbound(fwd)
    print(f"softmin on the side against the forward D={D}: {diff:.2e} = {diff / bound:.3f} x bound")
    assert diff <= bound


@pytest.mark.parametrize("D", [8, 24])
def test_empty_sizes(cuda, D):
    """M == 0 with N > 0: out is zeroed; V == 0: out is empty; N == 0: nothing to write."""
    N = 40
    x = torch.rand(1, N, D, device=cuda)
    out, soft = hip.plan_apply_p1_raw(x, torch.rand(1, 50, D, device=cuda), torch.zeros(1, 50, device=cuda),
                                      torch.ones(1, 50, 0, device=cuda), _eps(D), want_softmin=True)
    assert out.shape == (1, N, 0) and soft.shape == (1, N)
    out, soft = hip.plan_apply_p1_raw(x, torch.rand(1, 0, D, device=cuda), torch.zeros(1, 0, device=cuda),
                                      torch.ones(1, 0, 3, device=cuda), _eps(D), want_softmin=True)
    assert (out == 0).all() and not torch.isnan(soft).any() and (soft > 1e30).all()
    out = hip.plan_apply_p1_raw(x[:, :0], torch.rand(1, 50, D, device=cuda), torch.zeros(1, 50, device=cuda),
                                torch.ones(1, 50, 3, device=cuda), _eps(D))
    assert out.shape == (1, 0, 3)
    torch.cuda.synchronize()
