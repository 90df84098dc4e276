"""``hip.plan_apply_p1(..., resident=True)`` (GLHIP_FLAG_XD_PLAN_P1, geomloss_amd/csrc/glhip_dist_plan_xd.h) against float64 on the GPU.

Reference, input law, error measure and bounds are those of tests/test_plan_apply_p1_gpu.py, imported from it: ``out`` within 2e-5 of the
largest |feature| of its column, ``softmin`` within 12 x 2e-6 x max(1, |ref|max); no float32-torch escape (D <= 16 never needed it).
Every case prints its error over the bound (``pytest -s``).

Tiles.  The kernel sweeps tiles of 32 x min(8, budget / (NM + 4 NCH)) columns (NM = ceil(6 (D + 1) / 16), NCH = 1, 2 or 4 chunks of 32
features, budget 36 with one chunk and 60 beyond): 224 / 192 / 160 / 128 / 96 / 64 columns.  The M of the parity shapes are moved so that
each width that ships meets an M exactly one column past a tile: 225 (D = 1), 385 and 1153 (D = 3, 2: 192), 481 (D = 8, V = 33: 160), 129
(D = 8, V = 5: 128), 289 (D = 15: 96), 65 (D = 16, V = 70: 64).  (130, 70001, 3, 3) takes the column splits and their merge."""
import numpy as np
import pytest
import torch

from cloud_support import to_dev as _t
from geomloss_amd import apply_plan, barycentric_map, hip
from test_plan_apply_p1_gpu import BOUND, _apply, _check, _eps, _law, _ref, _sbound, _worst

pytestmark = pytest.mark.gpu

XD = hip.FLAG_XD_PLAN_P1
SHAPES = [(1, 1, 1, 1), (300, 385, 3, 7), (257, 1153, 2, 1), (97, 481, 8, 33), (260, 289, 15, 9), (64, 8, 16, 9), (130, 70001, 3, 3),
          (40, 225, 1, 3), (70, 129, 8, 5), (40, 65, 16, 70)]
_REFS = {}


def _case(N, M, D, V, eps):      # inputs and the float64 reference, computed once for every test that uses the shape
    key = (N, M, D, V, eps)
    if key not in _REFS:
        x, y, h = _law(np.random.default_rng(N + M + D), N, M, D)
        feat = np.random.default_rng(V).standard_normal((M, V)).astype(np.float32)
        _REFS[key] = (x, y, h, feat) + _ref(x, y, h, eps, feat)
    return _REFS[key]


def _verify(tag, dev, x, y, h, feat, eps, out, soft, ref, sref):
    _check(tag, dev, x, y, h, feat, eps, out, soft, ref, sref, x.shape[-1], escape=False)


# eps = 0.05 sqrt(D) with and without column splits, and the small blur eps = 0.05 on the shapes of D = 3 and 8
@pytest.mark.parametrize("N,M,D,V,eps,flags", [s + (_eps(s[2]), f) for s in SHAPES for f in (0, hip.FLAG_NO_SPLIT)]
                         + [s + (0.05, 0) for s in SHAPES if s[2] in (3, 8)])
def test_parity(cuda, N, M, D, V, eps, flags):
    x, y, h, feat, ref, sref = _case(N, M, D, V, eps)
    assert hip.load_library().glhip_plan_apply_p1_family(1, N, M, D, V, hip.F32, 0, XD | flags) == hip.FAMILY_XD
    out, soft = _apply(cuda, x, y, h, feat, eps, XD | flags)
    assert out.shape == (N, V) and soft.shape == (N,)
    _verify(f"parity N={N} M={M} D={D} V={V} eps={eps:.3f} flags={flags}", cuda, x, y, h, feat, eps, out, soft, ref, sref)


def test_operand_order(cuda):
    """One-hot plan rows and integer features on a grid of spacing 0.1 = 100 eps: a wrong K permutation, register-to-feature map or packed
    feature layout gives wrong integers."""
    n = 96
    rng = np.random.default_rng(5)
    cells = rng.permutation(1000)[:n]
    y = (0.1 * np.stack([cells // 100, (cells // 10) % 10, cells % 10], 1)).astype(np.float32)
    perm = rng.permutation(n)
    feat = (1000.0 * np.arange(n)[:, None] + np.arange(64)[None, :]).astype(np.float32)
    out = hip.plan_apply_p1(1e-3, _t(y[perm], cuda), _t(y, cuda), torch.zeros(n, device=cuda), _t(feat, cuda), resident=True).cpu().numpy()
    bad = np.argwhere(out != feat[perm])
    assert len(bad) == 0, f"first wrong (row, feature) {bad[0]}: got {out[tuple(bad[0])]!r}, want {feat[perm][tuple(bad[0])]!r}"


@pytest.mark.parametrize("D", [3, 16])
def test_near_pairs_carry_the_mass(cuda, D):
    """Every row's mass sits on four columns 1e-3 away, where the expanded form has lost its bits: fails if the repair, its row / column
    index map or the choice of the original against the centred points is wrong."""
    N, V = 300, 6
    rng = np.random.default_rng(D)
    x, _, _ = _law(rng, N, 1, D)
    y = (np.repeat(x, 4, axis=0) + 1e-3 * rng.standard_normal((4 * N, D))).astype(np.float32)
    h = rng.standard_normal(4 * N).astype(np.float32)
    feat = rng.standard_normal((4 * N, V)).astype(np.float32)
    eps = 1e-3 * float(np.sqrt(D))
    ref, sref = _ref(x, y, h, eps, feat)
    out, soft = _apply(cuda, x, y, h, feat, eps, XD)
    _verify(f"near pairs D={D}", cuda, x, y, h, feat, eps, out, soft, ref, sref)


def test_self_plan(cuda):
    """y = x: the diagonal sits on the clamp."""
    N, D, V = 300, 3, 6
    rng = np.random.default_rng(17)
    x, _, _ = _law(rng, N, 1, D)
    h = rng.standard_normal(N).astype(np.float32)
    feat = rng.standard_normal((N, V)).astype(np.float32)
    ref, sref = _ref(x, x, h, 0.05, feat)
    out, soft = _apply(cuda, x, x, h, feat, 0.05, XD)
    _verify("self-plan D=3", cuda, x, x, h, feat, 0.05, out, soft, ref, sref)


def test_batched_bf16(cuda):
    B, N, M, D, V = 3, 200, 260, 3, 20
    rng = np.random.default_rng(11)
    items = [_law(rng, N, M, D) for _ in range(B)]
    x, y, h = (np.stack([it[k] for it in items]) for k in range(3))
    feat = np.random.default_rng(2).standard_normal((B, M, V)).astype(np.float32)
    xt, yt = _t(x, cuda).bfloat16(), _t(y, cuda).bfloat16()
    x, y = xt.float().cpu().numpy(), yt.float().cpu().numpy()      # the reference sees the bf16-rounded points
    out, soft = (t.cpu().numpy() for t in hip.plan_apply_p1(_eps(D), xt, yt, _t(h, cuda), _t(feat, cuda), want_softmin=True, resident=True))
    assert out.shape == (B, N, V) and soft.shape == (B, N)
    for b in range(B):
        ref, sref = _ref(x[b], y[b], h[b], _eps(D), feat[b])
        _verify(f"batched bf16 item {b}", cuda, x[b], y[b], h[b], feat[b], _eps(D), out[b], soft[b], ref, sref)


def test_massless_columns_and_items(cuda):
    B, N, M, D, V = 2, 257, 300, 3, 10
    rng = np.random.default_rng(21)
    items = [_law(rng, N, M, D) for _ in range(B)]
    x, y, h = (np.stack([it[k] for it in items]) for k in range(3))
    plain = np.random.default_rng(6).standard_normal((B, M, V)).astype(np.float32)
    h[0, ::3] = -np.inf                      # a third of the columns carry no mass ...
    h[0, 64:96] = -np.inf                    # ... a whole group of 32 among them ...
    h[1, :] = -np.inf                        # ... and a batch item without any
    feat = plain.copy()
    feat[0, ~np.isfinite(h[0])] = 1e30       # whatever (finite) features they hold
    out, soft = _apply(cuda, x, y, h, feat, _eps(D), XD)
    out_plain, soft_plain = _apply(cuda, x, y, h, plain, _eps(D), XD)
    assert np.array_equal(out[0], out_plain[0]) and np.array_equal(soft[0], soft_plain[0])
    keep = np.isfinite(h[0])
    ref, sref = _ref(x[0], y[0][keep], h[0][keep], _eps(D), feat[0][keep])      # the reference without those columns
    _verify("massless columns", cuda, x[0], y[0][keep], h[0][keep], feat[0][keep], _eps(D), out[0], soft[0], ref, sref)
    assert (out[1] == 0.0).all() and not np.isnan(soft[1]).any() and (soft[1] > 1e30).all()


def test_passes(cuda):
    """A pass does not depend on the passes next to it: the leading `width` columns alone give the bits they give inside a wider call."""
    N, M, D = 257, 300, 3
    width = hip.load_library().glhip_plan_apply_p1_xd_pass_width(D)
    V = 2 * width + 1
    x, y, h = _law(np.random.default_rng(8), N, M, D)
    feat = np.random.default_rng(V).standard_normal((M, V)).astype(np.float32)
    full, sfull = _apply(cuda, x, y, h, feat, _eps(D), XD)
    alone, salone = _apply(cuda, x, y, h, feat[:, :width], _eps(D), XD)
    ref, sref = _ref(x, y, h, _eps(D), feat)
    _verify(f"passes V={V}", cuda, x, y, h, feat, _eps(D), full, sfull, ref, sref)
    assert np.array_equal(alone, full[:, :width]) and np.array_equal(salone, sfull)


def test_run_to_run(cuda):
    N, M, D, V = 300, 70001, 3, 16           # column splits and their merge included
    x, y, h = _law(np.random.default_rng(9), N, M, D)
    feat = np.random.default_rng(V).standard_normal((M, V)).astype(np.float32)
    a, sa = _apply(cuda, x, y, h, feat, _eps(D), XD)
    b, sb = _apply(cuda, x, y, h, feat, _eps(D), XD)
    assert np.array_equal(a, b) and np.array_equal(sa, sb)


def test_agreement_between_the_routes(cuda):
    N, M, D, V = SHAPES[3]
    x, y, h, feat, _, sref = _case(N, M, D, V, _eps(D))
    args = (_eps(D), _t(x, cuda), _t(y, cuda), _t(h, cuda), _t(feat, cuda))
    (a, sa), (b, sb) = (hip.plan_apply_p1(*args, want_softmin=True, resident=r) for r in (True, False))
    diff, sdiff = _worst(a.cpu().numpy(), b.cpu().numpy(), feat), float((sa - sb).abs().max())
    print(f"resident against default route: out {diff:.2e} = {diff / (2 * BOUND):.3f} x bound, softmin {sdiff:.2e} = {sdiff / (2 * _sbound(sref)):.3f} x bound")
    assert diff <= 2 * BOUND and sdiff <= 2 * _sbound(sref)


def test_through_the_public_interface(cuda):
    """``barycentric_map`` and the transposed ``apply_plan`` with ``p=1, resident=True``.  The latter returns (row mass) x (average); the
    same call on a feature of ones returns the row mass alone, from which the average and the soft-min are read and held to their bounds."""
    N, M, D, blur = 300, 385, 3, 0.05 * float(np.sqrt(3))
    x, y, _ = _law(np.random.default_rng(3), N, M, D)
    rng = np.random.default_rng(4)
    F, G = 0.05 * rng.standard_normal(N).astype(np.float32), 0.05 * rng.standard_normal(M).astype(np.float32)
    featT = rng.standard_normal((N, 5)).astype(np.float32)
    xt, yt, Ft, Gt = (_t(v, cuda) for v in (x, y, F, G))
    T = barycentric_map(xt, yt, Ft, Gt, blur, p=1, resident=True)
    assert T.shape == (N, D) and T.grad_fn is None
    h = (G.astype(np.float64) / blur - np.log(M)).astype(np.float32)
    ref, _ = _ref(x, y, h, blur, y)
    err = _worst(T.cpu().numpy(), ref, y)
    print(f"barycentric_map: {err:.2e} = {err / BOUND:.3f} x bound")
    assert err <= BOUND
    got = apply_plan(xt, yt, Ft, Gt, _t(featT, cuda), blur, p=1, transpose=True, resident=True)
    mass = apply_plan(xt, yt, Ft, Gt, torch.ones(N, device=cuda), blur, p=1, transpose=True, resident=True)
    assert got.shape == (M, 5) and got.grad_fn is None
    got, mass = got.double().cpu().numpy(), mass.double().cpu().numpy()
    hT = (F.astype(np.float64) / blur - np.log(N)).astype(np.float32)
    refT, srefT = _ref(y, x, hT, blur, featT)
    soft = G.astype(np.float64) - blur * (np.log(mass) + np.log(M))      # mass_j = exp((G_j - softmin_j) / blur) / M
    err, serr = _worst(got / mass[:, None], refT, featT), float(np.abs(soft - srefT).max())
    print(f"transposed apply_plan: out {err:.2e} = {err / BOUND:.3f} x bound, softmin {serr:.2e} = {serr / _sbound(srefT):.3f} x bound")
    assert err <= BOUND and serr <= _sbound(srefT)
