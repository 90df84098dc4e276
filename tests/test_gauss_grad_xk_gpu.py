"""``glhip_kernel_conv_bwd_x`` / ``glhip_kernel_conv_fwd_grad`` under ``GLHIP_FLAG_XK_GRAD``: the gaussian kernel gradient of
17 <= D <= 4095 on the matrix cores (geomloss_amd/csrc/glhip_gauss_grad_xk.h) against ``oracle_torch64.kconv_grad_x`` / ``kconv`` in
float64 on the same float32 (or bf16-rounded) inputs.

Error measure: the column weights are signed, so an error is ``max|out - ref| / max|ref_abs|`` with ``ref_abs`` the float64 result
for ``|v|`` and ``|g|`` — the scale of the terms that are summed (on these clouds the signed sums cancel about 10x).

Bound: the project's rule for this gradient (tests/test_anyd_kernels_gpu.py) — 5e-6, and for D > 64 max(5e-6, 4 e_ref) with e_ref the
error of the same gradient in plain float32 torch on the expanded cost |x|^2 - 2 x.y + |y|^2, computed here and normalised the same
way (the rule of tests/test_softmin_grad_xk_gpu.py).  The product that ``fwd_grad`` returns next to the gradient: 3e-6 max|ref_abs|.
Every figure is printed before it is asserted."""
import math

import numpy as np
import pytest
import torch

from cloud_support import to_dev as _t
from conftest import relerr
from geomloss_amd import SamplesLoss, hip
from geomloss_amd import kernel_samples
from oracle import oracle_torch64 as o64

pytestmark = pytest.mark.gpu

XK = hip.FLAG_XK_GRAD
FLAGS = [XK, XK | hip.FLAG_NO_SPLIT, XK | hip.FLAG_F16X2, XK | hip.FLAG_F16X2 | hip.FLAG_NO_SPLIT]
G = hip.GAUSSIAN


def _clouds(seed, N, M, D, B=None, offset=0.0):
    """Uniform clouds (``_clouds`` of tests/test_softmin_grad_xk_gpu.py), column weights of mixed sign, a standard normal upstream
    gradient."""
    rng = np.random.default_rng(seed)
    shp = (lambda n: (n, D)) if B is None else (lambda n: (B, n, D))
    x = rng.random(shp(N)).astype(np.float32) + np.float32(offset)
    y = (rng.random(shp(M)) * 0.8 + 0.1).astype(np.float32) + np.float32(offset)
    v = (rng.standard_normal(shp(M)[:-1]) / M).astype(np.float32)
    g = rng.standard_normal(shp(N)[:-1]).astype(np.float32)
    return x, y, v, g


def _blur(D):
    return 0.3 * math.sqrt(D / 3)


def _batched(f):
    """Applies a reference for one cloud to (B, ...) inputs item by item."""
    def run(dev, *arrs, **kw):
        if arrs[0].ndim == 2:
            return f(dev, *arrs, **kw)
        return np.stack([f(dev, *(a[b] if isinstance(a, np.ndarray) else a for a in arrs), **kw) for b in range(arrs[0].shape[0])])
    return run


@_batched
def _ref_grad(dev, x, y, v, g, blur):
    return o64.kconv_grad_x("gaussian", x, y, v, g, blur, device=dev)


@_batched
def _ref_out(dev, x, y, v, blur):
    return o64.kconv("gaussian", x, y, v, blur, device=dev)


@_batched
def _f32_grad(dev, x, y, v, g, blur):
    """The same gradient in plain float32 torch: expanded cost, one exponential, two matrix products."""
    xt, yt, vt, gt = (_t(a, dev) for a in (x, y, v, g))
    C = (xt * xt).sum(1)[:, None] - 2.0 * xt @ yt.t() + (yt * yt).sum(1)[None, :]
    Kv = torch.exp(-C / (2.0 * blur * blur)) * vt[None, :]
    return ((gt / (blur * blur))[:, None] * (Kv @ yt - xt * Kv.sum(1, keepdim=True))).cpu().numpy()


def _err(out, ref, ref_abs):
    return float(np.abs(np.asarray(out, np.float64) - ref).max() / np.abs(ref_abs).max())


def _bound(D, e_ref):
    return max(5e-6, 4.0 * e_ref) if D > 64 else 5e-6


class _Case:
    """Inputs with their float64 references: bwd_x (g), fwd_grad (g = 1, and the product), the |v|, |g| scales and e_ref."""

    def __init__(self, dev, x, y, v, g, blur, xr=None, yr=None):
        xr, yr = (x if xr is None else xr), (y if yr is None else yr)      # what the reference sees (bf16: the rounded points)
        one = np.ones_like(g)
        self.x, self.y, self.v, self.g, self.blur = x, y, v, g, blur
        self.ref = _ref_grad(dev, xr, yr, v, g, blur)
        self.ref_abs = _ref_grad(dev, xr, yr, np.abs(v), np.abs(g), blur)
        self.unit = _ref_grad(dev, xr, yr, v, one, blur)
        self.unit_abs = _ref_grad(dev, xr, yr, np.abs(v), one, blur)
        self.out = _ref_out(dev, xr, yr, v, blur)
        self.out_abs = _ref_out(dev, xr, yr, np.abs(v), blur)
        self.e_ref = _err(_f32_grad(dev, xr, yr, v, g, blur), self.ref, self.ref_abs)
        self.D = x.shape[-1]

    def bound(self):
        return _bound(self.D, self.e_ref)


def _launch(dev, c, flags, x=None, y=None, **kw):
    """Both entry points on the inputs of a case -> (grad_x, out, grad_unit) as NumPy, shaped like the inputs."""
    xb, yb = (_t(c.x, dev) if x is None else x), (_t(c.y, dev) if y is None else y)
    vb, gb = _t(c.v, dev), _t(c.g, dev)
    batched = xb.dim() == 3
    if not batched:
        xb, yb, vb, gb = xb[None], yb[None], vb[None], gb[None]
    gx = hip.kernel_conv_bwd_x_raw(G, xb, yb, vb, gb, c.blur, None, flags, **kw).cpu().numpy()
    out, gu = (t.cpu().numpy() for t in hip.kernel_conv_fwd_grad_raw(G, xb, yb, vb, c.blur, None, flags, **kw))
    return (gx, out, gu) if batched else (gx[0], out[0], gu[0])


def _check(tag, c, res, bound=None):
    gx, out, gu = res
    bound = c.bound() if bound is None else bound
    e_gx, e_gu, e_out = _err(gx, c.ref, c.ref_abs), _err(gu, c.unit, c.unit_abs), _err(out, c.out, c.out_abs)
    cancel = float(np.abs(c.ref_abs).max() / max(np.abs(c.ref).max(), 1e-300))
    print(f"{tag}: bwd_x {e_gx:.3e}   fwd_grad unit {e_gu:.3e} out {e_out:.3e}   float32 torch e_ref {c.e_ref:.3e}   bound {bound:.3e}"
          f"   (signed sums cancel {cancel:.1f}x)")
    assert gx.shape == c.ref.shape and gu.shape == c.ref.shape and out.shape == c.out.shape
    assert np.isfinite(gx).all() and np.isfinite(gu).all() and np.isfinite(out).all()
    assert e_gx <= bound
    assert e_gu <= bound
    assert e_out <= 3e-6


# (270, 310, 17): the first dimension            (257, 300, 65): a one-coordinate second pass, a one-row second row block
# (130, 600, 128): two full passes               (130, 600, 300): a long chain, five passes with a remainder
SHAPES = [(270, 310, 17), (300, 257, 31), (97, 513, 32), (257, 300, 65), (130, 600, 128), (64, 8, 64), (1, 1, 100), (130, 600, 300)]
_CASES = {}


def _parity_case(dev, N, M, D):      # inputs and float64 references, computed once for the four flag settings
    key = (N, M, D)
    if key not in _CASES:
        _CASES[key] = _Case(dev, *_clouds(N + M + D, N, M, D), _blur(D))
    return _CASES[key]


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("N,M,D", SHAPES)
def test_parity(cuda, N, M, D, flags):
    c = _parity_case(cuda, N, M, D)
    assert hip.kernel_conv_grad_uses_xk("gaussian", 1, N, M, D, flags=flags) == 1
    _check(f"parity N={N} M={M} D={D} flags={flags}", c, _launch(cuda, c, flags))


def test_column_splits(cuda):
    N, M, D = 130, 70001, 72
    lib = hip.load_library()
    nbytes = int(lib.glhip_kernel_conv_grad_workspace_bytes(1, N, M, D, XK))
    print(f"splits: workspace {nbytes} bytes = {nbytes // (N * 66 * 4)} splits of the 64-coordinate pass")
    assert nbytes >= 2 * N * 66 * 4
    c = _Case(cuda, *_clouds(D, N, M, D), _blur(D))
    split = _launch(cuda, c, XK)
    nows = _launch(cuda, c, XK, workspace=False)
    _check("splits, with a workspace", c, split)
    _check("splits, workspace=False", c, nows)
    among = [_err(a, b, s) for a, b, s in zip(split, nows, (c.ref_abs, c.out_abs, c.unit_abs))]
    print(f"splits N={N} M={M} D={D}: split against unsplit {among}")
    assert max(among) <= 2.0 * c.bound()      # each is within the bound of the reference


@pytest.mark.parametrize("D", [65, 128])
def test_batched(cuda, D):
    B, N, M = 3, 200, 260
    c = _Case(cuda, *_clouds(11 + D, N, M, D, B=B), _blur(D))
    assert hip.kernel_conv_grad_uses_xk("gaussian", B, N, M, D, flags=XK) == 1
    res = _launch(cuda, c, XK)
    assert res[0].shape == (B, N, D) and res[1].shape == (B, N)
    _check(f"batched B={B} D={D}", c, res)


def test_bf16(cuda):
    N, M, D = 200, 260, 40
    x, y, v, g = _clouds(13, N, M, D)
    xt, yt = _t(x, cuda).bfloat16(), _t(y, cuda).bfloat16()
    c = _Case(cuda, x, y, v, g, _blur(D), xr=xt.float().cpu().numpy(), yr=yt.float().cpu().numpy())      # the bf16-rounded points
    assert hip.kernel_conv_grad_uses_xk("gaussian", 1, N, M, D, dtype=hip.BF16, flags=XK) == 1
    res = _launch(cuda, c, XK, x=xt, y=yt)
    assert res[0].dtype == np.float32
    _check("bf16 D=40", c, res)


@pytest.mark.parametrize("flags", [XK, XK | hip.FLAG_F16X2])
def test_zero_signed_mass(cuda, flags):
    """Every row lies in the hyperplane x[0] = 0.5 and the columns come in pairs mirrored about it with weights +w, -w: each row is
    equidistant from the two columns of a pair, so U_i = sum_j k_ij v_j is 0 to rounding — of either sign — while the gradient along
    coordinate 0 is sum over pairs of 2 k w t / blur^2.  A row-without-mass test on the sign of the signed mass would zero such rows."""
    N, P, D = 300, 150, 40
    rng = np.random.default_rng(17)
    x = rng.random((N, D)).astype(np.float32)
    x[:, 0] = 0.5
    half = (rng.random((P, D)) * 0.8 + 0.1).astype(np.float32)
    t = (rng.integers(1, 256, P) / 1024.0).astype(np.float32)
    y = np.repeat(half, 2, axis=0)
    y[0::2, 0], y[1::2, 0] = 0.5 + t, 0.5 - t      # exact in float32
    w = (np.abs(rng.standard_normal(P)) / P).astype(np.float32)
    v = np.repeat(w, 2)
    v[1::2] *= -1
    g = rng.standard_normal(N).astype(np.float32)
    c = _Case(cuda, x, y, v, g, _blur(D))
    res = _launch(cuda, c, flags)
    _check(f"zero signed mass flags={flags}", c, res)
    gx, out, gu = res
    u_rel = float(np.abs(out).max() / np.abs(c.out_abs).max())
    g0 = float(np.abs(gu[:, 0]).min() / np.abs(c.unit_abs).max())
    print(f"zero signed mass flags={flags}: max|U| {u_rel:.3e} of the unsigned product ({(out > 0).sum()} rows > 0, {(out < 0).sum()} < 0, "
          f"{(out == 0).sum()} == 0); smallest |d U / d x_0| {g0:.3e} of the unsigned gradient")
    assert np.abs(c.out).max() <= 1e-12 * np.abs(c.out_abs).max()      # the construction: U is 0 in float64
    assert u_rel <= 3e-6
    assert (gu[:, 0] > 0).all() and g0 > 100 * 5e-6                    # and the gradient is not


@pytest.mark.parametrize("D", [40, 100])
def test_exactness_and_operand_order(cuda, D, flags=XK):
    """Grid points at multiples of 1/1024 (in a box of 32 steps), x_i = y_perm(i) + e_i with e a multiple of 1/4096, v = 1 and
    blur = 2^-8: every row sees one column (the others weigh less than 2^-100 of it), so with k_i = exp(-|e_i|^2 / 2 blur^2)

        out_i = k_i,   grad_unit_i = k_i (y_perm(i) - x_i) / blur^2 = -k_i e_i 2^16.

    Sums, centring and the difference are exact in float32 and 1 / blur^2 is a power of two, so grad_unit must equal the float32 product
    out_i * (-e_i), scaled by 2^16, BIT FOR BIT with the out_i the same launch returns.  A wrong K permutation or register-to-coordinate
    map gives another difference, and the position of the first one names the lane.  D = 100: a second pass.
    k_i itself is a rounded exponential of an exponent whose terms are s R^2 = log2(e) / blur^2 x (largest centred norm)^2 ~ 1e3 in size:
    it is held to the worst-case bound of glhip_softmin_xk.h, |du| <= 2^-24 (NM + 5) s R^2 in log2 units, NM = ceil((6 + 6 D) / 16)
    chained MFMAs (1e-3 ... 1e-2 here; the flat 3e-6 of the product belongs to exponents of size 10, where no row sees one column only).
    (bf16 x 3 exponents only: at this blur the exponents are outside the range contract of GLHIP_FLAG_F16X2.)"""
    n = 96
    blur = 2.0**-8
    rng = np.random.default_rng(5)
    y = (rng.integers(0, 32, (n, D)) / 1024.0).astype(np.float32)
    perm = rng.permutation(n)
    i, d = np.arange(n)[:, None], np.arange(D)[None, :]
    e = (((i + d) % 7 - 3) / 4096.0).astype(np.float32)
    x = y[perm] + e
    assert np.array_equal((x.astype(np.float64) - y[perm]).astype(np.float32), e)      # the construction is exact
    d2 = ((x.astype(np.float64)[:, None, :] - y.astype(np.float64)[None, :, :]) ** 2).sum(-1) / (2 * blur * blur)
    own = d2[np.arange(n), perm]
    d2[np.arange(n), perm] = np.inf
    assert ((d2.min(1) - own) / math.log(2) > 100).all()                               # every other column: below 2^-100 of the row's own
    v = np.ones(n, np.float32)
    out, gu = hip.kernel_conv_fwd_grad_raw(G, _t(x, cuda)[None], _t(y, cuda)[None], _t(v, cuda)[None], blur, None, flags)
    out, gu = out[0].cpu().numpy(), gu[0].cpu().numpy()
    k = np.exp(-own)
    R2 = max(((x.astype(np.float64) - x[0]) ** 2).sum(1).max(), ((y.astype(np.float64) - x[0]) ** 2).sum(1).max())      # centre: row 0
    NM = (6 + 6 * D + 15) // 16
    b_out = math.expm1(math.log(2) * 2.0**-24 * (NM + 5) * (math.log2(math.e) / blur**2) * R2)
    e_out = float(np.abs(out / k - 1).max())
    want = (out[:, None] * (-e)).astype(np.float32) * np.float32(2.0**16)
    bad = np.argwhere(gu != want)
    print(f"exactness D={D} flags={flags}: out / exp - 1 {e_out:.3e} (bound {b_out:.3e}, k in [{k.min():.3f}, {k.max():.3f}]); "
          f"{len(bad)} of {gu.size} entries of grad_unit differ, max |grad_unit - want| {np.abs(gu - want).max():.3e}")
    assert (out > 0).all() and e_out <= b_out
    assert len(bad) == 0, f"first wrong (row, coordinate) {bad[0]}: got {gu[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}"
    gx = hip.kernel_conv_bwd_x_raw(G, _t(x, cuda)[None], _t(y, cuda)[None], _t(v, cuda)[None], _t(v, cuda)[None], blur, None, flags)
    assert np.array_equal(gx[0].cpu().numpy(), gu)      # g = 1: the same numbers


@pytest.mark.parametrize("flags", [XK, XK | hip.FLAG_F16X2])
def test_rows_without_columns_in_reach(cuda, flags):
    """The last 100 of 300 rows (44 of them a row block of their own) are 30 away from the clouds in every coordinate: e^-15000 of
    every column.  They get exactly 0, nothing is NaN, and the rows in reach keep their bound."""
    N, M, D, far = 300, 310, 40, 200
    x, y, v, g = _clouds(23, N, M, D)
    x[far:] += np.float32(30.0)
    c = _Case(cuda, x, y, v, g, _blur(D))
    assert np.abs(c.ref[far:]).max() < 1e-300
    res = _launch(cuda, c, flags)
    _check(f"rows out of reach flags={flags}", c, res)
    for a in res:
        assert (a[far:] == 0.0).all()
    assert np.abs(res[0][:far]).max() > 0


@pytest.mark.parametrize("flags", [XK, XK | hip.FLAG_F16X2])
def test_cloud_far_from_the_origin(cuda, flags):
    """Both clouds offset by 100: the centred features keep S_i - (x_i - c) U_i free of cancellation."""
    N, M, D = 270, 310, 40
    x, y, v, g = _clouds(7, N, M, D, offset=100.0)
    assert x.dtype == np.float32 and x.min() >= 100.0
    c = _Case(cuda, x, y, v, g, _blur(D))
    _check(f"offset 100 flags={flags}", c, _launch(cuda, c, flags), bound=5e-6)


def test_m_zero_writes_zeros(cuda):
    x = torch.rand(1, 50, 40, device=cuda)
    y = torch.empty(1, 0, 40, device=cuda)
    v = torch.empty(1, 0, device=cuda)
    g = torch.ones(1, 50, device=cuda)
    gx = hip.kernel_conv_bwd_x_raw(G, x, y, v, g, 1.0, None, XK)
    out, gu = hip.kernel_conv_fwd_grad_raw(G, x, y, v, 1.0, None, XK)
    assert (gx == 0).all() and (out == 0).all() and (gu == 0).all()


def test_flag_is_inert_where_it_does_not_apply(cuda):
    """D <= 16, the laplacian kernel, NO_MFMA and the gaussian product are the launches of the flag-less call, bit for bit."""
    def args(D, N=270, M=310):
        x, y, v, g = (_t(a, cuda)[None] for a in _clouds(D, N, M, D))
        return x, y, v, g

    x, y, v, g = args(16)
    assert hip.kernel_conv_grad_uses_xk("gaussian", 1, 270, 310, 16, flags=XK) == 0
    assert torch.equal(hip.kernel_conv_bwd_x_raw(G, x, y, v, g, _blur(16), None, 0), hip.kernel_conv_bwd_x_raw(G, x, y, v, g, _blur(16), None, XK))
    for a, b in zip(hip.kernel_conv_fwd_grad_raw(G, x, y, v, _blur(16), None, 0), hip.kernel_conv_fwd_grad_raw(G, x, y, v, _blur(16), None, XK)):
        assert torch.equal(a, b)
    x, y, v, g = args(40)
    assert hip.kernel_conv_grad_uses_xk("laplacian", 1, 270, 310, 40, flags=XK) == 0
    a, b = (hip.kernel_conv_bwd_x_raw(hip.LAPLACIAN, x, y, v, g, _blur(40), None, fl) for fl in (0, XK))
    assert torch.equal(a, b) and torch.isfinite(a).all()
    assert hip.kernel_conv_grad_uses_xk("gaussian", 1, 270, 310, 40, flags=XK | hip.FLAG_NO_MFMA) == 0
    a, b = (hip.kernel_conv_bwd_x_raw(G, x, y, v, g, _blur(40), None, hip.FLAG_NO_MFMA | fl) for fl in (0, XK))
    assert torch.equal(a, b) and torch.isfinite(a).all()
    a, b = (hip.kernel_conv_fwd_raw(G, x, y, v, _blur(40), None, fl) for fl in (0, XK))
    assert torch.equal(a, b) and torch.isfinite(a).all()


def _spy(monkeypatch):
    """Records (entry point, kind, B, N, M, D, dtype, flags) of every raw kernel-product launch."""
    calls = []
    for name in ("kernel_conv_fwd_raw", "kernel_conv_bwd_x_raw", "kernel_conv_fwd_grad_raw"):
        real = getattr(hip, name)

        def wrapped(kind, x, y, *rest, _real=real, _name=name, **kw):
            at = 4 if _name == "kernel_conv_bwd_x_raw" else 3      # (v, [g,] blur, ranges, flags, ...)
            fl = kw["flags"] if "flags" in kw else (rest[at] if len(rest) > at else 0)
            calls.append((_name, int(kind), x.shape[0], x.shape[1], y.shape[1], x.shape[2], hip.BF16 if x.dtype == torch.bfloat16 else hip.F32,
                          int(fl)))
            return _real(kind, x, y, *rest, **kw)
        monkeypatch.setattr(hip, name, wrapped)
    return calls


def test_default_routing(cuda, monkeypatch):
    """``hip.kernel_conv(..., flags=0)`` keeps today's route at D = 40 — no launch of its forward or backward carries the flag — and the
    unflagged ``glhip_kernel_conv_fwd_grad`` still refuses D = 40."""
    calls = _spy(monkeypatch)
    N, M, D = 270, 310, 40
    x, y, v, g = (_t(a, cuda) for a in _clouds(3, N, M, D))
    x.requires_grad_(True)
    out = hip.kernel_conv("gaussian", x, y, v, _blur(D), flags=0)
    (gx,) = torch.autograd.grad((out * g).sum(), [x])
    print("default routing:", [(c[0], c[-1]) for c in calls])
    assert len(calls) >= 2 and any(c[0] == "kernel_conv_bwd_x_raw" for c in calls)
    assert not any(c[-1] & XK for c in calls)
    assert not any(c[0] == "kernel_conv_fwd_grad_raw" for c in calls)
    ref = o64.kconv_grad_x("gaussian", x.detach().cpu().numpy(), y.cpu().numpy(), v.cpu().numpy(), g.cpu().numpy(), _blur(D), device=cuda)
    assert relerr(gx.cpu().numpy(), ref) <= 1e-4
    with pytest.raises(NotImplementedError):
        hip.kernel_conv_fwd_grad_raw(G, x.detach()[None], y[None], v[None], _blur(D), None, 0)


_E2E = {}


def _e2e_case(dev, D):
    if D not in _E2E:
        N, M = 300, 257
        rng = np.random.default_rng(100 + D)
        x, y, _, _ = _clouds(D, N, M, D)
        a, b = rng.random(N) + 0.5, rng.random(M) + 0.5
        a, b = (a / a.sum()).astype(np.float32), (b / b.sum()).astype(np.float32)
        blur = _blur(D)
        loss, gx, ga = o64.kernel_loss("gaussian", x, y, a, b, blur, grad=True, device=dev)
        loss2, gy, gb = o64.kernel_loss("gaussian", y, x, b, a, blur, grad=True, device=dev)      # the norm is symmetric
        assert abs(loss - loss2) <= 1e-12 * abs(loss)
        _E2E[D] = (x, y, a, b, blur, loss, (gx, gy, ga, gb))
    return _E2E[D]


@pytest.mark.parametrize("D", [40, 128])
def test_end_to_end_samples_loss(cuda, monkeypatch, D):
    """``SamplesLoss("gaussian", backend="online")`` takes the new kernel by default in dimension 17 ... 4095: its launches carry the
    flag and the predicate is 1 for them; with ``kernel_samples._XK_GRAD`` off (``GEOMLOSS_HIP_XK_GRAD=0``, latched at import) the same
    loss runs unflagged.  Loss and the gradients in x, y and both weight vectors against the float64 oracle at the 1e-4 of
    tests/test_samples_loss_gpu.py, on both routes."""
    x, y, a, b, blur, loss64, grads64 = _e2e_case(cuda, D)
    calls = _spy(monkeypatch)
    loss_fn = SamplesLoss("gaussian", blur=blur, backend="online")

    def run(on):
        monkeypatch.setattr(kernel_samples, "_XK_GRAD", on)
        del calls[:]
        xt, yt, at, bt = (_t(t, cuda).requires_grad_(True) for t in (x, y, a, b))
        L = loss_fn(at, xt, bt, yt)
        grads = torch.autograd.grad(L, [xt, yt, at, bt])
        return float(L.detach()), [t.cpu().numpy() for t in grads], list(calls)

    assert kernel_samples._XK_GRAD is True      # the default
    l_on, g_on, c_on = run(True)
    l_off, g_off, c_off = run(False)
    print(f"end to end D={D}: launches on {[(c[0], c[-1]) for c in c_on]}, off {[(c[0], c[-1]) for c in c_off]}")
    flagged = [c for c in c_on if c[0] == "kernel_conv_fwd_grad_raw"]
    assert len(flagged) == 2 and all(c[-1] & XK for c in flagged)
    assert all(hip.kernel_conv_grad_uses_xk(*c[1:7], flags=c[7]) == 1 for c in flagged)
    assert c_off and not any(c[-1] & XK for c in c_off)
    assert not any(c[0] == "kernel_conv_fwd_grad_raw" for c in c_off) and any(c[0] == "kernel_conv_bwd_x_raw" for c in c_off)
    for tag, l, gs in (("on", l_on, g_on), ("off", l_off, g_off)):
        errs = [relerr(o, r) for o, r in zip(gs, grads64)]
        el = abs(l - loss64) / abs(loss64)
        print(f"end to end D={D} route {tag}: loss {l!r} (float64 {loss64!r}, rel {el:.3e}); gradients x, y, a, b {errs}")
        assert el < 1e-4
        assert max(errs) < 1e-4
    between = [relerr(o, r) for o, r in zip(g_on, g_off)]
    print(f"end to end D={D}: the two routes differ by {between}")
    assert max(between) < 1e-4


def test_second_order_is_untouched(cuda):
    """create_graph=True at D = 20: ``_UnionNorm._differentiable_backward`` (plain kernel products) still gives a second derivative;
    against the loss in dense float64 torch at the 1e-4 of tests/test_samples_loss_gpu.py::test_gaussian_second_order_derivatives."""
    N, M, D = 60, 70, 20
    blur = _blur(D)
    x, y, _, _ = _clouds(20, N, M, D)
    u = np.random.default_rng(21).standard_normal((N, D)).astype(np.float32)

    def dense(xs, ys):
        z = torch.cat((xs, ys), 0)
        w = torch.cat((torch.full((N,), 1.0 / N, dtype=xs.dtype, device=xs.device), torch.full((M,), -1.0 / M, dtype=xs.dtype, device=xs.device)))
        K = (-((z[:, None, :] - z[None, :, :]) ** 2).sum(-1) / (2 * blur**2)).exp()
        return 0.5 * w @ K @ w

    def second(loss, dtype):
        xs, ys, ut = _t(x, cuda).to(dtype).requires_grad_(True), _t(y, cuda).to(dtype), _t(u, cuda).to(dtype)
        (gx,) = torch.autograd.grad(loss(xs, ys), [xs], create_graph=True)
        (hv,) = torch.autograd.grad((gx * ut).sum(), [xs])
        return gx.detach().cpu().numpy(), hv.cpu().numpy()

    g64, hv64 = second(dense, torch.float64)
    g32, hv32 = second(SamplesLoss("gaussian", blur=blur, backend="online"), torch.float32)
    e1, e2 = relerr(g32, g64), relerr(hv32, hv64)
    print(f"second order D={D}: gradient {e1:.3e}, Hessian-vector product {e2:.3e}")
    assert np.abs(hv64).max() > 0
    assert e1 < 1e-4 and e2 < 1e-4
