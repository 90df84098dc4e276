"""The matrix-core distance reductions of 17 <= D <= 4095 (``GLHIP_FLAG_XK_DIST``, geomloss_amd/csrc/glhip_dist_xk.h) against float64:
p = 1 soft-min, fused half-step, laplacian and energy products.

References are float64 only (``oracle.oracle_c``); inputs follow the law of tests/test_dimension_sweep_gpu.py, whose helpers are
imported.  Every launch carries ``FLAG_XK_DIST`` and is preceded by the assertion that the library's own predicate names
``FAMILY_DIST``.  Bounds are the ones the sweep already states for this dimension range (there: the generic kernel):

    soft-min / half-step   12 x 2e-6 max(1, |f|max)            products   12 x 5e-6 |ref|max   (positive weights)

The worst error over the 12-times-tighter bound of D <= 16 is printed per operation (``pytest -s``; profiles/dist_xk.txt); only the
12 x bound is asserted."""
import functools
import math

import numpy as np
import pytest
import torch

from geomloss_amd import SamplesLoss, hip, kernel_samples, sinkhorn_samples
from oracle import oracle_c
from test_dimension_sweep_gpu import DAMPING, EPS1, _blur, _case, _finish, _items, _launches, _Report, _rows, _step_extras, _t, _weights

pytestmark = pytest.mark.gpu

XKD, NS = hip.FLAG_XK_DIST, hip.FLAG_NO_SPLIT
WIDE = 12
DIMS = list(range(17, 41)) + [47, 48, 49, 63, 64, 65, 70, 127, 130]
BIG = [257, 1024, 4095]
KINDS = ("laplacian", "energy")


def _sbound(ref):
    return WIDE * 2e-6 * max(1.0, float(np.abs(ref).max()))


def _kbound(ref):
    return WIDE * 5e-6 * float(np.abs(ref).max())


def _family_is_dist(B, N, M, D, flags, dtype=hip.F32):
    assert hip.softmin_fwd_family(B, N, M, D, 1, dtype, flags) == hip.FAMILY_DIST, (B, N, M, D, flags)
    for kind in KINDS:
        assert hip.kernel_conv_fwd_family(kind, B, N, M, D, dtype, flags) == hip.FAMILY_DIST, (kind, B, N, M, D, flags)


def _law(rng, N, M, D):
    """the sweep's input law (per-coordinate scales: coordinates are not exchangeable)"""
    s = 0.5 + 0.5 * rng.random(D)
    x = (rng.random((N, D)) * s).astype(np.float32)
    y = ((rng.random((M, D)) * 0.8 + 0.1) * s).astype(np.float32)
    h = rng.standard_normal(M).astype(np.float32)
    return x, y, h


def _check_all(rep, D, variant, dev, x, y, h, flags, sm_eps=EPS1, blur=None, layout="-"):
    """soft-min and both products of one 2-D problem (NumPy inputs) against the oracle, one launch each"""
    blur = _blur(D) if blur is None else blur
    xt, yt, ht = _t(x, dev), _t(y, dev), _t(h, dev)
    ref = oracle_c.softmin(sm_eps, x, y, h, 1)
    out = hip.softmin(sm_eps, xt, yt, ht, p=1, flags=flags).cpu().numpy()
    rep.add(D, f"softmin {variant}", np.abs(out - ref).max(), _sbound(ref), f"softmin {layout}")
    v = _weights(h)
    for kind in KINDS:
        kref = oracle_c.kconv(kind, x, y, v, blur)
        kout = hip.kernel_conv(kind, xt, yt, _t(v, dev), blur, flags=flags).cpu().numpy()
        rep.add(D, f"{kind} {variant}", np.abs(kout - kref).max(), _kbound(kref), f"{kind} {layout}")


def _print_tight(rep):
    for layout, (ratio, D, variant) in sorted(rep.worst.items()):
        print(f"dist_xk {rep.name} [{layout}]: worst error / tight (1x) bound {WIDE * ratio:.3f} at D = {D} ({variant})")


# ---- 1. dimensions -----------------------------------------------------------------------------------------------------------------
# teeth, on the host at the 12 x bounds: the float64 reference without the last coordinate moves by >= 567 / 262 / 107 bounds
# (soft-min / laplacian / energy) up to D = 130, 277 / 174 / 71 at 257, 59 / 39 / 16 at 1024, 7.9 / 4.9 / 2.0 at 4095
def _teeth(D):
    return 100 if D <= 130 else 10 if D <= 1024 else 1


@functools.lru_cache(maxsize=None)
def _host_dims(D):
    refs, moved = {}, {"softmin": math.inf, "laplacian": math.inf, "energy": math.inf}
    blur = _blur(D)
    for tag, x, y, h in _items(D, D in BIG):
        pot, prev = _step_extras(D, tag, x.shape[0], y.shape[0])
        hh = h.astype(np.float64) + pot.astype(np.float64) / EPS1
        soft0, soft = oracle_c.softmin(EPS1, x, y, h, 1), oracle_c.softmin(EPS1, x, y, hh, 1)
        v = _weights(h)
        prods = {kind: oracle_c.kconv(kind, x, y, v, blur) for kind in KINDS}
        refs[tag] = (soft0, DAMPING * soft0, soft, 0.5 * (prev.astype(np.float64) + DAMPING * soft), pot, prev, prods)
        xs, ys = np.ascontiguousarray(x[:, :-1]), np.ascontiguousarray(y[:, :-1])
        moved["softmin"] = min(moved["softmin"], np.abs(oracle_c.softmin(EPS1, xs, ys, h, 1) - soft0).max() / _sbound(soft0))
        for kind in KINDS:
            moved[kind] = min(moved[kind], np.abs(oracle_c.kconv(kind, xs, ys, v, blur) - prods[kind]).max() / _kbound(prods[kind]))
    return refs, moved


def test_dimensions(cuda):
    rep = _Report("dimensions")
    for D in DIMS + BIG:
        big, blur = D in BIG, _blur(D)
        refs, moved = _host_dims(D)
        for what, mv in moved.items():
            rep.teeth(D, what, mv, _teeth(D))
        for flags in (XKD, XKD | NS):
            assert hip.half_step_applies(D, 1, flags), D
            for tags, (x, y, h) in _launches(D, cuda, big):
                B = len(tags) if len(tags) > 1 else 1
                _family_is_dist(B, x.shape[-2], y.shape[-2], D, flags)
                pot = _t(np.stack([refs[t][4] for t in tags]), cuda).reshape(h.shape)
                prev = _t(np.stack([refs[t][5] for t in tags]), cuda).reshape(x.shape[:-1])
                f = _rows(hip.softmin(EPS1, x, y, h, p=1, flags=flags), tags)
                first = _rows(hip.sinkhorn_step(EPS1, x, y, h, None, None, DAMPING, p=1, flags=flags), tags)
                fused = _rows(hip.sinkhorn_step(EPS1, x, y, h, pot, prev, DAMPING, p=1, flags=flags), tags)
                v = h.abs() / h.shape[-1]
                prods = {kind: _rows(hip.kernel_conv(kind, x, y, v, blur, flags=flags), tags) for kind in KINDS}
                for k, tag in enumerate(tags):
                    soft0, first0, soft, want = refs[tag][:4]
                    rep.add(D, f"softmin flags={flags} {tag}", np.abs(f[k] - soft0).max(), _sbound(soft0), "softmin")
                    rep.add(D, f"first half-step flags={flags} {tag}", np.abs(first[k] - first0).max(), _sbound(soft0), "half-step")
                    rep.add(D, f"averaged half-step flags={flags} {tag}", np.abs(fused[k] - want).max(), _sbound(soft), "half-step")
                    for kind in KINDS:
                        ref = refs[tag][6][kind]
                        rep.add(D, f"{kind} flags={flags} {tag}", np.abs(prods[kind][k] - ref).max(), _kbound(ref), kind)
    _print_tight(rep)
    _finish(rep)


# ---- 2. several row blocks and tiles ---------------------------------------------------------------------------------------------
def test_row_blocks_and_tiles(cuda):
    """N = 300, M = 270: two row blocks (the second of 44 rows, centred on its own first row), three column tiles, the last of 14
    columns; float32 and bfloat16 clouds (the reference on the rounded inputs)."""
    rep = _Report("row blocks")
    N, M = 300, 270
    for D in (17, 64, 130):
        x, y, h = _law(np.random.default_rng(2000 + D), N, M, D)
        blur = _blur(D)
        _family_is_dist(1, N, M, D, XKD)
        _check_all(rep, D, "f32", cuda, x, y, h, XKD, layout="f32")
        # bfloat16 clouds
        _family_is_dist(1, N, M, D, XKD, hip.BF16)
        xb, yb, ht = _t(x, cuda).bfloat16(), _t(y, cuda).bfloat16(), _t(h, cuda)
        xr, yr = xb.float().cpu().numpy(), yb.float().cpu().numpy()
        ref = oracle_c.softmin(EPS1, xr, yr, h, 1)
        out = hip.softmin(EPS1, xb, yb, ht, p=1, flags=XKD).cpu().numpy()
        rep.add(D, "softmin bf16", np.abs(out - ref).max(), _sbound(ref), "softmin bf16")
        v = _weights(h)
        for kind in KINDS:
            kref = oracle_c.kconv(kind, xr, yr, v, blur)
            kout = hip.kernel_conv(kind, xb, yb, _t(v, cuda), blur, flags=XKD).cpu().numpy()
            rep.add(D, f"{kind} bf16", np.abs(kout - kref).max(), _kbound(kref), f"{kind} bf16")
    _print_tight(rep)
    _finish(rep)


# ---- 3. column splits ------------------------------------------------------------------------------------------------------------
def test_column_splits(cuda):
    """N = 130, M = 70001, D = 24: split (the XCD-aware grid: M >= 65536) and unsplit launches against the oracle and each other."""
    rep = _Report("column splits")
    N, M, D = 130, 70001, 24
    x, y, h = _law(np.random.default_rng(3024), N, M, D)
    blur, v = _blur(D), _weights(h)
    xt, yt, ht, vt = _t(x, cuda), _t(y, cuda), _t(h, cuda), _t(v, cuda)
    assert hip.load_library().glhip_workspace_bytes(1, N, M, D, 0) >= 8 * N * 2 * 4      # room for the soft-min's (m, s) of >= 8 splits
    ref = oracle_c.softmin(EPS1, x, y, h, 1)
    outs = {}
    for flags in (XKD, XKD | NS):
        _family_is_dist(1, N, M, D, flags)
        outs[flags] = hip.softmin(EPS1, xt, yt, ht, p=1, flags=flags).cpu().numpy()
        rep.add(D, f"softmin flags={flags}", np.abs(outs[flags] - ref).max(), _sbound(ref), "softmin")
    rep.add(D, "softmin split vs unsplit", np.abs(outs[XKD] - outs[XKD | NS]).max(), 2 * _sbound(ref), "softmin pair")
    for kind in KINDS:
        kref = oracle_c.kconv(kind, x, y, v, blur)
        kouts = {flags: hip.kernel_conv(kind, xt, yt, vt, blur, flags=flags).cpu().numpy() for flags in (XKD, XKD | NS)}
        for flags, out in kouts.items():
            rep.add(D, f"{kind} flags={flags}", np.abs(out - kref).max(), _kbound(kref), kind)
        rep.add(D, f"{kind} split vs unsplit", np.abs(kouts[XKD] - kouts[XKD | NS]).max(), 2 * _kbound(kref), f"{kind} pair")
    _print_tight(rep)
    _finish(rep)


# ---- 4. near pairs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [17, 64, 130])
def test_near_pairs(cuda, D):
    """What the guard is for.  (a) the self-term y = x: the diagonal sits exactly on the clamp of utils.py:61; (b) y = x + 1e-4 noise:
    on the host the expanded form alone misses the soft-min bound of (b) by 21x / 53x / 75x at D = 17 / 64 / 130, so this case fails
    when the guard, the exact re-evaluation or its row / column index map is wrong."""
    rep = _Report(f"near pairs D={D}")
    N = M = 300
    rng = np.random.default_rng(1000 + D)
    x, _, h = _law(rng, N, M, D)
    _family_is_dist(1, N, M, D, XKD)
    _check_all(rep, D, "y = x", cuda, x, x.copy(), h, XKD, layout="self")
    y = (x + 1e-4 * rng.standard_normal((M, D))).astype(np.float32)
    _check_all(rep, D, "y = x + 1e-4 noise", cuda, x, y, h, XKD, layout="near")
    _print_tight(rep)
    _finish(rep)


# ---- 5. infinities and padding ---------------------------------------------------------------------------------------------------
def test_infinities_and_padding(cuda):
    """D = 33.  A quarter of the duals at -inf: values within the bound.  All duals at -inf: the behaviour of the D <= 16 distance
    kernel on the same input (first 16 coordinates), which is: +inf when M is a multiple of 32; otherwise the padded columns of the
    last group of 32 carry the dual -1e30 and every row returns the float32 value of eps ln(2) 1e30 — bit-identical between the two
    kernels in both cases.  Product weights of mixed sign: error relative to the product of |v|."""
    rep = _Report("infinities")
    D = 33
    x, y, h, *_ = _case(D)
    N, M = x.shape[0], y.shape[0]
    _family_is_dist(1, N, M, D, XKD)
    xt, yt = _t(x, cuda), _t(y, cuda)
    hq = np.array(h)
    hq[::4] = -np.inf
    ref = oracle_c.softmin(EPS1, x, y, hq, 1)
    out = hip.softmin(EPS1, xt, yt, _t(hq, cuda), p=1, flags=XKD).cpu().numpy()
    assert np.isfinite(out).all()
    rep.add(D, "softmin, a quarter of h at -inf", np.abs(out - ref).max(), _sbound(ref), "softmin")
    for Mi in (M, 160):      # 150 columns: a padded last group;  160: none
        yy = np.concatenate([y, y[: Mi - M] + np.float32(0.01)]) if Mi > M else y
        allinf = torch.full((Mi,), -math.inf, device=cuda)
        got = hip.softmin(EPS1, xt, _t(yy, cuda), allinf, p=1, flags=XKD | NS)
        low = hip.softmin(EPS1, xt[:, :16].contiguous(), _t(yy[:, :16], cuda), allinf, p=1, flags=NS)
        assert hip.softmin_fwd_family(1, N, Mi, 16, 1, hip.F32, NS) == hip.FAMILY_DIST
        print(f"all duals -inf, M = {Mi}: D = 33 gives {got[0].item():.6e}, the D = 16 kernel {low[0].item():.6e}")
        assert torch.equal(got, low), Mi
        assert bool(torch.isinf(got).all() and (got > 0).all()) if Mi % 32 == 0 else bool(torch.isfinite(got).all())
    # weights of mixed sign
    rng = np.random.default_rng(533)
    v = (rng.standard_normal(M) / M).astype(np.float32)
    blur = _blur(D)
    for kind in KINDS:
        kref, kabs = oracle_c.kconv(kind, x, y, v, blur), oracle_c.kconv(kind, x, y, np.abs(v), blur)
        kout = hip.kernel_conv(kind, xt, yt, _t(v, cuda), blur, flags=XKD).cpu().numpy()
        rep.add(D, f"{kind}, signed weights", np.abs(kout - kref).max(), _kbound(kabs), kind)
    _print_tight(rep)
    _finish(rep)


# ---- 6. the flag is opt-in -------------------------------------------------------------------------------------------------------
def test_flag_is_opt_in(cuda):
    x, y, h, *_ = _case(17)
    xt, yt, ht = _t(x, cuda), _t(y, cuda), _t(h, cuda)
    assert hip.softmin_fwd_family(1, x.shape[0], y.shape[0], 17, 1, hip.F32, 0) == hip.FAMILY_GENERIC
    assert hip.softmin_fwd_family(1, x.shape[0], y.shape[0], 17, 1, hip.F32, hip.FLAG_NO_MFMA) == hip.FAMILY_GENERIC
    plain = hip.softmin(EPS1, xt, yt, ht, p=1)
    generic = hip.softmin(EPS1, xt, yt, ht, p=1, flags=hip.FLAG_NO_MFMA)      # the generic kernel, before and after
    assert torch.equal(plain, generic)
    flagged = hip.softmin(EPS1, xt, yt, ht, p=1, flags=XKD)
    assert not torch.equal(plain, flagged)      # (another kernel: another rounding)
    for kind in KINDS:
        assert torch.equal(hip.kernel_conv(kind, xt, yt, ht.abs(), 0.5), hip.kernel_conv(kind, xt, yt, ht.abs(), 0.5, flags=hip.FLAG_NO_MFMA))
    # p = 2 and the gaussian product ignore the flag bit for bit
    x, y, h, *_ = _case(33)
    xt, yt, ht = _t(x, cuda), _t(y, cuda), _t(h, cuda)
    eps = 0.05**2 * 33 / 3
    assert torch.equal(hip.softmin(eps, xt, yt, ht, p=2), hip.softmin(eps, xt, yt, ht, p=2, flags=XKD))
    assert torch.equal(hip.kernel_conv("gaussian", xt, yt, ht.abs(), _blur(33)), hip.kernel_conv("gaussian", xt, yt, ht.abs(), _blur(33), flags=XKD))


# ---- 7. one launch per half-step -------------------------------------------------------------------------------------------------
def test_half_step_is_one_launch(cuda, monkeypatch):
    D = 24
    x, y, h, *_ = _case(D)
    N, M = x.shape[0], y.shape[0]
    pot, prev = _step_extras(D, "u", N, M)
    xt, yt, ht, pt, pv = (_t(a, cuda) for a in (x, y, h, pot, prev))
    _family_is_dist(1, N, M, D, XKD)
    calls = []
    raw = hip.sinkhorn_step_raw
    monkeypatch.setattr(hip, "sinkhorn_step_raw", lambda *a, **k: (calls.append(a[-1]), raw(*a, **k))[1])
    got = hip.sinkhorn_step(EPS1, xt, yt, ht, pt, pv, DAMPING, p=1, flags=XKD)
    assert len(calls) == 1 and calls[0] & XKD      # ONE glhip_sinkhorn_step call
    comp = 0.5 * (pv + DAMPING * hip.softmin(EPS1, xt, yt, _t(h + pot / np.float32(EPS1), cuda), p=1, flags=XKD))
    err = (got - comp).abs().max().item()
    print(f"fused half-step vs composition: {err:.3e}")
    assert err < 2e-6      # the bar of test_anyd_kernels_gpu.py::test_softmin_batched_bf16_and_fused_step
    hip.sinkhorn_step(EPS1, xt, yt, ht, pt, pv, DAMPING, p=1)      # without the flag: the composition, no glhip_sinkhorn_step call
    assert len(calls) == 1
    # the raw entry point: GLHIP_OK under the flag (GLHIP_EUNSUPPORTED = -2 without, as before; it returns before any launch)
    lib = hip.load_library()
    out = torch.empty(N, device=cuda)
    args = lambda flags: (xt.data_ptr(), yt.data_ptr(), ht.data_ptr(), pt.data_ptr(), pv.data_ptr(), out.data_ptr(), 1, N, M, D,  # noqa: E731
                          float(EPS1), float(DAMPING), 1, hip.F32, None, None, None, 0, None, 0, flags, None)
    assert lib.glhip_sinkhorn_step(*args(XKD | NS)) == 0
    torch.cuda.synchronize()
    assert (out - got).abs().max().item() < 2e-6
    assert lib.glhip_sinkhorn_step(*args(NS)) == -2


# ---- 8. end to end ---------------------------------------------------------------------------------------------------------------
def _e2e_clouds(D):
    """Two clouds of clearly different laws (y is narrower and shifted): the losses are then not a difference of nearly equal terms,
    and a relative bar on them is a statement about the kernels."""
    rng = np.random.default_rng(8000 + D)
    s = 0.5 + 0.5 * rng.random(D)
    x = (rng.random((300, D)) * s).astype(np.float32)
    y = ((rng.random((270, D)) * 0.5 + 0.4) * s).astype(np.float32)
    return x, y


@pytest.mark.parametrize("D", [24, 72])
@pytest.mark.parametrize("loss", ["sinkhorn", "laplacian", "energy"])
def test_end_to_end(cuda, monkeypatch, loss, D):
    """Online SamplesLoss on the new kernels (the default) and with the module switch off (GEOMLOSS_HIP_XK_DIST=0, latched at import)
    against the tensorized backend on float64 CPU copies: loss and dL/dx within 1e-4 relative (tests/test_samples_loss_gpu.py)."""
    from conftest import relerr
    x, y = _e2e_clouds(D)
    kw = dict(sinkhorn=dict(p=1, blur=0.3), laplacian=dict(blur=0.5), energy=dict())[loss]
    x64 = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    L64 = SamplesLoss(loss, backend="tensorized", **kw)(x64, torch.tensor(y, dtype=torch.float64))
    (g64,) = torch.autograd.grad(L64, [x64])
    L64, g64 = float(L64.detach()), g64.numpy()
    assert sinkhorn_samples._XK_DIST is True and kernel_samples._XK_DIST is True      # the default
    seen = []
    fwd, step, conv = hip.softmin_fwd_raw, hip.sinkhorn_step_raw, hip.kernel_conv_fwd_raw
    monkeypatch.setattr(hip, "softmin_fwd_raw", lambda *a, **k: (seen.append(a[-1]), fwd(*a, **k))[1])
    monkeypatch.setattr(hip, "sinkhorn_step_raw", lambda *a, **k: (seen.append(a[-1]), step(*a, **k))[1])
    monkeypatch.setattr(hip, "kernel_conv_fwd_raw", lambda *a, **k: (seen.append(a[-1]), conv(*a, **k))[1])
    fn = SamplesLoss(loss, backend="online", **kw)
    res = {}
    for on in (True, False):
        monkeypatch.setattr(sinkhorn_samples, "_XK_DIST", on)
        monkeypatch.setattr(kernel_samples, "_XK_DIST", on)
        del seen[:]
        xt = _t(x, cuda).requires_grad_(True)
        L = fn(xt, _t(y, cuda))
        (g,) = torch.autograd.grad(L, [xt])
        res[on] = (float(L.detach()), g.cpu().numpy())
        assert len(seen) > 0 and all(bool(int(f) & XKD) == on for f in seen), (on, seen)
        print(f"{loss} D={D} flag {'on' if on else 'off'}: loss rel. err {abs(res[on][0] - L64) / abs(L64):.2e}, gradient {relerr(res[on][1], g64):.2e}")
        assert abs(res[on][0] - L64) <= 1e-4 * abs(L64), (on, res[on][0], L64)
        assert relerr(res[on][1], g64) <= 1e-4, on
    assert abs(res[True][0] - res[False][0]) < 1e-5 * abs(res[False][0])
