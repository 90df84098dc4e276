"""Clouds of dimension D > 16: the K-chunked matrix-core kernel (``csrc/glhip_softmin_xk.h``: p = 2 soft-min forward, fused Sinkhorn
half-step and gaussian product for 17 <= D <= 4095), gradients in any dimension (``csrc/glhip_generic.h``), the kernel-family query
of the C-ABI, and ``SamplesLoss`` end to end against reference-generated fixtures (tests/golden/make_golden_anyd.py).  Oracles:
``oracle/oracle_c.c`` in float64 on the same float32 (or bf16-rounded) inputs, sampled rows of ``oracle/oracle_torch64.py`` for the
big launches.  Every figure is printed before it is asserted (``pytest -s``)."""

import ctypes
import math

import numpy as np
import pytest
import torch

from cloud_support import clouds as _clouds, random_ranges as _random_ranges, to_dev as _t, tol as _tol
from conftest import load_golden, relerr
from geomloss_amd import SamplesLoss, hip
from geomloss_amd.cluster import from_matrix
from oracle import oracle_c
from oracle import oracle_torch64 as o64

pytestmark = pytest.mark.gpu

H2 = hip.FLAG_F16X2


# ---- 1. soft-min forward ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [17, 24, 32, 33, 64, 100, 128, 257])
@pytest.mark.parametrize("N,M", [(300, 257), (1030, 2100), (64, 8), (1, 1), (5, 3000)])
@pytest.mark.parametrize("eps_kind", ["one", "small"])
def test_softmin_fwd_vs_oracle(cuda, D, N, M, eps_kind):
    eps = 1.0 if eps_kind == "one" else 0.05**2 * D / 3
    x, y, h = _clouds(N + M + D, N, M, D)
    ref = oracle_c.softmin(eps, x, y, h, 2)
    assert hip.softmin_fwd_family(1, N, M, D, 2) == hip.FAMILY_XK
    for flags in (0, hip.FLAG_NO_SPLIT, H2, H2 | hip.FLAG_NO_SPLIT):
        out = hip.softmin(eps, _t(x, cuda), _t(y, cuda), _t(h, cuda), p=2, flags=flags).cpu().numpy()
        err = np.abs(out - ref).max()
        print(f"softmin D={D} N={N} M={M} eps={eps:.4g} flags={flags}: err {err:.3e} tol {_tol(ref, D):.3e}")
        assert err < _tol(ref, D), flags


# ---- 2. the paths of the launcher on big launches --------------------------------------------------------------------------

def _softmin_with_workspace(x, y, h, eps, ws_bytes, flags=0):
    """glhip_softmin_fwd through the C-ABI with a workspace of the caller's size (hip.softmin always hands over glhip_workspace_bytes)."""
    lib = hip.load_library()
    N, D = x.shape
    M = y.shape[0]
    out = torch.empty(N, dtype=torch.float32, device=x.device)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=x.device)
    rc = lib.glhip_softmin_fwd(x.data_ptr(), y.data_ptr(), h.data_ptr(), out.data_ptr(), 1, N, M, D, float(eps), 2, hip.F32, None, None, None, 0,
                               ctypes.c_void_p(ws.data_ptr()) if ws_bytes else None, ws_bytes, flags,
                               ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    assert rc == 0, lib.glhip_last_error()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("D,N,M", [(32, 700, 70_001), (64, 9_000, 66_000), (128, 40_000, 3_000)])
def test_softmin_fwd_large_launch_paths(cuda, D, N, M):
    """M >= 65536: the XCD-aware 1-D grid with 8 - 32 column splits (M not a multiple of the 128-column tile, late maxima in the last,
    short split); N = 40000: 157 row blocks, the last one partial, splits by choose_splits.  The kernel stages its tiles on the fly: there
    is no pre-packed path; a workspace too small for the splits the launch wants (3 splits' worth, then none) must still run.  100
    sampled rows against the float64 oracle, every row against the unsplit launch."""
    x, y, h = _clouds(D + N, N, M, D)
    h[-5:] += 30.0
    eps = 0.07**2 * D / 3
    rows = np.unique(np.r_[0, 255, 256, N - 1, np.random.default_rng(1).integers(0, N, 100)])
    ref = o64.softmin(eps, x, y, h, rows=rows, device=cuda)
    xt, yt, ht = _t(x, cuda), _t(y, cuda), _t(h, cuda)
    out = hip.softmin(eps, xt, yt, ht).cpu().numpy()
    err = np.abs(out[rows] - ref).max()
    print(f"large D={D} N={N} M={M}: err {err:.3e} tol {_tol(ref, D):.3e}")
    assert np.isfinite(out).all() and err < _tol(ref, D)
    want = hip.load_library().glhip_workspace_bytes(1, N, M, D, 0)
    assert want >= 2 * N * 8        # room for at least two splits of 2 floats per row
    for flags, ws in ((hip.FLAG_NO_SPLIT, want), (0, 3 * N * 8), (0, 0), (H2, want), (H2, 3 * N * 8)):
        alt = _softmin_with_workspace(xt, yt, ht, eps, ws, flags).cpu().numpy()
        d = np.abs(out - alt).max()
        print(f"   flags={flags} workspace={ws}: max diff to the default launch {d:.3e}")
        assert np.abs(alt[rows] - ref).max() < _tol(ref, D) and d < 2 * _tol(ref, D), (flags, ws)


# ---- 3. batches, bf16 clouds, the fused half-step --------------------------------------------------------------------------

def test_softmin_batched_bf16_and_fused_step(cuda):
    B, N, M, D = 3, 257, 300, 64
    x, y, logw = _clouds(3, N, M, D, B=B)
    xb, yb = _t(x, cuda).bfloat16(), _t(y, cuda).bfloat16()
    eps = 0.02 * D / 3
    ref = np.stack([oracle_c.softmin(eps, xb[b].float().cpu().numpy(), yb[b].float().cpu().numpy(), logw[b], 2) for b in range(B)])
    for flags in (0, H2):
        out = hip.softmin(eps, xb, yb, _t(logw, cuda), flags=flags).cpu().numpy()
        print(f"bf16 batch flags={flags}: err {np.abs(out - ref).max():.3e} tol {_tol(ref, D):.3e}")
        assert out.shape == (B, N) and np.abs(out - ref).max() < _tol(ref, D)
    # glhip_sinkhorn_step == (prev + damping * softmin(eps, C, logw + pot / eps)) / 2, composed in float64 from the float64 oracle
    rng = np.random.default_rng(8)
    pot = (rng.standard_normal(logw.shape) * 0.05).astype(np.float32)
    prev = rng.standard_normal(x.shape[:-1]).astype(np.float32)
    damping = 0.8
    hcol = logw.astype(np.float64) + pot.astype(np.float64) / eps
    soft = np.stack([oracle_c.softmin(eps, x[b], y[b], hcol[b], 2) for b in range(B)])
    want = 0.5 * (prev.astype(np.float64) + damping * soft)
    xt, yt = _t(x, cuda), _t(y, cuda)
    assert hip.half_step_applies(D, 2) and not hip.half_step_applies(D, 1) and not hip.half_step_applies(D, 2, hip.FLAG_NO_MFMA)
    assert hip.half_step_applies(4095, 2) and not hip.half_step_applies(4096, 2)
    for flags in (0, H2, hip.FLAG_NO_SPLIT):
        fused = hip.sinkhorn_step(eps, xt, yt, _t(logw, cuda), _t(pot, cuda), _t(prev, cuda), damping, flags=flags).cpu().numpy()
        # (float32 h = logw + pot / eps of the composition is rounded at ~2^-24 |h| eps on the potential: inside the bound)
        print(f"half-step flags={flags}: err {np.abs(fused - want).max():.3e} tol {_tol(soft, D):.3e}")
        assert np.abs(fused - want).max() < _tol(soft, D), flags
    first = hip.sinkhorn_step(eps, xt, yt, _t(logw, cuda), None, None, damping).cpu().numpy()
    ref1 = damping * np.stack([oracle_c.softmin(eps, x[b], y[b], logw[b], 2) for b in range(B)])
    assert np.abs(first - ref1).max() < _tol(ref1, D)
    # p = 1 and the VALU flags have no fused kernel beyond D = 16: the composition, same numbers as before
    for kw in (dict(p=1), dict(flags=hip.FLAG_NO_MFMA)):
        got = hip.sinkhorn_step(eps, xt, yt, _t(logw, cuda), _t(pot, cuda), _t(prev, cuda), damping, **kw)
        comp = 0.5 * (_t(prev, cuda) + damping * hip.softmin(eps, xt, yt, _t(logw + pot / np.float32(eps), cuda), **kw))
        assert (got - comp).abs().max().item() < 2e-6, kw


# ---- 4. block-sparse launches ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ci,cj", [(9, 11), (60, 70)])
def test_block_sparse_softmin_and_gaussian(cuda, ci, cj):
    """Ragged ranges at D = 32; 60 x 70 clusters: row clusters of ~40 points whose tiles gather several column intervals."""
    D = 32
    rng = np.random.default_rng(17)
    N, M = 2300, 2600
    x, y, h = _clouds(23, N, M, D)
    rg, tup, _, _, ri = _random_ranges(rng, N, M, ci, cj, 0.4, cuda)
    eps = 0.02 * D / 3
    ref = oracle_c.softmin(eps, x, y, h, 2, ranges=tup)
    empty = slice(ri[0, 0], ri[0, 1])
    live = np.ones(N, bool)
    live[empty] = False
    assert hip.softmin_fwd_family(1, N, M, D, 2, n_ranges=ci) == hip.FAMILY_XK
    for flags in (0, hip.FLAG_NO_SPLIT, H2, H2 | hip.FLAG_NO_SPLIT):
        out = hip.softmin(eps, _t(x, cuda), _t(y, cuda), _t(h, cuda), ranges=rg, flags=flags).cpu().numpy()
        print(f"sparse softmin {ci}x{cj} flags={flags}: err {np.abs(out[live] - ref[live]).max():.3e} tol {_tol(ref[live], D):.3e}")
        assert np.isposinf(out[empty]).all() and np.isposinf(ref[empty]).all(), flags
        assert np.abs(out[live] - ref[live]).max() < _tol(ref[live], D), flags
    v = (np.abs(h) / M).astype(np.float32)
    blur = 0.3 * math.sqrt(D / 3)
    refk = oracle_c.kconv("gaussian", x, y, v, blur, ranges=tup)
    assert hip.kernel_conv_fwd_family("gaussian", 1, N, M, D, n_ranges=ci) == hip.FAMILY_XK
    for flags in (0, H2):
        k = hip.kernel_conv("gaussian", _t(x, cuda), _t(y, cuda), _t(v, cuda), blur, ranges=rg, flags=flags).cpu().numpy()
        print(f"sparse gaussian {ci}x{cj} flags={flags}: relerr {relerr(k, refk):.3e}")
        assert (k[empty] == 0).all() and relerr(k, refk) < 1e-4, flags


# ---- 5. the explicit running maximum, infinities ---------------------------------------------------------------------------

def test_softmin_lazy_max_and_infinities(cuda):
    """Late maxima, -inf / -1e5 dual values, a row block whose columns are all massless, spikes of +1e4 late in h: both layouts."""
    D = 40
    N, M = 130, 2500
    x, y, h = _clouds(9 + D, N, M, D)
    h[:] = -50.0
    h[-1] = 80.0
    h[5] = -np.inf
    h[6] = -100000.0
    eps = 0.05**2 * D / 3
    ref = oracle_c.softmin(eps, x, y, h, 2)
    for flags in (0, hip.FLAG_NO_SPLIT, H2, H2 | hip.FLAG_NO_SPLIT):
        out = hip.softmin(eps, _t(x, cuda), _t(y, cuda), _t(h, cuda), flags=flags).cpu().numpy()
        print(f"lazy max flags={flags}: err {np.abs(out - ref).max():.3e} tol {_tol(ref, D):.3e}")
        assert np.isfinite(out).all() and np.abs(out - ref).max() < _tol(ref, D), flags
    h2 = (np.arange(M) // 64 * 48.0).astype(np.float32)
    h2[M // 2:] -= 3000.0
    h2[-3] = 1.0e4                                   # a late spike of +1e4
    h2[M // 3] = 1.0e4 - 7.0
    ref2 = oracle_c.softmin(eps, x, y, h2, 2)
    for flags in (0, H2):
        out2 = hip.softmin(eps, _t(x, cuda), _t(y, cuda), _t(h2, cuda), flags=flags).cpu().numpy()
        print(f"spikes flags={flags}: relerr {relerr(out2, ref2):.3e}")
        assert np.isfinite(out2).all() and relerr(out2, ref2) < 2e-6, flags
    # a measure without any mass, as xd_fwd_kernel: the bf16 x 3 layout is left with the -1e30 of its padded columns (a huge finite
    # potential; the reference returns +inf), the f16 x 2 layout recognises a row that never left its floor (+inf)
    allinf = hip.softmin(eps, _t(x, cuda), _t(y, cuda), torch.full((M,), -math.inf, device=cuda)).cpu().numpy()
    assert (allinf > 1e20).all()
    allinf = hip.softmin(eps, _t(x, cuda), _t(y, cuda), torch.full((M,), -math.inf, device=cuda), flags=H2).cpu().numpy()
    assert np.isposinf(allinf).all()
    # rows whose columns are all massless next to rows that see mass: block-sparse, row block 1 reduces over massless columns only
    ri = torch.tensor([[0, 64], [64, N]], dtype=torch.int32, device=cuda)
    rj = torch.tensor([[0, 1000], [1000, M]], dtype=torch.int32, device=cuda)
    keep = torch.tensor([[True, True], [False, True]], device=cuda)
    rg = from_matrix(ri, rj, keep)
    h3 = _clouds(1, N, M, D)[2]
    h3[1000:] = -np.inf
    tup = tuple(t.cpu().numpy() for t in (rg.ranges_i, rg.slices_i, rg.redranges_j))
    ref3 = oracle_c.softmin(eps, x, y, h3, 2, ranges=tup)
    assert np.isposinf(ref3[64:]).all() and np.isfinite(ref3[:64]).all()
    for flags in (0, H2):
        out3 = hip.softmin(eps, _t(x, cuda), _t(y, cuda), _t(h3, cuda), ranges=rg, flags=flags).cpu().numpy()
        assert np.abs(out3[:64] - ref3[:64]).max() < _tol(ref3[:64], D), flags
        assert (out3[64:] > 1e20).all(), flags      # +inf, or the huge finite value of the padded columns (bf16 x 3)
    # non-finite coordinates propagate to their rows, as in every kernel of the library
    xn = x.copy()
    xn[7, 3] = np.nan
    outn = hip.softmin(eps, _t(xn, cuda), _t(y, cuda), _t(h, cuda)).cpu().numpy()
    assert np.isnan(outn[7])


# ---- 6. gaussian product ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,N,M,B", [(D, N, M, B) for D in (17, 64, 128) for N, M, B in ((300, 257, None), (1030, 2100, None), (150, 170, 3))]
                         + [(64, 700, 70_001, None)])      # (the many-column launch for one dimension)
def test_gaussian_product_vs_oracle(cuda, D, N, M, B):
    x, y, v = _clouds(77 + D, N, M, D, B=B)
    v = np.abs(v) / M
    v[..., ::7] *= -1.0                                    # signed weights are legal
    blur = 0.25 * math.sqrt(D / 3)
    one = lambda xa, ya, va: oracle_c.kconv("gaussian", xa, ya, va, blur)      # noqa: E731
    ref = one(x, y, v) if B is None else np.stack([one(x[b], y[b], v[b]) for b in range(B)])
    bound = one(x, y, np.abs(v)) if B is None else np.stack([one(x[b], y[b], np.abs(v[b])) for b in range(B)])
    tol = 3e-6 * np.abs(ref).max() + 2.4e-7 * D / blur**2 * np.abs(bound).max()     # as tests/test_xd_kernels_gpu.py
    assert hip.kernel_conv_fwd_family("gaussian", B or 1, N, M, D) == hip.FAMILY_XK       # the launch's own predicate: no silent fallback
    assert hip.kernel_conv_fwd_family("gaussian", B or 1, N, M, D, flags=hip.FLAG_NO_MFMA) == hip.FAMILY_GENERIC
    for flags in (0, hip.FLAG_NO_SPLIT, H2, hip.FLAG_NO_MFMA):
        out = hip.kernel_conv("gaussian", _t(x, cuda), _t(y, cuda), _t(v, cuda), blur, flags=flags).cpu().numpy()
        print(f"gaussian D={D} N={N} M={M} B={B} flags={flags}: err {np.abs(out - ref).max():.3e} tol {tol:.3e}")
        assert np.abs(out - ref).max() < tol, flags


# ---- 7. gradients in any dimension -----------------------------------------------------------------------------------------

GRAD_D = [65, 100, 128, 300]
# Reference: the float64 oracle of oracle/oracle_torch64.py — the C oracle's gradients (oracle_c.softmin_grad_x / kconv_grad_x) keep 64
# accumulators per row and leave the coordinates beyond them unwritten, so they cannot referee D > 64.  Both restate the same closed
# form; tests/test_oracle_golden.py pins them to the reference.


def _f32_torch_softmin_grad_error(eps, x, y, h, g, ref):
    """e_ref: the p = 2 soft-min gradient in plain float32 torch (the reference's tensorized arithmetic) against float64."""
    if x.ndim == 3:
        return max(_f32_torch_softmin_grad_error(eps, x[b], y[b], h[b], g[b], ref[b]) for b in range(x.shape[0]))
    xt = torch.from_numpy(x).requires_grad_(True)
    yt, ht = torch.from_numpy(y), torch.from_numpy(h)
    C = ((xt[:, None, :] - yt[None, :, :]) ** 2).sum(-1) / 2
    out = -eps * torch.logsumexp(ht[None, :] - C / eps, dim=1)
    (gx,) = torch.autograd.grad(out, [xt], grad_outputs=torch.from_numpy(g))
    return relerr(gx.numpy(), ref)


@pytest.mark.parametrize("D", GRAD_D)
@pytest.mark.parametrize("p", [2, 1])
@pytest.mark.parametrize("B", [None, 3])
def test_softmin_gradient_any_dimension(cuda, D, p, B):
    """Inputs and eps of tests/test_hip_kernels.py::test_generic_dimension_softmin, bound 5e-6 of the largest entry.  These raised
    NotImplementedError before the gradient kernel swept its output coordinates in passes of 64.

    p = 2 at D = 300 misses 5e-6 in the batched case (measured on an MI355X, relerr / e_ref: D = 65: 7.1e-7 / 3.7e-7, 100: 1.3e-6 /
    5.1e-7, 128: 1.2e-6 / 5.8e-7, 300: 4.7e-6 / 1.8e-6 unbatched; batched 8.6e-7, 2.1e-6, 2.0e-6, 5.9e-6): the kernel sums the D squares
    of a distance serially in float32.  There the bound is max(5e-6, 4 e_ref), e_ref = the error of the same gradient in plain float32
    torch (pairwise sums) on the same inputs, computed here — 4: a serial sum against a pairwise one.  profiles/r08_anyd.txt."""
    N, M = 270, 310
    x, y, h = _clouds(51 + D, N, M, D, B=B)
    g = np.random.default_rng(6).standard_normal(x.shape[:-1]).astype(np.float32)
    eps = 0.3
    one = lambda xa, ya, ha, ga: o64.softmin_grad_x(eps, xa, ya, ha, ga, p, device=cuda)        # noqa: E731
    ref = one(x, y, h, g) if B is None else np.stack([one(x[b], y[b], h[b], g[b]) for b in range(B)])
    xt = _t(x, cuda).requires_grad_(True)
    out = hip.softmin(eps, xt, _t(y, cuda), _t(h, cuda), p=p)
    (gx,) = torch.autograd.grad(out, [xt], grad_outputs=_t(g, cuda))
    err = relerr(gx.cpu().numpy(), ref)
    e_ref = _f32_torch_softmin_grad_error(eps, x, y, h, g, ref) if p == 2 else float("nan")
    bound = max(5e-6, 4 * e_ref) if (p == 2 and D == 300) else 5e-6
    print(f"softmin gradient D={D} p={p} B={B}: relerr {err:.3e}   float32 torch e_ref {e_ref:.3e}   bound {bound:.3e}")
    assert gx.shape == xt.shape and err < bound


@pytest.mark.parametrize("D", GRAD_D)
@pytest.mark.parametrize("kind", ["gaussian", "laplacian", "energy"])
@pytest.mark.parametrize("B", [None, 3])
def test_kernel_gradient_any_dimension(cuda, D, kind, B):
    N, M = 270, 310
    x, y, v = _clouds(61 + D, N, M, D, B=B)
    v = (np.abs(v) / M).astype(np.float32)
    g = np.random.default_rng(7).standard_normal(x.shape[:-1]).astype(np.float32)
    blur = 0.3 * math.sqrt(D / 3)
    one = lambda xa, ya, va, ga: o64.kconv_grad_x(kind, xa, ya, va, ga, blur, device=cuda)        # noqa: E731
    ref = one(x, y, v, g) if B is None else np.stack([one(x[b], y[b], v[b], g[b]) for b in range(B)])
    xt = _t(x, cuda).requires_grad_(True)
    out = hip.kernel_conv(kind, xt, _t(y, cuda), _t(v, cuda), blur)
    (gx,) = torch.autograd.grad(out, [xt], grad_outputs=_t(g, cuda))
    err = relerr(gx.cpu().numpy(), ref)
    print(f"{kind} gradient D={D} B={B}: relerr {err:.3e}")
    assert gx.shape == xt.shape and err < 5e-6


def _masked_f64_gradients(eps, blur, x, y, h, v, g, tup, dev):
    """float64 autograd through the masked dense matrices: gradients of the block-sparse p = 2 / p = 1 soft-min and gaussian product."""
    ri, si, rj = tup
    mask = torch.zeros(x.shape[0], y.shape[0], dtype=torch.bool, device=dev)
    for k in range(len(ri)):
        for q in range(0 if k == 0 else si[k - 1], si[k]):
            mask[ri[k, 0]:ri[k, 1], rj[q, 0]:rj[q, 1]] = True
    xt = torch.from_numpy(x).double().to(dev).requires_grad_(True)
    yt, ht, vt, gt = (torch.from_numpy(t).double().to(dev) for t in (y, h, v, g))
    d2 = ((xt * xt).sum(1)[:, None] + (yt * yt).sum(1)[None, :] - 2 * xt @ yt.T).clamp_min(0)
    out = {}
    live = mask.any(1)
    for name, f in (("p2", lambda: -eps * torch.logsumexp(torch.where(mask, ht[None, :] - d2 / (2 * eps), -math.inf)[live], 1)),
                    ("p1", lambda: -eps * torch.logsumexp(torch.where(mask, ht[None, :] - d2.clamp_min(1e-8).sqrt() / eps, -math.inf)[live], 1)),
                    ("gaussian", lambda: ((torch.exp(-d2 / (2 * blur**2)) * mask) @ vt)[live])):
        (gx,) = torch.autograd.grad(f(), [xt], grad_outputs=gt[live], retain_graph=True)
        out[name] = gx.cpu().numpy()
    return out


def test_block_sparse_gradients_any_dimension(cuda):
    D = 100
    rng = np.random.default_rng(19)
    N, M = 900, 1000
    x, y, h = _clouds(29, N, M, D)
    rg, tup, _, _, ri = _random_ranges(rng, N, M, 9, 11, 0.5, cuda)
    live = np.ones(N, bool)
    live[ri[0, 0]:ri[0, 1]] = False
    g = rng.standard_normal(N).astype(np.float32)
    eps = 0.3
    v = (np.abs(h) / M).astype(np.float32)
    blur = 0.3 * math.sqrt(D / 3)
    refs = _masked_f64_gradients(eps, blur, x, y, h, v, g, tup, cuda)
    for p in (2, 1):
        ref = refs[f"p{p}"]
        xt = _t(x, cuda).requires_grad_(True)
        out = hip.softmin(eps, xt, _t(y, cuda), _t(h, cuda), p=p, ranges=rg)
        (gx,) = torch.autograd.grad(out, [xt], grad_outputs=_t(g, cuda))
        err = relerr(gx.cpu().numpy()[live], ref[live])
        print(f"block-sparse softmin gradient p={p}: relerr {err:.3e}")
        assert err < 5e-6, p
    refk = refs["gaussian"]
    xt = _t(x, cuda).requires_grad_(True)
    out = hip.kernel_conv("gaussian", xt, _t(y, cuda), _t(v, cuda), blur, ranges=rg)
    (gx,) = torch.autograd.grad(out, [xt], grad_outputs=_t(g, cuda))
    err = relerr(gx.cpu().numpy(), refk)
    print(f"block-sparse gaussian gradient: relerr {err:.3e}")
    assert err < 5e-6


# ---- 8. SamplesLoss end to end against the reference -----------------------------------------------------------------------

@pytest.mark.parametrize("name", ["sinkhorn_d32", "sinkhorn_d128", "gaussian_d128"])
def test_samples_loss_matches_reference(cuda, name):
    """backend="online" on float32 clouds of D = 32 / 128 against the reference's float64 tensorized run: loss, gradients and
    potentials at the 1e-4 relative bar of tests/test_samples_loss_gpu.py.  (D = 128: the gradient raised before.)"""
    rec = load_golden("reference_anyd_" + name)
    a, x, b, y = (_t(rec[k], cuda) for k in ("a", "x", "b", "y"))
    x.requires_grad_(True)
    a.requires_grad_(True)
    L = SamplesLoss(backend="online", **rec["kwargs"])(a, x, b, y)
    gx, ga = torch.autograd.grad(L, [x, a])
    F, G = SamplesLoss(backend="online", potentials=True, **rec["kwargs"])(a.detach(), x.detach(), b, y)
    figs = dict(loss=relerr(L.item(), rec["loss_f64"]), gx=relerr(gx.cpu().numpy(), rec["gx_f64"]), ga=relerr(ga.cpu().numpy(), rec["ga_f64"]),
                F=relerr(F.cpu().numpy().reshape(-1), rec["F_f64"].reshape(-1)), G=relerr(G.cpu().numpy().reshape(-1), rec["G_f64"].reshape(-1)))
    print(name, {k: f"{v:.2e}" for k, v in figs.items()})
    assert all(v < 1e-4 for v in figs.values()), figs


def test_multiscale_with_user_labels_reaches_the_block_sparse_kernel(cuda, monkeypatch):
    """The reference's recipe for D > 3: clusters given as labels, the two-scale solver on 24-D clouds — against the online backend
    (truncation error of a two-scale run ~1e-3 of the loss, as tests/test_xd_kernels_gpu.py::test_multiscale_4d_with_user_labels).
    The raw launchers are watched: the fine level must issue block-sparse launches in D = 24, and the library's own predicate must
    put those shapes on the K-chunked matrix-core kernel."""
    seen = []
    for fn in ("softmin_fwd_raw", "sinkhorn_step_raw"):
        orig = getattr(hip, fn)

        def spy(x, y, *a, _orig=orig, _ri=(5 if fn == "softmin_fwd_raw" else 8), **k):
            ranges = k.get("ranges", a[_ri - 2] if len(a) > _ri - 2 else None)
            flags = k.get("flags", a[_ri - 1] if len(a) > _ri - 1 else 0)
            seen.append((x.shape[0], x.shape[1], y.shape[1], x.shape[2], None if ranges is None else int(ranges.ranges_i.shape[0]), int(flags)))
            return _orig(x, y, *a, **k)

        monkeypatch.setattr(hip, fn, spy)
    g = torch.Generator().manual_seed(7)
    N, M, D = 3000, 3500, 24
    x = torch.rand(N, D, generator=g).to(cuda)
    y = (torch.rand(M, D, generator=g) * 0.8 + 0.1).to(cuda)

    def lab(t):       # voxels of the first three coordinates, in voxel order
        code = ((t[:, :3] / 0.25).floor().long() * torch.tensor([16, 4, 1], device=cuda)).sum(1)
        return torch.unique(code, return_inverse=True)[1].int()

    kw = dict(p=2, blur=0.3, scaling=0.7)
    a, b = torch.full((N,), 1.0 / N, device=cuda), torch.full((M,), 1.0 / M, device=cuda)
    import geomloss_amd.sinkhorn_samples as ss
    monkeypatch.setattr(ss, "_DENSE_SWITCH", "0")      # keep the truncated pattern of the fine level (the switch may run it dense: a cost model)
    Lm = SamplesLoss("sinkhorn", backend="multiscale", **kw)(lab(x), a, x, lab(y), b, y)
    Lo = SamplesLoss("sinkhorn", backend="online", **kw)(x, y)
    sparse = [s for s in seen if s[4] is not None]
    print(f"multiscale {Lm.item():.6e} online {Lo.item():.6e}; {len(sparse)} block-sparse launches of {len(seen)}")
    assert sparse and all(s[3] == D for s in sparse)
    for B_, N_, M_, D_, nr, fl in sparse:
        assert hip.softmin_fwd_family(B_, N_, M_, D_, 2, hip.F32, fl, nr) == hip.FAMILY_XK, (N_, M_, nr, fl)
    assert abs(Lm.item() - Lo.item()) < 5e-3 * abs(Lo.item())


# ---- 9. which kernel a shape selects ---------------------------------------------------------------------------------------

def test_kernel_family_query():
    """glhip_softmin_fwd_family: the predicate of the launch itself, host arithmetic only (no device is touched)."""
    F = hip.softmin_fwd_family
    NM, DI = hip.FLAG_NO_MFMA, hip.FLAG_DIRECT
    cases = [
        # (B, N, M, D, p, flags, n_ranges) -> family
        ((1, 1000, 1000, 1, 2, 0, 0), hip.FAMILY_X32), ((1, 1000, 1000, 3, 2, 0, 0), hip.FAMILY_X32), ((1, 1000, 1000, 3, 2, 0, 12), hip.FAMILY_X32),
        ((1, 1000, 1000, 3, 2, NM, 0), hip.FAMILY_VALU), ((1, 1000, 1000, 3, 2, DI, 0), hip.FAMILY_VALU), ((1, 1000, 1000, 3, 1, 0, 0), hip.FAMILY_VALU),
        ((1, 1000, 1000, 3, 1, hip.FLAG_MFMA_DIST, 12), hip.FAMILY_DIST), ((1, 40000, 70000, 3, 2, H2, 0), hip.FAMILY_XD),
        ((1, 1000, 1000, 4, 2, 0, 0), hip.FAMILY_XD), ((4, 1000, 1000, 16, 2, 0, 0), hip.FAMILY_XD), ((1, 1000, 1000, 16, 2, 0, 12), hip.FAMILY_XD),
        ((1, 1000, 1000, 16, 2, NM, 0), hip.FAMILY_GENERIC), ((1, 1000, 1000, 4, 1, 0, 0), hip.FAMILY_DIST), ((1, 1000, 1000, 16, 1, 0, 12), hip.FAMILY_GENERIC),
        ((1, 1000, 1000, 17, 2, 0, 0), hip.FAMILY_XK), ((3, 1000, 1000, 64, 2, H2, 0), hip.FAMILY_XK), ((1, 1000, 1000, 64, 2, 0, 12), hip.FAMILY_XK),
        ((1, 1000, 1000, 4095, 2, 0, 0), hip.FAMILY_XK), ((1, 1000, 1000, 64, 2, NM, 0), hip.FAMILY_GENERIC), ((1, 1000, 1000, 64, 2, DI, 0), hip.FAMILY_GENERIC),
        ((1, 1000, 1000, 17, 1, 0, 0), hip.FAMILY_GENERIC), ((1, 1000, 1000, 64, 1, 0, 12), hip.FAMILY_GENERIC), ((1, 1000, 1000, 4096, 2, 0, 0), hip.FAMILY_GENERIC),
    ]
    for (B, N, M, D, p, flags, nr), want in cases:
        for dt in (hip.F32, hip.BF16):
            assert F(B, N, M, D, p, dt, flags, nr) == want, (B, N, M, D, p, flags, nr)
    assert F(1, 1000, 1000, 17, 2, hip.F32, 0, 0) == hip.FAMILY_XK == 3
    assert hip.MFMA_FWD_MAX_DIM == 4095 and F(1, 10, 10, hip.MFMA_FWD_MAX_DIM, 2) == hip.FAMILY_XK != F(1, 10, 10, hip.MFMA_FWD_MAX_DIM + 1, 2)
    # big dense D <= 3 launches sort their clouds and run block-sparse: p = 1 on the distance kernels, p = 2 (>= 1e11 pairs) on the x32 kernel
    assert F(1, 100_000, 100_000, 3, 1) == hip.FAMILY_DIST and F(1, 100_000, 100_000, 3, 1, flags=hip.FLAG_NO_SORT) == hip.FAMILY_VALU
    assert F(1, 1_000_000, 1_000_000, 3, 2) == hip.FAMILY_X32
    for bad in (dict(D=0), dict(p=3), dict(dtype=7), dict(N=-1)):
        with pytest.raises(ValueError):
            F(**{**dict(B=1, N=10, M=10, D=3, p=2, dtype=hip.F32), **bad})
    # kernel products: glhip_kernel_conv_fwd_family
    K = hip.kernel_conv_fwd_family
    for (kind, B, D, flags, nr), want in [
            (("gaussian", 1, 3, 0, 0), hip.FAMILY_X32), (("gaussian", 1, 3, NM, 0), hip.FAMILY_VALU), (("gaussian", 2, 8, 0, 0), hip.FAMILY_XD),
            (("gaussian", 1, 16, 0, 12), hip.FAMILY_XD), (("gaussian", 1, 17, 0, 0), hip.FAMILY_XK), (("gaussian", 3, 128, H2, 0), hip.FAMILY_XK),
            (("gaussian", 1, 64, 0, 12), hip.FAMILY_XK), (("gaussian", 1, 4095, DI, 0), hip.FAMILY_XK), (("gaussian", 1, 64, NM, 0), hip.FAMILY_GENERIC),
            (("gaussian", 1, 4096, 0, 0), hip.FAMILY_GENERIC), (("laplacian", 1, 3, 0, 0), hip.FAMILY_VALU),
            (("energy", 1, 3, hip.FLAG_MFMA_DIST, 12), hip.FAMILY_DIST), (("laplacian", 1, 8, 0, 0), hip.FAMILY_DIST),
            (("energy", 1, 8, 0, 12), hip.FAMILY_GENERIC), (("laplacian", 1, 64, 0, 0), hip.FAMILY_GENERIC)]:
        assert K(kind, B, 1000, 1000, D, hip.F32, flags, nr) == want, (kind, B, D, flags, nr)
    assert K("energy", 1, 100_000, 100_000, 3) == hip.FAMILY_DIST      # sorted inside the library
    with pytest.raises(ValueError):
        K(5, 1, 10, 10, 3)
    lib = hip.load_library()
    assert lib.glhip_version() >= 121
    assert lib.glhip_workspace_bytes(1, 10_000, 10_000, 64, 0) > 0 and lib.glhip_workspace_bytes(1, 10_000, 10_000, 4096, 0) == 0


def test_beyond_the_matrix_core_range_stays_on_the_generic_kernel(cuda):
    N, M, D = 40, 50, 4096
    x, y, h = _clouds(5, N, M, D)
    eps = 0.05**2 * D / 3
    ref = oracle_c.softmin(eps, x, y, h, 2)
    out = hip.softmin(eps, _t(x, cuda), _t(y, cuda), _t(h, cuda)).cpu().numpy()
    assert hip.softmin_fwd_family(1, N, M, D, 2) == hip.FAMILY_GENERIC
    assert relerr(out, ref) < 3e-6
    D = 4095
    x, y, h = _clouds(6, N, M, D)
    ref = oracle_c.softmin(eps, x, y, h, 2)
    for flags in (0, H2):
        out = hip.softmin(eps, _t(x, cuda), _t(y, cuda), _t(h, cuda), flags=flags).cpu().numpy()
        print(f"D=4095 flags={flags}: err {np.abs(out - ref).max():.3e} tol {_tol(ref, D):.3e}")
        assert np.abs(out - ref).max() < _tol(ref, D), flags
