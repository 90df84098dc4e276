"""``hip.plan_bilinear`` (glhip_plan_bilinear, geomloss_amd/csrc/glhip_plan_bilinear_xk.h) against float64 on the GPU.

The bound on both outputs is ``max(2e-5, 4 x e32)``: e32 is the error of the same expression in plain dense float32 torch on the same
inputs (transport_grad_support.bilinear_dense), measured here against the same float64 reference — the rule of
tests/test_plan_apply_nd_gpu.py::test_parity.  Errors are relative to the unsigned sums (transport_grad_support.bilinear_errors).  Every
measured error is printed with its e32 (``pytest -s``); profiles/plan_bilinear.txt holds one such run."""
import functools

import numpy as np
import pytest
import torch

from cloud_support import to_dev
from geomloss_amd import hip
from transport_grad_support import bilinear_dense, bilinear_errors, bilinear_ref, clouds

pytestmark = pytest.mark.gpu

# (N, M, D, K): the smallest shapes at which each mechanism engages
SHAPES = (
    (1, 1, 1, 1),              # the smallest case
    (300, 257, 3, 3),          # low D on the chunked chain, a one-column third tile
    (97, 513, 16, 64),         # D = 16 | 17; K at two chunks ...
    (97, 513, 17, 65),         # ... and one past
    (257, 300, 40, 33),        # a one-row second row block, two coordinate passes
    (64, 8, 64, 1),            # M below one column group; K = 1
    (130, 600, 130, 40),       # five coordinate passes (three at width 64)
    (100, 200, 8, 300),        # K >> D: a weight chain of several stages
    (130, 70001, 24, 16),      # column splits and the merge
)
FLAGS = {"default": 0, "no_split": hip.FLAG_NO_SPLIT, "f16x2": hip.FLAG_F16X2}


def _eps(D):
    return 0.1 * D / 3


def _bound(e32):
    return max(2e-5, 4 * e32)


@functools.lru_cache(maxsize=None)
def _case(N, M, D, K, seed=0):
    """Inputs, the float64 reference and e32 of a shape: computed once, shared by the flags, never modified."""
    x, y, h = clouds(seed, N, M, D)
    rng = np.random.default_rng(seed + 100)
    rf = rng.standard_normal((N, K)).astype(np.float32)
    cf = rng.standard_normal((M, K)).astype(np.float32)
    ref = bilinear_ref(x, y, h, _eps(D), rf, cf)
    o32, w32 = bilinear_dense(x, y, h, _eps(D), rf, cf)
    return (x, y, h, rf, cf), ref, bilinear_errors(o32.numpy(), w32.numpy(), ref)


def _run(dev, x, y, h, rf, cf, eps, flags=0, **kw):
    out, wsum = hip.plan_bilinear(eps, *(to_dev(t, dev) for t in (x, y, h, rf, cf)), flags=flags, **kw)
    assert out.grad_fn is None and wsum.grad_fn is None and out.dtype == torch.float32
    return out.cpu().numpy(), wsum.cpu().numpy()


@pytest.mark.parametrize("flag", sorted(FLAGS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity(cuda, shape, flag):
    N, M, D, K = shape
    inputs, ref, e32 = _case(*shape)
    out, wsum = _run(cuda, *inputs, _eps(D), FLAGS[flag])
    eo, ew = bilinear_errors(out, wsum, ref)
    print(f"plan_bilinear N={N} M={M} D={D} K={K} {flag}: out {eo:.2e} (e32 {e32[0]:.2e})  wsum {ew:.2e} (e32 {e32[1]:.2e})")
    assert np.isfinite(out).all() and np.isfinite(wsum).all()
    assert eo <= _bound(e32[0]) and ew <= _bound(e32[1]), (eo, ew, e32)


def test_batched_bf16(cuda):
    B, N, M, D, K = 3, 200, 260, 48, 20
    x, y, h = clouds(3, N, M, D, B)
    rng = np.random.default_rng(4)
    rf, cf = rng.standard_normal((B, N, K)).astype(np.float32), rng.standard_normal((B, M, K)).astype(np.float32)
    xb, yb = to_dev(x, cuda).bfloat16(), to_dev(y, cuda).bfloat16()
    out, wsum = hip.plan_bilinear(_eps(D), xb, yb, to_dev(h, cuda), to_dev(rf, cuda), to_dev(cf, cuda))
    assert out.shape == (B, N, D) and wsum.shape == (B, N) and out.dtype == torch.float32
    xr, yr = xb.float().cpu().numpy(), yb.float().cpu().numpy()      # the clouds as the kernel reads them
    for k in range(B):
        ref = bilinear_ref(xr[k], yr[k], h[k], _eps(D), rf[k], cf[k])
        o32, w32 = bilinear_dense(xr[k], yr[k], h[k], _eps(D), rf[k], cf[k])
        e32 = bilinear_errors(o32.numpy(), w32.numpy(), ref)
        eo, ew = bilinear_errors(out[k].cpu().numpy(), wsum[k].cpu().numpy(), ref)
        print(f"plan_bilinear bf16 batch {k}: out {eo:.2e} (e32 {e32[0]:.2e})  wsum {ew:.2e} (e32 {e32[1]:.2e})")
        assert eo <= _bound(e32[0]) and ew <= _bound(e32[1]), (k, eo, ew, e32)


def test_massless_rows_and_columns(cuda):
    B, N, M, D, K = 2, 257, 300, 24, 10
    x, y, h = clouds(5, N, M, D, B)
    rng = np.random.default_rng(6)
    rf, cf = rng.standard_normal((B, N, K)).astype(np.float32), rng.standard_normal((B, M, K)).astype(np.float32)
    dead = np.zeros(M, bool)
    dead[[0, 7, 31, 32, 127, 128, 255, 256, 299]] = True
    dead[40:72] = True                                               # a whole column group
    h = h.copy()
    h[0, dead] = -np.inf
    h[1, :] = -np.inf                                                # one batch item entirely without mass
    hostile = cf.copy()
    hostile[0, dead] = 1e30
    hostile[1] = 1e30
    out, wsum = _run(cuda, x, y, h, rf, hostile, _eps(D))
    assert np.isfinite(out).all() and np.isfinite(wsum).all()
    assert (out[1] == 0).all() and (wsum[1] == 0).all()
    calm, calm_w = _run(cuda, x, y, h, rf, cf, _eps(D))              # the same plan, ordinary features on the massless columns
    assert np.array_equal(out[0], calm[0]) and np.array_equal(wsum[0], calm_w[0])      # bit for bit
    live = ~dead
    ref = bilinear_ref(x[0], y[0][live], h[0][live], _eps(D), rf[0], cf[0][live])      # the plan without those columns
    o32, w32 = bilinear_dense(x[0], y[0][live], h[0][live], _eps(D), rf[0], cf[0][live])
    e32 = bilinear_errors(o32.numpy(), w32.numpy(), ref)
    eo, ew = bilinear_errors(out[0], wsum[0], ref)
    print(f"plan_bilinear massless columns: out {eo:.2e} (e32 {e32[0]:.2e})  wsum {ew:.2e} (e32 {e32[1]:.2e})")
    assert eo <= _bound(e32[0]) and ew <= _bound(e32[1])


def test_scales(cuda):
    N, M, D, K = 257, 300, 24, 10
    inputs, ref, e32 = _case(N, M, D, K, seed=7)
    x, y, h, rf, cf = inputs
    bo, bw = _bound(e32[0]), _bound(e32[1])
    for k in (20, -20):                                              # tau unchanged: the outputs stay within the bound
        out, wsum = _run(cuda, x, y, h, rf * np.float32(2.0**k), cf * np.float32(2.0**-k), _eps(D))
        eo, ew = bilinear_errors(out, wsum, ref)
        print(f"plan_bilinear rowfeat 2^{k}, colfeat 2^{-k}: out {eo:.2e}  wsum {ew:.2e} (bounds {bo:.2e}, {bw:.2e})")
        assert eo <= bo and ew <= bw
    for k in (15, -15):                                              # tau times 2^(2k): so are the outputs, exactly a power of two
        out, wsum = _run(cuda, x, y, h, rf * np.float32(2.0**k), cf * np.float32(2.0**k), _eps(D))
        assert np.isfinite(out).all() and np.isfinite(wsum).all()
        eo, ew = bilinear_errors(out.astype(np.float64) * 2.0**(-2 * k), wsum.astype(np.float64) * 2.0**(-2 * k), ref)
        print(f"plan_bilinear both 2^{k}: out {eo:.2e}  wsum {ew:.2e} (bounds {bo:.2e}, {bw:.2e})")
        assert eo <= bo and ew <= bw


def test_deterministic_and_fwd_offset(cuda):
    N, M, D, K = 130, 70001, 24, 16                                  # with column splits
    inputs, ref, e32 = _case(N, M, D, K)
    a = _run(cuda, *inputs, _eps(D))
    b = _run(cuda, *inputs, _eps(D))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    x, y, h = (to_dev(t, cuda) for t in inputs[:3])
    fwd = hip.softmin(_eps(D), x, y, h) + 3 * _eps(D)                # the saved soft-min off by 3 eps: it only centres the weights
    out, wsum = _run(cuda, *inputs, _eps(D), fwd=fwd)
    eo, ew = bilinear_errors(out, wsum, ref)
    print(f"plan_bilinear fwd + 3 eps: out {eo:.2e} (e32 {e32[0]:.2e})  wsum {ew:.2e} (e32 {e32[1]:.2e})")
    assert eo <= _bound(e32[0]) and ew <= _bound(e32[1])


def test_degenerate_sizes_and_refusals(cuda):
    x, y, h = (to_dev(t, cuda) for t in clouds(1, 40, 50, 24))
    rf, cf = torch.ones(40, 5, device=cuda), torch.ones(50, 5, device=cuda)
    out, wsum = hip.plan_bilinear(0.8, x, y, h, rf[:, :0], cf[:, :0])                    # K == 0: zeros
    assert out.shape == (40, 24) and (out == 0).all() and (wsum == 0).all()
    out, wsum = hip.plan_bilinear(0.8, x, y[:0], h[:0], rf, cf[:0], fwd=torch.zeros(40, device=cuda))      # M == 0: zeros
    assert (out == 0).all() and (wsum == 0).all()
    out, wsum = hip.plan_bilinear(0.8, x[:0], y, h, rf[:0], cf, fwd=torch.zeros(0, device=cuda))           # N == 0: nothing
    assert out.shape == (0, 24) and wsum.shape == (0,)
    with pytest.raises(NotImplementedError):
        hip.plan_bilinear(0.8, x.double(), y.double(), h, rf, cf)
    with pytest.raises(NotImplementedError):
        hip.plan_bilinear(0.8, x, y, h, rf, cf, p=1)
    with pytest.raises(NotImplementedError):
        hip.plan_bilinear(0.8, x, y, h, rf, cf, ranges=object())
    with pytest.raises(ValueError):
        hip.plan_bilinear(0.8, x, y, h, rf, cf[:, :4])
    xb, yb, hb = x[None], y[None], h[None]
    with pytest.raises(NotImplementedError):                                             # the library's own refusal
        hip.plan_bilinear_raw(xb, yb, hb, torch.zeros(1, 40, device=cuda), rf[None], cf[None], 0.8, p=1)
