"""``hip.plan_bilinear(..., resident=True)`` (GLHIP_FLAG_XD_BILINEAR, geomloss_amd/csrc/glhip_plan_bilinear_xd.h) against float64 on the GPU.

The bound on both outputs is ``max(2e-5, 4 x e32)``, e32 from ``bilinear_dense`` on the same inputs: the rule of
tests/test_plan_bilinear_gpu.py::test_parity, with the same ``_eps``.  The kernel's tiles are whole groups of 32 columns, as many as
fit 36 KiB at NM + NMK + 4 KiB a group (60 KiB where NM + NMK > 10): 128 columns at (D, K) = (3, 4), (2, 1), (3, 3) and (5, 5), 96 at
(5, 6), 64 at (8, 9), (16, 17) and (16, 32).  So M = 257, 1153 and 513 are each one column past a tile with the sizes that ship; no M
had to be adjusted.  Every measured error is printed with its e32 (``pytest -s``)."""
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
    (300, 257, 3, 4),          # barycentric_map's shape; a one-column last group, one past a tile
    (257, 1153, 2, 1),         # a one-row second row block; one past the ninth tile
    (97, 513, 8, 9),           # mid-range D with K = D + 1
    (97, 513, 16, 17),         # NM = 7; the first K of the last bucket
    (64, 8, 16, 32),           # M below one group; both limits
    (100, 200, 5, 5),          # a bucket edge of K ...
    (100, 200, 5, 6),          # ... and one past
    (130, 70001, 3, 3),        # column splits and the merge
)


def _eps(D):
    return 0.1 * D / 3


@functools.lru_cache(maxsize=None)
def _case(N, M, D, K, seed=0, quantum=0.0):
    """Inputs, the float64 reference and e32 of a shape: computed once, shared by the flags, never modified."""
    x, y, h = clouds(seed, N, M, D)
    if quantum:
        x, y = np.round(x / quantum) * np.float32(quantum), np.round(y / quantum) * np.float32(quantum)
    rng = np.random.default_rng(seed + 100)
    rf = rng.standard_normal((N, K)).astype(np.float32)
    cf = rng.standard_normal((M, K)).astype(np.float32)
    ref = bilinear_ref(x, y, h, _eps(D), rf, cf)
    o32, w32 = bilinear_dense(x, y, h, _eps(D), rf, cf)
    return (x, y, h, rf, cf), ref, bilinear_errors(o32.numpy(), w32.numpy(), ref)


def _run(dev, x, y, h, rf, cf, eps, flags=0, resident=True):
    out, wsum = hip.plan_bilinear(eps, *(to_dev(t, dev) for t in (x, y, h, rf, cf)), flags=flags, resident=resident)
    assert out.grad_fn is None and wsum.grad_fn is None and out.dtype == torch.float32
    return out.cpu().numpy(), wsum.cpu().numpy()


def _within(label, out, wsum, ref, e32):
    eo, ew = bilinear_errors(out, wsum, ref)
    print(f"plan_bilinear xd {label}: out {eo:.2e} (e32 {e32[0]:.2e})  wsum {ew:.2e} (e32 {e32[1]:.2e})")
    assert np.isfinite(out).all() and np.isfinite(wsum).all()
    assert eo <= max(2e-5, 4 * e32[0]) and ew <= max(2e-5, 4 * e32[1]), (label, eo, ew, e32)


@pytest.mark.parametrize("flag", (0, hip.FLAG_NO_SPLIT))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity(cuda, shape, flag):
    inputs, ref, e32 = _case(*shape)
    _within(f"{shape} flags={flag}", *_run(cuda, *inputs, _eps(shape[2]), flag), ref, e32)


def test_exact_translate(cuda):
    # clouds on a grid of 2^-12, moved by 8: every coordinate stays exact, so the reference and e32 are those of the clouds at the origin
    (x, y, h, rf, cf), ref, e32 = _case(257, 300, 3, 4, seed=2, quantum=2.0**-12)
    _within("translated by 8", *_run(cuda, x + np.float32(8.0), y + np.float32(8.0), h, rf, cf, _eps(3)), ref, e32)


def test_batched_bf16(cuda):
    B, N, M, D, K = 3, 200, 260, 3, 4
    x, y, h = clouds(3, N, M, D, B)
    rng = np.random.default_rng(4)
    rf, cf = rng.standard_normal((B, N, K)).astype(np.float32), rng.standard_normal((B, M, K)).astype(np.float32)
    xb, yb = to_dev(x, cuda).bfloat16(), to_dev(y, cuda).bfloat16()
    out, wsum = hip.plan_bilinear(_eps(D), xb, yb, to_dev(h, cuda), to_dev(rf, cuda), to_dev(cf, cuda), resident=True)
    assert out.shape == (B, N, D) and wsum.shape == (B, N) and out.dtype == torch.float32
    xr, yr = xb.float().cpu().numpy(), yb.float().cpu().numpy()      # the clouds as the kernel reads them
    for k in range(B):
        ref = bilinear_ref(xr[k], yr[k], h[k], _eps(D), rf[k], cf[k])
        o32, w32 = bilinear_dense(xr[k], yr[k], h[k], _eps(D), rf[k], cf[k])
        _within(f"bf16 batch {k}", out[k].cpu().numpy(), wsum[k].cpu().numpy(), ref, bilinear_errors(o32.numpy(), w32.numpy(), ref))


def test_massless_rows_and_columns(cuda):
    B, N, M, D, K = 2, 257, 300, 3, 4
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
    _within("massless columns", out[0], wsum[0], ref, bilinear_errors(o32.numpy(), w32.numpy(), ref))


@pytest.mark.parametrize("k", (20, -20))
def test_scales(cuda, k):
    (x, y, h, rf, cf), ref, e32 = _case(257, 300, 3, 4, seed=7)      # tau unchanged: the outputs stay within the bound of the unscaled case
    _within(f"rowfeat 2^{k}, colfeat 2^{-k}", *_run(cuda, x, y, h, rf * np.float32(2.0**k), cf * np.float32(2.0**-k), _eps(3)), ref, e32)


def test_deterministic_with_and_without_splits(cuda):
    inputs, ref, e32 = _case(130, 70001, 3, 3)
    a = _run(cuda, *inputs, _eps(3))
    b = _run(cuda, *inputs, _eps(3))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    _within("split", *a, ref, e32)
    _within("no split", *_run(cuda, *inputs, _eps(3), hip.FLAG_NO_SPLIT), ref, e32)


def test_routing(cuda):
    lib = hip.load_library()
    fam = lambda D, K, fl: lib.glhip_plan_bilinear_family(1, 97, 300, D, K, 2, hip.F32, 0, fl)  # noqa: E731
    assert fam(16, 32, hip.FLAG_XD_BILINEAR) == hip.FAMILY_XD and fam(3, 4, hip.FLAG_XD_BILINEAR | hip.FLAG_NO_SPLIT) == hip.FAMILY_XD
    assert fam(17, 4, hip.FLAG_XD_BILINEAR) == fam(3, 33, hip.FLAG_XD_BILINEAR) == fam(3, 4, 0) == hip.FAMILY_XK
    for D, K in ((17, 4), (3, 33)):                                  # outside the domain the flag is ignored, bit for bit
        inputs = _case(97, 300, D, K)[0]
        plain = _run(cuda, *inputs, _eps(D), resident=False)
        flagged = _run(cuda, *inputs, _eps(D), hip.FLAG_XD_BILINEAR, resident=False)
        assert np.array_equal(plain[0], flagged[0]) and np.array_equal(plain[1], flagged[1])
        with pytest.raises(NotImplementedError):
            _run(cuda, *inputs, _eps(D))
    x, y, h, rf, cf = (to_dev(t, cuda)[None] for t in _case(97, 300, 3, 4)[0])
    fwd = hip.softmin(_eps(3), x, y, h)
    with pytest.raises(ValueError):                                  # GLHIP_EINVAL: a flagged call in the domain needs its whole workspace
        hip.plan_bilinear_raw(x, y, h, fwd, rf, cf, _eps(3), flags=hip.FLAG_XD_BILINEAR, workspace=4096)
