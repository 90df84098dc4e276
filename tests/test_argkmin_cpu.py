"""Host side of ``glhip_argkmin`` (version 138; geomloss_amd/csrc/glhip_api_argkmin.hip) — exported symbols, the limit on k, the support
query, the workspace sizing, the wrapper's exceptions — and the host logic of ``geomloss_amd.knn``, ``transport.plan_topk`` and
``OTResultSample.sparse_plan`` with the arg-reduction replaced by a float64 torch ``topk`` on CPU tensors.  No device."""
import ctypes

import numpy as np
import pytest
import torch

import geomloss_amd
from geomloss_amd import hip
from geomloss_amd.ot.sample import ArrayProperties, OTResultSample

F32, BF16 = 0, 1
EINVAL = -1
NEW_SYMBOLS = ("glhip_argkmin", "glhip_argkmin_supported", "glhip_argkmin_workspace_bytes", "glhip_argkmin_max_k")


@pytest.fixture(scope="module")
def lib():
    assert hip.library_available(), "libgeomloss_hip.so is not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = hip.SIGNATURES[name]
    lib.glhip_version.restype = ctypes.c_int
    return lib


def test_symbols_and_version(lib):
    assert lib.glhip_version() >= 138
    for name in NEW_SYMBOLS:
        assert hip._SINCE[name] == 138
    assert lib.glhip_argkmin_max_k() >= 16
    assert hip.ARGKMIN_MAX_K == lib.glhip_argkmin_max_k()
    for name in ("argkmin", "argkmin_supported"):
        assert callable(getattr(hip, name))
    for name in ("knn", "plan_topk"):
        assert name in geomloss_amd.__all__ and callable(getattr(geomloss_amd, name))
    assert geomloss_amd.transport.plan_topk is geomloss_amd.plan_topk and geomloss_amd.cluster.knn is geomloss_amd.knn
    assert callable(OTResultSample.sparse_plan)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_supported(lib, dtype):
    kmax = lib.glhip_argkmin_max_k()
    sup = lambda D, k=16, p=2, n_ranges=0, N=1000, dt=dtype: lib.glhip_argkmin_supported(1, N, 2000, D, k, p, dt, n_ranges)  # noqa: E731
    for D in (1, 16, 17, 4095):
        assert sup(D) == 1 and sup(D, k=1) == 1 and sup(D, k=kmax) == 1
    assert sup(4096) == 0
    assert sup(64, p=1) == 0
    assert sup(64, n_ranges=1) == 0
    assert sup(64, k=kmax + 1) == 0
    assert sup(64, k=0) == EINVAL
    assert sup(0) == EINVAL
    assert sup(64, dt=7) == EINVAL
    assert sup(64, N=-1) == EINVAL


def test_supported_wrapper():
    assert hip.argkmin_supported(1, 1000, 2000, 1, 16) is True
    assert hip.argkmin_supported(3, 1000, 2000, 4095, 4, dtype=hip.BF16) is True
    assert hip.argkmin_supported(1, 1000, 2000, 4096, 4) is False
    assert hip.argkmin_supported(1, 1000, 2000, 8, 4, p=1) is False
    assert hip.argkmin_supported(1, 1000, 2000, 8, hip.ARGKMIN_MAX_K + 1) is False
    with pytest.raises(ValueError):
        hip.argkmin_supported(1, 1000, 2000, 8, 0)
    with pytest.raises(ValueError):
        hip.argkmin_supported(1, 1000, 2000, 0, 4)


def test_workspace_bytes(lib):
    ws = lib.glhip_argkmin_workspace_bytes
    assert ws(0, 100, 100, 4, 8) == 0 and ws(1, 0, 100, 4, 8) == 0 and ws(1, 100, 0, 4, 8) == 0
    assert ws(1, 40, 5000, 24, 16) > 0                  # one row block, 5000 columns: the columns are split
    for N in (40, 3000, 200000):
        for k in (1, 8, 16):
            sizes = [ws(1, N, M, 24, k) for M in (1, 100, 511, 1024, 5000, 20000, 65535, 65536, 200000, 10**6)]
            assert sizes == sorted(sizes), (N, k, sizes)
    for N, M in ((40, 5000), (3000, 20000), (200000, 200000)):
        sizes = [ws(1, N, M, 24, k) for k in range(1, 17)]
        assert sizes == sorted(sizes), (N, M, sizes)
    assert ws(1, 10**6, 10**6, 64, 16) <= 2**30
    # k = 1 keeps the partial of glhip_argmin: two floats per row and split
    assert ws(1, 40, 5000, 24, 1) % (40 * 2 * 4) == 0


def test_wrapper_exceptions():
    """What ``hip.argkmin`` refuses before it looks at a device."""
    x, y = torch.rand(50, 3), torch.rand(60, 3)
    with pytest.raises(NotImplementedError):
        hip.argkmin(x.double(), y.double(), 4)
    with pytest.raises(NotImplementedError):
        hip.argkmin(x, y, 4, p=1)
    with pytest.raises(NotImplementedError):
        hip.argkmin(torch.rand(4, 4096), torch.rand(5, 4096), 4)
    with pytest.raises(NotImplementedError):
        hip.argkmin(x, y, hip.ARGKMIN_MAX_K + 1)
    for k in (0, -3):
        with pytest.raises(ValueError):
            hip.argkmin(x, y, k)
    with pytest.raises(NotImplementedError):
        geomloss_amd.plan_topk(x, y, torch.zeros(50), torch.zeros(60), 0.1, 4, p=1)


# ---- knn, plan_topk and sparse_plan on the CPU, hip.argkmin replaced by a float64 torch topk --------------------------------------

def _argkmin64(x, y, k, g=None, return_value=False, flags=0, p=2):
    """The semantics of hip.argkmin in float64: (cost ascending, index ascending), g = -inf never returned, (-1, +inf) beyond."""
    C = ((x.double()[:, None, :] - y.double()[None, :, :]) ** 2).sum(-1) / 2
    if g is not None:
        C = C - g.double()[None, :]
    N, M = C.shape
    order = torch.argsort(C, dim=1, stable=True)[:, :k]
    val = torch.gather(C, 1, order)
    idx = torch.where(torch.isfinite(val), order, torch.full_like(order, -1))
    pad = k - idx.shape[1]
    idx = torch.cat((idx, torch.full((N, pad), -1, dtype=idx.dtype)), 1).int()
    val = torch.cat((val, torch.full((N, pad), float("inf"), dtype=val.dtype)), 1)
    return (idx, val.float()) if return_value else idx


@pytest.fixture()
def cpu_argkmin(monkeypatch):
    monkeypatch.setattr(hip, "argkmin", _argkmin64)


def _dense_topk(P, k):
    """Top-k of a dense float64 plan per row: (heaviest first, smaller column first among equals), zero entries never returned."""
    N, M = P.shape
    order = np.argsort(-P, axis=1, kind="stable")[:, :k]
    w = np.take_along_axis(P, order, 1)
    idx = np.where(w > 0, order, -1)
    pad = k - idx.shape[1]
    return np.concatenate((idx, np.full((N, pad), -1)), 1), np.concatenate((w, np.zeros((N, pad))), 1)


def test_knn_host_logic(cpu_argkmin):
    rng = np.random.default_rng(0)
    x, y = rng.random((40, 5)).astype(np.float32), rng.random((30, 5)).astype(np.float32)
    idx, sq = geomloss_amd.knn(torch.from_numpy(x), torch.from_numpy(y), 6)
    D2 = ((x.astype(np.float64)[:, None, :] - y.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    assert idx.dtype == torch.int32 and sq.dtype == torch.float32 and idx.shape == (40, 6) and sq.shape == (40, 6)
    assert np.array_equal(idx.numpy(), np.argsort(D2, 1, kind="stable")[:, :6])
    assert np.abs(sq.numpy() - np.sort(D2, 1)[:, :6]).max() <= 1e-6
    # fewer points than k
    idx, sq = geomloss_amd.knn(torch.from_numpy(x), torch.from_numpy(y[:4]), 6)
    assert (idx.numpy()[:, 4:] == -1).all() and np.isinf(sq.numpy()[:, 4:]).all() and (idx.numpy()[:, :4] >= 0).all()


@pytest.mark.parametrize("M,k", [(30, 6), (4, 6)])
def test_plan_topk_host_logic(cpu_argkmin, M, k):
    rng = np.random.default_rng(1)
    N, D, blur = 40, 3, 0.3
    eps = blur**2
    x, y = rng.random((N, D)).astype(np.float32), rng.random((M, D)).astype(np.float32)
    a, b = rng.random(N).astype(np.float32) + 0.1, rng.random(M).astype(np.float32) + 0.1
    b[2] = 0.0
    a, b = a / a.sum(), b / b.sum()
    F, G = (0.05 * rng.standard_normal(N)).astype(np.float32), (0.05 * rng.standard_normal(M)).astype(np.float32)
    d = lambda v: v.astype(np.float64)  # noqa: E731
    C = ((d(x)[:, None, :] - d(y)[None, :, :]) ** 2).sum(-1) / 2
    P = d(a)[:, None] * d(b)[None, :] * np.exp((d(F)[:, None] + d(G)[None, :] - C) / eps)
    want_i, want_w = _dense_topk(P, k)
    t = torch.from_numpy
    idx, w = geomloss_amd.plan_topk(t(x), t(y), t(F), t(G), blur, k, a=t(a), b=t(b))
    assert idx.dtype == torch.int32 and w.dtype == torch.float32 and idx.shape == (N, k) and w.shape == (N, k)
    assert np.array_equal(idx.numpy(), want_i)
    assert not (idx.numpy() == 2).any()
    assert np.abs(w.numpy() - want_w).max() <= 1e-5 * P.max()
    assert (w.numpy()[idx.numpy() < 0] == 0).all()
    # uniform weights by default
    idx_u, w_u = geomloss_amd.plan_topk(t(x), t(y), t(F), t(G), blur, k)
    Pu = np.exp((d(F)[:, None] + d(G)[None, :] - C) / eps) / (N * M)
    wi, ww = _dense_topk(Pu, k)
    assert np.array_equal(idx_u.numpy(), wi) and np.abs(w_u.numpy() - ww).max() <= 1e-5 * Pu.max()


def _result(x, y, a, b, f, g, reg, library="torch", dtype=torch.float32):
    """An OTResultSample on CPU tensors, as solve_sample builds it."""
    from geomloss_amd.ot.sinkhorn_ot import SinkhornPotentials
    t = (lambda v: torch.from_numpy(v)) if isinstance(x, np.ndarray) else (lambda v: v)
    pots = SinkhornPotentials(f_aa=None, g_bb=None, g_ab=t(g), f_ba=t(f))
    props = ArrayProperties(B=0, N=x.shape[0], M=y.shape[0], dtype=dtype, device="cpu", library=library)
    return OTResultSample(X_a=t(x), X_b=t(y), a=t(a), b=t(b), cost="sqeuclidean", reg=reg, reg_type="KL", unbalanced=None,
                          unbalanced_type="KL", debias=False, potentials=pots, array_properties=props)


@pytest.mark.parametrize("M,k", [(30, 5), (3, 5)])
def test_sparse_plan_host_logic(cpu_argkmin, M, k):
    rng = np.random.default_rng(2)
    N, D, reg = 25, 2, 0.2
    x, y = rng.random((N, D)).astype(np.float32), rng.random((M, D)).astype(np.float32)
    a, b = rng.random(N).astype(np.float32) + 0.1, rng.random(M).astype(np.float32) + 0.1
    b[1] = 0.0
    a, b = a / a.sum(), b / b.sum()
    f, g = (0.1 * rng.standard_normal(N)).astype(np.float32), (0.1 * rng.standard_normal(M)).astype(np.float32)
    res = _result(x, y, a, b, f, g, reg)
    P = res.plan.double().numpy()                       # its own dense plan: a_i b_j exp((f_i + g_j - |x - y|^2) / reg)
    want_i, want_w = _dense_topk(P, k)
    idx, w = res.sparse_plan(k)
    assert idx.dtype == torch.int32 and w.dtype == torch.float32 and idx.shape == (N, k)
    assert np.array_equal(idx.numpy(), want_i)
    assert not (idx.numpy() == 1).any()
    assert np.abs(w.numpy() - want_w).max() <= 1e-5 * P.max()
    # NumPy callers get NumPy arrays in their dtype
    idx_n, w_n = _result(x, y, a, b, f, g, reg, library="numpy", dtype=np.float64).sparse_plan(k)
    assert isinstance(idx_n, np.ndarray) and idx_n.dtype == np.int32 and w_n.dtype == np.float64 and np.array_equal(idx_n, want_i)


def test_sparse_plan_names_plan_where_the_reduction_does_not_apply():
    rng = np.random.default_rng(3)
    x, y = torch.from_numpy(rng.random((5, 2))), torch.from_numpy(rng.random((6, 2)))      # float64 clouds
    res = _result(x, y, torch.full((5,), 0.2), torch.full((6,), 1 / 6), torch.zeros(5), torch.zeros(6), 0.1)
    with pytest.raises(NotImplementedError, match="plan"):
        res.sparse_plan(3)
