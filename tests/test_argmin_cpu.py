"""Host side of ``glhip_argmin`` (version 129; geomloss_amd/csrc/glhip_api_argmin.hip) — exported symbols, the support query, the workspace
sizing — and the host logic of ``geomloss_amd.kmeans`` with the arg-reduction replaced by a float64 torch argmin on CPU tensors.
No device."""
import ctypes

import numpy as np
import pytest
import torch

import geomloss_amd
from geomloss_amd import hip

F32, BF16 = 0, 1
EINVAL = -1
NEW_SYMBOLS = ("glhip_argmin", "glhip_argmin_supported", "glhip_argmin_workspace_bytes")


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
    assert lib.glhip_version() >= 129
    assert hip.ARGMIN_MAX_DIM == 4095
    for name in ("argmin", "argmin_supported"):
        assert callable(getattr(hip, name))
    assert "kmeans" in geomloss_amd.__all__ and callable(geomloss_amd.kmeans)
    assert "plan_argmax" in geomloss_amd.__all__ and callable(geomloss_amd.plan_argmax)
    assert geomloss_amd.transport.plan_argmax is geomloss_amd.plan_argmax


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_supported(lib, dtype):
    sup = lambda D, p=2, n_ranges=0, N=1000, dt=dtype: lib.glhip_argmin_supported(1, N, 2000, D, p, dt, n_ranges)  # noqa: E731
    for D in (1, 16, 17, 4095):
        assert sup(D) == 1
    assert sup(64, p=1) == 0
    assert sup(4096) == 0
    assert sup(64, n_ranges=1) == 0
    assert sup(0) == EINVAL
    assert sup(64, dt=7) == EINVAL
    assert sup(64, N=-1) == EINVAL


def test_supported_wrapper():
    assert hip.argmin_supported(1, 1000, 2000, 1) is True
    assert hip.argmin_supported(3, 1000, 2000, 4095, dtype=hip.BF16) is True
    assert hip.argmin_supported(1, 1000, 2000, 4096) is False
    assert hip.argmin_supported(1, 1000, 2000, 8, p=1) is False
    with pytest.raises(ValueError):
        hip.argmin_supported(1, 1000, 2000, 0)


def test_workspace_bytes(lib):
    ws = lib.glhip_argmin_workspace_bytes
    assert ws(0, 100, 100, 4) == 0 and ws(1, 0, 100, 4) == 0 and ws(1, 100, 0, 4) == 0
    assert ws(1, 40, 5000, 24) > 0                      # one row block, 5000 columns: the columns are split
    for N in (40, 3000, 200000):
        sizes = [ws(1, N, M, 24) for M in (1, 100, 511, 1024, 5000, 20000, 65535, 65536, 200000, 10**6)]
        assert sizes == sorted(sizes), (N, sizes)
    assert ws(1, 10**6, 10**6, 64) <= 2**30


# ---- geomloss_amd.kmeans on the CPU, hip.argmin replaced by a float64 torch argmin -------------------------------------------

def _argmin64(x, y, g=None, return_value=False, flags=0, p=2):
    C = ((x.double()[:, None, :] - y.double()[None, :, :]) ** 2).sum(-1) / 2
    if g is not None:
        C = C - g.double()[None, :]
    val, idx = C.min(dim=1)
    return (idx.int(), val.float()) if return_value else idx.int()


@pytest.fixture()
def cpu_argmin(monkeypatch):
    monkeypatch.setattr(hip, "argmin", _argmin64)


def _tutorial_loop(x, c, n_iter, w=None):
    """The loop of the reference's tutorial (plot_optimal_transport_cluster.py:176-180) in NumPy / float64: nearest centroid, then
    ``bincount(cl, weights=x[:, d]) / bincount(cl)`` — with weights, and with an empty cluster left where it was."""
    x, c = x.astype(np.float64), c.astype(np.float64).copy()
    K = c.shape[0]
    w = np.ones(len(x)) if w is None else w.astype(np.float64)
    for _ in range(n_iter):
        cl = ((x[:, None, :] - c[None, :, :]) ** 2).sum(-1).argmin(1)
        Ncl = np.bincount(cl, weights=w, minlength=K)
        for d in range(x.shape[1]):
            s = np.bincount(cl, weights=w * x[:, d], minlength=K)
            c[:, d] = np.where(Ncl > 0, s / np.where(Ncl > 0, Ncl, 1.0), c[:, d])
    return cl, c


def test_kmeans_one_iteration_is_the_tutorial_loop(cpu_argmin):
    rng = np.random.default_rng(0)
    x = rng.random((500, 5)).astype(np.float32)
    init = x[rng.permutation(500)[:20]].copy()
    lab, c = geomloss_amd.kmeans(torch.from_numpy(x), 20, n_iter=1, init=torch.from_numpy(init))
    cl, cref = _tutorial_loop(x, init, 1)
    assert lab.dtype == torch.int32 and lab.shape == (500,) and c.dtype == torch.float32 and c.shape == (20, 5)
    assert np.array_equal(lab.numpy(), cl)
    assert np.abs(c.numpy() - cref).max() <= 1e-6
    # three iterations: labels of the last assignment, centroids updated once more
    lab3, c3 = geomloss_amd.kmeans(torch.from_numpy(x), 20, n_iter=3, init=torch.from_numpy(init))
    cl3, cref3 = _tutorial_loop(x, init, 3)
    assert np.array_equal(lab3.numpy(), cl3) and np.abs(c3.numpy() - cref3).max() <= 1e-6


def test_kmeans_empty_cluster_keeps_its_centroid(cpu_argmin):
    rng = np.random.default_rng(1)
    x = rng.random((200, 3)).astype(np.float32)
    init = np.concatenate([x[:4], np.full((1, 3), 50.0, np.float32), x[4:6], np.full((1, 3), -50.0, np.float32)])   # clusters 4 and 7 (the last) stay empty
    lab, c = geomloss_amd.kmeans(torch.from_numpy(x), 8, n_iter=2, init=torch.from_numpy(init))
    assert not np.isin(lab.numpy(), (4, 7)).any()
    assert np.array_equal(c.numpy()[4], init[4]) and np.array_equal(c.numpy()[7], init[7])
    assert np.isfinite(c.numpy()).all()
    _, cref = _tutorial_loop(x, init, 2)
    assert np.abs(c.numpy() - cref).max() <= 1e-6


def test_kmeans_weighted_means(cpu_argmin):
    rng = np.random.default_rng(2)
    x = rng.random((300, 4)).astype(np.float32)
    w = (rng.random(300) + 0.05).astype(np.float32)
    w[:30] = 0.0
    init = x[100:110].copy()
    lab, c = geomloss_amd.kmeans(torch.from_numpy(x), 10, n_iter=1, init=torch.from_numpy(init), weights=torch.from_numpy(w))
    cl, cref = _tutorial_loop(x, init, 1, w)
    assert np.array_equal(lab.numpy(), cl)
    assert np.abs(c.numpy() - cref).max() <= 1e-6
    _, cu = geomloss_amd.kmeans(torch.from_numpy(x), 10, n_iter=1, init=torch.from_numpy(init))
    assert np.abs(c.numpy() - cu.numpy()).max() > 1e-4      # the weights matter


def test_kmeans_random_init_and_determinism(cpu_argmin):
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.random((400, 6)).astype(np.float32))
    runs = [geomloss_amd.kmeans(x, 15, n_iter=4, generator=torch.Generator().manual_seed(5)) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])      # bit-identical
    # n_iter = 0: the initial centroids are K distinct points of x
    lab0, c0 = geomloss_amd.kmeans(x, 15, n_iter=0, generator=torch.Generator().manual_seed(5))
    rows = [int((x == c0[k]).all(1).nonzero()[0, 0]) for k in range(15)]
    assert len(set(rows)) == 15
    assert torch.equal(lab0[rows].long(), torch.arange(15))
    with pytest.raises(ValueError):
        geomloss_amd.kmeans(x, 401)
    with pytest.raises(ValueError):
        geomloss_amd.kmeans(x, 15, init=torch.zeros(15, 5))
