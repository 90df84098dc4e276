"""``geomloss_amd.kmeans`` on the GPU: Lloyd iterations against a float64 oracle, and the capability it exists for — cluster labels
for the two-scale Sinkhorn solver in dimension D > 3 (the reference's plot_optimal_transport_cluster.py recipe)."""
import numpy as np
import pytest
import torch

from geomloss_amd import SamplesLoss, kmeans

pytestmark = pytest.mark.gpu


def _sqdist64(x, c):
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    S = np.zeros((x.shape[0], c.shape[0]))
    for d in range(x.shape[1]):
        S += (x[:, d, None] - c[None, :, d]) ** 2
    return S


def _cloud():
    rng = np.random.default_rng(104)
    x = rng.random((3000, 4)).astype(np.float32)
    return x, x[rng.permutation(3000)[:200]].copy()


def test_one_lloyd_iteration(cuda):
    x, init = _cloud()
    lab, c = kmeans(torch.from_numpy(x).to(cuda), 200, n_iter=1, init=torch.from_numpy(init).to(cuda))
    assert lab.dtype == torch.int32 and lab.shape == (3000,) and c.dtype == torch.float32 and c.shape == (200, 4)
    S = _sqdist64(x, init)
    s = np.sort(S, 1)
    tol = 2 * ((6 + 6 * 4 + 15) // 16 + 5) * 2.0**-24 * 4      # the bound of hip.argmin on |x - c|^2 / 2 (tests/test_argmin_gpu.py), D = 4
    assert (s[:, 1] - s[:, 0]).min() / 2 > tol      # no runner-up inside it among these inputs: the float64 labels are THE labels
    want = S.argmin(1)
    assert np.array_equal(lab.cpu().numpy(), want)
    cref = np.stack([x[want == k].astype(np.float64).mean(0) for k in range(200)])      # (every cluster holds its own seed point)
    err = np.abs(c.cpu().numpy() - cref).max()
    print(f"one Lloyd iteration: centroid error {err:.2e}")
    assert err <= 1e-6
    # bit-identical on a second run
    lab2, c2 = kmeans(torch.from_numpy(x).to(cuda), 200, n_iter=1, init=torch.from_numpy(init).to(cuda))
    assert torch.equal(lab, lab2) and torch.equal(c, c2)


def test_inertia_never_increases(cuda):
    x, init = _cloud()
    xt, c = torch.from_numpy(x).to(cuda), torch.from_numpy(init).to(cuda)
    inertia = []
    for _ in range(10):
        lab, c = kmeans(xt, 200, n_iter=1, init=c)
        diff = x.astype(np.float64) - c.cpu().numpy().astype(np.float64)[lab.cpu().numpy()]
        inertia.append(float((diff**2).sum()))
    print("inertia:", " ".join(f"{v:.6f}" for v in inertia))
    for before, after in zip(inertia, inertia[1:]):
        assert after <= before * (1 + 1e-6)
    assert inertia[-1] < 0.9 * inertia[0]
    # ten iterations in one call are the same ten iterations
    lab10, c10 = kmeans(xt, 200, n_iter=10, init=torch.from_numpy(init).to(cuda))
    assert torch.equal(lab10, lab) and torch.equal(c10, c)


def test_multiscale_4d_with_kmeans_labels(cuda):
    """The clouds and keyword arguments of tests/test_xd_kernels_gpu.py::test_multiscale_4d_with_user_labels with the voxel labels
    replaced by K-means labels and the tutorial's cluster_scale = max(std_x, std_y): the two-scale loss within 5e-3 relative of the
    online loss, the bar the voxel-label test holds the same problem to."""
    g = torch.Generator().manual_seed(7)
    N, M = 6000, 7000
    x = torch.rand(N, 4, generator=g).to(cuda)
    y = (torch.rand(M, 4, generator=g) * torch.tensor([0.7, 0.7, 0.7, 1.0]) + torch.tensor([0.2, 0.2, 0.2, 0.0])).to(cuda)
    gk = torch.Generator().manual_seed(11)
    lab_x, c_x = kmeans(x, 200, generator=gk)
    lab_y, c_y = kmeans(y, 200, generator=gk)
    assert lab_x.shape == (N,) and lab_y.shape == (M,) and int(lab_x.max()) < 200 and int(lab_x.min()) >= 0
    std_x = ((x - c_x[lab_x.long()]) ** 2).sum(1).mean().sqrt().item()
    std_y = ((y - c_y[lab_y.long()]) ** 2).sum(1).mean().sqrt().item()
    kw = dict(p=2, blur=0.05, scaling=0.7)
    a, b = torch.full((N,), 1.0 / N, device=cuda), torch.full((M,), 1.0 / M, device=cuda)
    Lm = SamplesLoss("sinkhorn", backend="multiscale", cluster_scale=max(std_x, std_y), **kw)(lab_x, a, x, lab_y, b, y)
    Lo = SamplesLoss("sinkhorn", backend="online", **kw)(x, y)
    rel = abs(Lm.item() - Lo.item()) / abs(Lo.item())
    print(f"K-means labels: cluster stds {std_x:.4f} / {std_y:.4f}, multiscale {Lm.item():.8e}, online {Lo.item():.8e}, relative deviation {rel:.2e}")
    assert rel < 5e-3
