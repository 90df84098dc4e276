"""One launch per split policy of geomloss_amd/csrc/glhip_split_policy.h through the C-ABI, each with four workspaces:

    sized   what glhip_workspace_bytes asks for (4 x for glhip_sinkhorn_iter4, as hip.sinkhorn_iter4_raw asks)
    half    half of it
    4096    4096 bytes
    none    no workspace: one split, no pre-packed columns

against the GLHIP_FLAG_NO_SPLIT result of the same launch.  A plan is capped at what its workspace holds (tests/test_split_policy_cpu.py
checks the bounds on the host); here the launchers execute such plans — fewer splits, the XCD-aware grid lost, pre-packed columns lost
— and the result may only move by the reordering of a float32 sum.  Tolerances are those of the existing test of each kernel, named
at each case; figures are printed before they are asserted.  Shapes are the smallest that reach each branch:

    rule only, dense                 N = 300, M = 4096:      D = 3 p = 1 (VALU skeleton), D = 8 p = 1 (glhip_dist_xd.h, small-launch rule),
                                                             D = 32 p = 2 (glhip_softmin_xk.h)
    XCD-aware grid                   N = 300, M = 65536:     the same, and the policies below
    x32 forward, pre-packed          D = 3 p = 2 under GLHIP_FLAG_PREPACK, both K layouts
    weighted sum                     gaussian product D = 3, with and without GLHIP_FLAG_PREPACK
    xd, pre-packed and free splits   N = 32768, M = 16384, D = 4 (5.4e8 pairs: the smallest "big" launch), and D = 8 at the shapes above
    block-sparse with chunk table    N = M = 2000, 7 ranges, with and without GLHIP_FLAG_SMALL_ROW_BLOCKS, p = 2 and p = 1
    multi launch                     glhip_sinkhorn_iter4 at N = M = 3072 and 2000 (the tiny rule), D in {3, 8}, p in {1, 2}
"""
import ctypes

import numpy as np
import pytest
import torch

import test_hip_kernels as th
from geomloss_amd import hip

pytestmark = pytest.mark.gpu

NS, PRE, H2, SMALL = hip.FLAG_NO_SPLIT, hip.FLAG_PREPACK, hip.FLAG_F16X2, hip.FLAG_SMALL_ROW_BLOCKS
MODES = ("sized", "half", "4096", "none")


def _bytes(mode, sized):
    return {"sized": sized, "half": sized // 2, "4096": 4096, "none": 0}[mode]


def _ws_args(dev, nbytes):
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    return ws, (ctypes.c_void_p(ws.data_ptr()) if nbytes else None, nbytes)


def _softmin(x, y, h, eps, p, flags, mode, ranges=None):
    """glhip_softmin_fwd on (N, D), (M, D), (M,) device tensors with the workspace of `mode`"""
    lib = hip.load_library()
    (N, D), M = x.shape, y.shape[0]
    rargs = hip._NO_RANGES if ranges is None else ranges.c_args()
    sized = int(lib.glhip_workspace_bytes(1, N, M, D, rargs[3]))
    out = torch.empty(N, dtype=torch.float32, device=x.device)
    ws, args = _ws_args(x.device, _bytes(mode, sized))
    with torch.cuda.device(x.device):
        rc = lib.glhip_softmin_fwd(x.data_ptr(), y.data_ptr(), h.data_ptr(), out.data_ptr(), 1, N, M, D, float(eps), int(p), hip.F32, *rargs, *args,
                                   int(flags), hip._stream(x))
    assert rc == 0, lib.glhip_last_error()
    return out.cpu().numpy()


def _gauss(x, y, v, blur, flags, mode):
    lib = hip.load_library()
    (N, D), M = x.shape, y.shape[0]
    sized = int(lib.glhip_workspace_bytes(1, N, M, D, 0))
    out = torch.empty(N, dtype=torch.float32, device=x.device)
    ws, args = _ws_args(x.device, _bytes(mode, sized))
    with torch.cuda.device(x.device):
        rc = lib.glhip_kernel_conv_fwd(hip.GAUSSIAN, x.data_ptr(), y.data_ptr(), v.data_ptr(), out.data_ptr(), 1, N, M, D, float(blur), hip.F32,
                                       *hip._NO_RANGES, *args, int(flags), hip._stream(x))
    assert rc == 0, lib.glhip_last_error()
    return out.cpu().numpy()


def _iter4(x, y, a_log, b_log, pots, eps, damping, p, flags, mode):
    """glhip_sinkhorn_iter4 (an averaged update of four potentials) on (1, N, D), (1, M, D) clouds"""
    lib = hip.load_library()
    (B, N, D), M = x.shape, y.shape[1]
    L = max(N, M)
    sized = 4 * int(lib.glhip_workspace_bytes(B, L, L, D, 0))
    outs = [torch.empty((B, n), dtype=torch.float32, device=x.device) for n in (N, M, N, M)]
    ws, args = _ws_args(x.device, _bytes(mode, sized))
    with torch.cuda.device(x.device):
        rc = lib.glhip_sinkhorn_iter4(x.data_ptr(), y.data_ptr(), a_log.data_ptr(), b_log.data_ptr(), *[t.data_ptr() for t in pots],
                                      *[t.data_ptr() for t in outs], B, N, M, D, float(eps), float(damping), int(p), hip.F32, 0, *args, int(flags),
                                      hip._stream(x))
    assert rc == 0, lib.glhip_last_error()
    return [t.cpu().numpy() for t in outs]


def _tol_softmin(ref, D):
    return 4e-7 * D + 2e-6 * np.abs(ref).max()      # test_hip_kernels / test_xd_kernels_gpu / test_anyd_kernels_gpu: test_softmin_fwd_vs_oracle


def _tol_dist_xd(ref, D):
    return 2e-6 * max(1.0, np.abs(ref).max())       # test_xd_kernels_gpu: the dense p = 1 soft-min of 4 <= D <= 16


DENSE = [  # (D, p, flags, tolerance)
    (3, 1, 0, _tol_softmin), (8, 1, 0, _tol_dist_xd), (32, 2, 0, _tol_softmin),                 # rule only (+ XCD-aware grid at M = 65536)
    (3, 2, 0, _tol_softmin), (3, 2, PRE, _tol_softmin), (3, 2, PRE | H2, _tol_softmin),         # x32 forward
    (8, 2, 0, _tol_softmin), (8, 2, H2, _tol_softmin),                                          # xd
]


@pytest.mark.parametrize("D,p,flags,tol_of", DENSE)
@pytest.mark.parametrize("M", [4096, 65536])
def test_dense_softmin(cuda, M, D, p, flags, tol_of):
    N = 300
    x, y, h = (th._t(a, cuda) for a in th._clouds(M + D, N, M, D))
    eps = 0.05**2 * max(D, 3) / 3 if p == 2 else 0.05
    ref = _softmin(x, y, h, eps, p, flags | NS, "sized")
    for mode in MODES:
        err = np.abs(_softmin(x, y, h, eps, p, flags, mode) - ref).max()
        print(f"softmin N={N} M={M} D={D} p={p} flags={flags} workspace {mode}: vs NO_SPLIT {err:.3e} tol {tol_of(ref, D):.3e}")
        assert np.isfinite(ref).all() and err < tol_of(ref, D), mode


@pytest.mark.parametrize("flags", [0, PRE])
@pytest.mark.parametrize("M", [4096, 65536])
def test_dense_gaussian_product(cuda, M, flags):
    N, D, blur = 300, 3, 0.2
    x, y, v = (th._t(a, cuda) for a in th._clouds(M + 7, N, M, D))
    ref = _gauss(x, y, v, blur, flags | NS, "sized")
    bound = _gauss(x, y, v.abs(), blur, flags | NS, "sized")
    tol = 3e-6 * np.abs(ref).max() + 2.4e-7 * D / blur**2 * np.abs(bound).max()      # test_hip_kernels: test_kernel_conv_vs_oracle
    for mode in MODES:
        err = np.abs(_gauss(x, y, v, blur, flags, mode) - ref).max()
        print(f"gaussian N={N} M={M} D={D} flags={flags} workspace {mode}: vs NO_SPLIT {err:.3e} tol {tol:.3e}")
        assert err < tol, mode


def test_xd_prepacked_and_free_splits(cuda):
    N, M, D = 32768, 16384, 4
    x, y, h = (th._t(a, cuda) for a in th._clouds(5, N, M, D))
    eps = 0.07**2
    ref = _softmin(x, y, h, eps, 2, NS, "sized")
    for mode in MODES:
        err = np.abs(_softmin(x, y, h, eps, 2, 0, mode) - ref).max()
        print(f"softmin N={N} M={M} D={D} workspace {mode}: vs NO_SPLIT {err:.3e} tol {_tol_softmin(ref, D):.3e}")
        assert err < _tol_softmin(ref, D), mode


@pytest.mark.parametrize("p", [2, 1])
@pytest.mark.parametrize("flags", [0, SMALL])
def test_block_sparse_with_chunk_table(cuda, flags, p):
    N = M = 2000
    D = 3
    x, y, h = (th._t(a, cuda) for a in th._clouds(23, N, M, D))
    rg = th._random_ranges(np.random.default_rng(17), N, M, 7, 9, 0.5, cuda)[0]
    eps = 0.02
    ref = _softmin(x, y, h, eps, p, flags | NS, "sized", rg)
    live = np.isfinite(ref)
    assert 0 < (~live).sum() < N and np.isposinf(ref[~live]).all()      # the row block with nothing to reduce over
    tol = 1.2e-6 + 2e-6 * np.abs(ref[live]).max()                       # test_hip_kernels: test_softmin_block_sparse_vs_oracle
    for mode in MODES:
        out = _softmin(x, y, h, eps, p, flags, mode, rg)
        err = np.abs(out[live] - ref[live]).max()
        print(f"block-sparse N={N} p={p} flags={flags} workspace {mode}: vs NO_SPLIT {err:.3e} tol {tol:.3e}")
        assert np.isposinf(out[~live]).all() and err < tol, mode


@pytest.mark.parametrize("p", [2, 1])
@pytest.mark.parametrize("D", [3, 8])
@pytest.mark.parametrize("N", [3072, 2000])
def test_multi_launch(cuda, N, D, p):
    M = N
    x, y, _ = th._clouds(90 + N, N, M, D, B=1)
    rng = np.random.default_rng(4)
    a_log, b_log = (np.log(rng.random((1, n)) + 0.1).astype(np.float32) for n in (N, M))
    pots = [th._t((rng.standard_normal((1, n)) * 0.1).astype(np.float32), cuda) for n in (N, M, N, M)]
    xt, yt, al, bl = (th._t(a, cuda) for a in (x, y, a_log, b_log))
    eps, damping = (0.02 if p == 2 else 0.1), 0.9
    tol = 2e-6 if p == 2 else 4e-6      # test_hip_kernels: test_iter4_equals_four_fused_steps
    ref = _iter4(xt, yt, al, bl, pots, eps, damping, p, NS, "sized")
    for mode in MODES:
        got = _iter4(xt, yt, al, bl, pots, eps, damping, p, 0, mode)
        err = max(float(np.abs(g - r).max()) for g, r in zip(got, ref))
        print(f"iter4 N=M={N} D={D} p={p} workspace {mode}: vs NO_SPLIT {err:.3e} tol {tol:.3e}")
        assert err < tol, mode
