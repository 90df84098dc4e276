"""``hip.argkmin`` for 16 < k <= 128 (floored passes, geomloss_amd/csrc/glhip_argkmin_xk.h): oracle, tolerance and criteria (a), (b), (c)
of tests/test_argkmin_gpu.py.  With up to 129 order statistics per row more rows have a near-tie: (c) may leave out 25 % of the rows — a
condition on the float64 costs alone (CASES: 0.013 / 0.000 / 0.072 / 0.107 / 0.130 / 0.125 / 0.133 / 0.203) — and is exact on the others."""
import numpy as np
import pytest
import torch

from geomloss_amd import hip
from test_argmin_gpu import case, tol_of
from test_argkmin_gpu import gpu, judge

pytestmark = pytest.mark.gpu

# (N, M, D, gs, k): one rank on the list of 4 in a second pass; M < k; two full passes; 16 + 16 + 8 with duals, D = 17; a long K loop,
# remainder 5 on the list of 8; column splits in every pass, remainder on the list of 4; the maximum, eight passes, twice
CASES = [(300, 129, 3, 0.0, 17), (257, 20, 3, 0.0, 24), (500, 300, 2, 0.0, 32), (1000, 700, 17, 0.1, 40), (600, 200, 65, 0.0, 21),
         (40, 5000, 24, 0.0, 36), (300, 200, 4, 0.05, 128), (300, 400, 3, 0.0, 128)]


@pytest.mark.parametrize("N,M,D,gs,k", CASES)
def test_passes_against_float64(cuda, N, M, D, gs, k):
    x, y, g, C = case(N, M, D, gs)
    xt, yt, gt = gpu(cuda, x, y, g)
    idx, val = hip.argkmin(xt, yt, k, gt if gs else None, return_value=True)
    assert judge(idx.cpu().numpy(), val.cpu().numpy(), C, k, tol_of(D, float(np.abs(g).max())), f"argkmin {(N, M, D, gs, k)}") <= 0.25
    assert torch.equal(hip.argkmin(xt, yt, k, gt if gs else None), idx)


@pytest.mark.parametrize("N,M,D,gs", [(40, 5000, 24, 0.0), (3000, 200, 4, 0.05)])
def test_prefixes_launch_forms_and_batches(cuda, N, M, D, gs):
    x, y, g, _ = case(N, M, D, gs)
    xt, yt, gt = gpu(cuda, x, y, g)
    run = lambda k, flags=0: hip.argkmin(xt, yt, k, gt, return_value=True, flags=flags)  # noqa: E731
    r16, r20, r48, r128 = run(16), run(20), run(48), run(128)
    for small, big, k in ((r16, r48, 16), (r20, r48, 20), (r48, r128, 48), (run(48, hip.FLAG_NO_SPLIT), r48, 48)):
        assert torch.equal(big[0][:, :k], small[0]) and torch.equal(big[1][:, :k], small[1]), k
    gb = gpu(cuda, (0.05 * np.random.default_rng(7).standard_normal((3, M))).astype(np.float32))[0]      # a batch of three, a dual vector each
    ib, vb = hip.argkmin(xt.expand(3, N, D).contiguous(), yt.expand(3, M, D).contiguous(), 48, gb, return_value=True)
    for b in range(3):
        i1, v1 = hip.argkmin(xt, yt, 48, gb[b], return_value=True)
        assert torch.equal(ib[b], i1) and torch.equal(vb[b], v1), b


@pytest.mark.parametrize("copies", [3, 5])
def test_ties_across_pass_boundaries(cuda, copies):
    """Copies of every column share their exponent bit for bit: with k = 16 copies the tie groups straddle the ranks 15 | 16, 31 | 32, ..."""
    N, M, D = 40, 5000, 24
    xt, yt = gpu(cuda, *case(N, M, D, 0.0)[:2])
    i16, v16 = hip.argkmin(xt, yt, 16, return_value=True)
    shift = M * torch.arange(copies, device=cuda, dtype=torch.int32)
    for flags in (0, hip.FLAG_NO_SPLIT):
        ic, vc = hip.argkmin(xt, torch.cat((yt,) * copies), 16 * copies, return_value=True, flags=flags)
        assert torch.equal(ic, (i16[:, :, None] + shift).reshape(N, -1)), flags      # rank copies r + c: column i16[:, r] + c M
        assert torch.equal(vc, v16[:, :, None].expand(N, 16, copies).reshape(N, -1)), flags


def test_masked_columns_leave_the_last_ranks_empty(cuda):
    N, M, D, gs, k = 3000, 200, 4, 0.05, 128
    x, y, g, C = case(N, M, D, gs)
    off = np.random.default_rng(5).permutation(M) < M // 2
    xt, yt, gm = gpu(cuda, x, y, np.where(off, -np.inf, g).astype(np.float32))
    idx, val = hip.argkmin(xt, yt, k, gm, return_value=True)
    assert bool((idx[:, 100:] == -1).all()) and bool((val[:, 100:] == float("inf")).all())
    judge(idx[:, :100].cpu().numpy(), val[:, :100].cpu().numpy(), np.where(off, np.inf, C), 100, tol_of(D, float(np.abs(g).max())), "100 admissible", exact=False)
