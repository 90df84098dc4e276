"""The one-launch Sinkhorn iteration of p = 1 clouds of 17 <= D <= 4095 on pre-packed operands (geomloss_amd/csrc/glhip_dist_xkp.h,
library version 147, hip.FLAG_XK_ITER_DIST) against float64: the kernel through hip.sinkhorn_iter4, the library loop through
hip.Iter4Plan, the driver through SamplesLoss under sinkhorn_samples._XK_ITER_P1."""

import ctypes
import functools

import numpy as np
import pytest
import torch

from geomloss_amd import SamplesLoss, hip
from geomloss_amd import sinkhorn_samples as ss
from oracle import oracle_c

pytestmark = pytest.mark.gpu

EPS1, DAMP = 0.05, 0.8      # the p = 1 temperature and damping of tests/test_dimension_sweep_gpu.py


def _flag():
    return hip.FLAG_XK_ITER_DIST


def _sbound(ref):      # the bound of the p = 1 matrix-core family (tests/test_dist_xk_gpu.py)
    return 12 * 2e-6 * max(1.0, float(np.abs(ref).max()))


@functools.lru_cache(maxsize=None)
def _case(N, M, D, B, kind):
    """Clouds in the unit cube (bfloat16-representable for the batched case; moved by 8 for "shift"; y = x + 1e-4 noise for "near"),
    log-weights (-inf on a third of the columns for "neginf"), old potentials, and per batch item the float64 soft-mins of the
    initialisation and of the update for (f_ba, g_ab, f_aa, g_bb)."""
    rng = np.random.default_rng([N, M, D, B or 0])
    nb = B or 1
    x, y = rng.random((nb, N, D), dtype=np.float32), rng.random((nb, M, D), dtype=np.float32) * 0.8 + 0.1
    if B:
        x, y = (torch.tensor(t).bfloat16().float().numpy() for t in (x, y))
    if kind == "shift":
        x, y = x + np.float32(8), y + np.float32(8)
    if kind == "near":
        y = (x[:, :M] + 1e-4 * rng.standard_normal((nb, M, D))).astype(np.float32)
    al, bl = (np.log(rng.random((nb, n)) + 0.1).astype(np.float32) for n in (N, M))
    if kind == "neginf":
        bl[:, ::3] = -np.inf
    old = [(0.1 * rng.standard_normal((nb, n))).astype(np.float32) for n in (N, M, N, M)]
    sm = lambda r, c, lw, pot=None: oracle_c.softmin(EPS1, r, c, lw.astype(np.float64) + (0 if pot is None else pot.astype(np.float64) / EPS1), 1)  # noqa: E731
    init, soft = [], []
    for b in range(nb):
        probs = ((x[b], y[b], bl[b], old[1][b]), (y[b], x[b], al[b], old[0][b]), (x[b], x[b], al[b], old[2][b]), (y[b], y[b], bl[b], old[3][b]))
        init.append([sm(r, c, lw) for r, c, lw, _ in probs])
        soft.append([sm(r, c, lw, pot) for r, c, lw, pot in probs])
    for a in (x, y, al, bl, *old):
        a.setflags(write=False)
    return x, y, al, bl, old, init, soft


SHAPES = [(300, 257, None), (1030, 2100, None), (150, 170, 3), (40, 1, None)]
CASES = [(N, M, D, B, "plain") for D in (17, 24, 41, 257) for N, M, B in SHAPES] + [(300, 257, 41, None, k) for k in ("neginf", "shift", "near")]


@pytest.mark.parametrize("debias", [True, False])
@pytest.mark.parametrize("N,M,D,B,kind", CASES)
def test_iter4_against_float64(cuda, N, M, D, B, kind, debias):
    x, y, al, bl, old, init, soft = _case(N, M, D, B, kind)
    sh = (lambda a: a) if B else (lambda a: a[0])
    dev = lambda a, dt=torch.float32: torch.tensor(sh(a)).to(cuda).to(dt)      # noqa: E731
    dt = torch.bfloat16 if B else torch.float32
    xt, yt, alt, blt = dev(x, dt), dev(y, dt), dev(al), dev(bl)
    k = 4 if debias else 2
    got0 = hip.sinkhorn_iter4(EPS1, xt, yt, alt, blt, None, DAMP, debias, flags=_flag(), p=1)
    got1 = hip.sinkhorn_iter4(EPS1, xt, yt, alt, blt, tuple(dev(o) for o in old[:k]), DAMP, debias, flags=_flag(), p=1)
    assert len(got0) == k and len(got1) == k
    for j in range(k):
        for b in range(B or 1):
            a0, a1 = (g[j].reshape(B or 1, -1)[b].cpu().numpy() for g in (got0, got1))
            # the bound applies to the soft-min: of the initialisation (damping * soft-min) and inside the averaged update
            e0 = np.abs(a0 / DAMP - init[b][j]).max()
            e1 = np.abs((2.0 * a1 - old[j][b].astype(np.float64)) / DAMP - soft[b][j]).max()
            print(f"D={D} N={N} M={M} B={B} {kind} out[{j}] item {b}: init {e0:.2e} / {_sbound(init[b][j]):.2e}, update {e1:.2e} / {_sbound(soft[b][j]):.2e}")
            assert e0 <= _sbound(init[b][j]) and e1 <= _sbound(soft[b][j])


def test_anneal_is_the_loop_of_runs_and_the_null_workspace(cuda):
    N, M, D = 300, 257, 41
    x, y, al, bl = (torch.tensor(a[0]).to(cuda) for a in _case(N, M, D, None, "plain")[:4])
    eps_list, damps = [4.0 * EPS1, 2.0 * EPS1, EPS1], [0.9, 0.95, 1.0]
    final, _ = hip.Iter4Plan(x, y, al, bl, flags=_flag(), p=1).anneal(eps_list, damps)
    final = [t.clone() for t in final]
    plan = hip.Iter4Plan(x, y, al, bl, flags=_flag(), p=1)
    assert plan.ws_args[1] == plan.lib.glhip_sinkhorn_iter4_dist_workspace_bytes(1, N, M, D) > 0
    pots = plan.run(eps_list[0], damps[0], None)
    for e, d in zip(eps_list, damps):
        pots = plan.run(e, d, pots)
    for a, b in zip(final, pots):      # the same launches on the same packed operands
        assert torch.equal(a, b)
    again = hip.Iter4Plan(x, y, al, bl, flags=_flag(), p=1).anneal(eps_list, damps)[0]
    for a, b in zip(final, again):     # bit-identical run to run
        assert torch.equal(a, b)

    # the non-averaged last update, sized and with a NULL workspace (two or four launches of the half-step kernel): both against float64
    last = plan.run(EPS1, DAMP, pots, last=True)
    P = [t.cpu().numpy().astype(np.float64) for t in pots]
    xn, yn, aln, bln = (t.cpu().numpy() for t in (x, y, al, bl))
    refs = [oracle_c.softmin(EPS1, r, c, lw + pot / EPS1, 1)
            for r, c, lw, pot in ((xn, yn, bln, P[1]), (yn, xn, aln, P[0]), (xn, xn, aln, P[2]), (yn, yn, bln, P[3]))]
    outs = [torch.empty_like(t) for t in last]
    rc = plan.lib.glhip_sinkhorn_iter4(*plan.fixed, *[t.data_ptr() for t in pots], *[t.data_ptr() for t in outs], 1, N, M, D, EPS1, DAMP, 1,
                                       plan.dtype, 2, None, 0, _flag(), ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream))
    assert rc == 0, plan.lib.glhip_last_error()
    for sized, null, ref in zip(last, outs, refs):
        es, en = (np.abs(t.cpu().numpy() / DAMP - ref).max() for t in (sized, null))
        print(f"last update: sized {es:.2e}, NULL workspace {en:.2e} / {_sbound(ref):.2e}")
        assert es <= _sbound(ref) and en <= _sbound(ref)


def test_samples_loss_with_and_without_the_packed_iteration(cuda):
    """Tolerances of the p = 2 test (tests/test_iter4_xk_gpu.py): loss 2e-6 relative, gradient 2e-5 of its max-norm."""
    L = SamplesLoss("sinkhorn", p=1, blur=0.3, scaling=0.6, backend="online")
    torch.manual_seed(5)
    x = torch.rand(500, 64, device=cuda).requires_grad_(True)
    y = torch.rand(600, 64, device=cuda)
    res, was = {}, ss._XK_ITER_P1
    for on in (True, False):
        ss._XK_ITER_P1 = on
        try:
            v = L(x, y).sum()
            (g,) = torch.autograd.grad(v, [x])
            res[on] = (v.item(), g.float())
        finally:
            ss._XK_ITER_P1 = was
    (v1, g1), (v0, g0) = res[True], res[False]
    print(f"loss {v1:.8e} / {v0:.8e} (rel {abs(v1 - v0) / abs(v0):.2e}), gradient {(g1 - g0).abs().max().item() / g0.abs().max().item():.2e} of its max-norm")
    assert abs(v1 - v0) <= 2e-6 * abs(v0) + 1e-9
    assert (g1 - g0).abs().max().item() <= 2e-5 * g0.abs().max().item() + 1e-9
