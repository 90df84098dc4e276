"""The one-launch Sinkhorn iteration of p = 2 clouds of 17 <= D <= 4095 on pre-packed operands (geomloss_amd/csrc/glhip_softmin_xkp.h,
library version 146) against float64: the kernel through hip.sinkhorn_iter4, the library loop through hip.Iter4Plan, the driver through
SamplesLoss."""

import ctypes
import functools

import numpy as np
import pytest
import torch

from geomloss_amd import SamplesLoss, hip
from geomloss_amd import sinkhorn_samples as ss
from oracle import oracle_c

pytestmark = pytest.mark.gpu

DAMP = 0.9


def _eps(D):
    return 0.05**2 * D / 3      # the suite's small p = 2 temperature (tests/test_dimension_sweep_gpu.py)


def _bound(ref, D):
    return 4e-7 * D + 2e-6 * np.abs(ref).max()      # tests/test_hip_kernels.py::test_iter4_equals_four_fused_steps


@functools.lru_cache(maxsize=None)
def _case(N, M, D, B, kind):
    """Clouds in the unit cube (bfloat16-representable for the batched case, moved by 8 for "shift"), log-weights (-inf on a third of the
    columns for "neginf"), old potentials, and per batch item the float64 initialisation and averaged update of (f_ba, g_ab, f_aa, g_bb)."""
    rng = np.random.default_rng([N, M, D, B or 0])
    nb = B or 1
    x, y = rng.random((nb, N, D), dtype=np.float32), rng.random((nb, M, D), dtype=np.float32) * 0.8 + 0.1
    if B:
        x, y = (torch.tensor(t).bfloat16().float().numpy() for t in (x, y))
    if kind == "shift":
        x, y = x + np.float32(8), y + np.float32(8)
    al, bl = (np.log(rng.random((nb, n)) + 0.1).astype(np.float32) for n in (N, M))
    if kind == "neginf":
        bl[:, ::3] = -np.inf
    old = [(0.1 * rng.standard_normal((nb, n))).astype(np.float32) for n in (N, M, N, M)]
    eps = _eps(D)
    sm = lambda r, c, lw, pot=None: oracle_c.softmin(eps, r, c, lw.astype(np.float64) + (0 if pot is None else pot.astype(np.float64) / eps), 2)  # noqa: E731
    init, soft, new = [], [], []
    for b in range(nb):
        probs = ((x[b], y[b], bl[b], old[1][b]), (y[b], x[b], al[b], old[0][b]), (x[b], x[b], al[b], old[2][b]), (y[b], y[b], bl[b], old[3][b]))
        init.append([DAMP * sm(r, c, lw) for r, c, lw, _ in probs])
        soft.append([sm(r, c, lw, pot) for r, c, lw, pot in probs])
        new.append([0.5 * (old[k][b].astype(np.float64) + DAMP * s) for k, s in enumerate(soft[-1])])
    for a in (x, y, al, bl, *old):
        a.setflags(write=False)
    return x, y, al, bl, old, init, soft, new


SHAPES = [(300, 257, None), (1030, 2100, None), (150, 170, 3), (40, 1, None)]
CASES = [(N, M, D, B, "plain") for D in (17, 24, 41, 100, 257) for N, M, B in SHAPES] + [(300, 257, 41, None, "neginf"), (300, 257, 41, None, "shift")]


@pytest.mark.parametrize("debias", [True, False])
@pytest.mark.parametrize("N,M,D,B,kind", CASES)
def test_iter4_against_float64(cuda, N, M, D, B, kind, debias):
    x, y, al, bl, old, init, soft, new = _case(N, M, D, B, kind)
    sh = (lambda a: a) if B else (lambda a: a[0])
    dev = lambda a, dt=torch.float32: torch.tensor(sh(a)).to(cuda).to(dt)      # noqa: E731
    dt = torch.bfloat16 if B else torch.float32
    xt, yt, alt, blt = dev(x, dt), dev(y, dt), dev(al), dev(bl)
    k = 4 if debias else 2
    got0 = hip.sinkhorn_iter4(_eps(D), xt, yt, alt, blt, None, DAMP, debias)
    got1 = hip.sinkhorn_iter4(_eps(D), xt, yt, alt, blt, tuple(dev(o) for o in old[:k]), DAMP, debias)
    assert len(got0) == k and len(got1) == k
    for j in range(k):
        for b in range(B or 1):
            a0, a1 = (g[j].reshape(B or 1, -1)[b].cpu().numpy() for g in (got0, got1))
            e0, e1 = np.abs(a0 - init[b][j]).max(), np.abs(a1 - new[b][j]).max()
            print(f"D={D} N={N} M={M} B={B} {kind} out[{j}] item {b}: init {e0:.2e} / {_bound(init[b][j], D):.2e}, update {e1:.2e} / {_bound(soft[b][j], D):.2e}")
            assert e0 <= _bound(init[b][j], D) and e1 <= _bound(soft[b][j], D)


def test_anneal_is_the_loop_of_runs_and_the_last_update(cuda):
    N, M, D = 300, 257, 41
    x, y, al, bl = (torch.tensor(a[0]).to(cuda) for a in _case(N, M, D, None, "plain")[:4])
    eps_list, damps = [4.0 * _eps(D), 2.0 * _eps(D), _eps(D)], [0.9, 0.95, 1.0]
    final, _ = hip.Iter4Plan(x, y, al, bl).anneal(eps_list, damps)
    final = [t.clone() for t in final]
    plan = hip.Iter4Plan(x, y, al, bl)
    pots = plan.run(eps_list[0], damps[0], None)
    for e, d in zip(eps_list, damps):
        pots = plan.run(e, d, pots)
    for a, b in zip(final, pots):      # the same launches on the same packed operands
        assert torch.equal(a, b)

    eps = eps_list[-1]
    last = plan.run(eps, DAMP, pots, last=True)
    P = [t.cpu().numpy().astype(np.float64) for t in pots]
    xn, yn, aln, bln = (t.cpu().numpy() for t in (x, y, al, bl))
    refs = [DAMP * oracle_c.softmin(eps, r, c, lw + pot / eps, 2)
            for r, c, lw, pot in ((xn, yn, bln, P[1]), (yn, xn, aln, P[0]), (xn, xn, aln, P[2]), (yn, yn, bln, P[3]))]
    for got, ref in zip(last, refs):
        assert np.abs(got.cpu().numpy() - ref).max() <= _bound(ref, D)

    # the same update without a workspace: two or four launches of the half-step kernel.  The two kernels centre the clouds differently,
    # so their difference scales with the clouds, not with one output: max|ref| is taken over the potentials of the call (f_aa and
    # g_bb alone are ~0.035 here, f_ba and g_ab ~1.2)
    scale = max(np.abs(ref).max() for ref in refs)
    outs = [torch.empty_like(t) for t in last]
    rc = plan.lib.glhip_sinkhorn_iter4(*plan.fixed, *[t.data_ptr() for t in pots], *[t.data_ptr() for t in outs], 1, N, M, D, eps, DAMP, 2,
                                       plan.dtype, 2, None, 0, 0, ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream))
    assert rc == 0, plan.lib.glhip_last_error()
    for got, sized in zip(outs, last):
        print(f"no workspace against sized: {(got - sized).abs().max().item():.2e} / {2e-6 * scale:.2e}")
        assert (got - sized).abs().max().item() <= 2e-6 * scale


def test_samples_loss_with_and_without_the_packed_iteration(cuda):
    L = SamplesLoss("sinkhorn", p=2, blur=0.3, scaling=0.6, backend="online")
    for B, dtype in ((None, torch.float32), (3, torch.bfloat16)):
        torch.manual_seed(5)
        shp = (lambda n: (n, 64)) if B is None else (lambda n: (B, n, 64))
        x = torch.rand(shp(500), device=cuda).to(dtype).requires_grad_(True)
        y = torch.rand(shp(600), device=cuda).to(dtype)
        res, was = {}, ss._XK_ITER
        for on in (True, False):
            ss._XK_ITER = on
            try:
                v = L(x, y).sum()
                (g,) = torch.autograd.grad(v, [x])
                res[on] = (v.item(), g.float())
            finally:
                ss._XK_ITER = was
        (v1, g1), (v0, g0) = res[True], res[False]
        gtol = 2e-5 if dtype == torch.float32 else 2 ** -7
        print(f"B={B} {dtype}: loss {v1:.8e} / {v0:.8e} (rel {abs(v1 - v0) / abs(v0):.2e}), gradient {(g1 - g0).abs().max().item() / g0.abs().max().item():.2e} of its max-norm")
        assert abs(v1 - v0) <= 2e-6 * abs(v0) + 1e-9
        assert (g1 - g0).abs().max().item() <= gtol * g0.abs().max().item() + 1e-9
