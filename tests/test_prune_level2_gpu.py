"""Second, in-kernel level of the exact pruning of big dense p = 2 soft-min launches (csrc/glhip_softmin_x32.h: P2; glhip_autosort.h).

Inside the column intervals the first level keeps, every wavefront skips the groups of 32 columns that cannot matter to its 32 rows.
What tests/test_exact_prune_gpu.py cannot see: laws where the second level removes far more than the first, dual values with rare
columns far above the rest, special values inside groups that would otherwise be skipped and inside home blocks, the half-step, shapes
that are no multiples of 32, D < 3, stream capture.  Every case runs the same call with GLHIP_FLAG_NO_SORT (the dense launch) next to
it and is held to prune_support.close: |pruned - dense| <= 4e-7 diam^2 + 2e-6 max|out| with the same NaN / infinity pattern, and on 256
sampled rows (prune_support.check_rows) an error against float64 of at most 1.5 x the dense launch's + 2 ulp.
"""

import ctypes
import math

import pytest
import torch

from geomloss_amd import hip

import prune_support as ps

pytestmark = pytest.mark.gpu

DEV, NO_SORT, LAYOUTS = ps.DEV, ps.NO_SORT, ps.LAYOUTS


# (a) laws where the second level removes much more than the first
@LAYOUTS
def test_small_eps_flat_duals(flags):
    # the law of test_most_pruned_at_small_eps: eps = 0.015^2, diameter^2 / eps = 1.3e4 (inside the f16 x 2 contract)
    x, y, h = ps.law(320000, 320000, 6)
    ps.compare(x, y, torch.zeros_like(h), 0.015**2, flags)


def test_headline_law_at_tiny_eps_bf16x3():
    # eps = 0.01^2: diameter^2 / eps = 3e4 with dual values of +-400 nats — outside the f16 x 2 contract (profiles/r07_prune_curve.txt)
    x, y, h = ps.law(320000, 320000, 12)
    ps.compare(x, y, h, 0.01**2, 0)


@LAYOUTS
def test_bf16_input(flags):
    x, y, h = ps.law(300000, 340000, 13, dtype=torch.bfloat16)
    ps.compare(x, y, torch.zeros_like(h), 0.02**2, flags)


# (b) a few columns far above the rest: whole groups stay for one member, and the home-block seed is not the row's maximum
@LAYOUTS
def test_rare_high_duals(flags):
    x, y, h = ps.law(320000, 320000, 14, noise=0.001)
    h = h.clone()
    h[0, ::10000] += 40.0
    ps.compare(x, y, h, 0.02**2, flags)


# (c) special values inside groups that would otherwise be skipped, and (every ~5000th column: dozens of blocks) inside home blocks
@LAYOUTS
@pytest.mark.parametrize("what", ["y_nan", "y_pinf", "y_minf", "h_nan", "h_pinf", "h_minf", "x_nan", "x_inf"])
def test_special_values(flags, what):
    x, y, h = ps.law(300000, 340000, 15)
    h = torch.zeros_like(h)
    x, y, h = x.clone(), y.clone(), h.clone()
    if what == "y_nan":
        y[0, 777::5003, 1] = math.nan
    elif what == "y_pinf":
        y[0, 777::5003, 0] = math.inf
    elif what == "y_minf":
        y[0, 777::5003, 2] = -math.inf
    elif what == "h_nan":
        h[0, 777::5003] = math.nan
    elif what == "h_pinf":
        h[0, 777::5003] = math.inf
    elif what == "h_minf":
        h[0, 777::5003] = -math.inf
        h[0, 100000:140000] = -math.inf      # whole blocks and groups without mass
    elif what == "x_nan":
        x[0, 555::7001, 1] = math.nan
    else:
        x[0, 555::7001, 0] = math.inf
    ps.compare(x, y, h, 0.02**2, flags)


# (d) the half-step, with pot and prev
@LAYOUTS
def test_half_step(flags):
    x, y, h = ps.law(300000, 340000, 16, noise=0.002)
    eps, damping = 0.02**2, 0.9
    g = torch.Generator().manual_seed(17)
    m, n = y.shape[1], x.shape[1]
    logw = torch.full((1, m), -math.log(m)).to(DEV)
    pot = ((h - logw) * eps).contiguous()      # logw + pot / eps = h
    prev = (0.01 * torch.randn(1, n, generator=g)).to(DEV)
    rows = torch.linspace(0, n - 1, 256, device=DEV).long()
    for p_, v_ in ((pot, prev), (pot, None)):
        a = hip.sinkhorn_step_raw(x, y, logw, p_, v_, eps, damping, 2, None, flags)
        b = hip.sinkhorn_step_raw(x, y, logw, p_, v_, eps, damping, 2, None, flags | NO_SORT)
        ps.close(a, b, ps.diam2(x, y))
        f = ps.oracle_rows(x, y, logw.double() + p_.double() / eps, eps, rows)
        ref = (0.5 * damping * f + 0.5 * v_[0, rows].double()) if v_ is not None else damping * f
        ps.check_rows(a, b, ref, rows)


# (e) N and M no multiples of 32 (nor of the 256-row slab, the 256-column block)
@LAYOUTS
def test_uneven_shapes(flags):
    x, y, h = ps.law(300017, 340003, 18)
    ps.compare(x, y, torch.zeros_like(h), 0.02**2, flags)


# D < 3: the group records carry empty boxes beyond D, the sort's minor key has 3^2 / 8 sub-voxels
@LAYOUTS
@pytest.mark.parametrize("D", [1, 2])
def test_lower_dimensions(flags, D):
    x, y, h = ps.law(320000, 320000, 19 + D, D=D, noise=0.001)
    ps.compare(x, y, h, 0.03**2, flags)


# (f) stream capture and replay equal the eager call, bit for bit
@LAYOUTS
def test_stream_capture(flags):
    x, y, h = ps.law(320000, 320000, 22)
    h = torch.zeros_like(h)
    eps = 0.02**2
    lib = hip.load_library()
    ws, nbytes = ps.workspace(lib, 320000, 320000, 3)
    out = torch.empty((1, 320000), dtype=torch.float32, device=DEV)

    def run():
        rc = lib.glhip_softmin_fwd(x.data_ptr(), y.data_ptr(), h.data_ptr(), out.data_ptr(), 1, 320000, 320000, 3, float(eps), 2,
                                   hip._dtype_code(x), None, None, None, 0, ctypes.c_void_p(ws.data_ptr()), nbytes, int(flags),
                                   hip._stream(x))
        assert rc == 0, lib.glhip_last_error()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                       # the library's kernels are loaded outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager = out.clone()
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    ps.close(out, ps.fwd(x, y, h, eps, flags | NO_SORT), ps.diam2(x, y))
