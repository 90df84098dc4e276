"""Group-major columns of the sorted p = 2 launch (csrc/glhip_softmin_x32.h: GSRC; csrc/glhip_launch.h).

On the f16 x 2 layout the pruned call packs its sorted columns group by group of 32 — the layout of the LDS tile — and stages every
tile, and the home block of the seed, by a linear copy (the bf16 x 3 layout keeps one record run per column and gathers; it runs the
same cases).  That rests on the intervals being whole blocks of 256 sorted columns, so what can go wrong
sits at the end of the cloud: a last group with fewer than 32 real columns, a last block with fewer than 8 groups, a home block
that is that last block, special values among the last real columns.  The shapes here have M mod 32 = 5 and M mod 256 = 37 (the
last group holds 5 real columns, the last block 2 groups) and are the smallest the call prunes (N M >= 1e11).

Every case runs the same call with GLHIP_FLAG_NO_SORT (the dense launch) next to it and is held to prune_support.close:
|pruned - dense| <= 4e-7 diam^2 + 2e-6 max|out| with the same NaN / infinity pattern, and on 256 sampled rows
(prune_support.check_rows) an error against float64 of at most 1.5 x the dense launch's + 2 ulp.
"""

import ctypes
import math

import numpy as np
import pytest
import torch

from geomloss_amd import hip

import prune_support as ps

pytestmark = pytest.mark.gpu

DEV, F16X2, NO_SORT, LAYOUTS = ps.DEV, ps.F16X2, ps.NO_SORT, ps.LAYOUTS
N, M = 317000, 320037
EPS = 0.05**2
assert M % 32 == 5 and M % 256 == 37 and N * M >= 1e11 and M * N >= 1e11


# 1. the headline law at the uneven shape, and with the two sizes swapped (then N mod 32 = 5: a last row tile of 5 rows)
@LAYOUTS
@pytest.mark.parametrize("shape", [(N, M), (M, N)], ids=["M_uneven", "N_uneven"])
def test_headline_law_uneven(flags, shape):
    x, y, h = ps.law(shape[0], shape[1], 41)
    ps.compare(x, y, h, EPS, flags)


# 2. the home block of some slabs is the cloud's last block: 37 columns, 2 groups, the second with 5 real columns
@LAYOUTS
def test_home_block_is_the_partial_last_block(flags):
    x, y, h = ps.law(N, M, 42)
    rec = ps.inspect(x, y, h, EPS)
    nT = (M + 255) // 256
    last = torch.from_numpy(rec["perm_y"][(nT - 1) * 256:].astype(np.int64)).to(DEV)
    assert len(last) == 37
    h = h.clone()
    h[0, last] += 8.0
    rec = ps.inspect(x, y, h, EPS)      # (the dual values do not enter the sort: the same order)
    n_home = int((rec["home"] == nT - 1).sum())
    print(f"{n_home} slabs have the last, partial block as their home block")
    assert n_home >= 1
    ps.compare(x, y, h, EPS, flags)


# 3. special values among the 5 real columns of the padded last group
@LAYOUTS
@pytest.mark.parametrize("what", ["h_nan", "h_minf", "y_nan"])
def test_special_values_in_the_padded_last_group(flags, what):
    x, y, h = ps.law(N, M, 43)
    rec = ps.inspect(x, y, h, EPS)
    y, h = y.clone(), h.clone()
    if what == "y_nan":
        # A NaN in the last coordinate leaves the bounding box alone and changes only the last digit of a point's path key: a point
        # stays inside its run of voxels along the last axis.  With it in every one of the last 4000 sorted columns (more than the
        # ~2800 of a whole run), the path's last run, and so the last group, holds such columns only.
        idx = torch.from_numpy(rec["perm_y"][-4000:].astype(np.int64)).to(DEV)
        y[0, idx, 2] = math.nan
        rec = ps.inspect(x, y, h, EPS)
        tail = torch.from_numpy(rec["perm_y"][-5:].astype(np.int64)).to(DEV)
        assert bool(y[0, tail, 2].isnan().all())
    else:
        j = int(rec["perm_y"][M - 2])
        h[0, j] = math.nan if what == "h_nan" else -math.inf
    ps.compare(x, y, h, EPS, flags)


# 4. D < 3, and bf16 inputs, at the uneven shape
@pytest.mark.parametrize("D", [1, 2])
def test_lower_dimensions_uneven(D):
    x, y, h = ps.law(N, M, 44 + D, D=D, noise=0.001)
    ps.compare(x, y, h, 0.03**2, F16X2)


@LAYOUTS
def test_bf16_input_uneven(flags):
    x, y, h = ps.law(N, M, 47, dtype=torch.bfloat16)
    ps.compare(x, y, h, EPS, flags)


# 5. the half-step: its thresholds are those of the forward call on the dual values it forms
def test_half_step_uneven():
    eps, damping = 0.03**2, 0.9
    x, y, logw = ps.law(N, M, 48, noise=0.001)
    g = torch.Generator().manual_seed(5)
    pot = (0.002 * torch.randn(1, M, generator=g)).to(DEV)
    scale = np.float32(1.0) / np.float32(eps)
    hcol = (pot.double() * float(scale) + logw.double()).float()      # fma(pot, 1 / eps, logw): one rounding
    a = ps.inspect(x, y, logw, eps, pot)
    b = ps.inspect(x, y, hcol, eps)
    assert (a["home"] >= 0).any() and np.isfinite(a["t2"]).any()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    rows = torch.linspace(0, N - 1, 256, device=DEV).long()
    for flags in (F16X2, 0):
        p = hip.sinkhorn_step_raw(x, y, logw, pot, None, eps, damping, 2, None, flags)
        d = hip.sinkhorn_step_raw(x, y, logw, pot, None, eps, damping, 2, None, flags | NO_SORT)
        ps.close(p, d, ps.diam2(x, y))
        ps.check_rows(p, d, damping * ps.oracle_rows(x, y, hcol, eps, rows), rows)


# 6. stream capture and replay equal the eager call, bit for bit
def test_stream_capture_uneven():
    x, y, h = ps.law(N, M, 49)
    lib = hip.load_library()
    ws, nbytes = ps.workspace(lib, N, M, 3)
    out = torch.empty((1, N), dtype=torch.float32, device=DEV)

    def run():
        rc = lib.glhip_softmin_fwd(x.data_ptr(), y.data_ptr(), h.data_ptr(), out.data_ptr(), 1, N, M, 3, float(EPS), 2,
                                   hip._dtype_code(x), None, None, None, 0, ctypes.c_void_p(ws.data_ptr()), nbytes, int(F16X2),
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
    ps.close(out, ps.fwd(x, y, h, EPS, F16X2 | NO_SORT), ps.diam2(x, y))
