"""Exact block pruning of big dense p = 2 soft-min reductions (csrc/glhip_autosort.h, glhip_prune.hip: prune_slabs_kernel).

Big dense p = 2 launches (B = 1, D <= 3, N >= 65536, N M >= 1e11) sort both clouds inside the library and reduce only the column blocks
that can change a float32 result.  Every case runs the same call with GLHIP_FLAG_NO_SORT (the dense launch) next to it: the two differ
by the rounding of the dense path itself (another summation order, another f16 x 2 centre), never by dropped mass.
"""

import ctypes
import math

import pytest
import torch

from geomloss_amd import hip

import prune_support as ps

pytestmark = pytest.mark.gpu

DEV, F16X2, NO_SORT, LAYOUTS = ps.DEV, ps.F16X2, ps.NO_SORT, ps.LAYOUTS
EPS = 0.05**2


def _check_oracle(x, y, h, eps, flags, pruned):
    """the pruned result is as close to float64 as the dense launch is (plus one float32 ulp of the output)"""
    n = x.shape[1]
    rows = torch.linspace(0, n - 1, 256, device=DEV).long()
    ref = ps.oracle_rows(x.float(), y.float(), h, eps, rows)
    dense = ps.fwd(x, y, h, eps, flags | NO_SORT)
    ep = float((pruned[0, rows].double() - ref).abs().max())
    ed = float((dense[0, rows].double() - ref).abs().max())
    assert ep <= 1.5 * ed + 2 * float(ref.abs().max()) * 2**-24, (ep, ed)


@LAYOUTS
def test_headline_law_matches_dense(flags):
    x, y, h = ps.law(320000, 320000, 1)
    a = ps.fwd(x, y, h, EPS, flags)
    ps.close(a, ps.fwd(x, y, h, EPS, flags | NO_SORT), ps.diam2(x, y))
    _check_oracle(x, y, h, EPS, flags, a)


@LAYOUTS
def test_uneven_shapes(flags):
    # N != M, N not a multiple of the 256-row slab, M not a multiple of the 256-column block
    x, y, h = ps.law(250001, 400007, 2)
    a = ps.fwd(x, y, h, EPS, flags)
    ps.close(a, ps.fwd(x, y, h, EPS, flags | NO_SORT), ps.diam2(x, y))
    _check_oracle(x, y, h, EPS, flags, a)


@LAYOUTS
def test_bf16_input(flags):
    x, y, h = ps.law(300000, 340000, 3, dtype=torch.bfloat16)
    ps.close(ps.fwd(x, y, h, EPS, flags), ps.fwd(x, y, h, EPS, flags | NO_SORT), ps.diam2(x, y))


@LAYOUTS
def test_clusters_with_far_outlier(flags):
    g = torch.Generator().manual_seed(4)
    n = 327680
    cx = torch.rand(16, 3, generator=g)
    x = cx[torch.randint(0, 16, (n,), generator=g)] + 0.02 * torch.randn(n, 3, generator=g)
    y = cx[torch.randint(0, 16, (n,), generator=g)] + 0.02 * torch.randn(n, 3, generator=g)
    x[12345] = torch.tensor([3.0, 3.0, 3.0])      # far from everything: its row keeps whatever its bound asks for
    y[777] = torch.tensor([-2.0, 2.5, 0.5])
    h = 0.3 * torch.randn(n, generator=g)
    x, y, h = x[None].to(DEV).contiguous(), y[None].to(DEV).contiguous(), h[None].to(DEV).contiguous()
    eps = 0.1**2      # diameter^2 / eps ~ 4e3: inside the f16 x 2 range contract
    a = ps.fwd(x, y, h, eps, flags)
    ps.close(a, ps.fwd(x, y, h, eps, flags | NO_SORT), ps.diam2(x, y))
    _check_oracle(x, y, h, eps, flags, a)


@LAYOUTS
def test_nothing_pruned_at_large_eps(flags):
    x, y, h = ps.law(320000, 320000, 5)
    ps.close(ps.fwd(x, y, h, 1.0, flags), ps.fwd(x, y, h, 1.0, flags | NO_SORT), ps.diam2(x, y))


def test_most_pruned_at_small_eps():
    # eps = 0.015^2: diameter^2 / eps = 1.3e4, inside the f16 x 2 contract; the CPU model (tools/prune_model.py) keeps < 10 % here
    x, y, h = ps.law(320000, 320000, 6)
    h = torch.zeros_like(h)
    eps = 0.015**2
    for flags in (F16X2, 0):
        a = ps.fwd(x, y, h, eps, flags)
        ps.close(a, ps.fwd(x, y, h, eps, flags | NO_SORT), ps.diam2(x, y))
        _check_oracle(x, y, h, eps, flags, a)


@LAYOUTS
def test_half_step_matches_dense(flags):
    x, y, h = ps.law(300000, 340000, 7)
    g = torch.Generator().manual_seed(8)
    m, n = y.shape[1], x.shape[1]
    logw = torch.full((1, m), -math.log(m)).to(DEV)
    pot = (h - logw) * EPS      # logw + pot / EPS = h
    prev = (0.01 * torch.randn(1, n, generator=g)).to(DEV)
    for p_, v_ in ((pot, prev), (pot, None), (None, None)):
        a = hip.sinkhorn_step_raw(x, y, logw if p_ is not None else h, p_, v_, EPS, 0.9, 2, None, flags)
        b = hip.sinkhorn_step_raw(x, y, logw if p_ is not None else h, p_, v_, EPS, 0.9, 2, None, flags | NO_SORT)
        ps.close(a, b, ps.diam2(x, y))


@LAYOUTS
def test_special_values(flags):
    x, y, h = ps.law(300000, 340000, 9)
    # -inf entries: whole blocks of them may go
    hm = h.clone()
    hm[0, ::3] = -math.inf
    hm[0, 1000:90000] = -math.inf
    ps.close(ps.fwd(x, y, hm, EPS, flags), ps.fwd(x, y, hm, EPS, flags | NO_SORT), ps.diam2(x, y))
    # all -inf: every slab keeps everything
    hi = torch.full_like(h, -math.inf)
    ps.close(ps.fwd(x, y, hi, EPS, flags), ps.fwd(x, y, hi, EPS, flags | NO_SORT), ps.diam2(x, y))
    # one NaN in h: the dense launch's NaN pattern
    hn = h.clone()
    hn[0, 4321] = math.nan
    ps.close(ps.fwd(x, y, hn, EPS, flags), ps.fwd(x, y, hn, EPS, flags | NO_SORT), ps.diam2(x, y))
    # one NaN coordinate in x, then in y
    xn = x.clone()
    xn[0, 555, 1] = math.nan
    ps.close(ps.fwd(xn, y, h, EPS, flags), ps.fwd(xn, y, h, EPS, flags | NO_SORT), ps.diam2(xn, y))
    yn = y.clone()
    yn[0, 666, 2] = math.nan
    ps.close(ps.fwd(x, yn, h, EPS, flags), ps.fwd(x, yn, h, EPS, flags | NO_SORT), ps.diam2(x, yn))


def test_small_workspace_falls_back_to_dense():
    x, y, h = ps.law(320000, 320000, 10)
    lib = hip.load_library()
    full = int(lib.glhip_workspace_bytes(1, 320000, 320000, 3, 0))
    small = full // 8
    # too small for the sorted call: the dense launch on the same (smaller) workspace, bit for bit
    assert torch.equal(ps.fwd(x, y, h, EPS, F16X2, small), ps.fwd(x, y, h, EPS, F16X2 | NO_SORT, small))


def test_stream_capture():
    x, y, h = ps.law(320000, 320000, 11)
    lib = hip.load_library()
    ws, nbytes = ps.workspace(lib, 320000, 320000, 3)
    out = torch.empty((1, 320000), dtype=torch.float32, device=DEV)

    def run():
        rc = lib.glhip_softmin_fwd(x.data_ptr(), y.data_ptr(), h.data_ptr(), out.data_ptr(), 1, 320000, 320000, 3, float(EPS), 2,
                                   hip._dtype_code(x), None, None, None, 0, ctypes.c_void_p(ws.data_ptr()), nbytes, F16X2,
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
