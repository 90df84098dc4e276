"""Group-major columns of the sorted p = 2 launch (csrc/glhip_softmin_x32.h: GSRC; csrc/glhip_launch.h).

On the f16 x 2 layout the pruned call packs its sorted columns group by group of 32 — the layout of the LDS tile — and stages every
tile, and the home block of the seed, by a linear copy (the bf16 x 3 layout keeps one record run per column and gathers; it runs the
same cases).  That rests on the intervals being whole blocks of 256 sorted columns, so what can go wrong
sits at the end of the cloud: a last group with fewer than 32 real columns, a last block with fewer than 8 groups, a home block
that is that last block, special values among the last real columns.  The shapes here have M mod 32 = 5 and M mod 256 = 37 (the
last group holds 5 real columns, the last block 2 groups) and are the smallest the call prunes (N M >= 1e11).

Every case runs the same call with GLHIP_FLAG_NO_SORT (the dense launch) next to it and is held to the rule of
tests/test_prune_level2_gpu.py: |pruned - dense| <= 4e-7 diam^2 + 2e-6 max|out| with the same NaN / infinity pattern, and on 256
sampled rows an error against float64 of at most 1.5 x the dense launch's + 2 ulp.
"""

import ctypes
import math

import numpy as np
import pytest
import torch

from geomloss_amd import hip

pytestmark = pytest.mark.gpu

F16X2, NO_SORT = hip.FLAG_F16X2, hip.FLAG_NO_SORT
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
LAYOUTS = pytest.mark.parametrize("flags", [F16X2, 0], ids=["f16x2", "bf16x3"])
N, M = 317000, 320037
EPS = 0.05**2
assert M % 32 == 5 and M % 256 == 37 and N * M >= 1e11 and M * N >= 1e11


def _law(n, m, seed, D=3, dtype=torch.float32, noise=0.01):
    """the headline law (bench.make_problem) in D dimensions: uniform unit cube, h = -log M + N(0, noise^2) / 0.05^2"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(1, n, D, generator=g)
    y = torch.rand(1, m, D, generator=g)
    h = torch.full((1, m), -math.log(m)) + noise * torch.randn(1, m, generator=g) / (0.05**2)
    return x.to(DEV, dtype).contiguous(), y.to(DEV, dtype).contiguous(), h.to(DEV).contiguous()


def _workspace(lib, n, m, D):
    nbytes = int(lib.glhip_workspace_bytes(1, n, m, D, 0))
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=DEV), nbytes


def _fwd(x, y, h, eps, flags):
    lib = hip.load_library()
    B, n, D = x.shape
    m = y.shape[1]
    ws, nbytes = _workspace(lib, n, m, D)
    out = torch.empty((B, n), dtype=torch.float32, device=DEV)
    rc = lib.glhip_softmin_fwd(x.data_ptr(), y.data_ptr(), h.data_ptr(), out.data_ptr(), B, n, m, D, float(eps), 2, hip._dtype_code(x),
                               None, None, None, 0, ctypes.c_void_p(ws.data_ptr()), nbytes, int(flags), hip._stream(x))
    assert rc == 0, lib.glhip_last_error()
    return out


def _inspect(x, y, logw, pot, eps):
    """glhip_prune_inspect -> NumPy records"""
    lib = hip.load_library()
    _, n, D = x.shape
    m = y.shape[1]
    C, S, nt = (n + 255) // 256, int(lib.glhip_prune_inspect_slots(m)), (n + 31) // 32
    i32, f64 = dict(dtype=torch.int32, device=DEV), dict(dtype=torch.float64, device=DEV)
    r = dict(perm_x=torch.empty(n, **i32), perm_y=torch.empty(m, **i32), mlb=torch.empty(C, **f64), t1=torch.empty(C, **f64),
             home=torch.empty(C, **i32), intervals=torch.empty((C, S, 2), **i32), t2=torch.empty(nt, dtype=torch.float32, device=DEV))
    ws, nbytes = _workspace(lib, n, m, D)
    rc = lib.glhip_prune_inspect(x.data_ptr(), y.data_ptr(), logw.data_ptr(), None if pot is None else pot.data_ptr(), n, m, D, float(eps),
                                 hip._dtype_code(x), *[r[k].data_ptr() for k in ("perm_x", "perm_y", "mlb", "t1", "home", "intervals", "t2")],
                                 ctypes.c_void_p(ws.data_ptr()), nbytes, hip._stream(x))
    assert rc == 0, lib.glhip_last_error()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _diam2(x, y):
    z = torch.cat([x[0].float(), y[0].float()])
    z = z[torch.isfinite(z).all(1)]
    return float(((z.max(0).values - z.min(0).values) ** 2).sum())


def _close(a, b, diam2):
    """tests/test_exact_prune_gpu.py: the dense launch's own rounding, same NaN / infinity pattern"""
    assert torch.equal(a.isnan(), b.isnan())
    fin = ~b.isnan()
    if not bool(fin.any()):
        return
    assert torch.equal(a[fin].isinf(), b[fin].isinf()) and torch.equal(a[fin & a.isinf()], b[fin & b.isinf()])
    ok = fin & ~b.isinf()
    if bool(ok.any()):
        av, bv = a[ok].double(), b[ok].double()
        err = float((av - bv).abs().max())
        print(f"max|pruned - dense| {err:.3e} (bound {4e-7 * diam2 + 2e-6 * float(bv.abs().max()):.3e})")
        assert err <= 4e-7 * diam2 + 2e-6 * float(bv.abs().max()), (err, diam2)


def _oracle_rows(x, y, hcol, eps, rows):
    """float64 soft-min of a sample of rows; hcol: the column vector as the kernels form it"""
    xi = x[0, rows].double()
    e = hcol[0].double()[None] - torch.cdist(xi, y[0].double()).pow(2) / (2 * eps)
    return -eps * torch.logsumexp(e, 1)


def _check_rows(pruned, dense, ref, rows):
    """on the sampled rows where float64 and the dense launch are finite: the pruned result is as close to float64 as the dense one
    (+ 2 float32 ulp of the output); elsewhere _close has already compared the two launches' patterns"""
    ok = torch.isfinite(ref) & torch.isfinite(dense[0, rows])
    if not bool(ok.any()):
        return
    ep = float((pruned[0, rows].double() - ref)[ok].abs().max())
    ed = float((dense[0, rows].double() - ref)[ok].abs().max())
    print(f"error against float64: pruned {ep:.3e} dense {ed:.3e}")
    assert ep <= 1.5 * ed + 2 * float(ref[ok].abs().max()) * 2**-24, (ep, ed)


def _compare(x, y, h, eps, flags):
    a = _fwd(x, y, h, eps, flags)
    b = _fwd(x, y, h, eps, flags | NO_SORT)
    _close(a, b, _diam2(x, y))
    rows = torch.linspace(0, x.shape[1] - 1, 256, device=DEV).long()
    _check_rows(a, b, _oracle_rows(x.float(), y.float(), h, eps, rows), rows)
    return a


# 1. the headline law at the uneven shape, and with the two sizes swapped (then N mod 32 = 5: a last row tile of 5 rows)
@LAYOUTS
@pytest.mark.parametrize("shape", [(N, M), (M, N)], ids=["M_uneven", "N_uneven"])
def test_headline_law_uneven(flags, shape):
    x, y, h = _law(shape[0], shape[1], 41)
    _compare(x, y, h, EPS, flags)


# 2. the home block of some slabs is the cloud's last block: 37 columns, 2 groups, the second with 5 real columns
@LAYOUTS
def test_home_block_is_the_partial_last_block(flags):
    x, y, h = _law(N, M, 42)
    rec = _inspect(x, y, h, None, EPS)
    nT = (M + 255) // 256
    last = torch.from_numpy(rec["perm_y"][(nT - 1) * 256:].astype(np.int64)).to(DEV)
    assert len(last) == 37
    h = h.clone()
    h[0, last] += 8.0
    rec = _inspect(x, y, h, None, EPS)      # (the dual values do not enter the sort: the same order)
    n_home = int((rec["home"] == nT - 1).sum())
    print(f"{n_home} slabs have the last, partial block as their home block")
    assert n_home >= 1
    _compare(x, y, h, EPS, flags)


# 3. special values among the 5 real columns of the padded last group
@LAYOUTS
@pytest.mark.parametrize("what", ["h_nan", "h_minf", "y_nan"])
def test_special_values_in_the_padded_last_group(flags, what):
    x, y, h = _law(N, M, 43)
    rec = _inspect(x, y, h, None, EPS)
    y, h = y.clone(), h.clone()
    if what == "y_nan":
        # A NaN in the last coordinate leaves the bounding box alone and changes only the last digit of a point's path key: a point
        # stays inside its run of voxels along the last axis.  With it in every one of the last 4000 sorted columns (more than the
        # ~2800 of a whole run), the path's last run, and so the last group, holds such columns only.
        idx = torch.from_numpy(rec["perm_y"][-4000:].astype(np.int64)).to(DEV)
        y[0, idx, 2] = math.nan
        rec = _inspect(x, y, h, None, EPS)
        tail = torch.from_numpy(rec["perm_y"][-5:].astype(np.int64)).to(DEV)
        assert bool(y[0, tail, 2].isnan().all())
    else:
        j = int(rec["perm_y"][M - 2])
        h[0, j] = math.nan if what == "h_nan" else -math.inf
    _compare(x, y, h, EPS, flags)


# 4. D < 3, and bf16 inputs, at the uneven shape
@pytest.mark.parametrize("D", [1, 2])
def test_lower_dimensions_uneven(D):
    x, y, h = _law(N, M, 44 + D, D=D, noise=0.001)
    _compare(x, y, h, 0.03**2, F16X2)


@LAYOUTS
def test_bf16_input_uneven(flags):
    x, y, h = _law(N, M, 47, dtype=torch.bfloat16)
    _compare(x, y, h, EPS, flags)


# 5. the half-step: its thresholds are those of the forward call on the dual values it forms
def test_half_step_uneven():
    eps, damping = 0.03**2, 0.9
    x, y, logw = _law(N, M, 48, noise=0.001)
    g = torch.Generator().manual_seed(5)
    pot = (0.002 * torch.randn(1, M, generator=g)).to(DEV)
    scale = np.float32(1.0) / np.float32(eps)
    hcol = (pot.double() * float(scale) + logw.double()).float()      # fma(pot, 1 / eps, logw): one rounding
    a = _inspect(x, y, logw, pot, eps)
    b = _inspect(x, y, hcol, None, eps)
    assert (a["home"] >= 0).any() and np.isfinite(a["t2"]).any()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    rows = torch.linspace(0, N - 1, 256, device=DEV).long()
    for flags in (F16X2, 0):
        p = hip.sinkhorn_step_raw(x, y, logw, pot, None, eps, damping, 2, None, flags)
        d = hip.sinkhorn_step_raw(x, y, logw, pot, None, eps, damping, 2, None, flags | NO_SORT)
        _close(p, d, _diam2(x, y))
        _check_rows(p, d, damping * _oracle_rows(x, y, hcol, eps, rows), rows)


# 6. stream capture and replay equal the eager call, bit for bit
def test_stream_capture_uneven():
    x, y, h = _law(N, M, 49)
    lib = hip.load_library()
    ws, nbytes = _workspace(lib, N, M, 3)
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
    _close(out, _fwd(x, y, h, EPS, F16X2 | NO_SORT), _diam2(x, y))
