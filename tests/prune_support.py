"""What the tests of the pruned p = 2 soft-min (big dense launches: B = 1, D <= 3, N >= 65536, N M >= 1e11) share: the headline law, the
C-ABI calls (glhip_softmin_fwd with its workspace, glhip_prune_inspect), the float64 rows, and the acceptance rule ``close`` of a pruned
launch against the same call under GLHIP_FLAG_NO_SORT.  A plain module, imported as ``import prune_support as ps``; its host-side checks
are in tests/test_support_cpu.py.  A test of this family imports its call wrappers and its acceptance rule, it does not paste them."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

from geomloss_amd import hip

_TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if _TOOLS not in sys.path:
    sys.path.insert(0, _TOOLS)

import prune_model as pm  # noqa: E402,F401

DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
F16X2, NO_SORT = hip.FLAG_F16X2, hip.FLAG_NO_SORT
LAYOUTS = pytest.mark.parametrize("flags", [F16X2, 0], ids=["f16x2", "bf16x3"])
RECORDS = ("perm_x", "perm_y", "mlb", "t1", "home", "intervals", "t2")      # the output arguments of glhip_prune_inspect, in its order


def law(n, m, seed, D=3, dtype=torch.float32, noise=0.01):
    """the headline law (bench.make_problem) in D dimensions: uniform unit cube, h = -log M + N(0, noise^2) / 0.05^2.  Drawn in the order
    x, y, noise; x (1, n, D) and y (1, m, D) in ``dtype``, h (1, m) float32, on DEV"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(1, n, D, generator=g)
    y = torch.rand(1, m, D, generator=g)
    h = torch.full((1, m), -math.log(m)) + noise * torch.randn(1, m, generator=g) / (0.05**2)
    return x.to(DEV, dtype).contiguous(), y.to(DEV, dtype).contiguous(), h.to(DEV).contiguous()


def workspace(lib, n, m, D, B=1):
    """(buffer, nbytes) of glhip_workspace_bytes"""
    nbytes = int(lib.glhip_workspace_bytes(B, n, m, D, 0))
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=DEV), nbytes


def fwd(x, y, h, eps, flags, ws_bytes=None):
    """one glhip_softmin_fwd call (p = 2) through the C-ABI; ws_bytes: a workspace of that many bytes instead of glhip_workspace_bytes"""
    lib = hip.load_library()
    B, n, D = x.shape
    m = y.shape[1]
    if ws_bytes is None:
        ws, nbytes = workspace(lib, n, m, D, B)
    else:
        ws, nbytes = torch.empty(max(int(ws_bytes), 1), dtype=torch.uint8, device=DEV), int(ws_bytes)
    out = torch.empty((B, n), dtype=torch.float32, device=DEV)
    rc = lib.glhip_softmin_fwd(x.data_ptr(), y.data_ptr(), h.data_ptr(), out.data_ptr(), B, n, m, D, float(eps), 2, hip._dtype_code(x),
                               None, None, None, 0, ctypes.c_void_p(ws.data_ptr()), nbytes, int(flags), hip._stream(x))
    assert rc == 0, lib.glhip_last_error()
    return out


def inspect_call(x, y, logw, eps, pot=None, records=RECORDS):
    """glhip_prune_inspect -> (return code, {record: device tensor}); records not named are passed as NULL and not allocated"""
    lib = hip.load_library()
    _, n, D = x.shape
    m = y.shape[1]
    C, S, nt = (n + 255) // 256, int(lib.glhip_prune_inspect_slots(m)), (n + 31) // 32
    shape = dict(perm_x=(n, torch.int32), perm_y=(m, torch.int32), mlb=(C, torch.float64), t1=(C, torch.float64), home=(C, torch.int32),
                 intervals=((C, S, 2), torch.int32), t2=(nt, torch.float32))
    r = {k: torch.empty(shape[k][0], dtype=shape[k][1], device=DEV) for k in RECORDS if k in records}
    ws, nbytes = workspace(lib, n, m, D)
    rc = lib.glhip_prune_inspect(x.data_ptr(), y.data_ptr(), logw.data_ptr(), None if pot is None else pot.data_ptr(), n, m, D, float(eps),
                                 hip._dtype_code(x), *[r[k].data_ptr() if k in r else None for k in RECORDS],
                                 ctypes.c_void_p(ws.data_ptr()), nbytes, hip._stream(x))
    return rc, r


def inspect(x, y, logw, eps, pot=None, records=RECORDS):
    """glhip_prune_inspect -> NumPy records"""
    rc, r = inspect_call(x, y, logw, eps, pot, records)
    assert rc == 0, hip.load_library().glhip_last_error()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def diam2(x, y):
    """squared diagonal of the bounding box of the finite points of both clouds"""
    z = torch.cat([x[0].float(), y[0].float()])
    z = z[torch.isfinite(z).all(1)]
    return float(((z.max(0).values - z.min(0).values) ** 2).sum())


def close(a, b, diam2, what="dense", require_finite=False):
    """The acceptance rule of a pruned launch ``a`` against ``b``, the same call under GLHIP_FLAG_NO_SORT (or float64 rows): the same NaN
    entries, the same infinite entries with the same sign, and on the entries finite in both
        max|a - b| <= 4e-7 diam2 + 2e-6 max|b|,
    the dense launch's own rounding.  Both constants are those tests/test_hip_kernels.py (its module docstring, "EXPANDED form") holds the
    p = 2 soft-min to against float64: the exponent is a sum of terms of size diam^2 / eps, so the output carries an absolute error of a
    few 2^-24 diam^2 whatever eps is, plus the 2e-6 relative term of the direct form.  require_finite: at least one entry finite in both
    must exist; without it the function returns None when there is none.  Prints the figures and returns (err, bound)."""
    assert torch.equal(a.isnan(), b.isnan())
    assert torch.equal(a.isinf(), b.isinf())
    inf = b.isinf()
    assert torch.equal(a[inf], b[inf])
    ok = ~b.isnan() & ~inf
    if not bool(ok.any()):
        assert not require_finite
        return None
    av, bv = a[ok].double(), b[ok].double()
    err = float((av - bv).abs().max())
    bound = 4e-7 * diam2 + 2e-6 * float(bv.abs().max())
    print(f"max|pruned - {what}| {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (err, bound, diam2)
    return err, bound


def oracle_rows(x, y, hcol, eps, rows):
    """float64 soft-min of a sample of rows; hcol: the column vector as the kernels form it"""
    xi = x[0, rows].double()
    e = hcol[0].double()[None] - torch.cdist(xi, y[0].double()).pow(2) / (2 * eps)
    return -eps * torch.logsumexp(e, 1)


def check_rows(pruned, dense, ref, rows):
    """on the sampled rows where float64 and the dense launch are finite: the pruned result is as close to float64 as the dense one
    (+ 2 float32 ulp of the output); elsewhere ``close`` has already compared the two launches' patterns"""
    ok = torch.isfinite(ref) & torch.isfinite(dense[0, rows])
    if not bool(ok.any()):
        return
    ep = float((pruned[0, rows].double() - ref)[ok].abs().max())
    ed = float((dense[0, rows].double() - ref)[ok].abs().max())
    print(f"error against float64: pruned {ep:.3e} dense {ed:.3e}")
    assert ep <= 1.5 * ed + 2 * float(ref[ok].abs().max()) * 2**-24, (ep, ed)


def compare(x, y, h, eps, flags):
    """the pruned forward against the dense launch (``close``) and, on 256 rows, against float64 (``check_rows``) -> the pruned output"""
    a = fwd(x, y, h, eps, flags)
    b = fwd(x, y, h, eps, flags | NO_SORT)
    close(a, b, diam2(x, y))
    rows = torch.linspace(0, x.shape[1] - 1, 256, device=DEV).long()
    check_rows(a, b, oracle_rows(x.float(), y.float(), h, eps, rows), rows)
    return a


def covered(rec, c, nT):
    """the column blocks (of nT) that the non-empty intervals of slab c cover"""
    k = np.zeros(nT, bool)
    for a, b in rec["intervals"][c]:
        if b > a:
            k[a // pm.BLOCK:(b + pm.BLOCK - 1) // pm.BLOCK] = True
    return k
