"""GPU: raw glhip_softmin_fwd(p = 2) at N = M = 1e6 (the clouds and dual vector of bench.make_problem, seed 1000) over eps, both exponent
layouts: the sorted, pruned call against the same call with GLHIP_FLAG_NO_SORT.  HIP events, mean of 3 launches after one warm-up.
GEOMLOSS_HIP_LIB=<another build of the library> runs the same curve on that build (A/B against a parent commit).

    python tools/prune_curve.py          (from the repository root)
"""
import ctypes
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geomloss_amd import hip  # noqa: E402

DEV = torch.device("cuda:0")
lib = hip.load_library()
print("version", lib.glhip_version(), "(GEOMLOSS_HIP_LIB)" if os.environ.get("GEOMLOSS_HIP_LIB") else "(tree build)", flush=True)
n = 1000000
g = torch.Generator(device="cpu").manual_seed(1000)
x = torch.rand(n, 3, generator=g); y = torch.rand(n, 3, generator=g)
h = torch.full((n,), -math.log(n)) + 0.01 * torch.randn(n, generator=g) / (0.05**2)
x, y, h = x[None].to(DEV).contiguous(), y[None].to(DEV).contiguous(), h[None].to(DEV).contiguous()
nbytes = int(lib.glhip_workspace_bytes(1, n, n, 3, 0))
ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)

def timed(eps, flags):
    out = torch.empty((1, n), dtype=torch.float32, device=DEV)
    def run():
        rc = lib.glhip_softmin_fwd(x.data_ptr(), y.data_ptr(), h.data_ptr(), out.data_ptr(), 1, n, n, 3, float(eps), 2, 0, None, None, None, 0,
                                   ctypes.c_void_p(ws.data_ptr()), nbytes, int(flags), hip._stream(x))
        assert rc == 0, lib.glhip_last_error()
    run(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(3): run()
    b.record(); torch.cuda.synchronize()
    return out, a.elapsed_time(b) / 3

for eps in (0.01**2, 0.05**2, 0.1**2, 0.2**2, 1.0):
    for flags in (hip.FLAG_F16X2, 0):
        if flags and eps < 0.02**2:
            continue
        p, tp = timed(eps, flags)
        d, td = timed(eps, flags | hip.FLAG_NO_SORT)
        print(f"1e6 eps={eps:.4g} flags={flags}: pruned {tp:.2f} ms  dense {td:.2f} ms  ratio {tp / td:.3f}  max|diff| {float((p - d).abs().max()):.3e} nan {int(p.isnan().sum())}", flush=True)
