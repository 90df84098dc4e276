"""Host side of the one-launch p = 1 iteration of 17 <= D <= 4095 (library version 147, hip.FLAG_XK_ITER_DIST):
glhip_sinkhorn_iter4_dist_workspace_bytes and the gate of _HipSoftmin._iter4_plan.  Needs the built library, no GPU."""

import torch

from geomloss_amd import hip
from geomloss_amd import sinkhorn_samples as ss

GRID = [(1, 1, 1), (1, 40, 1), (1, 300, 257), (1, 1030, 2100), (3, 150, 170), (3, 2048, 2048), (32, 1024, 1024)]      # tests/test_iter4_xk_cpu.py


def test_dist_workspace_bytes():
    assert hip.FLAG_XK_ITER_DIST == 65536
    lib = hip.load_library()
    size = lib.glhip_sinkhorn_iter4_dist_workspace_bytes
    prev = None
    for D in (17, 64, 4095):
        got = [size(B, N, M, D) for B, N, M in GRID]
        assert all(g > 0 for g in got)
        for (B, N, M), g in zip(GRID, got):      # non-decreasing in N, M and D
            assert size(B, N + 1, M, D) >= g and size(B, N, M + 31, D) >= g and size(B, N, M, D + 1 if D < 4095 else D) >= g
        assert prev is None or all(g >= q for g, q in zip(got, prev))
        prev = got
    assert size(1, 300, 257, 16) == 0 and size(1, 300, 257, 4096) == 0
    assert size(1, 0, 257, 64) == 0 and size(1, 300, 0, 64) == 0 and size(0, 300, 257, 64) == 0
    assert lib.glhip_sinkhorn_iter4_workspace_bytes(1, 300, 257, 17, 1) == 0      # the route is opt-in


def test_iter4_plan_gate(monkeypatch):
    monkeypatch.setattr(hip, "Iter4Plan", lambda *a, **kw: ("plan", kw.get("p"), kw.get("flags")))
    x, y = torch.rand(7, 64), torch.rand(7, 64)
    a_log = b_log = torch.zeros(7)

    def plan(dtype=torch.float32, multiscale=False):
        return ss._HipSoftmin(1, multiscale)._iter4_plan((x.to(dtype), y.to(dtype), None, None, None), a_log, b_log, True, create=True)

    assert plan() is None      # off by default
    monkeypatch.setattr(ss, "_XK_ITER_P1", True)
    assert plan() == ("plan", 1, hip.FLAG_XK_ITER_DIST)
    assert plan(dtype=torch.float64) is None and plan(multiscale=True) is None
    monkeypatch.setattr(hip, "ENV_FLAGS", hip.FLAG_NO_MFMA)
    assert plan() is None
