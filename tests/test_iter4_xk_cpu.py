"""Host side of the one-launch iteration of 17 <= D <= 4095 (library version 146): glhip_sinkhorn_iter4_workspace_bytes and the gate
of _HipSoftmin._iter4_plan.  Needs the built library, no GPU."""

import pytest
import torch

from geomloss_amd import hip
from geomloss_amd import sinkhorn_samples as ss

GRID = [(1, 1, 1), (1, 40, 1), (1, 300, 257), (1, 1030, 2100), (3, 150, 170), (3, 2048, 2048), (32, 1024, 1024)]


def test_workspace_bytes():
    lib = hip.load_library()
    size = lib.glhip_sinkhorn_iter4_workspace_bytes
    for D in (1, 3, 16):
        for B, N, M in GRID:
            assert size(B, N, M, D, 2) == 4 * lib.glhip_workspace_bytes(B, max(N, M), max(N, M), D, 0)
    prev = None
    for D in (17, 64, 4095):
        got = [size(B, N, M, D, 2) for B, N, M in GRID]
        assert all(g > 0 for g in got)
        for (B, N, M), g in zip(GRID, got):      # non-decreasing in N, M and D
            assert size(B, N + 1, M, D, 2) >= g and size(B, N, M + 31, D, 2) >= g and size(B, N, M, D + 1 if D < 4095 else D, 2) >= g
        assert prev is None or all(g >= q for g, q in zip(got, prev))
        prev = got
    assert size(1, 300, 257, 4096, 2) == 0 and size(1, 300, 257, 17, 1) == 0
    assert size(1, 0, 257, 64, 2) == 0 and size(1, 300, 0, 64, 2) == 0 and size(0, 300, 257, 64, 2) == 0 and size(1, 0, 257, 3, 2) == 0


def test_iter4_plan_gate(monkeypatch):
    monkeypatch.setattr(hip, "Iter4Plan", lambda *a, **kw: ("plan", kw.get("p")))
    x, y = torch.rand(7, 64), torch.rand(7, 64)
    a_log = b_log = torch.zeros(7)

    def plan(p=2, dtype=torch.float32):
        return ss._HipSoftmin(p, False)._iter4_plan((x.to(dtype), y.to(dtype)), a_log, b_log, True, create=True)

    monkeypatch.setattr(ss, "_XK_ITER", True)
    assert plan() == ("plan", 2)
    assert plan(p=1) is None and plan(dtype=torch.float64) is None
    monkeypatch.setattr(hip, "ENV_FLAGS", hip.FLAG_NO_MFMA)
    assert plan() is None
    monkeypatch.setattr(hip, "ENV_FLAGS", 0)
    monkeypatch.setattr(ss, "_XK_ITER", False)
    assert plan() is None
