"""The five workspace sizing calls of the plan family (geomloss_amd/csrc/glhip_launch_plan.h: plan application for D <= 16 and
17 <= D <= 4095, the soft-min and gaussian gradients of 17 <= D <= 4095, argmin) against the values recorded from the library before
their launchers and sizing rules were merged (tests/golden/reference_plan_family_sizing.npz, written by make_golden_plan_family_sizing.py).  A
launcher takes the splits its sizing call promised, so the values are part of the contract: equality on every row.  No device."""
import ctypes
import os

import numpy as np
import pytest

from geomloss_amd import hip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_plan_family_sizing.npz")
CALLS = ("glhip_plan_apply_workspace_bytes", "glhip_plan_apply_nd_workspace_bytes", "glhip_softmin_bwd_x_workspace_bytes",
         "glhip_kernel_conv_grad_workspace_bytes", "glhip_argmin_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    assert hip.library_available(), "libgeomloss_hip.so is not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in CALLS:
        assert hasattr(lib, name), f"{name} is not exported"
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = hip.SIGNATURES[name]
    return lib


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", CALLS)
def test_sizing_matches_the_recorded_values(lib, golden, name):
    args, want = golden[name + ":args"], golden[name + ":bytes"]
    assert len(args) == len(want) >= 1000 and (want > 0).any() and (want == 0).any()
    fn = getattr(lib, name)
    got = np.array([fn(*map(int, r)) for r in args], dtype=np.int64)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{name}: {bad.size} of {len(want)} rows differ; first {args[bad[0]].tolist()} -> {got[bad[0]]}, recorded {want[bad[0]]}"
