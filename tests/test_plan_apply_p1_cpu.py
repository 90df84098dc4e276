"""Host side of ``glhip_plan_apply_p1`` (version 135; geomloss_amd/csrc/glhip_api_plan_p1.hip): exported symbols, the predicate, the pass
width, the workspace sizing and the refusals of the Python wrapper.  Host arithmetic only: no device."""
import ctypes

import pytest
import torch

from geomloss_amd import hip

F32, BF16 = 0, 1
EINVAL = -1
NEW_SYMBOLS = ("glhip_plan_apply_p1", "glhip_plan_apply_p1_workspace_bytes", "glhip_plan_apply_p1_supported", "glhip_plan_apply_p1_pass_width")


@pytest.fixture(scope="module")
def lib():
    assert hip.library_available(), "libgeomloss_hip.so is not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = hip.SIGNATURES[name]
    lib.glhip_version.restype = ctypes.c_int
    return lib


def test_symbols_and_version(lib):
    assert lib.glhip_version() >= 135
    assert hip.PLAN_P1_MAX_DIM == 4095
    for name in NEW_SYMBOLS:
        assert hip._SINCE[name] == 135
    for name in ("plan_apply_p1", "plan_apply_p1_raw", "plan_apply_p1_applies"):
        assert callable(getattr(hip, name))


def test_supported(lib):
    ok = lambda D, dt=F32, n_ranges=0, B=1, N=1000, M=2000, V=8: lib.glhip_plan_apply_p1_supported(B, N, M, D, V, dt, n_ranges)  # noqa: E731
    for dt in (F32, BF16):
        assert [ok(D, dt) for D in (0, 1, 16, 17, 4095, 4096)] == [EINVAL, 1, 1, 1, 1, 0]
        for D in (1, 16, 17, 4095):
            assert ok(D, dt, n_ranges=1) == 0                   # block-sparse ranges: in the ABI for later
            assert [ok(D, dt, B=B) for B in (1, 65535, 65536)] == [1, 1, 0]
    for D in (0, 1, 16, 17, 4095, 4096):
        assert ok(D, dt=7) == EINVAL                            # a bad dtype code
        assert ok(D, dt=7, n_ranges=1) == EINVAL
    assert ok(24, N=-1) == EINVAL and ok(24, M=-1) == EINVAL and ok(24, B=-1) == EINVAL and ok(24, V=-1) == EINVAL
    assert ok(24, n_ranges=-1) == EINVAL
    assert ok(24, N=0) == 1 and ok(24, M=0) == 1 and ok(24, V=0) == 1 and ok(24, B=0) == 1      # degenerate sizes are served


def test_pass_width(lib):
    assert lib.glhip_plan_apply_p1_pass_width() in (32, 64)


def test_workspace_bytes(lib):
    ws = lib.glhip_plan_apply_p1_workspace_bytes
    for args in ((0, 130, 70001, 24, 16), (1, 0, 70001, 24, 16), (1, 130, 0, 24, 16), (1, 130, 70001, 0, 16), (1, 130, 70001, 24, 0),
                 (1, 130, 70001, 4096, 16), (-1, 130, 70001, 24, 16)):
        assert ws(*args) == 0, args
    assert ws(1, 130, 70001, 24, 16) > 0
    width = lib.glhip_plan_apply_p1_pass_width()
    for D in (1, 3, 16, 17, 64, 4095):
        assert ws(1, 10**6, 10**6, D, 4096) <= 2**30
        for shape in ((1, 130, 70001), (3, 1000, 20000), (1, 10**6, 10**6)):
            at_width = ws(*shape, D, width)
            for V in (width + 1, 2 * width, 4096):
                assert ws(*shape, D, V) == at_width, (shape, D, V)


def test_applies_agrees_with_the_library(lib):
    for D in (1, 16, 17, 4095, 4096):
        for dtype, code in ((torch.float32, F32), (torch.bfloat16, BF16)):
            x = torch.empty(0, D, dtype=dtype)
            assert hip.plan_apply_p1_applies(x) == (lib.glhip_plan_apply_p1_supported(1, 1000, 2000, D, 8, code, 0) == 1), (D, dtype)
            assert hip.plan_apply_p1_applies(x, ranges=object()) == (lib.glhip_plan_apply_p1_supported(1, 1000, 2000, D, 8, code, 1) == 1)
    assert not hip.plan_apply_p1_applies(torch.empty(0, 24, dtype=torch.float64))


def test_refusals_before_any_device_call():
    x, y, h, feat = torch.rand(40, 24), torch.rand(50, 24), torch.zeros(50), torch.ones(50, 2)
    with pytest.raises(NotImplementedError):
        hip.plan_apply_p1(0.8, x.double(), y.double(), h, feat)
    with pytest.raises(NotImplementedError):
        hip.plan_apply_p1(100.0, torch.rand(40, 4096), torch.rand(50, 4096), h, feat)
    with pytest.raises(NotImplementedError):
        hip.plan_apply_p1(0.8, x, y, h, feat, ranges=object())
    with pytest.raises(ValueError):
        hip.plan_apply_p1(0.8, x, y, h, torch.ones(49, 2))
    with pytest.raises(ValueError):
        hip.plan_apply_p1(0.8, x, y, h, torch.ones(50, 2, 2))
