"""Host side of ``glhip_plan_bilinear`` (version 139; geomloss_amd/csrc/glhip_api_plan_bilinear.hip): exported symbols, the predicate, the
pass width, the workspace sizing and the refusals of the Python wrapper.  Host arithmetic only: no device."""
import ctypes

import pytest
import torch

from geomloss_amd import hip

F32, BF16 = 0, 1
EINVAL = -1
NEW_SYMBOLS = ("glhip_plan_bilinear", "glhip_plan_bilinear_workspace_bytes", "glhip_plan_bilinear_supported", "glhip_plan_bilinear_pass_width")
DIMS = (0, 1, 16, 17, 4095, 4096)


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
    assert lib.glhip_version() >= 139
    assert hip.PLAN_BILINEAR_MAX_DIM == 4095
    for name in NEW_SYMBOLS:
        assert hip._SINCE[name] == 139
    for name in ("plan_bilinear", "plan_bilinear_raw", "plan_bilinear_applies"):
        assert callable(getattr(hip, name))


def test_supported(lib):
    ok = lambda D, K=8, dt=F32, n_ranges=0, B=1, N=1000, M=2000, p=2: lib.glhip_plan_bilinear_supported(B, N, M, D, K, p, dt, n_ranges)  # noqa: E731
    for dt in (F32, BF16):
        assert [ok(D, dt=dt) for D in DIMS] == [EINVAL, 1, 1, 1, 1, 0]
        assert [ok(24, K, dt=dt) for K in DIMS] == [1, 1, 1, 1, 1, 0]      # K == 0 is served: the outputs are zeroed
        for D in (1, 16, 17, 4095):
            assert ok(D, dt=dt, n_ranges=1) == 0                           # block-sparse ranges: in the ABI for later
            assert ok(D, dt=dt, p=1) == 0                                  # p = 1: no kernel
            assert [ok(D, dt=dt, B=B) for B in (1, 65535, 65536)] == [1, 1, 0]
    for D in DIMS:
        assert ok(D, dt=7) == EINVAL                                       # a bad dtype code
        assert ok(D, dt=7, n_ranges=1) == EINVAL
    assert ok(24, N=-1) == EINVAL and ok(24, M=-1) == EINVAL and ok(24, B=-1) == EINVAL and ok(24, K=-1) == EINVAL
    assert ok(24, n_ranges=-1) == EINVAL and ok(24, p=0) == EINVAL and ok(24, p=3) == EINVAL
    assert ok(24, N=0) == 1 and ok(24, M=0) == 1 and ok(24, B=0) == 1      # degenerate sizes are served


def test_pass_width(lib):
    assert lib.glhip_plan_bilinear_pass_width() in (32, 64)


def test_workspace_bytes(lib):
    ws = lib.glhip_plan_bilinear_workspace_bytes
    for args in ((0, 130, 70001, 24, 16), (1, 0, 70001, 24, 16), (1, 130, 0, 24, 16), (1, 130, 70001, 0, 16), (1, 130, 70001, 24, 0),
                 (1, 130, 70001, 4096, 16), (1, 130, 70001, 24, 4096), (-1, 130, 70001, 24, 16)):
        assert ws(*args) == 0, args
    assert ws(1, 130, 70001, 24, 16) > 0
    width = lib.glhip_plan_bilinear_pass_width()
    for D in (1, 3, 16, 17, 64, 4095):
        assert ws(1, 10**6, 10**6, D, 4095) <= 2**30
        for shape in ((1, 130, 70001), (3, 1000, 20000), (1, 10**6, 10**6)):
            for K in (1, 17, 4095):                                        # the partials do not depend on K
                assert ws(*shape, D, K) == ws(*shape, D, 1), (shape, D, K)
            if D >= width:                                                 # nor on D beyond one pass
                assert ws(*shape, D, 8) == ws(*shape, width, 8), (shape, D)


def test_applies_agrees_with_the_library(lib):
    for D in (1, 16, 17, 4095, 4096):
        for dtype, code in ((torch.float32, F32), (torch.bfloat16, BF16)):
            x = torch.empty(0, D, dtype=dtype)
            assert hip.plan_bilinear_applies(x) == (lib.glhip_plan_bilinear_supported(1, 1000, 2000, D, 8, 2, code, 0) == 1), (D, dtype)
            assert hip.plan_bilinear_applies(x, ranges=object()) == (lib.glhip_plan_bilinear_supported(1, 1000, 2000, D, 8, 2, code, 1) == 1)
    assert not hip.plan_bilinear_applies(torch.empty(0, 24, dtype=torch.float64))


def test_refusals_before_any_device_call():
    x, y, h = torch.rand(40, 24), torch.rand(50, 24), torch.zeros(50)
    rf, cf = torch.ones(40, 5), torch.ones(50, 5)
    with pytest.raises(NotImplementedError):
        hip.plan_bilinear(0.8, x.double(), y.double(), h, rf, cf)
    with pytest.raises(NotImplementedError):
        hip.plan_bilinear(0.8, x, y, h, rf, cf, p=1)
    with pytest.raises(NotImplementedError):
        hip.plan_bilinear(0.8, x, y, h, rf, cf, ranges=object())
    with pytest.raises(NotImplementedError):
        hip.plan_bilinear(100.0, torch.rand(40, 4096), torch.rand(50, 4096), h, rf, cf)
    with pytest.raises(NotImplementedError):
        hip.plan_bilinear(0.8, x, y, h, torch.ones(40, 4096), torch.ones(50, 4096))
    for bad in (dict(rowfeat=torch.ones(39, 5)), dict(colfeat=torch.ones(50, 4)), dict(colfeat=torch.ones(50, 5, 1)), dict(h=torch.zeros(49)),
                dict(fwd=torch.zeros(41)), dict(y=torch.rand(50, 23))):
        args = dict(x=x, y=y, h=h, rowfeat=rf, colfeat=cf)
        args.update(bad)
        with pytest.raises(ValueError):
            hip.plan_bilinear(0.8, **args)
