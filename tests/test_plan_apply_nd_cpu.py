"""Host side of ``glhip_plan_apply_nd`` (version 125; geomloss_amd/csrc/glhip_api_plan_xk.hip): exported symbols, the family query, the pass
width and the workspace sizing.  Host arithmetic only: no device."""
import ctypes

import pytest

from geomloss_amd import hip

F32, BF16 = 0, 1
EINVAL, EUNSUPPORTED = -1, -2
NEW_SYMBOLS = ("glhip_plan_apply_nd", "glhip_plan_apply_nd_workspace_bytes", "glhip_plan_apply_nd_family", "glhip_plan_apply_nd_pass_width")


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
    assert lib.glhip_version() >= 125
    assert hip.PLAN_MAX_DIM == 4095
    for name in ("plan_apply_nd", "plan_apply_nd_raw", "plan_apply_nd_applies", "plan_apply_nd_family"):
        assert callable(getattr(hip, name))


@pytest.mark.parametrize("flags", [0, hip.FLAG_F16X2])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_family(lib, dtype, flags):
    fam = lambda D, p=2, n_ranges=0, N=1000, dt=dtype: lib.glhip_plan_apply_nd_family(1, N, 2000, D, 8, p, dt, flags, n_ranges)  # noqa: E731
    for D in (1, 3, 16):
        assert fam(D) == hip.FAMILY_XD
    for D in (17, 64, 4095):
        assert fam(D) == hip.FAMILY_XK
    assert fam(4096) == EUNSUPPORTED
    assert fam(64, p=1) == EUNSUPPORTED
    assert fam(64, n_ranges=12) == EUNSUPPORTED
    assert fam(0) == EINVAL
    assert fam(64, dt=7) == EINVAL
    assert fam(64, N=-1) == EINVAL


def test_family_wrapper():
    assert hip.plan_apply_nd_family(1, 1000, 2000, 16, 8) == hip.FAMILY_XD
    assert hip.plan_apply_nd_family(1, 1000, 2000, 17, 8) == hip.FAMILY_XK
    with pytest.raises(NotImplementedError):
        hip.plan_apply_nd_family(1, 1000, 2000, 4096, 8)
    with pytest.raises(ValueError):
        hip.plan_apply_nd_family(1, 1000, 2000, 0, 8)


def test_pass_width(lib):
    assert [lib.glhip_plan_apply_nd_pass_width(D) for D in (3, 8, 16)] == [128, 64, 32]
    for D in (17, 64, 4095):
        w = lib.glhip_plan_apply_nd_pass_width(D)
        assert w % 32 == 0 and 32 <= w <= 128


def test_workspace_bytes(lib):
    assert lib.glhip_plan_apply_nd_workspace_bytes(1, 130, 70001, 24, 16) > 0
    assert lib.glhip_plan_apply_nd_workspace_bytes(1, 10**6, 10**6, 64, 128) <= 2**30
    # D <= 16: the sizing call of glhip_plan_apply
    assert lib.glhip_plan_apply_nd_workspace_bytes(1, 130, 70001, 8, 16) == lib.glhip_plan_apply_workspace_bytes(1, 130, 70001, 8, 16)
