"""Host side of the matrix-core distance reductions of 17 <= D <= 4095 (version 131; geomloss_amd/csrc/glhip_dist_xk.h): the opt-in flag
``GLHIP_FLAG_XK_DIST`` in the family predicates ``glhip_softmin_fwd_family`` (p = 1) and ``glhip_kernel_conv_fwd_family`` (laplacian /
energy), what ignores it, and ``hip.half_step_applies``.  Host arithmetic only: no device."""
import ctypes

import pytest

from geomloss_amd import hip

F32, BF16 = 0, 1
GAUSSIAN, LAPLACIAN, ENERGY = 0, 1, 2
UNSUPPORTED = -2
SYMBOLS = ("glhip_softmin_fwd_family", "glhip_kernel_conv_fwd_family", "glhip_kernel_conv_grad_uses_xk", "glhip_softmin_bwd_x_uses_plan",
           "glhip_kernel_conv_fwd_grad")


@pytest.fixture(scope="module")
def lib():
    assert hip.library_available(), "libgeomloss_hip.so is not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = hip.SIGNATURES[name]
    lib.glhip_version.restype = ctypes.c_int
    return lib


def _families(lib, dtype):
    """(name, family(D, flags, n_ranges=0, B=1)) of the three distance operations"""
    soft = lambda D, flags, n_ranges=0, B=1: lib.glhip_softmin_fwd_family(B, 1000, 2000, D, 1, dtype, flags, n_ranges)  # noqa: E731
    conv = lambda kind: (lambda D, flags, n_ranges=0, B=1: lib.glhip_kernel_conv_fwd_family(kind, B, 1000, 2000, D, dtype, flags, n_ranges))  # noqa: E731
    return (("soft-min p = 1", soft), ("laplacian", conv(LAPLACIAN)), ("energy", conv(ENERGY)))


def test_version_and_constants(lib):
    assert lib.glhip_version() >= 131
    assert hip.FLAG_XK_DIST == 2048
    assert hip.DIST_XK_MAX_DIM == 4095


@pytest.mark.parametrize("extra", [0, hip.FLAG_NO_SPLIT, hip.FLAG_F16X2])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_family_under_the_flag(lib, dtype, extra):
    XK = hip.FLAG_XK_DIST | extra
    for name, fam in _families(lib, dtype):
        for D in (17, 64, 65, 4095):
            assert fam(D, XK) == hip.FAMILY_DIST, (name, D)
            assert fam(D, extra) == hip.FAMILY_GENERIC, (name, D)      # without the flag nothing changes
        assert fam(4096, XK) == hip.FAMILY_GENERIC, name
        assert fam(64, XK, n_ranges=12) == hip.FAMILY_GENERIC, name
        assert fam(64, XK | hip.FLAG_NO_MFMA) == hip.FAMILY_GENERIC, name
        assert fam(64, XK | hip.FLAG_DIRECT) == hip.FAMILY_GENERIC, name
        assert fam(64, XK, B=65536) == hip.FAMILY_GENERIC, name
        assert fam(64, XK, B=65535) == hip.FAMILY_DIST, name
        assert fam(16, XK) == hip.FAMILY_DIST and fam(16, extra) == hip.FAMILY_DIST, name      # glhip_dist_xd.h either way


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_everything_else_ignores_the_flag(lib, dtype):
    XK = hip.FLAG_XK_DIST
    for D in (3, 16, 17, 64, 4095, 4096):
        for extra in (0, hip.FLAG_F16X2, hip.FLAG_NO_MFMA, hip.FLAG_DIRECT):
            for nr in (0, 12):
                B = 1
                a = lib.glhip_softmin_fwd_family(B, 1000, 2000, D, 2, dtype, extra, nr)
                assert lib.glhip_softmin_fwd_family(B, 1000, 2000, D, 2, dtype, extra | XK, nr) == a, (D, extra, nr)
                g = lib.glhip_kernel_conv_fwd_family(GAUSSIAN, B, 1000, 2000, D, dtype, extra, nr)
                assert lib.glhip_kernel_conv_fwd_family(GAUSSIAN, B, 1000, 2000, D, dtype, extra | XK, nr) == g, (D, extra, nr)
        for kind in (GAUSSIAN, LAPLACIAN, ENERGY):
            for base in (0, hip.FLAG_XK_GRAD):
                u = lib.glhip_kernel_conv_grad_uses_xk(kind, 1, 1000, 2000, D, dtype, base, 0)
                assert lib.glhip_kernel_conv_grad_uses_xk(kind, 1, 1000, 2000, D, dtype, base | XK, 0) == u, (kind, D, base)
        for p in (1, 2):
            for base in (0, hip.FLAG_XK_GRAD):
                u = lib.glhip_softmin_bwd_x_uses_plan(1, 1000, 2000, D, p, dtype, base, 0)
                assert lib.glhip_softmin_bwd_x_uses_plan(1, 1000, 2000, D, p, dtype, base | XK, 0) == u, (p, D, base)


@pytest.mark.parametrize("kind", [LAPLACIAN, ENERGY])
def test_product_and_gradient_mode_stays_unsupported(lib, kind):
    """glhip_kernel_conv_fwd_grad on empty clouds (every return of that call comes before its first HIP call): the support rule"""
    fn = lib.glhip_kernel_conv_fwd_grad
    for flags in (hip.FLAG_XK_DIST, hip.FLAG_XK_DIST | hip.FLAG_XK_GRAD):
        for dtype in (F32, BF16):
            assert fn(kind, None, None, None, None, None, 1, 0, 0, 64, 0.5, dtype, None, None, None, 0, None, 0, flags, None) == UNSUPPORTED


def test_half_step_applies():
    XK = hip.FLAG_XK_DIST
    assert hip.half_step_applies(17, 1) is False
    assert hip.half_step_applies(17, 1, XK) is True
    assert hip.half_step_applies(4095, 1, XK) is True
    assert hip.half_step_applies(17, 1, XK, sparse=True) is False
    assert hip.half_step_applies(4096, 1, XK) is False
    assert hip.half_step_applies(17, 1, XK | hip.FLAG_NO_MFMA) is False
    assert hip.half_step_applies(17, 1, XK | hip.FLAG_DIRECT) is False
    # unchanged: the kernels of D <= 16 and p = 2
    assert hip.half_step_applies(16, 1) and hip.half_step_applies(16, 1, XK)
    assert hip.half_step_applies(17, 2) and hip.half_step_applies(17, 2, XK) and not hip.half_step_applies(4096, 2, XK)
