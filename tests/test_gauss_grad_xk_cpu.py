"""Host side of the matrix-core gaussian kernel gradient of 17 <= D <= 4095 (version 130; geomloss_amd/csrc/glhip_api_convgrad_xk.hip):
the second meaning of ``GLHIP_FLAG_XK_GRAD``, the predicate ``glhip_kernel_conv_grad_uses_xk`` and the sizing call
``glhip_kernel_conv_grad_workspace_bytes``.  Host arithmetic only: no device."""
import ctypes

import pytest

from geomloss_amd import hip

F32, BF16 = 0, 1
GAUSSIAN, LAPLACIAN, ENERGY = 0, 1, 2
EINVAL = -1
NEW_SYMBOLS = ("glhip_kernel_conv_grad_uses_xk", "glhip_kernel_conv_grad_workspace_bytes")


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
    assert lib.glhip_version() >= 130
    assert hip.FLAG_XK_GRAD == 1024
    assert (hip.GAUSSIAN, hip.LAPLACIAN, hip.ENERGY) == (GAUSSIAN, LAPLACIAN, ENERGY)
    assert callable(hip.kernel_conv_grad_uses_xk)


@pytest.mark.parametrize("extra", [0, hip.FLAG_F16X2, hip.FLAG_NO_SPLIT])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_predicate(lib, dtype, extra):
    XK = hip.FLAG_XK_GRAD | extra
    use = lambda D, flags=XK, kind=GAUSSIAN, n_ranges=0, B=1, N=1000, dt=dtype: lib.glhip_kernel_conv_grad_uses_xk(  # noqa: E731
        kind, B, N, 2000, D, dt, flags, n_ranges)
    for D in (17, 64, 65, 4095):
        assert use(D) == 1
        assert use(D, flags=extra) == 0                    # without the flag nothing changes
    assert use(16) == 0 and use(1) == 0 and use(4096) == 0
    assert use(64, kind=LAPLACIAN) == 0 and use(64, kind=ENERGY) == 0
    assert use(64, n_ranges=12) == 0
    assert use(64, flags=XK | hip.FLAG_NO_MFMA) == 0
    assert use(64, flags=XK | hip.FLAG_DIRECT) == 0
    assert use(64, B=65535) == 1 and use(64, B=65536) == 0
    assert use(64, N=-1) == EINVAL
    assert use(64, B=-1) == EINVAL
    assert use(0) == EINVAL
    assert use(64, kind=3) == EINVAL and use(64, kind=-1) == EINVAL
    assert use(64, n_ranges=-1) == EINVAL
    assert use(64, dt=7) == EINVAL


def test_predicate_wrapper():
    XK = hip.FLAG_XK_GRAD
    assert hip.kernel_conv_grad_uses_xk("gaussian", 1, 1000, 2000, 17, flags=XK) == 1
    assert hip.kernel_conv_grad_uses_xk(hip.GAUSSIAN, 1, 1000, 2000, 17, flags=XK) == 1
    assert hip.kernel_conv_grad_uses_xk("gaussian", 1, 1000, 2000, 17, dtype=hip.BF16, flags=XK) == 1
    assert hip.kernel_conv_grad_uses_xk("gaussian", 1, 1000, 2000, 17) == 0
    assert hip.kernel_conv_grad_uses_xk("laplacian", 1, 1000, 2000, 17, flags=XK) == 0
    assert hip.kernel_conv_grad_uses_xk("energy", 1, 1000, 2000, 17, flags=XK) == 0
    assert hip.kernel_conv_grad_uses_xk("gaussian", 1, 1000, 2000, 4096, flags=XK) == 0
    with pytest.raises(ValueError):
        hip.kernel_conv_grad_uses_xk("gaussian", 1, -1, 2000, 17, flags=XK)


def test_workspace_bytes(lib):
    XK = hip.FLAG_XK_GRAD
    ws = lib.glhip_kernel_conv_grad_workspace_bytes
    assert ws(1, 130, 70001, 72, XK) > 0
    assert ws(1, 130, 70001, 72, XK) % (130 * (64 + 2) * 4) == 0          # whole splits of the widest pass: 64 sums, signed mass, maximum
    assert ws(1, 130, 70001, 72, XK) // (130 * (64 + 2) * 4) >= 2
    assert ws(1, 130, 70001, 24, XK) % (130 * (24 + 2) * 4) == 0
    assert ws(1, 130, 70001, 72, XK | hip.FLAG_F16X2) == ws(1, 130, 70001, 72, XK)
    # 0 wherever the predicate is 0 (those launches size their workspace with glhip_workspace_bytes, as before)
    for D, flags in ((72, 0), (16, XK), (4096, XK), (72, XK | hip.FLAG_NO_MFMA), (72, XK | hip.FLAG_DIRECT)):
        assert lib.glhip_kernel_conv_grad_uses_xk(GAUSSIAN, 1, 130, 70001, D, F32, flags, 0) == 0
        assert ws(1, 130, 70001, D, flags) == 0
    assert ws(1, 130, 70001, 72, XK | hip.FLAG_NO_SPLIT) == 0              # no splits, no partials
    assert ws(0, 130, 70001, 72, XK) == 0 and ws(1, 0, 70001, 72, XK) == 0 and ws(1, 130, 0, 72, XK) == 0
    assert ws(1, 10**6, 10**6, 4095, XK) <= 2**30
    assert ws(65535, 1000, 70001, 4095, XK) <= 2**30
    assert ws(65536, 1000, 70001, 72, XK) == 0                             # B beyond the grid: the predicate is 0
