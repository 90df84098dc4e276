"""Host side of the resident-operand arg-reductions (version 142; geomloss_amd/csrc/glhip_api_arg_xd.hip): the family predicate
``glhip_arg_family``, the sizing ``glhip_arg_xd_workspace_bytes``, the unchanged sizing of the K-chunked family and the wrapper's
``resident=`` keyword.  No device."""
import itertools

import pytest
import torch

from geomloss_amd import hip

XD, XK, EINVAL, EUNSUPPORTED = hip.FAMILY_XD, hip.FAMILY_XK, -1, -2


@pytest.fixture(scope="module")
def lib():
    return hip.load_library()


def test_flag_and_symbols(lib):
    assert hip.FLAG_XD_ARG == 8192 and lib.glhip_version() >= 142
    assert hip._SINCE["glhip_arg_family"] == 142 and hip._SINCE["glhip_arg_xd_workspace_bytes"] == 142


@pytest.mark.parametrize("D,k,p,dtype,n_ranges,flag", itertools.product((1, 16, 17), (1, 16, 17, 128, 129), (1, 2), (hip.F32, hip.BF16), (0, 1),
                                                                       (0, hip.FLAG_XD_ARG)))
def test_family(lib, D, k, p, dtype, n_ranges, flag):
    fam = lib.glhip_arg_family(1, 1000, 2000, D, k, p, dtype, n_ranges, flag | hip.FLAG_NO_SPLIT)
    if p != 2 or n_ranges or k > 128:
        assert fam == EUNSUPPORTED
    else:
        assert fam == (XD if flag and D <= 16 else XK)


def test_family_limits_and_bad_arguments(lib):
    fam = lambda B=1, N=1000, M=2000, D=4, k=4, p=2, dt=hip.F32, nr=0: lib.glhip_arg_family(B, N, M, D, k, p, dt, nr, hip.FLAG_XD_ARG)  # noqa: E731
    assert fam() == XD and fam(B=65535) == XD and fam(N=0) == XD and fam(D=4095) == XK
    assert fam(B=65536) == EUNSUPPORTED and fam(D=4096) == EUNSUPPORTED
    for bad in (fam(k=0), fam(D=0), fam(p=3), fam(dt=7), fam(N=-1), fam(M=-1), fam(nr=-1)):
        assert bad == EINVAL


def test_workspace_bytes(lib):
    ws = lib.glhip_arg_xd_workspace_bytes
    for D, k in itertools.product((1, 3, 4, 8, 16), (1, 4, 5, 16, 17, 128)):
        assert ws(1, 1000, 1000, D, k) > 0 and ws(3, 257, 1, D, k) > 0
        assert ws(1, 0, 1000, D, k) == 0 and ws(1, 1000, 0, D, k) == 0
        sizes = [ws(1, 3000, M, D, k) for M in (1, 31, 32, 33, 511, 1024, 5000, 65535, 65536, 200000)]
        assert sizes == sorted(sizes)
    for D, M in itertools.product((3, 16), (200, 5000, 100000)):
        sizes = [ws(1, 3000, M, D, k) for k in range(1, 129)]
        assert sizes == sorted(sizes)
    assert ws(1, 1000, 1000, 17, 4) == 0 and ws(1, 1000, 1000, 4, 129) == 0 and ws(1, 1000, 1000, 4, 0) == 0
    # the sizing of the K-chunked family is what it was before the new one existed
    assert lib.glhip_argmin_workspace_bytes(1, 1000, 1000, 4) == 0
    assert lib.glhip_argkmin_workspace_bytes(1, 1000, 1000, 4, 16) == 0
    assert lib.glhip_argmin_workspace_bytes(1, 40, 5000, 24) == 2880 and lib.glhip_argkmin_workspace_bytes(1, 40, 5000, 24, 16) == 46080


def test_resident_beyond_16_raises_before_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(hip, "load_library", no_library)
    x, y = torch.rand(10, 17), torch.rand(12, 17)
    with pytest.raises(NotImplementedError):
        hip.argmin(x, y, resident=True)
    with pytest.raises(NotImplementedError):
        hip.argkmin(x, y, 4, resident=True)
    assert hip.resident_kw(None) == {} and hip.resident_kw(True) == {"resident": True}
