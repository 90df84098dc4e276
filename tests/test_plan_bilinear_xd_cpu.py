"""Host side of the resident-operand bilinear plan kernel (version 144; geomloss_amd/csrc/glhip_api_plan_bilinear_xd.hip): the family
predicate ``glhip_plan_bilinear_family``, the sizing ``glhip_plan_bilinear_xd_workspace_bytes`` and the knob behind ``resident=None``.
No device."""
import itertools
import os
import subprocess
import sys

import pytest

from geomloss_amd import hip

XD, XK = hip.FAMILY_XD, hip.FAMILY_XK


@pytest.mark.parametrize("D,K,p,n_ranges,flag", itertools.product((1, 16, 17), (0, 1, 32, 33), (1, 2), (0, 1), (0, hip.FLAG_XD_BILINEAR)))
def test_family(D, K, p, n_ranges, flag):
    lib = hip.load_library()
    assert hip.FLAG_XD_BILINEAR == 16384 and lib.glhip_version() >= 144
    fam = lib.glhip_plan_bilinear_family(1, 1000, 2000, D, K, p, hip.F32, n_ranges, flag | hip.FLAG_NO_SPLIT | hip.FLAG_F16X2)
    if p != 2 or n_ranges:
        assert fam == 0
    else:
        assert fam == (XD if flag and D <= 16 and 1 <= K <= 32 else XK)
    assert (fam > 0) == bool(lib.glhip_plan_bilinear_supported(1, 1000, 2000, D, K, p, hip.F32, n_ranges))


def test_workspace_bytes():
    lib = hip.load_library()
    ws = lib.glhip_plan_bilinear_xd_workspace_bytes
    for D, K in itertools.product((1, 3, 8, 16), (1, 5, 6, 17, 32)):
        assert ws(1, 1000, 1000, D, K) > 0 and ws(3, 257, 1, D, K) > 0
        assert ws(1, 0, 1000, D, K) == 0 and ws(1, 1000, 0, D, K) == 0
        sizes = [ws(1, 3000, M, D, K) for M in (1, 31, 32, 33, 511, 1024, 5000, 65535, 65536, 200000)]
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    for D, M in itertools.product((3, 16), (200, 100000)):
        sizes = [ws(1, 3000, M, D, K) for K in range(1, 33)]
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    assert ws(1, 1000, 1000, 17, 4) == 0 and ws(1, 1000, 1000, 4, 33) == 0 and ws(1, 1000, 1000, 4, 0) == 0
    assert lib.glhip_plan_bilinear_workspace_bytes(1, 130, 70001, 24, 16) > 0      # the sizing of the other family is still there


@pytest.mark.parametrize("knob", ("0", "1"))
def test_knob_is_what_resident_none_means(knob):
    """GEOMLOSS_HIP_XD_BILINEAR is read once per process: a fresh child reports the flag ``resident=None`` resolves to."""
    code = ("from geomloss_amd import hip; f = lambda D, K, r=None: hip._resident('t', r, D, hip.FLAG_XD_BILINEAR, hip._XD_BILINEAR_DEFAULT, K, 32); "
            "print(f(3, 4), f(16, 32), f(17, 4), f(3, 33), f(3, 4, False), f(3, 4, True))")
    env = dict(os.environ, GEOMLOSS_HIP_XD_BILINEAR=knob, PYTHONPATH=os.pathsep.join(sys.path))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout.split()
    on = str(hip.FLAG_XD_BILINEAR) if knob == "1" else "0"
    assert out == [on, on, "0", "0", "0", str(hip.FLAG_XD_BILINEAR)]
    assert hip._resident("argmin", True, 16) == hip.FLAG_XD_ARG                     # the arg-reductions read it as before
