"""Host side of the resident-operand p = 1 plan kernel (version 145; geomloss_amd/csrc/glhip_api_plan_p1_xd.hip): the family predicate
``glhip_plan_apply_p1_family``, the sizing ``glhip_plan_apply_p1_xd_workspace_bytes``, the pass width and ``resident=True`` beyond D = 16.
No GPU."""
import itertools

import pytest
import torch

from geomloss_amd import hip

XD = hip.FLAG_XD_PLAN_P1


@pytest.mark.parametrize("D,V,flags", itertools.product((1, 3, 16, 17, 4095, 4096), (0, 1, 33, 300), (0, XD, XD | hip.FLAG_NO_SPLIT | hip.FLAG_F16X2)))
def test_family_predicate(D, V, flags):
    lib = hip.load_library()
    assert XD == 32768 and lib.glhip_version() >= 145
    fam = lambda **k: lib.glhip_plan_apply_p1_family(*[{**dict(B=1, N=1000, M=2000, D=D, V=V, dt=hip.F32, nr=0, fl=flags), **k}[n]  # noqa: E731
                                                       for n in ("B", "N", "M", "D", "V", "dt", "nr", "fl")])
    supported = lib.glhip_plan_apply_p1_supported(1, 1000, 2000, D, V, hip.F32, 0)
    want = 0 if supported == 0 else (hip.FAMILY_XD if (flags & XD) and D <= 16 else hip.FAMILY_XK)
    assert fam() == fam(dt=hip.BF16) == fam(B=65535) == want
    assert fam(nr=1) == fam(B=65536) == 0                      # block-sparse ranges, a batch beyond the grid: no kernel under either flag
    assert fam(fl=flags & ~XD) in (0, hip.FAMILY_XK)           # XD only under the flag
    for bad in (dict(D=0), dict(V=-1), dict(N=-1), dict(dt=7), dict(nr=-1)):
        assert fam(**bad) < 0 and fam(**bad) == lib.glhip_plan_apply_p1_supported(*[{**dict(B=1, N=1000, M=2000, D=D, V=V, dt=hip.F32, nr=0), **bad}[n]
                                                                                     for n in ("B", "N", "M", "D", "V", "dt", "nr")])


@pytest.mark.parametrize("D", [0, 1, 2, 3, 8, 15, 16, 17])
def test_pass_width_and_workspace(D):
    lib = hip.load_library()
    width, ws = lib.glhip_plan_apply_p1_xd_pass_width(D), lib.glhip_plan_apply_p1_xd_workspace_bytes
    if not 1 <= D <= 16:
        assert width == 0 and ws(1, 1000, 2000, D, 8) == 0
        return
    assert width > 0 and width % 32 == 0
    assert ws(0, 1000, 2000, D, 8) == ws(1, 0, 2000, D, 8) == ws(1, 1000, 0, D, 8) == ws(1, 1000, 2000, D, -1) == 0
    sizes = [ws(1, N, M, D, V) for N, M, V in itertools.product((1, 33, 1000, 70000), (1, 33, 2000, 70001), (0, 1, 32, 33, width, width + 1, 4 * width))]
    assert all(s > 0 and s % 16 == 0 for s in sizes)
    for V in (1, 33, width):
        assert ws(1, 1000, 2000, D, V) <= ws(1, 1001, 2000, D, V) <= ws(1, 70000, 2000, D, V)
        assert ws(1, 1000, 2000, D, V) <= ws(1, 1000, 2001, D, V) <= ws(1, 1000, 70001, D, V)
    by_v = [ws(2, 1000, 70001, D, V) for V in range(0, width + 2)]
    assert by_v == sorted(by_v) and by_v[width] == by_v[width + 1] == ws(2, 1000, 70001, D, 10 * width)      # min(V, pass width)


def test_resident_beyond_the_domain():
    x, y, h, feat = torch.rand(40, 17), torch.rand(50, 17), torch.zeros(50), torch.ones(50, 2)
    with pytest.raises(NotImplementedError, match="resident=True"):
        hip.plan_apply_p1(0.8, x, y, h, feat, resident=True)      # CPU tensors: raised before any device is touched
    assert hip._resident("plan_apply_p1", False, 3, XD, True) == 0 and hip._resident("plan_apply_p1", None, 17, XD, True) == 0
