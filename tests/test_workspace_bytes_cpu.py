"""glhip_workspace_bytes against the values recorded from the library before the sizing call was reassembled from the pieces of
geomloss_amd/csrc/glhip_split_policy.h (tests/golden/reference_workspace_bytes.npz, written by make_golden_workspace_bytes.py from a build of
the parent commit).  The value decides how many column splits every forward, half-step, product and D <= 16 gradient launch takes and
whether it pre-packs its columns, so it is part of the contract: equality at every grid point, no tolerance.  No device."""
import ctypes
import os

import numpy as np
import pytest

from geomloss_amd import hip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_workspace_bytes.npz")


@pytest.fixture(scope="module")
def sizing():
    assert hip.library_available(), "libgeomloss_hip.so is not built (python -c 'import __graft_entry__ as g; g.build()')"
    fn = ctypes.CDLL(hip.LIB_PATH).glhip_workspace_bytes
    fn.restype, fn.argtypes = hip.SIGNATURES["glhip_workspace_bytes"]
    return fn


def test_workspace_bytes_match_the_recorded_values(sizing):
    golden = np.load(GOLDEN)
    args, want = golden["args"], golden["bytes"]
    # the whole grid of the generator: 4 batch sizes dense, B = 1 for three numbers of ranges, 13 x 13 x 12 shapes each
    assert len(args) == len(want) == (4 + 3) * 13 * 13 * 12 and (want > 0).any() and (want == 0).any()
    got = np.array([sizing(*map(int, r)) for r in args], dtype=np.int64)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (f"{bad.size} of {len(want)} grid points differ; first (B, N, M, D, n_ranges) = {args[bad[0]].tolist()} -> "
                           f"{got[bad[0]]}, recorded {want[bad[0]]}")
