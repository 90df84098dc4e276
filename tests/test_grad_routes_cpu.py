"""What the library says on the host about the routes of its gradient entry points, against the values recorded from the library before
that routing was gathered into softmin_bwd_family / conv_family (geomloss_amd/csrc/glhip_family.h):
tests/golden/reference_grad_routes.npz, written by tests/golden/make_golden_grad_routes.py, whose column functions this test runs on the
axes stored in the file.  The three exported gradient predicates, the three gradient sizing calls, and the return codes of
glhip_softmin_bwd_x, glhip_softmin_fwd_grad, glhip_kernel_conv_bwd_x and glhip_kernel_conv_fwd_grad on empty clouds (the support rules as
host functions) and on one-point clouds with NULL outputs and a zero eps / blur (the order of the validation returns, all of which come
before the first HIP call).  Equality on every row.  No device."""
import ctypes
import os
import sys

import numpy as np
import pytest

from geomloss_amd import hip

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN_DIR)
import make_golden_grad_routes as recorded  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "reference_grad_routes.npz"))


@pytest.fixture(scope="module")
def columns(golden):
    assert hip.library_available(), "libgeomloss_hip.so is not built (python -c 'import __graft_entry__ as g; g.build()')"
    axes = {k[5:]: [tuple(v) if np.ndim(v) else int(v) for v in golden[k].tolist()] for k in golden.files if k.startswith("axis:")}
    return recorded.columns(recorded.bind(ctypes.CDLL(hip.LIB_PATH)), axes)


NAMES = list(recorded.PREDICATES) + list(recorded.SIZING) + [p + e for e in recorded.ENTRIES for p in ("empty_", "null_")]


@pytest.mark.parametrize("name", NAMES)
def test_column_matches_the_recorded_values(golden, columns, name):
    got, want = columns[name], golden[name]
    assert len(got) == len(want) >= 1000 and len(set(want.tolist())) >= 2, f"{name}: the recorded column proves nothing"
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{name}: {bad.size} of {len(want)} rows differ; first at row {bad[0]}: {got[bad[0]]}, recorded {want[bad[0]]}"


def test_supported_and_unsupported_launches_both_occur(golden):
    for entry in recorded.ENTRIES:
        assert {0, -2} <= set(golden["empty_" + entry].tolist()), entry
