"""Which kernel the host side of the kernel products picks (conv_family and conv_typed<MODE> of geomloss_amd/csrc/glhip_launch.h, the
GLHIP_FLAG_XK_GRAD predicate of glhip_api_convgrad_xk.hip) against the values recorded from the library before that dispatch was
gathered into one predicate (tests/golden/reference_conv_family.npz, written by make_golden_conv_family.py): glhip_kernel_conv_fwd_family,
glhip_kernel_conv_grad_uses_xk, and the return code of glhip_kernel_conv_fwd_grad on empty clouds, which is the support rule of the
product-and-gradient mode (every return of that call comes before its first HIP call).  Equality on every row.  No device."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from geomloss_amd import hip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_conv_family.npz")
PREDICATES = {"family": "glhip_kernel_conv_fwd_family", "uses_xk": "glhip_kernel_conv_grad_uses_xk"}


@pytest.fixture(scope="module")
def lib():
    assert hip.library_available(), "libgeomloss_hip.so is not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in list(PREDICATES.values()) + ["glhip_kernel_conv_fwd_grad"]:
        assert hasattr(lib, name), f"{name} is not exported"
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = hip.SIGNATURES[name]
    return lib


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _axes(golden, *names):
    return [[tuple(v) if np.ndim(v) else int(v) for v in golden["axis:" + n].tolist()] for n in names]


def _compare(name, rows, got, want):
    assert len(rows) == len(want) >= 1000 and len(set(want.tolist())) >= 2, f"{name}: the recorded column proves nothing"
    bad = np.nonzero(np.asarray(got) != want)[0]
    assert bad.size == 0, f"{name}: {bad.size} of {len(want)} rows differ; first {rows[bad[0]]} -> {got[bad[0]]}, recorded {want[bad[0]]}"


@pytest.mark.parametrize("name", sorted(PREDICATES))
def test_predicate_matches_the_recorded_values(lib, golden, name):
    rows = list(itertools.product(*_axes(golden, "kind", "B", "NM", "D", "dtype", "n_ranges", "flags")))
    fn = getattr(lib, PREDICATES[name])
    got = [fn(kind, B, N, M, D, dt, flags, nr) for kind, B, (N, M), D, dt, nr, flags in rows]
    _compare(PREDICATES[name], rows, got, golden[name])


def test_fwd_grad_support_rule_matches_the_recorded_return_codes(lib, golden):
    rows = list(itertools.product(*_axes(golden, "kind", "B", "D", "dtype", "n_ranges", "flags")))
    table = (ctypes.c_int32 * 16)()      # block-sparse rows: a range table that nothing reads (N = 0 returns before any launch)
    tp = ctypes.cast(table, ctypes.c_void_p)
    fn = lib.glhip_kernel_conv_fwd_grad
    got = [fn(kind, None, None, None, None, None, B, 0, 0, D, 0.5, dt, tp if nr else None, tp if nr else None, tp if nr else None, nr,
              None, 0, flags, None) for kind, B, D, dt, nr, flags in rows]
    _compare("glhip_kernel_conv_fwd_grad on empty clouds", rows, got, golden["fwd_grad"])
    assert {0, -2} <= set(golden["fwd_grad"].tolist())      # supported and GLHIP_EUNSUPPORTED both occur
