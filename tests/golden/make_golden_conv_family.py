"""Generates tests/golden/reference_conv_family.npz: which kernel the host side of the kernel products picks, recorded from a build of
the commit BEFORE that dispatch was gathered into conv_family / conv_typed<MODE> (geomloss_amd/csrc/glhip_launch.h; the hash is stored
in the file).  tests/test_conv_family_cpu.py holds every later library to these values.  Host arithmetic only: no device.  The
`reference_` prefix keeps the file out of ``conftest.golden_cases()``, which takes every other .npz here for a loss case.

    python tests/golden/make_golden_conv_family.py PATH/TO/libgeomloss_hip.so PARENT_HASH

Three columns:
  family    glhip_kernel_conv_fwd_family          on kind x B x (N, M) x D x dtype x n_ranges x flags
  uses_xk   glhip_kernel_conv_grad_uses_xk        on the same rows
  fwd_grad  the return code of glhip_kernel_conv_fwd_grad with N = M = 0 and NULL clouds, on kind x B x D x dtype x n_ranges x flags:
            every return of that call comes before its first HIP call (check_common, the kind, the support test, then N == 0), so the
            code is the support rule of the product-and-gradient mode as a host function.  Block-sparse rows pass a dummy range table
            (check_common refuses NULL ones before the rule is reached); nothing reads it.
Rows are the cross product of the axes in the order of ``itertools.product``; the axes are stored, the rows are not."""

import ctypes
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from geomloss_amd import hip  # noqa: E402  (signatures and flag values only)

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_conv_family.npz")
AXES = {
    "kind": (hip.GAUSSIAN, hip.LAPLACIAN, hip.ENERGY, 7),      # 7: no such kind
    "B": (1, 3, 70000),
    "NM": ((1000, 1000), (65536, 7630), (65536, 7629), (200000, 200000)),      # 65536 x 7630 >= 5e8: the smallest launch that autosorts
    "D": (1, 2, 3, 4, 8, 16, 17, 64, 4095, 4096),
    "dtype": (hip.F32, hip.BF16),
    "n_ranges": (0, 5),
    "flags": (0, hip.FLAG_NO_MFMA, hip.FLAG_DIRECT, hip.FLAG_XDL16, hip.FLAG_MFMA_DIST, hip.FLAG_NO_SORT, hip.FLAG_F16X2, hip.FLAG_XK_GRAD,
              hip.FLAG_XK_GRAD | hip.FLAG_NO_MFMA, hip.FLAG_MFMA_DIST | hip.FLAG_NO_SORT),
}
PREDICATES = {"family": "glhip_kernel_conv_fwd_family", "uses_xk": "glhip_kernel_conv_grad_uses_xk"}


def bind(lib):
    for name in list(PREDICATES.values()) + ["glhip_kernel_conv_fwd_grad"]:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = hip.SIGNATURES[name]
    return lib


def predicate_rows():
    a = AXES
    return itertools.product(a["kind"], a["B"], a["NM"], a["D"], a["dtype"], a["n_ranges"], a["flags"])


def predicate_column(lib, name):
    fn = getattr(lib, PREDICATES[name])
    return np.array([fn(kind, B, N, M, D, dt, flags, nr) for kind, B, (N, M), D, dt, nr, flags in predicate_rows()], dtype=np.int8)


def fwd_grad_rows():
    a = AXES
    return itertools.product(a["kind"], a["B"], a["D"], a["dtype"], a["n_ranges"], a["flags"])


def fwd_grad_column(lib):
    """glhip_kernel_conv_fwd_grad(kind, x, y, v, out, grad_unit, B, 0, 0, D, blur, dtype, ranges..., n_ranges, ws, 0, flags, stream)"""
    table = (ctypes.c_int32 * 16)()      # block-sparse rows: a range table that nothing reads
    tp = ctypes.cast(table, ctypes.c_void_p)
    fn = lib.glhip_kernel_conv_fwd_grad
    return np.array([fn(kind, None, None, None, None, None, B, 0, 0, D, 0.5, dt, tp if nr else None, tp if nr else None, tp if nr else None,
                        nr, None, 0, flags, None) for kind, B, D, dt, nr, flags in fwd_grad_rows()], dtype=np.int8)


def main():
    lib = bind(ctypes.CDLL(sys.argv[1]))
    arrays = {"parent": np.array(sys.argv[2])}
    for k, v in AXES.items():
        arrays["axis:" + k] = np.array(v, dtype=np.int64)
    for name in PREDICATES:
        arrays[name] = predicate_column(lib, name)
    arrays["fwd_grad"] = fwd_grad_column(lib)
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes;", {k: (len(v), sorted(set(v.tolist()))) for k, v in arrays.items() if v.dtype == np.int8})


if __name__ == "__main__":
    main()
