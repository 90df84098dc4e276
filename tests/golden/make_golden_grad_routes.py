"""Generates tests/golden/reference_grad_routes.npz: what the library says on the host about the routes of its gradient entry points,
recorded from a build of the commit BEFORE that routing was gathered into softmin_bwd_family / conv_family
(geomloss_amd/csrc/glhip_family.h; the hash is stored in the file).  tests/test_grad_routes_cpu.py holds every later library to these
values.  Host arithmetic only: no device.  Second to reference_conv_family.npz (make_golden_conv_family.py), whose axes it takes, with
three more flag combinations.

    python tests/golden/make_golden_grad_routes.py PATH/TO/libgeomloss_hip.so PARENT_HASH

Columns (rows: the cross product of the named axes in the order of ``itertools.product``; the axes are stored, the rows are not):
  uses_plan        glhip_softmin_bwd_x_uses_plan             p x B x NM x D x dtype x n_ranges x flags       (p = 3: no such exponent)
  dist_uses_xk     glhip_dist_grad_uses_xk                   kind x ...  (the ops are 0 soft-min p = 1, 1 laplacian, 2 energy; 7: none)
  conv_uses_xk     glhip_kernel_conv_grad_uses_xk            kind x ...
  bytes_*          the three sizing calls glhip_softmin_bwd_x_workspace_bytes, glhip_kernel_conv_grad_workspace_bytes,
                   glhip_dist_grad_workspace_bytes           B x NM x D x flags
  empty_*          the return codes of glhip_softmin_bwd_x, glhip_softmin_fwd_grad (p x ...), glhip_kernel_conv_bwd_x and
                   glhip_kernel_conv_fwd_grad (kind x ...) on B x D x dtype x n_ranges x flags with N = M = 0 and NULL pointers
  null_*           the same calls with N = M = 1, clouds that nothing reads, NULL outputs and eps = blur = 0: every return of these calls
                   comes before the first HIP call, in the order argument check, support, empty launch, NULL outputs, scalars
Block-sparse rows pass a dummy range table (check_common refuses NULL ones before anything else is reached); nothing reads it."""
import ctypes
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from geomloss_amd import hip  # noqa: E402  (signatures and flag values only)
from make_golden_conv_family import AXES as CONV_AXES  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_grad_routes.npz")
AXES = dict(CONV_AXES, p=(1, 2, 3), flags=CONV_AXES["flags"] + (hip.FLAG_XK_DIST_GRAD, hip.FLAG_XK_DIST_GRAD | hip.FLAG_NO_MFMA,
                                                                hip.FLAG_XK_GRAD | hip.FLAG_XK_DIST_GRAD))
PREDICATES = {"uses_plan": ("glhip_softmin_bwd_x_uses_plan", "p"), "dist_uses_xk": ("glhip_dist_grad_uses_xk", "kind"),
              "conv_uses_xk": ("glhip_kernel_conv_grad_uses_xk", "kind")}
SIZING = {"bytes_softmin": "glhip_softmin_bwd_x_workspace_bytes", "bytes_conv": "glhip_kernel_conv_grad_workspace_bytes",
          "bytes_dist": "glhip_dist_grad_workspace_bytes"}
ENTRIES = {"softmin_bwd_x": "p", "softmin_fwd_grad": "p", "kernel_conv_bwd_x": "kind", "kernel_conv_fwd_grad": "kind"}


def bind(lib):
    for name in [v[0] for v in PREDICATES.values()] + list(SIZING.values()) + ["glhip_" + e for e in ENTRIES]:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = hip.SIGNATURES[name]
    return lib


def rows(axes, *names):
    return itertools.product(*(axes[n] for n in names))


def entry_call(lib, entry, first, B, n, D, dt, nr, flags, cloud, table):
    """One call with N = M = n, NULL outputs, NULL workspace and eps = blur = 0 (n = 0: NULL clouds too)."""
    c = cloud if n else None
    rg = (table, table, table, nr) if nr else (None, None, None, 0)
    if entry == "softmin_bwd_x":       # x, y, h, out, grad_out, grad_x, B, N, M, D, eps, p, dtype, ranges..., workspace, bytes, flags, stream
        return lib.glhip_softmin_bwd_x(c, c, c, None, None, None, B, n, n, D, 0.0, first, dt, *rg, None, 0, flags, None)
    if entry == "softmin_fwd_grad":    # x, y, h, guess, margin, out, grad_unit, B, N, M, D, eps, p, dtype, ...
        return lib.glhip_softmin_fwd_grad(c, c, c, None, 0.0, None, None, B, n, n, D, 0.0, first, dt, *rg, None, 0, flags, None)
    if entry == "kernel_conv_bwd_x":   # kind, x, y, v, g, grad_x, B, N, M, D, blur, dtype, ...
        return lib.glhip_kernel_conv_bwd_x(first, c, c, c, None, None, B, n, n, D, 0.0, dt, *rg, None, 0, flags, None)
    return lib.glhip_kernel_conv_fwd_grad(first, c, c, c, None, None, B, n, n, D, 0.0, dt, *rg, None, 0, flags, None)


def columns(lib, axes):
    """Every recorded column from `lib` on `axes` (the generator: AXES; the test: the axes stored in the file)."""
    cols = {}
    for name, (symbol, first) in PREDICATES.items():
        fn = getattr(lib, symbol)
        cols[name] = np.array([fn(a, B, N, M, D, dt, flags, nr) for a, B, (N, M), D, dt, nr, flags
                               in rows(axes, first, "B", "NM", "D", "dtype", "n_ranges", "flags")], dtype=np.int8)
    for name, symbol in SIZING.items():
        fn = getattr(lib, symbol)
        cols[name] = np.array([fn(B, N, M, D, flags) for B, (N, M), D, flags in rows(axes, "B", "NM", "D", "flags")], dtype=np.int64)
    table_buf, cloud_buf = (ctypes.c_int32 * 16)(), (ctypes.c_float * 4096)()      # a range table and a cloud that nothing reads
    table, cloud = ctypes.cast(table_buf, ctypes.c_void_p), ctypes.cast(cloud_buf, ctypes.c_void_p)
    for entry, first in ENTRIES.items():
        for prefix, n in (("empty_", 0), ("null_", 1)):
            cols[prefix + entry] = np.array([entry_call(lib, entry, a, B, n, D, dt, nr, flags, cloud, table) for a, B, D, dt, nr, flags
                                             in rows(axes, first, "B", "D", "dtype", "n_ranges", "flags")], dtype=np.int8)
    return cols


def main():
    lib = bind(ctypes.CDLL(sys.argv[1]))
    arrays = {"parent": np.array(sys.argv[2])}
    for k, v in AXES.items():
        arrays["axis:" + k] = np.array(v, dtype=np.int64)
    arrays.update(columns(lib, AXES))
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes;", {k: (len(v), sorted(set(v.tolist()))[:8]) for k, v in arrays.items() if v.dtype in (np.int8, np.int64) and v.ndim == 1 and not k.startswith("axis:")})


if __name__ == "__main__":
    main()
