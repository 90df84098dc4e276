"""Generates tests/golden/reference_plan_family_sizing.npz: what the five workspace sizing calls of the plan family return, recorded from a build
of the commit BEFORE their launchers and sizing rules were merged into geomloss_amd/csrc/glhip_launch_plan.h (the hash is stored in the
file).  tests/test_plan_family_sizing_cpu.py holds every later library to these values.  Host arithmetic only: no device.  The `reference_` prefix
keeps the file out of ``conftest.golden_cases()``, which takes every other .npz here for a loss case.

    python tests/golden/make_golden_plan_family_sizing.py PATH/TO/libgeomloss_hip.so PARENT_HASH

The grid crosses every branch of the rule: one and several row blocks, batches, M on both sides of 65536 and of the 2048 columns per
split, partials that do and do not fit 8 or 32 times into 1 GiB, every pass width, both plan families, the flags that switch the
gradient route off.  The cross product is thinned (every row whose running index is a multiple of THIN, a stride coprime to every
axis length) where it would not fit a few tens of kilobytes."""

import ctypes
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from geomloss_amd import hip  # noqa: E402  (signatures and flag values only)

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_plan_family_sizing.npz")
B = (1, 3, 300)
N = (1, 130, 257, 5000, 10**5, 10**6)
M = (1, 511, 1023, 1024, 5000, 20000, 65535, 65536, 70001, 200000, 10**6)
D = (3, 8, 16, 17, 24, 64, 100, 4095)
V = (1, 16, 33, 64, 70, 128, 200)
FLAGS = (0, hip.FLAG_XK_GRAD, hip.FLAG_XK_GRAD | hip.FLAG_NO_SPLIT, hip.FLAG_XK_GRAD | hip.FLAG_NO_MFMA)
CALLS = {
    # name: (axes after B, N, M; stride of the thinning)
    "glhip_plan_apply_workspace_bytes": ((D, V), 5),
    "glhip_plan_apply_nd_workspace_bytes": ((D, V), 5),
    "glhip_softmin_bwd_x_workspace_bytes": ((D, FLAGS), 1),
    "glhip_kernel_conv_grad_workspace_bytes": ((D, FLAGS), 1),
    "glhip_argmin_workspace_bytes": ((D,), 1),
}


def main():
    lib = ctypes.CDLL(sys.argv[1])
    arrays = {"parent": np.array(sys.argv[2])}
    for name, (axes, thin) in CALLS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = hip.SIGNATURES[name]
        rows = [r for i, r in enumerate(itertools.product(B, N, M, *axes)) if i % thin == 0]
        args = np.array(rows, dtype=np.int64)
        arrays[name + ":args"] = args
        arrays[name + ":bytes"] = np.array([fn(*map(int, r)) for r in rows], dtype=np.int64)
        for k, axis in enumerate((B, N, M) + axes):      # the thinning keeps every value of every axis
            assert set(args[:, k]) == set(axis), (name, k)
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes;", {k: len(v) for k, v in arrays.items() if k.endswith(":bytes")})


if __name__ == "__main__":
    main()
