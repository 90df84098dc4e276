"""Generates tests/golden/reference_workspace_bytes.npz: what glhip_workspace_bytes returns on a grid of shapes, recorded from a build of the
PARENT commit — the one BEFORE the split policy of the forward launchers moved into geomloss_amd/csrc/glhip_split_policy.h and the sizing
call was reassembled from its pieces (the hash is stored in the file).  The value decides how many column splits every launch takes and
whether it pre-packs its columns, so tests/test_workspace_bytes_cpu.py holds every later library to these values.  Host arithmetic only:
no device.  The `reference_` prefix keeps the file out of ``conftest.golden_cases()``, which takes every other .npz here for a loss case.

    python tests/golden/make_golden_workspace_bytes.py PATH/TO/libgeomloss_hip.so PARENT_HASH

The grid: the thresholds of the rules sit in N and M (one and several row blocks of 128 / 256 / 512 rows, M on both sides of 16384,
of 65536 and of the 2048 columns per split, launches on both sides of 5e8 pairs); D covers the three dimension ranges and their edges
(4096: no split kernel); block-sparse launches (n_ranges > 0) come with B = 1, as the library requires."""

import ctypes
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from geomloss_amd import hip  # noqa: E402  (the signature only)

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_workspace_bytes.npz")
B = (1, 4, 64, 256)
NM = (1, 127, 128, 1000, 4096, 16384, 16385, 32768, 65535, 65536, 100000, 300000, 1000000)
D = (1, 2, 3, 4, 5, 8, 12, 16, 17, 64, 4095, 4096)
RANGES = (0, 1, 7, 2000)


def grid():
    """(B, N, M, D, n_ranges) rows, int64"""
    rows = [(b, n, m, d, r) for r in RANGES for b in (B if r == 0 else (1,)) for n, m, d in itertools.product(NM, NM, D)]
    return np.array(rows, dtype=np.int64)


def main():
    lib = ctypes.CDLL(sys.argv[1])
    fn = lib.glhip_workspace_bytes
    fn.restype, fn.argtypes = hip.SIGNATURES["glhip_workspace_bytes"]
    args = grid()
    out = np.array([fn(*map(int, r)) for r in args], dtype=np.int64)
    np.savez_compressed(OUT, parent=np.array(sys.argv[2]), args=args, bytes=out)
    print(OUT, os.path.getsize(OUT), "bytes;", len(out), "rows,", int((out > 0).sum()), "non-zero")


if __name__ == "__main__":
    main()
