"""Which kernel family the gradient entry points route a launch to (softmin_bwd_family and conv_family, modes 1 and 2, of
geomloss_amd/csrc/glhip_family.h) against the kernels the library launched BEFORE that routing was gathered into one predicate:
tests/golden/reference_grad_family.npz holds, per call of the grid of tools/grad_route_cases.py, the family of the kernel in the parent
build's kernel trace on an MI355X (the table from kernel names to GLHIP_FAMILY_* codes is in that tool; the parent's hash is in the file).
The header is plain C++: the stand-alone program tools/grad_family_cases.cpp, built by the host compiler alone, answers for every row.
Equality on every row.  No device."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from geomloss_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_grad_family.npz")
FAMILIES = {hip.FAMILY_VALU, hip.FAMILY_X32, hip.FAMILY_XD, hip.FAMILY_XK, hip.FAMILY_DIST, hip.FAMILY_GENERIC}


@pytest.fixture(scope="module")
def cases_exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("grad_family") / "cases"
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "geomloss_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "grad_family_cases.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_gradient_family_matches_the_kernels_the_parent_launched(cases_exe):
    golden = np.load(GOLDEN)
    assert golden["columns"].tolist() == "entry p_or_kind mode D bf16 B n_ranges flags".split()
    rows, want = golden["rows"], golden["family"]
    N, M = int(golden["N"]), int(golden["M"])
    assert len(rows) == len(want) >= 1000 and set(want.tolist()) == FAMILIES, "the recorded column proves nothing"
    lines = "".join(f"{e} {pk} {mode} {B} {N} {M} {D} {flags} {nr}\n" for e, pk, mode, D, _, B, nr, flags in rows.tolist())
    got = np.array(subprocess.run([cases_exe], input=lines, capture_output=True, text=True, check=True).stdout.split(), dtype=np.int64)
    assert len(got) == len(want)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (f"{bad.size} of {len(want)} rows differ; first (entry, p or kind, mode, D, bf16, B, n_ranges, flags) = "
                           f"{rows[bad[0]].tolist()} -> {got[bad[0]]}, the parent launched {want[bad[0]]}")
