"""The memory bounds of every column-split launch, from the plan functions themselves (geomloss_amd/csrc/glhip_split_policy.h).  The header is
plain C++; the stand-alone program tools/split_policy_cases.cpp, built by the host compiler alone, runs every plan function — in every
launcher configuration: workgroup heights, partial widths, K layouts, share mode — over the grid of shapes of
tests/golden/make_golden_workspace_bytes.py, under four workspaces per shape (what the sizing rule of the same header gives, half of it,
4096 bytes, none) and every combination of the Scratch booleans (GLHIP_FLAG_NO_SPLIT, GLHIP_FLAG_PREPACK), and checks for every plan that

  * n_splits >= 1, and n_splits * per_split <= bytes whenever n_splits > 1;
  * the XCD-aware grid implies a dense launch, M >= 65536 and a multiple of 8 splits;
  * pre-packed columns start behind the partials of the splits, on a multiple of 256 bytes, and end inside the workspace;
  * the bytes the plan says it touches lie inside the workspace;
  * no workspace gives one split and no pre-packed columns, and so does GLHIP_FLAG_NO_SPLIT for the splits.

The launchers of glhip_launch.h / glhip_mapreduce.h execute these plans and decide nothing themselves.  No device."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "geomloss_amd", "csrc")
PROGRAM = os.path.join(ROOT, "tools", "split_policy_cases.cpp")
SHAPES = (4 + 3) * 13 * 13 * 12      # the grid: 4 batch sizes dense, B = 1 for three numbers of ranges, 13 x 13 x 12 shapes each


@pytest.fixture(scope="module")
def cases_exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("split_policy") / "cases"
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", HEADER_DIR, PROGRAM, "-o", str(exe)], check=True)
    return str(exe)


def test_every_plan_stays_inside_its_workspace(cases_exe):
    out = subprocess.run([cases_exe, "check"], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    tail = out[-1].split()
    assert tail[0::2] == ["shapes", "plans", "violations"], out[-1]
    shapes, plans, violations = map(int, tail[1::2])
    assert violations == 0 and len(out) == 1, "\n".join(out[:20])
    # every shape, and per shape at least one launcher configuration x 4 workspaces x 4 flag combinations (D = 4096 has no split kernel)
    assert shapes == SHAPES and plans >= 16 * SHAPES * 11 // 12


def test_the_report_lists_capped_launches(cases_exe):
    """`report` mode (tools/split_policy_report.py): the configuration a launcher takes under default flags, sized against unlimited workspace."""
    out = subprocess.run([cases_exe, "report"], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    tail = out[-1].split()
    assert tail[0::2] == ["shapes", "plans", "capped"], out[-1]
    shapes, plans, capped = map(int, tail[1::2])
    assert shapes == SHAPES and plans >= shapes and capped == len(out) - 1
