"""Where the workspace glhip_workspace_bytes promises caps a launch: writes profiles/split_policy_caps.txt.

Compiles tools/split_policy_cases.cpp (a stand-alone host program around geomloss_amd/csrc/glhip_split_policy.h: no HIP, no device) and runs
it in `report` mode: for every shape of the sizing grid and the configuration each launcher takes there under default flags, the plan under
the sized workspace next to the plan under an unlimited one, wherever the two differ in splits, XCD-aware grid or pre-packed columns.

    python tools/split_policy_report.py [OUT]

The list is the to-do of a later performance change.  NO TIMING STANDS BEHIND IT: whether a capped launch is slower than the uncapped one
has not been measured on an MI355X."""
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = """\
# Launches that the workspace of glhip_workspace_bytes caps: the plan of glhip_split_policy.h under the sized workspace next to the plan
# under an unlimited one, wherever they differ.  Written by tools/split_policy_report.py (host arithmetic only, no device).
# NO TIMING STANDS BEHIND THIS LIST: whether a capped launch is slower has not been measured on an MI355X.  It is the to-do list of a
# later performance change; glhip_workspace_bytes is pinned until then (tests/test_workspace_bytes_cpu.py).
# Grid: B in {1, 4, 64, 256}; N, M in {1, 127, 128, 1000, 4096, 16384, 16385, 32768, 65535, 65536, 100000, 300000, 1000000};
# D in {1, 2, 3, 4, 5, 8, 12, 16, 17, 64, 4095, 4096}; n_ranges in {0, 1, 7, 2000} (B = 1 when > 0); default flags, bf16 x 3 layout; per
# shape the workgroup shape its launcher picks.  `bytes`: the sized workspace.  Last line: shapes, plans compared, plans capped.
"""


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "split_policy_caps.txt")
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "cases")
        subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "geomloss_amd", "csrc"),
                        os.path.join(ROOT, "tools", "split_policy_cases.cpp"), "-o", exe], check=True)
        text = subprocess.run([exe, "report"], capture_output=True, text=True, check=True).stdout
    with open(out, "w") as f:
        f.write(HEADER + text)
    print(out, text.strip().split("\n")[-1])


if __name__ == "__main__":
    main()
