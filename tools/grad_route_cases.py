"""Which kernel every gradient entry point launches, and what it computes, on a fixed grid of small calls: the A/B workload of a refactor
of the host-side routing (profiles/grad_family.txt).  GPU box; ``GEOMLOSS_HIP_LIB`` selects the build, as everywhere.

    python tools/grad_route_cases.py --out A.npz                      # every call once; saves every output array
    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/grad_route_cases.py       # the same calls, nothing saved
    python tools/grad_route_cases.py --kernels DIR --json A.json      # the ordered kernel names of every call, from that trace
    python tools/grad_route_cases.py --compare A.npz B.npz            # bit for bit
    python tools/grad_route_cases.py --compare-kernels A.json B.json
    python tools/grad_route_cases.py --golden PARENT.json HASH        # tests/golden/reference_grad_family.npz, from the PARENT's trace

The grid: softmin_bwd_x (p = 1, 2), softmin_fwd_grad, kernel_conv_bwd_x and kernel_conv_fwd_grad of the three kinds, softmin_fwd (p = 1, 2)
and sinkhorn_step with pot / prev present and absent; D in DIMS; float32 and bfloat16 clouds; one problem, a batch of two, and a
block-sparse launch of 3 row blocks; FLAGS; with the sized workspace and (gradients) with none; N = 300, M = 500: more than one 256-row
block, a ragged last tile of 128 and of 32 columns.  Coordinates lie in [0, 1] and eps = 0.05, so GLHIP_FLAG_F16X2 is within its contract.
Calls the library refuses by contract (the product-and-gradient entry points outside their dimensions, a fused half-step without a
fused kernel) are left out by the rules of `supported` below; every call made must return 0.

Every input is made on the host and copied, and between two calls the tool launches one torch kernel: in a kernel trace the library's
kernels between two foreign ones are those of one call.  A watchdog ends the process if a call takes longer than CALL_LIMIT seconds; the first
non-zero return or HIP error ends the run."""
import argparse
import csv
import faulthandler
import glob
import json
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from geomloss_amd import hip  # noqa: E402

N, M, EPS, BLUR, CALL_LIMIT = 300, 500, 0.05, 0.3, 20
DIMS = (1, 3, 4, 8, 9, 16, 17, 33, 70)
FLAGS = (0, hip.FLAG_NO_MFMA, hip.FLAG_DIRECT, hip.FLAG_NO_SPLIT, hip.FLAG_XDL16, hip.FLAG_F16X2, hip.FLAG_XK_GRAD, hip.FLAG_XK_DIST_GRAD,
         hip.FLAG_XK_GRAD | hip.FLAG_NO_MFMA)
LAYOUTS = ((1, 0), (2, 0), (1, 3))      # (B, n_ranges)
# (entry point, p or kind, mode of softmin_bwd_family / conv_family or -1 for the forward calls)
SOFTMIN_BWD, SOFTMIN_FWD_GRAD, CONV_BWD, CONV_FWD_GRAD, SOFTMIN_FWD, STEP = range(6)
ENTRIES = ([(SOFTMIN_BWD, 1, 1), (SOFTMIN_BWD, 2, 1), (SOFTMIN_FWD_GRAD, 2, 2)] + [(CONV_BWD, k, 1) for k in range(3)] +
           [(CONV_FWD_GRAD, k, 2) for k in range(3)] + [(SOFTMIN_FWD, 1, -1), (SOFTMIN_FWD, 2, -1)] +
           [(STEP + v, p, -1) for p in (1, 2) for v in range(4)])      # STEP + v: bit 0 pot present, bit 1 prev present
OFF_MFMA = hip.FLAG_NO_MFMA | hip.FLAG_DIRECT
FAMILY_OF_KERNEL = {"mapreduce": hip.FAMILY_VALU, "wsum_mfma": hip.FAMILY_X32, "wsum_x32": hip.FAMILY_X32, "wsum_t32": hip.FAMILY_XD,
                    "wsum_t32q": hip.FAMILY_XD, "xk_plan": hip.FAMILY_XK, "dist_xd_grad": hip.FAMILY_DIST, "xk_dist_grad": hip.FAMILY_DIST,
                    "dist_grad_x32": hip.FAMILY_DIST, "generic": hip.FAMILY_GENERIC}
HELPERS = ("merge", "plan_merge", "build_row_chunks", "wsum_pack")      # kernels next to the one that names the family
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "reference_grad_family.npz")


def supported(entry, pk, D, B, n_ranges, flags):
    """The contract of include/glhip.h for the entry points that refuse launches."""
    dense_xk = 17 <= D and n_ranges == 0 and not flags & OFF_MFMA
    if entry == SOFTMIN_FWD_GRAD:
        return D <= 16 and not flags & OFF_MFMA
    if entry == CONV_FWD_GRAD:
        if D <= 3:
            return True
        if pk == hip.GAUSSIAN:
            return (D <= 16 and not flags & hip.FLAG_NO_MFMA) or (dense_xk and bool(flags & hip.FLAG_XK_GRAD))
        return dense_xk and bool(flags & hip.FLAG_XK_DIST_GRAD)
    if entry > STEP and D > 3:      # a fused half-step of D > 3: the matrix-core kernels only
        if pk == 2:
            return not flags & OFF_MFMA
        return D <= 16 and n_ranges == 0 and not flags & OFF_MFMA
    return True


def grid():
    """Every call, in order: (entry, p or kind, mode, D, bf16, B, n_ranges, flags, workspace)."""
    for entry, pk, mode in ENTRIES:
        for D in DIMS:
            for bf16 in (0, 1):
                for B, n_ranges in LAYOUTS:
                    for flags in FLAGS:
                        for ws in ((1, 0) if entry in (SOFTMIN_BWD, CONV_BWD, CONV_FWD_GRAD) else (1,)):      # the others always size one
                            if supported(entry, pk, D, B, n_ranges, flags):
                                yield entry, pk, mode, D, bf16, B, n_ranges, flags, ws


def run(out_path):
    import torch

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)

    def up(a, bf16=False):
        t = torch.from_numpy(np.ascontiguousarray(a))
        return (t.to(torch.bfloat16) if bf16 else t).to(dev)

    clouds = {}
    for D in DIMS:
        x, y = rng.random((2, N, D), dtype=np.float32), rng.random((2, M, D), dtype=np.float32)
        clouds[D] = [(up(x, b), up(y, b)) for b in (False, True)]
    h, pot, prev, g = (up(a) for a in (rng.standard_normal((2, M), dtype=np.float32), 0.1 * rng.standard_normal((2, M), dtype=np.float32),
                                        rng.standard_normal((2, N), dtype=np.float32), rng.standard_normal((2, N), dtype=np.float32)))
    v = up(rng.random((2, M), dtype=np.float32) / M)
    i32 = lambda rows: up(np.array(rows, dtype=np.int32))      # noqa: E731
    blocks = hip.BlockRanges(i32([[0, 100], [100, 200], [200, 300]]), i32([1, 2, 3]), i32([[0, 200], [150, 400], [300, 500]]),
                             i32([[0, 500]]), i32([1]), i32([[0, 300]]))      # (the transposed orientation is not used)
    # the soft-min values softmin_bwd_x reads and softmin_fwd_grad takes for its guess (margin / eps = 10): of the dense launches and of
    # the block-sparse one
    value = {(D, b, p): (hip.softmin_fwd_raw(*clouds[D][b], h, EPS, p=p),
                         hip.softmin_fwd_raw(clouds[D][b][0][:1], clouds[D][b][1][:1], h[:1], EPS, p=p, ranges=blocks))
             for D in DIMS for b in (0, 1) for p in (1, 2)}
    marker = up(np.zeros(1, dtype=np.float32))      # (a copy: no kernel)
    marker.add_(1.0)                         # the first separator of the kernel trace: what ran before it is the setup
    saved, calls = {}, 0
    for i, (entry, pk, mode, D, bf16, B, n_ranges, flags, ws) in enumerate(grid()):
        x, y = (t[:B] for t in clouds[D][bf16])
        a = dict(ranges=blocks if n_ranges else None, flags=flags)
        hh, vv, gg = h[:B], v[:B], g[:B]
        faulthandler.dump_traceback_later(CALL_LIMIT, exit=True)
        if entry == SOFTMIN_BWD:
            outs = [hip.softmin_bwd_x_raw(x, y, hh, value[D, bf16, pk][1 if n_ranges else 0][:B], gg, EPS, p=pk, workspace=bool(ws), **a)]
        elif entry == SOFTMIN_FWD_GRAD:
            outs = hip.softmin_fwd_grad_raw(x, y, hh, value[D, bf16, 2][1 if n_ranges else 0][:B], 0.5, EPS, **a)
        elif entry == CONV_BWD:
            outs = [hip.kernel_conv_bwd_x_raw(pk, x, y, vv, gg, BLUR, workspace=bool(ws), **a)]
        elif entry == CONV_FWD_GRAD:
            outs = hip.kernel_conv_fwd_grad_raw(pk, x, y, vv, BLUR, workspace=bool(ws), **a)
        elif entry == SOFTMIN_FWD:
            outs = [hip.softmin_fwd_raw(x, y, hh, EPS, p=pk, **a)]
        else:
            var = entry - STEP
            outs = [hip.sinkhorn_step_raw(x, y, hh, pot[:B] if var & 1 else None, prev[:B] if var & 2 else None, EPS, 0.8 if var else 1.0, p=pk, **a)]
        torch.cuda.synchronize()      # a HIP error of this call surfaces here
        faulthandler.cancel_dump_traceback_later()
        if out_path:
            for k, t in enumerate(outs):
                saved[f"{i}:{k}"] = t.cpu().numpy()
        marker.add_(1.0)              # the separator of the kernel trace
        calls += 1
    torch.cuda.synchronize()
    if out_path:
        np.savez(out_path, **saved)
    print(f"{calls} calls, {len(saved)} arrays saved, library version {hip.load_library().glhip_version()}", flush=True)


def short_name(name):
    """[void glhip::]NAME_kernel<...> (demangled) or _ZN5glhip<len>NAME_kernel... (mangled) -> NAME; None for torch's kernels, "" for the
    HIP runtime's own copy kernels."""
    if "at::" in name or "at6native" in name:
        return None
    if name.startswith("__amd_rocclr_"):
        return ""
    m2 = re.match(r"_ZN5glhip(\d+)", name)
    base = name[m2.end():m2.end() + int(m2.group(1))] if m2 else name.split("<")[0].split("(")[0]
    m = re.search(r"(\w+)_kernel$", base)
    assert m, f"neither torch's nor the library's kernel: {name}"
    return m.group(1)


def kernels_of_trace(trace_dir):
    """[[kernel names of call 0], ...] from the kernel-trace csv under `trace_dir`."""
    (path,) = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    groups, cur = [], []
    for r in rows:
        name = short_name(r["Kernel_Name"])
        if name is None:      # torch's: a separator
            groups.append(cur)
            cur = []
        elif name:
            cur.append(name)
    assert not cur, "library kernels after the last separator"
    assert all(groups[1:]), "a call without a library kernel, or two foreign kernels in a row"
    return groups[1:]         # (the first group is the setup: the soft-min values)


def family_of(names):
    fams = {FAMILY_OF_KERNEL[n] for n in names if n not in HELPERS}      # KeyError: a kernel the table does not know
    assert len(fams) == 1, names
    return fams.pop()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--kernels")
    ap.add_argument("--json")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--compare-kernels", nargs=2)
    ap.add_argument("--golden", nargs=2)
    a = ap.parse_args()
    if a.kernels:
        calls = kernels_of_trace(a.kernels)
        n = sum(1 for _ in grid())
        assert len(calls) == n, f"{len(calls)} separated groups of kernels for {n} calls"
        json.dump(calls, open(a.json, "w"))
        print(f"{n} calls, {sum(map(len, calls))} library kernels, {len({k for c in calls for k in c})} distinct names")
    elif a.compare:
        A, Bz = np.load(a.compare[0]), np.load(a.compare[1])
        assert sorted(A.files) == sorted(Bz.files), "the two runs saved different arrays"
        bad = [k for k in A.files if A[k].shape != Bz[k].shape or A[k].tobytes() != Bz[k].tobytes()]
        nonfinite = sum(1 for k in A.files if not np.isfinite(A[k]).all())
        print(f"{len(A.files)} arrays compared bit for bit ({nonfinite} with non-finite entries), {len(bad)} differ", bad[:10])
        sys.exit(1 if bad else 0)
    elif a.compare_kernels:
        A, Bz = (json.load(open(p)) for p in a.compare_kernels)
        bad = [i for i in range(max(len(A), len(Bz))) if i >= len(A) or i >= len(Bz) or A[i] != Bz[i]]
        print(f"{len(A)} / {len(Bz)} calls, {sum(map(len, A))} / {sum(map(len, Bz))} kernels, {len(bad)} calls differ", bad[:10])
        sys.exit(1 if bad else 0)
    elif a.golden:
        calls = json.load(open(a.golden[0]))
        rows, fam = [], []
        for case, names in zip(grid(), calls):
            if case[2] > 0:      # the gradient entry points
                rows.append(case[:8])
                fam.append(family_of(names))
        assert len(calls) == sum(1 for _ in grid())
        np.savez_compressed(GOLDEN, parent=np.array(a.golden[1]), columns=np.array("entry p_or_kind mode D bf16 B n_ranges flags".split()),
                            N=N, M=M, rows=np.array(rows, dtype=np.int32), family=np.array(fam, dtype=np.int8))
        print(GOLDEN, os.path.getsize(GOLDEN), "bytes;", len(rows), "rows; families", {f: fam.count(f) for f in sorted(set(fam))})
    else:
        run(a.out)


if __name__ == "__main__":
    main()
