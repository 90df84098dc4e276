"""GPU box: the top-k arg-reduction ``hip.argkmin`` (glhip_argkmin), timed against ``hip.argmin`` and against the route a user has
without it, chunked ``torch.cdist`` + ``topk``.

    python tools/bench_argkmin.py [--n 200000] [--dims 32 64 128] [--ks 1 4 16] [--rounds 7] [--warmup 2] [--torch-rounds 3]
                                  [--mem-gib 8] [--low-n 1000000] [--low-d 3] [--low-k 8]

Part 1 — float32 clouds uniform in the unit cube, N = M = --n, g = None, index and value returned by every launch.  ``hip.argmin``
(the kernel whose staging and MFMA chain the top-k kernel runs) and ``hip.argkmin`` for every k of --ks, alternated in one process on
one GPU, each call between two HIP events: medians, minima, the spread (max - min) / median, and per k the ratio of the medians to
argmin.  The torch route runs in the first --torch-rounds rounds of the same alternation: ``torch.cdist(x[r0:r1], y)`` +
``topk(k, largest=False)`` with k = the largest of --ks, in the largest row chunks whose distance matrix fits --mem-gib (cdist's own
temporaries and the outputs come on top).  Before timing, the first 256 rows of the largest k are checked against a float64 torch
evaluation of the same costs.

Part 2 — one low-dimension line, N = M = --low-n, D = --low-d, k = --low-k: argmin, argkmin, and the torch route timed on ONE chunk of
rows and scaled to all of them (the line says so).

No ratio is asserted: the figures are printed."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from geomloss_amd import hip  # noqa: E402


def one_call(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def line(D, name, ms, pairs, scale=1.0):
    ms = [m * scale for m in ms]
    med, lo = statistics.median(ms), min(ms)
    print(f"  {D:4d} {name:40s} {med:10.3f} {lo:10.3f} {(max(ms) - lo) / med:7.1%} {pairs / (med * 1e-3):10.3e}", flush=True)
    return med, (max(ms) - lo)


def chunk_rows(M, mem_gib):
    return max(1, int(mem_gib * 2**30) // (4 * M))


def torch_topk(x, y, k, chunk, rows=None):
    """cdist + topk in row chunks of `chunk` rows (chunk x M floats at a time) over the first `rows` rows (default: all)."""
    n = x.shape[0] if rows is None else rows
    idx = torch.empty((n, k), dtype=torch.int64, device=x.device)
    val = torch.empty((n, k), dtype=torch.float32, device=x.device)
    for r0 in range(0, n, chunk):
        r1 = min(n, r0 + chunk)
        v, i = torch.cdist(x[r0:r1], y).topk(k, dim=1, largest=False)
        idx[r0:r1], val[r0:r1] = i, v
    return idx, val


def check(x, y, k, rows=256):
    idx = hip.argkmin(x, y, k)[:rows].long()
    C = (torch.cdist(x[:rows].double(), y.double()) ** 2) / 2
    stat = C.topk(k, dim=1, largest=False)[0]
    excess = float((C.gather(1, idx) - stat).abs().max())
    wrong = int((idx != C.topk(k, dim=1, largest=False)[1]).any(1).sum())
    return wrong, excess


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--dims", type=int, nargs="*", default=[32, 64, 128])
    ap.add_argument("--ks", type=int, nargs="*", default=[1, 4, 16])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-rounds", type=int, default=3)
    ap.add_argument("--mem-gib", type=float, default=8.0)
    ap.add_argument("--low-n", type=int, default=1000000)
    ap.add_argument("--low-d", type=int, default=3)
    ap.add_argument("--low-k", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_argkmin: no GPU — nothing is timed without one")
    dev = torch.device("cuda:0")
    lib = hip.load_library()
    n, kt = args.n, max(args.ks)
    chunk = chunk_rows(n, args.mem_gib)
    print(f"# libgeomloss_hip {lib.glhip_version()}; {torch.cuda.get_device_name(0)}; one process, launches alternated")
    print(f"# part 1: float32 clouds, N = M = {n}, g = None, index + value; median (min, spread) of {args.rounds} calls after {args.warmup}, HIP events")
    print(f"#   torch route: cdist + topk({kt}, largest=False) in chunks of {chunk} rows ({args.mem_gib:g} GiB of distances at a time), "
          f"{args.torch_rounds} calls in the same alternation after 1")
    print(f"# {'D':>4s} {'launch':40s} {'ms':>10s} {'min':>10s} {'spread':>7s} {'pairs/s':>10s}")
    for D in args.dims:
        g = torch.Generator().manual_seed(n + D)
        x, y = torch.rand(n, D, generator=g).to(dev), torch.rand(n, D, generator=g).to(dev)
        launches = [("glhip_argmin", lambda: hip.argmin(x, y, None, return_value=True))]
        for k in args.ks:
            launches.append((f"glhip_argkmin k = {k}", lambda k=k: hip.argkmin(x, y, k, return_value=True)))
        tname = f"torch cdist + topk({kt}), chunked"
        wrong, excess = check(x, y, kt)
        for _ in range(args.warmup):
            for _, fn in launches:
                fn()
        if args.torch_rounds:
            torch_topk(x, y, kt, chunk)
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in launches}
        ms[tname] = []
        for r in range(args.rounds):
            for name, fn in launches:
                ms[name].append(one_call(fn))
            if r < args.torch_rounds:
                ms[tname].append(one_call(lambda: torch_topk(x, y, kt, chunk)))
        res = {name: line(D, name, ms[name], float(n) * n) for name, _ in launches}
        base = res["glhip_argmin"][0]
        ratios = ", ".join(f"k = {k}: {res[f'glhip_argkmin k = {k}'][0] / base:.3f}" for k in args.ks)
        print(f"  {D:4d} argkmin / argmin: {ratios}; first 256 rows of k = {kt} against float64: {wrong} rows differ, largest cost excess {excess:.2e}",
              flush=True)
        if ms[tname]:
            tm, ts = line(D, tname, ms[tname], float(n) * n)
            km, ks_ = res[f"glhip_argkmin k = {kt}"]
            verdict = "argkmin is faster by more than both spreads" if tm - km > ts + ks_ else "argkmin is NOT faster by more than the spreads"
            print(f"  {D:4d} torch / argkmin (k = {kt}) = {tm / km:.1f}: {verdict}", flush=True)
        del x, y
        torch.cuda.empty_cache()

    N, D, k = args.low_n, args.low_d, args.low_k
    if N > 0:
        chunk = chunk_rows(N, args.mem_gib)
        print(f"# part 2: float32 clouds, N = M = {N}, D = {D}, k = {k}; median (min, spread) of {args.rounds} calls after {args.warmup}; the torch "
              f"route is timed on ONE chunk of {chunk} rows ({args.torch_rounds} calls after 1) and scaled by {N / chunk:.1f}")
        g = torch.Generator().manual_seed(N + D)
        x, y = torch.rand(N, D, generator=g).to(dev), torch.rand(N, D, generator=g).to(dev)
        launches = [("glhip_argmin", lambda: hip.argmin(x, y, None, return_value=True)),
                    (f"glhip_argkmin k = {k}", lambda: hip.argkmin(x, y, k, return_value=True))]
        wrong, excess = check(x, y, k, rows=64)
        for _ in range(args.warmup):
            for _, fn in launches:
                fn()
        if args.torch_rounds:
            torch_topk(x, y, k, chunk, rows=chunk)
        ms = {name: [] for name, _ in launches}
        tms = []
        for r in range(args.rounds):
            for name, fn in launches:
                ms[name].append(one_call(fn))
            if r < args.torch_rounds:
                tms.append(one_call(lambda: torch_topk(x, y, k, chunk, rows=chunk)))
        res = {name: line(D, name, ms[name], float(N) * N) for name, _ in launches}
        km, ks_ = res[f"glhip_argkmin k = {k}"]
        print(f"  {D:4d} argkmin / argmin: k = {k}: {km / res['glhip_argmin'][0]:.3f}; first 64 rows against float64: {wrong} rows differ, "
              f"largest cost excess {excess:.2e}", flush=True)
        if tms:
            tm, ts = line(D, f"torch cdist + topk({k}), one chunk, scaled", tms, float(N) * N, scale=N / chunk)
            verdict = "argkmin is faster by more than both spreads" if tm - km > ts + ks_ else "argkmin is NOT faster by more than the spreads"
            print(f"  {D:4d} torch / argkmin (k = {k}) = {tm / km:.1f}: {verdict}", flush=True)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
