"""GPU box: the arg-reduction ``hip.argmin`` (glhip_argmin) and ``geomloss_amd.kmeans``, timed.

    python tools/bench_argmin.py [--n 200000] [--dims 32 64 128] [--rounds 7] [--warmup 2]
                                 [--kmeans-n 1000000] [--kmeans-dims 4 64] [--kmeans-k 2000] [--kmeans-rounds 3]

Part 1 — against the soft-min forward.  ``hip.argmin(x, y, g)`` and ``hip.softmin_fwd_raw(x, y, h, eps)`` with flags = 0 (the
bf16 x 3 forward of glhip_softmin_xk.h, the kernel whose staging and MFMA chain the arg-reduction runs), float32 clouds uniform in the
unit cube, N = M = --n, alternated in one process on one GPU, each call between two HIP events: medians, minima, the spread
(max - min) / median and the ratio of the medians.  Before timing, the indices of the first 512 rows are checked against a
float64 torch evaluation of the same costs.

Part 2 — ``kmeans(x, K, n_iter=10)`` against the route a user has without it: ``torch.cdist`` + ``argmin`` in row chunks that fit
memory, followed by the same centroid update (``cluster.kmeans_update``).  Host clock around calls that end in a synchronise,
alternated; both routes start from the same centroids and their final labels are compared.

No ratio is asserted: the figures are printed."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from geomloss_amd import hip, kmeans  # noqa: E402
from geomloss_amd.cluster import kmeans_update  # noqa: E402


def one_call(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def line(D, name, ms, pairs):
    med, lo = statistics.median(ms), min(ms)
    print(f"  {D:4d} {name:34s} {med:10.3f} {lo:10.3f} {(max(ms) - lo) / med:7.1%} {pairs / (med * 1e-3):10.3e}", flush=True)
    return med


def torch_kmeans(x, c, n_iter, chunk):
    """cdist + argmin in row chunks of `chunk` rows (chunk x K floats at a time), then the same centroid update."""
    lab = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    for _ in range(n_iter):
        for r0 in range(0, x.shape[0], chunk):
            lab[r0:r0 + chunk] = torch.cdist(x[r0:r0 + chunk], c).argmin(1)
        c = kmeans_update(x, lab, c)
    return lab.int(), c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--dims", type=int, nargs="*", default=[32, 64, 128])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kmeans-n", type=int, default=1000000)
    ap.add_argument("--kmeans-dims", type=int, nargs="*", default=[4, 64])
    ap.add_argument("--kmeans-k", type=int, default=2000)
    ap.add_argument("--kmeans-rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_argmin: no GPU — nothing is timed without one")
    dev = torch.device("cuda:0")
    lib = hip.load_library()
    n = args.n
    print(f"# libgeomloss_hip {lib.glhip_version()}; {torch.cuda.get_device_name(0)}; one process, launches alternated")
    print(f"# part 1: float32 clouds, N = M = {n}, flags 0; median (min, spread) of {args.rounds} calls after {args.warmup}, HIP events")
    print(f"# {'D':>4s} {'launch':34s} {'ms':>10s} {'min':>10s} {'spread':>7s} {'pairs/s':>10s}")
    for D in args.dims:
        eps = 0.1 * D / 3
        g = torch.Generator().manual_seed(n + D)
        x, y = torch.rand(1, n, D, generator=g).to(dev), torch.rand(1, n, D, generator=g).to(dev)
        h = (torch.randn(1, n, generator=g) * 0.05).to(dev)
        assert hip.softmin_fwd_family(1, n, n, D) == (hip.FAMILY_XK if D > hip.XD_MAX_DIM else hip.FAMILY_XD)
        launches = [
            ("glhip_softmin_fwd (bf16 x 3)", lambda: hip.softmin_fwd_raw(x, y, h, eps, 2, None, 0)),
            ("glhip_argmin", lambda: hip.argmin(x, y, h)),
            ("glhip_argmin + value, g = None", lambda: hip.argmin(x, y, None, return_value=True)),
        ]
        # the indices of the first rows against float64
        idx = hip.argmin(x, y, h)[0, :512].long()
        C = (torch.cdist(x[0, :512].double(), y[0].double()) ** 2) / 2 - h[0].double()[None, :]
        excess = float((C.gather(1, idx[:, None])[:, 0] - C.min(1)[0]).max())
        wrong = int((idx != C.argmin(1)).sum())
        del C
        for _ in range(args.warmup):
            for _, fn in launches:
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in launches}
        for _ in range(args.rounds):
            for name, fn in launches:
                ms[name].append(one_call(fn))
        med = [line(D, name, ms[name], float(n) * n) for name, _ in launches]
        print(f"  {D:4d} argmin / soft-min = {med[1] / med[0]:.3f} (with value, g = None: {med[2] / med[0]:.3f}); first 512 rows against float64: "
              f"{wrong} indices differ, largest cost excess {excess:.2e}", flush=True)
        del x, y, h

    K, N = args.kmeans_k, args.kmeans_n
    print(f"# part 2: kmeans(x, {K}, n_iter=10), float32 cloud of N = {N} points; host clock around synchronised calls, "
          f"median (min, spread) of {args.kmeans_rounds} after 1; torch route: cdist + argmin in chunks of 32768 rows + the same update")
    for D in args.kmeans_dims:
        g = torch.Generator().manual_seed(N + D)
        x = torch.rand(N, D, generator=g).to(dev)
        init = x[torch.randperm(N, generator=g)[:K].to(dev)].clone()
        routes = [("geomloss_amd.kmeans", lambda: kmeans(x, K, n_iter=10, init=init)),
                  ("torch cdist + argmin, chunked", lambda: torch_kmeans(x, init.clone(), 10, 32768))]
        outs = [fn() for _, fn in routes]      # warm-up, and the results
        differ = int((outs[0][0] != outs[1][0]).sum())
        cdiff = float((outs[0][1] - outs[1][1]).abs().max())
        ms = {name: [] for name, _ in routes}
        for _ in range(args.kmeans_rounds):
            for name, fn in routes:
                ms[name].append(wall(fn)[0])
        med = [line(D, name, ms[name], 10.0 * N * K) for name, _ in routes]
        t_arg = statistics.median(one_call(lambda: hip.argmin(x, init)) for _ in range(5))
        print(f"  {D:4d} torch / kmeans = {med[1] / med[0]:.2f}; one hip.argmin of the loop: {t_arg:.3f} ms = {float(N) * K / (t_arg * 1e-3):.3e} pairs/s; "
              f"after 10 iterations {differ} of {N} labels differ between the routes, centroids by {cdiff:.2e}", flush=True)
        del x, outs
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
