"""GPU box: ``hip.plan_bilinear`` (glhip_plan_bilinear) timed against one ``hip.plan_apply_nd`` pass and against the only route to the same
numbers without it, and the wall time of ``barycentric_map`` forward and forward + backward.

    python tools/bench_plan_bilinear.py [--n 200000] [--shapes 3,3 3,32 32,32 64,64 128,128] [--rounds 5] [--warmup 1]
                                        [--route-cols 1024] [--route-rounds 3] [--map-dims 3 64] [--out profiles/plan_bilinear.txt]

Part 1 — float32 clouds (x uniform in the unit cube, y in its middle), N = M = --n, eps = 0.1 D / 3, standard-normal features, the
saved soft-min given to every launch.  Per (D, K), alternated in one process on one GPU, each call between two HIP events:
  (i)   ``hip.plan_bilinear``;
  (ii)  one ``hip.plan_apply_nd`` of K feature columns: the "one pass" yardstick;
  (iii) the route without the kernel: ``hip.plan_apply_nd`` on the K D columns ``colfeat (x) (y - c)``, contracted with ``rowfeat`` in
        torch.  The columns are built and applied --route-cols at a time (K D floats per point do not fit otherwise); when K D exceeds
        that, ONE such slice is timed and scaled by K D / --route-cols, and the line says so.
Medians, minima, the spread (max - min) / median; then (i) / (ii) and (iii) / (i).  Before timing, the first 128 rows of (i) are checked
against float64.  No ratio is asserted: the figures are printed.

Part 2 — ``barycentric_map`` at N = M = --n for every D of --map-dims: wall time (host clock around a synchronised call) of the forward
pass without a graph, and of forward + backward of ``(T - target)^2`` with x and y requiring grad."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from geomloss_amd import barycentric_map, hip  # noqa: E402

LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def one_call(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def line(tag, name, ms, scale=1.0):
    ms = [m * scale for m in ms]
    med, lo = statistics.median(ms), min(ms)
    say(f"  {tag:>9s} {name:58s} {med:10.3f} {lo:10.3f} {(max(ms) - lo) / med:7.1%}")
    return med


def check(eps, x, y, h, rf, cf, fwd, rows=128):
    """Largest error of the first rows against float64, relative to the unsigned sums."""
    out, wsum = hip.plan_bilinear(eps, x, y, h, rf, cf, fwd=fwd)
    xd, yd, hd, rd, cd = (t.double() for t in (x[:rows], y, h, rf[:rows], cf))
    E = hd[None, :] - torch.cdist(xd, yd) ** 2 / (2 * eps)
    q = torch.softmax(E, 1) * (rd @ cd.T)
    ref = q @ yd - xd * q.sum(1, keepdim=True)
    unsigned = (q.abs() @ yd.abs() + xd.abs() * q.abs().sum(1, keepdim=True)).max()      # an upper bound of sum_j pi |tau| |y_j - x_i|
    return float((out[:rows].double() - ref).abs().max() / unsigned), float((wsum[:rows].double() - q.sum(1)).abs().max() / q.abs().sum(1).max())


def route_slice(eps, x, y, h, fwd, rf, cf, yc, c0, c1):
    """Columns c0 .. c1 - 1 of colfeat (x) (y - c), applied and contracted: the contribution of those (k, d) pairs to out."""
    K, D = cf.shape[1], yc.shape[1]
    ks = torch.arange(c0, c1, device=x.device)
    k_of, d_of = ks // D, ks % D
    Z = hip.plan_apply_nd(eps, x, y, h, cf[:, k_of] * yc[:, d_of], fwd=fwd)              # (N, c1 - c0)
    out = torch.zeros(x.shape[0], D, device=x.device)
    out.index_add_(1, d_of, Z * rf[:, k_of])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--shapes", nargs="*", default=["3,3", "3,32", "32,32", "64,64", "128,128"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--route-cols", type=int, default=1024)
    ap.add_argument("--route-rounds", type=int, default=3)
    ap.add_argument("--map-dims", type=int, nargs="*", default=[3, 64])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "plan_bilinear.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_plan_bilinear: no GPU — nothing is timed without one")
    dev = torch.device("cuda:0")
    lib = hip.load_library()
    n = args.n
    say(f"# libgeomloss_hip {lib.glhip_version()}; {torch.cuda.get_device_name(0)}; one process, launches alternated; pass width "
        f"{lib.glhip_plan_bilinear_pass_width()}")
    say(f"# part 1: float32 clouds, N = M = {n}, eps = 0.1 D / 3; median (min, spread) of {args.rounds} calls after {args.warmup}, HIP events, ms")
    say(f"#   (iii) in slices of {args.route_cols} columns, {args.route_rounds} calls after 1 in the same alternation")
    say(f"# {'D, K':>9s} {'launch':58s} {'ms':>10s} {'min':>10s} {'spread':>7s}")
    for shape in args.shapes:
        D, K = (int(v) for v in shape.split(","))
        tag = f"{D}, {K}"
        eps = 0.1 * D / 3
        g = torch.Generator().manual_seed(n + 7 * D + K)
        x = torch.rand(n, D, generator=g).to(dev)
        y = (torch.rand(n, D, generator=g) * 0.8 + 0.1).to(dev)
        h = torch.randn(n, generator=g).to(dev)
        rf, cf = torch.randn(n, K, generator=g).to(dev), torch.randn(n, K, generator=g).to(dev)
        fwd = hip.softmin(eps, x, y, h)
        yc = y - y.mean(0, keepdim=True)
        cols = K * D
        c1 = min(cols, args.route_cols)
        scale = cols / c1
        launches = [("(i)   plan_bilinear", lambda: hip.plan_bilinear(eps, x, y, h, rf, cf, fwd=fwd)),
                    (f"(ii)  plan_apply_nd, V = {K}", lambda: hip.plan_apply_nd(eps, x, y, h, cf, fwd=fwd))]
        rname = f"(iii) plan_apply_nd on {cols} columns + contraction" + (f" [one slice of {c1}, x {scale:.1f}]" if scale > 1 else "")
        eo, ew = check(eps, x, y, h, rf, cf, fwd)
        for _ in range(args.warmup):
            for _, fn in launches:
                fn()
        if args.route_rounds:
            route_slice(eps, x, y, h, fwd, rf, cf, yc, 0, c1)
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in launches}
        rms = []
        for r in range(args.rounds):
            for name, fn in launches:
                ms[name].append(one_call(fn))
            if r < args.route_rounds:
                rms.append(one_call(lambda: route_slice(eps, x, y, h, fwd, rf, cf, yc, 0, c1)))
        med = [line(tag, name, ms[name]) for name, _ in launches]
        text = f"  {tag:>9s} (i) / (ii) = {med[0] / med[1]:.2f}"
        if rms:
            rmed = line(tag, rname, rms, scale)
            text += f";  (iii) / (i) = {rmed / med[0]:.2f}"
        say(text + f";  first 128 rows against float64: out {eo:.2e}, wsum {ew:.2e} of the unsigned sums")
        del x, y, h, rf, cf, fwd, yc
        torch.cuda.empty_cache()

    say(f"# part 2: barycentric_map, float32 clouds, N = M = {n}, blur = 0.1 sqrt(D / 3), G = 0; wall time (host clock, synchronised), "
        f"median (min) of {args.rounds} calls after {args.warmup}, ms")
    for D in args.map_dims:
        blur = 0.1 * (D / 3) ** 0.5
        g = torch.Generator().manual_seed(n + D)
        x = torch.rand(n, D, generator=g).to(dev)
        y = (torch.rand(n, D, generator=g) * 0.8 + 0.1).to(dev)
        F, G = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        target = torch.rand(n, D, generator=g).to(dev)

        def forward():
            with torch.no_grad():
                barycentric_map(x, y, F, G, blur)

        def both():
            xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
            (barycentric_map(xg, yg, F, G, blur) - target).pow(2).sum().backward()

        for name, fn in (("forward", forward), ("forward + backward (x, y)", both)):
            ts = []
            for r in range(args.warmup + args.rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if r >= args.warmup:
                    ts.append((time.perf_counter() - t0) * 1e3)
            say(f"  D = {D:4d} barycentric_map {name:28s} {statistics.median(ts):10.3f} {min(ts):10.3f}")
    say("# not timed: bfloat16 clouds, batches, D > 128, gradients of apply_plan")
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
