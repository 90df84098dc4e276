"""GPU box: ``hip.plan_apply_sparse`` (glhip_plan_apply_sparse) on the two-scale solver's pattern, timed against the dense
``hip.plan_apply`` on the same sorted clouds and against one block-sparse soft-min on the same ranges.

    python tools/bench_plan_apply_sparse.py [--sizes 100000 1000000] [--features 3 32 128] [--rounds 5] [--warmup 1]
                                            [--d8 200000] [--resources build.txt] [--out profiles/plan_apply_sparse.txt]

Uniform unit cube, N = M = --sizes, D = 3, blur 0.05.  Potentials: ``SamplesLoss("sinkhorn", p=2, blur=0.05, potentials=True,
debias=False, backend="multiscale")``; order and ranges: ``transport.plan_ranges``.  Per size and V, alternated in one process on one GPU, each call
between two HIP events, after --warmup calls of each: (s) the sparse call, (d) the dense call, (f) one block-sparse soft-min forward.
Medians, minima, the spread (max - min) / median; then (s) / (d) next to the kept fraction of the pairs, the cost per kept pair of (s)
over the cost per pair of (d), and the largest |sparse - dense| of ``out`` over the largest feature: the truncation's own error
(reported, not asserted).  --d8: one D = 8 point at that N = M with row blocks from ``geomloss_amd.kmeans`` labels (0: skipped);
--resources: a text file (tools/kernel_resources.py on the build log of glhip_api_plan_sparse.hip) copied into the output."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from geomloss_amd import SamplesLoss, cluster, hip, transport  # noqa: E402

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


def line(tag, name, ms):
    med, lo = statistics.median(ms), min(ms)
    say(f"  {tag:>4s} {name:52s} {med:10.3f} {lo:10.3f} {(max(ms) - lo) / med:7.1%}")
    return med


def kept_fraction(rg, N, M):
    """The share of the N x M pairs the pattern keeps: rows of a block times the columns of its slice."""
    red = rg.redranges_j[:int(rg.slices_i[-1])].long()
    total = torch.cat([red.new_zeros(1), (red[:, 1] - red[:, 0]).cumsum(0)])
    ends = rg.slices_i.long()
    cols = total[ends] - total[torch.cat([ends.new_zeros(1), ends[:-1]])]
    rows = (rg.ranges_i[:, 1] - rg.ranges_i[:, 0]).long()
    return float((rows.double() * cols.double()).sum()) / (float(N) * float(M)), float(cols.double().mean()), int(red.shape[0])


def measure(xs, ys, h, rg, eps, features, rounds, warmup):
    N, M = xs.shape[0], ys.shape[0]
    frac, cols, n_iv = kept_fraction(rg, N, M)
    say(f"  {rg.ranges_i.shape[0]} row blocks, {n_iv} column intervals, {cols:.0f} kept columns per block on average, "
        f"kept fraction of the pairs {frac:.4f}")
    fwd_s = hip.softmin(eps, xs, ys, h, ranges=rg)
    fwd_d = hip.softmin(eps, xs, ys, h)
    say(f"  {'':4s} {'':52s} {'median ms':>10s} {'min ms':>10s} {'spread':>7s}")
    for V in features:
        feat = torch.randn(M, V, device=xs.device)
        calls = {"s": lambda: hip.plan_apply_sparse(eps, xs, ys, h, feat, rg, fwd=fwd_s),
                 "d": lambda: hip.plan_apply(eps, xs, ys, h, feat, fwd=fwd_d),
                 "f": lambda: hip.softmin(eps, xs, ys, h, ranges=rg)}
        for _ in range(warmup):
            for fn in calls.values():
                fn()
        ms = {k: [] for k in calls}
        for _ in range(rounds):
            for k, fn in calls.items():
                ms[k].append(one_call(fn))
        s = line("(s)", f"plan_apply_sparse, V = {V}", ms["s"])
        d = line("(d)", f"plan_apply on the same sorted clouds, V = {V}", ms["d"])
        f = line("(f)", "block-sparse soft-min forward on the same ranges", ms["f"])
        gap = float((calls["s"]() - calls["d"]()).abs().max() / feat.abs().max())
        say(f"       V = {V}: (s) / (d) = {s / d:.3f} at kept fraction {frac:.4f}; per kept pair (s) costs {s / d / frac:.2f} x the dense "
            f"kernel's cost per pair; (s) / (f) = {s / f:.2f}; max |sparse - dense| / max |feat| = {gap:.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[100000, 1000000])
    ap.add_argument("--features", type=int, nargs="*", default=[3, 32, 128])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--d8", type=int, default=200000)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dev = torch.device("cuda:0")
    blur, eps = 0.05, 0.05 ** 2
    say(f"plan_apply_sparse against plan_apply: {torch.cuda.get_device_name(0)}, libgeomloss_hip {hip.load_library().glhip_version()}, "
        f"{args.rounds} rounds after {args.warmup} warm-up, HIP events")
    gen = torch.Generator(device=dev).manual_seed(0)
    for n in args.sizes:
        x, y = torch.rand(n, 3, device=dev, generator=gen), torch.rand(n, 3, device=dev, generator=gen)
        # (debias=False: the potentials of the plan itself; they come back in the shape of the generated weights)
        F, G = (t.reshape(-1) for t in SamplesLoss("sinkhorn", p=2, blur=blur, potentials=True, debias=False, backend="multiscale")(x, y))
        px, py, rg = transport.plan_ranges(x, y, F, G, blur)
        say(f"\nN = M = {n}, D = 3, blur {blur}: uniform unit cube, potentials of the multiscale backend, ranges of transport.plan_ranges")
        measure(x[px].contiguous(), y[py].contiguous(), G[py] / eps - torch.log(torch.tensor(float(n))), rg, eps, args.features,
                args.rounds, args.warmup)
    if args.d8 > 0:
        # D = 8: no device clustering beyond D = 3 — row blocks from K-means labels, the keep rule evaluated on the centroids with the
        # potentials of the online backend averaged per cluster (cluster.from_matrix on the dense cluster mask)
        n, D, K, eps8 = args.d8, 8, 512, 0.1 * 8 / 3
        x, y = torch.rand(n, D, device=dev, generator=gen), torch.rand(n, D, device=dev, generator=gen)
        F, G = (t.reshape(-1) for t in SamplesLoss("sinkhorn", p=2, blur=eps8 ** 0.5, potentials=True, debias=False, backend="online")(x, y))
        sides = []
        for pts, pot in ((x, F), (y, G)):
            lab, cents = cluster.kmeans(pts, K, n_iter=5)
            perm = torch.argsort(lab.long(), stable=True)
            counts = torch.bincount(lab.long(), minlength=K)
            ends = counts.cumsum(0)
            ranges = torch.stack([ends - counts, ends], 1).int()
            mean = torch.zeros(K, device=dev).index_add_(0, lab.long(), pot.float()) / counts.clamp(min=1)
            sides.append((perm, ranges, cents.float(), mean))
        (px, rx, cx, fc), (py, ry, cy, gc) = sides
        keep = fc[:, None] + gc[None, :] > torch.cdist(cx, cy) ** 2 / 2 - 5 * eps8
        rg = cluster.from_matrix(rx, ry, keep)
        say(f"\nN = M = {n}, D = {D}, eps {eps8:.3f}: {K} K-means clusters per cloud (geomloss_amd.kmeans), keep rule on the centroids")
        measure(x[px].contiguous(), y[py].contiguous(), G[py] / eps8 - torch.log(torch.tensor(float(n))), rg, eps8, [32], args.rounds,
                args.warmup)
    if args.resources:
        say("\nresources of the shipped instantiations (hipcc -Rpass-analysis=kernel-resource-usage, tools/kernel_resources.py):")
        for text in open(args.resources).read().splitlines():
            say(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
