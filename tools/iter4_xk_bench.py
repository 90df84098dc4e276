"""A/B timings of the one-launch Sinkhorn iteration of 17 <= D <= 4095 (glhip_softmin_xkp.h) on an MI355X -> profiles/iter4_xk.txt.

    python tools/iter4_xk_bench.py --parent /path/to/the/parent/commit's/libgeomloss_hip.so [--out FILE]

Part 1: online SamplesLoss("sinkhorn", p=2, blur=0.3), float32, forward and forward + backward: the parent build (four half-step launches
per temperature) against this build with GEOMLOSS_HIP_XK_ITER on, alternated in one process, `--reps` repetitions of a window of at least
`--window` seconds each; median and spread (max - min) per point.
Part 2: one raw iteration (hip.Iter4Plan.run: pack + one launch + merge) against the four hip.sinkhorn_step launches it replaces, this build.

    python tools/iter4_xk_bench.py --p 1 [--out FILE]      -> profiles/iter4_xk_p1.txt

The same two parts for p = 1 (glhip_dist_xkp.h): GEOMLOSS_HIP_XK_ITER_P1 off (four half-step launches of xk_dist_kernel per temperature,
the default) against on, both from THIS build's library, alternated in one process."""

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from geomloss_amd import SamplesLoss, _glhip, hip
from geomloss_amd import sinkhorn_samples as ss


def timed(fn, window, reps_hint=3):
    """Seconds per call of ``fn`` over a window of at least ``window`` seconds, ending in a device synchronise."""
    for _ in range(reps_hint):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    n = max(3, int(window / max(time.perf_counter() - t0, 1e-5)))
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def stats(ts):
    return statistics.median(ts) * 1e3, (max(ts) - min(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="p = 2: the parent commit's library")
    ap.add_argument("--p", type=int, default=2, choices=(1, 2))
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--quick", action="store_true", help="two small shapes only (rehearsal)")
    a = ap.parse_args()
    if a.p == 2 and not a.parent:
        ap.error("--p 2 needs --parent")
    p = a.p
    out = open(a.out, "w") if a.out else sys.stdout
    say = lambda s: (print(s, file=out, flush=True), print(s, flush=True) if a.out else None)      # noqa: E731
    dev = torch.device("cuda:0")
    say(f"# {' '.join(sys.argv)}\n# {torch.cuda.get_device_name(0)}; {a.reps} repetitions of >= {a.window} s windows, builds alternated; ms per call: median (max - min)")

    builds = {"parent": (a.parent if p == 2 else _glhip.LIB_PATH, False), "packed": (_glhip.LIB_PATH, True)}      # p = 1: "parent" = knob off

    def use(name):
        path, on = builds[name]
        _glhip.load_library(path)
        if p == 2:
            ss._XK_ITER = on
        else:
            ss._XK_ITER_P1 = on

    say(f"\n## online SamplesLoss('sinkhorn', p={p}, blur=0.3), float32\n# B N D | forward: {'parent' if p == 2 else 'knob off'}, packed, ratio | forward + backward: likewise")
    L = SamplesLoss("sinkhorn", p=p, blur=0.3, backend="online")
    shapes = [(None, N, D) for N in (512, 2000, 8000) for D in (32, 64, 128, 512)] + [(32, 1024, 64)]
    if a.quick:
        shapes = [(None, 512, 32), (2, 300, 64)]
    big = ss._XK_ITER_MAX_PAIRS
    ss._XK_ITER_MAX_PAIRS = float("inf")      # every shape takes the route that is being timed
    for B, N, D in shapes:
        torch.manual_seed(0)
        shp = (N, D) if B is None else (B, N, D)
        x, y = torch.rand(shp, device=dev), torch.rand(shp, device=dev)
        xg = x.clone().requires_grad_(True)
        fwd = lambda: L(x, y)                                              # noqa: E731
        both = lambda: torch.autograd.grad(L(xg, y).sum(), [xg])           # noqa: E731
        res = {(b, k): [] for b in builds for k in ("f", "fb")}
        vals = {}
        for _ in range(a.reps):
            for b in builds:
                use(b)
                vals[b] = float(L(x, y).sum())
                res[b, "f"].append(timed(fwd, a.window))
                res[b, "fb"].append(timed(both, a.window))
        row = f"{B or 1:3d} {N:6d} {D:4d} |"
        for k in ("f", "fb"):
            (mp, sp), (mn, sn) = stats(res["parent", k]), stats(res["packed", k])
            row += f" {mp:8.3f} ({sp:.3f})  {mn:8.3f} ({sn:.3f})  x{mp / mn:.2f} |"
        say(row + f" loss rel diff {abs(vals['packed'] - vals['parent']) / abs(vals['parent']):.1e}")
    ss._XK_ITER_MAX_PAIRS = big

    say("\n## one raw iteration, float32, debias: four sinkhorn_step launches | Iter4Plan.run (pack + launch + merge) | ratio | pairs per soft-min")
    use("packed")
    raw = [(N, D) for N in (2000, 8000, 30000) for D in ((64, 128) if p == 2 else (64,))]
    if a.quick:
        raw = [(2000, 64)]
    for N, D in raw:
        torch.manual_seed(0)
        x, y = torch.rand(N, D, device=dev), torch.rand(N, D, device=dev)
        lw = torch.full((N,), -float(torch.log(torch.tensor(float(N)))), device=dev)
        eps, damp = 0.3**p, 1.0
        pots = tuple(0.1 * torch.rand(N, device=dev) for _ in range(4))
        plan = hip.Iter4Plan(x, y, lw, lw, True, flags=hip.FLAG_XK_ITER_DIST if p == 1 else 0, p=p)
        step = lambda r, c, pot, prev: hip.sinkhorn_step(eps, r, c, lw, pot, prev, damp, p=p, flags=hip.FLAG_XK_DIST if p == 1 else 0)      # noqa: E731
        four = lambda: (step(x, y, pots[1], pots[0]), step(y, x, pots[0], pots[1]), step(x, x, pots[2], pots[2]), step(y, y, pots[3], pots[3]))  # noqa: E731
        one = lambda: plan.run(eps, damp, pots)                                                                                                      # noqa: E731
        t4, t1 = [], []
        for _ in range(a.reps):
            t4.append(timed(four, a.window))
            t1.append(timed(one, a.window))
        (m4, s4), (m1, s1) = stats(t4), stats(t1)
        say(f"{N:6d} {D:4d} | {m4:8.3f} ({s4:.3f}) | {m1:8.3f} ({s1:.3f}) | x{m4 / m1:.2f} | {float(N) * N:.1e}")


if __name__ == "__main__":
    main()
