"""GPU box: ``glhip_softmin_bwd_x`` for clouds of 17 <= D <= 4095, timed with HIP events — the one-thread-per-row kernel of
glhip_generic.h (flag off: the launch of version 125) against the matrix-core gradient (``GLHIP_FLAG_XK_GRAD``,
glhip_softmin_grad_xk.h), alternated in one process, next to the forward reduction alone and one 64-feature pass of
``glhip_plan_apply_nd``.  float32 clouds, N = M = --n (default 1e5), eps = 0.1 D / 3, D in --dims (default 32 64 128 256).

    python tools/softmin_grad_bench.py [--n 100000] [--dims 32 64 128 256] [--rounds 5] [--warmup 1] [--f16x2]

Per dimension: --warmup calls of every launch, then --rounds rounds of (forward, flag off, flag on, plan pass), each call between two
events; medians, minima and the spread (max - min) / median.  The two gradients are compared on the same inputs before they are timed
(largest difference relative to the largest entry).  No ratio is asserted."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--dims", type=int, nargs="+", default=[32, 64, 128, 256])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--f16x2", action="store_true", help="exponents of the matrix-core launches from f16 x 2 pieces")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("softmin_grad_bench: no GPU — nothing is timed without one")
    dev = torch.device("cuda:0")
    lib = hip.load_library()
    base = hip.FLAG_F16X2 if args.f16x2 else 0
    n = args.n
    print(f"# libgeomloss_hip {lib.glhip_version()}; float32 clouds; N = M = {n}; flags {base}; one process, launches alternated; "
          f"median (min, spread) of {args.rounds} calls after {args.warmup}; {torch.cuda.get_device_name(0)}")
    print(f"# {'D':>4s} {'launch':28s} {'ms':>10s} {'min':>10s} {'spread':>7s} {'pairs/s':>10s}")
    for D in args.dims:
        eps = 0.1 * D / 3
        g = torch.Generator().manual_seed(n + D)
        x, y = torch.rand(1, n, D, generator=g).to(dev), torch.rand(1, n, D, generator=g).to(dev)
        h = (torch.randn(1, n, generator=g) * 2).to(dev)
        go = torch.randn(1, n, generator=g).to(dev)
        fwd = hip.softmin_fwd_raw(x, y, h, eps, 2, None, base)
        feat = y[..., :64].contiguous()
        assert hip.softmin_bwd_x_uses_plan(1, n, n, D, flags=base | hip.FLAG_XK_GRAD) == 1
        launches = [
            ("glhip_softmin_fwd", lambda: hip.softmin_fwd_raw(x, y, h, eps, 2, None, base)),
            ("glhip_softmin_bwd_x flag off", lambda: hip.softmin_bwd_x_raw(x, y, h, fwd, go, eps, 2, None, base)),
            ("glhip_softmin_bwd_x XK_GRAD", lambda: hip.softmin_bwd_x_raw(x, y, h, fwd, go, eps, 2, None, base | hip.FLAG_XK_GRAD)),
            (f"glhip_plan_apply_nd V={feat.shape[-1]}", lambda: hip.plan_apply_nd_raw(x, y, h, fwd, feat, eps, base)),
        ]
        old, new = launches[1][1](), launches[2][1]()
        diff = float((old - new).abs().max() / old.abs().max())
        del old, new
        for _ in range(args.warmup):
            for _, fn in launches:
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in launches}
        for _ in range(args.rounds):
            for name, fn in launches:
                ms[name].append(one_call(fn))
        for name, _ in launches:
            med, lo = statistics.median(ms[name]), min(ms[name])
            print(f"  {D:4d} {name:28s} {med:10.3f} {lo:10.3f} {(max(ms[name]) - lo) / med:7.1%} {float(n) * n / (med * 1e-3):10.3e}", flush=True)
        f, a, b, pa = (statistics.median(ms[name]) for name, _ in launches)
        passes = (D + 63) // 64
        print(f"  {D:4d} flag off / XK_GRAD = {a / b:.2f}; XK_GRAD / forward = {b / f:.2f} ({passes} pass{'es' if passes > 1 else ''}: "
              f"{b / f / passes:.2f} per pass); plan pass / forward = {pa / f:.2f}; the two gradients differ by {diff:.2e} of the largest entry",
              flush=True)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
