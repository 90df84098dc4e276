"""GPU box: the transport plan applied to feature matrices, timed with HIP events — ``plan_operator @ S`` of an ``ot.solve_sample``
result and the raw ``glhip_plan_apply`` launch, D = 3, N = M = --n (default 2e5), V in {1 mixed-sign, 2, 3, 32, 128}; optionally one
V = 32 product at --big (1e6: 3 calls after 1).  Medians over --launches calls after --warmup warm-up calls, with the spread
(max - min) / median.

    python tools/plan_apply_bench.py                 # one forward reduction + one matrix-core application per product
    python tools/plan_apply_bench.py --legacy        # the log-domain path for every width: 2 V forward reductions per product.  Copied
                                                     # into a checkout of a commit without glhip_plan_apply, this is how that commit is timed
    python tools/plan_apply_bench.py --dims 32 64 128 --n 100000 --widths 1 2 3 8 32 128 --budget-ms 4000
                                                     # feature spaces (glhip_plan_apply_nd, eps = 0.1 D / 3); with --legacy and
                                                     # GEOMLOSS_HIP_LIB=<library of the parent commit> this times that library's route:
                                                     # symbols it does not export yet are not bound
    python tools/plan_apply_bench.py --p 1 --dims 3 32 128 --widths 3 32 128 --legacy --budget-ms 4000
                                                     # the p = 1 product (glhip_plan_apply_p1), one p = 1 forward reduction and, with
                                                     # --legacy, the loop of 2 V reductions it replaces, alternated in one process

The solve itself is not timed: the potentials are a few Sinkhorn iterations at a moderate temperature, enough for a well-formed plan."""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from geomloss_amd import hip, ot  # noqa: E402


def timed(fn, launches, warmup, budget_ms=0.0):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    if budget_ms > 0:      # long products (the log-domain loop at V = 128): as many calls as fit the budget, at least 3
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        launches = max(3, min(launches, int(budget_ms / max(a.elapsed_time(b), 1e-3))))
    ms = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    med = statistics.median(ms)
    return med, min(ms), (max(ms) - min(ms)) / med


def features(n, V, g, dev):
    return torch.randn(n, V, generator=g).to(dev)      # standard normal: every column changes sign


def run_dims(args, lib, dev):
    """--dims: `plan_operator @ S`, the forward reduction alone and the raw application for clouds of each dimension."""
    mode = "log-domain path (2 V forward reductions)" if args.legacy else "1 forward reduction + 1 application from the threshold on"
    print(f"# libgeomloss_hip {lib.glhip_version()}; {mode}; float32; median (min, spread) of up to {args.launches} calls after "
          f"{args.warmup}; {torch.cuda.get_device_name(0)}")
    n = args.n
    for D in args.dims:
        eps = 0.01 if D <= 3 else 0.1 * D / 3
        g = torch.Generator().manual_seed(n + D)
        x, y = torch.rand(n, D, generator=g).to(dev), torch.rand(n, D, generator=g).to(dev)
        res = ot.solve_sample(x, y, reg=2 * eps, max_iter=5)
        op = res.plan_operator
        for V in args.widths:
            S = features(n, V, g, dev)
            med, lo, spread = timed(lambda: op @ S, args.launches, args.warmup, args.budget_ms)
            print(f"plan_operator @ S   D={D:4d} N=M={n:8d} V={V:4d}  {med:10.3f} ms (min {lo:10.3f}, spread {spread:5.1%})", flush=True)
        xb, yb = x[None].contiguous(), y[None].contiguous()
        hb = (torch.randn(1, n, generator=g) * 2).to(dev)
        fwd = hip.softmin_fwd_raw(xb, yb, hb, eps, 2, None, 0)
        med, lo, spread = timed(lambda: hip.softmin_fwd_raw(xb, yb, hb, eps, 2, None, 0), args.launches, args.warmup, args.budget_ms)
        print(f"glhip_softmin_fwd   D={D:4d} N=M={n:8d}         {med:10.3f} ms (min {lo:10.3f}, spread {spread:5.1%})", flush=True)
        if args.legacy:
            continue
        for V in args.widths:
            S = features(n, V, g, dev)[None].contiguous()
            med, lo, spread = timed(lambda: hip.plan_apply_nd_raw(xb, yb, hb, fwd, S, eps, 0), args.launches, args.warmup, args.budget_ms)
            print(f"glhip_plan_apply_nd D={D:4d} N=M={n:8d} V={V:4d}  {med:10.3f} ms (min {lo:10.3f}, spread {spread:5.1%})", flush=True)
    torch.cuda.synchronize()


def run_p1(args, lib, dev):
    """--p 1: the raw ``glhip_plan_apply_p1`` product (glhip_dist_plan_xk.h) for clouds of each dimension and width, one plain
    ``hip.softmin(p=1)`` forward reduction of the same shape and, with --legacy, the log-domain loop the product replaces — 2 V forward
    reductions, the positive and the negative part of every column — alternated with it in the same process.  FLAG_XK_DIST where D > 16;
    eps = 0.05 sqrt(D).  The loop is timed with one warm-up call."""
    print(f"# libgeomloss_hip {lib.glhip_version()}; p = 1; float32; pass width {lib.glhip_plan_apply_p1_pass_width()}; median (min, spread) "
          f"of up to {args.launches} calls after {args.warmup}; {torch.cuda.get_device_name(0)}")
    n = args.n
    for D in args.dims if args.dims is not None else [3]:
        eps = 0.05 * D**0.5
        flags = hip.FLAG_XK_DIST if D > 16 else 0
        g = torch.Generator().manual_seed(n + D)
        x, y = torch.rand(n, D, generator=g).to(dev), torch.rand(n, D, generator=g).to(dev)
        h = (torch.randn(n, generator=g) * 2).to(dev)
        xb, yb, hb = x[None].contiguous(), y[None].contiguous(), h[None].contiguous()
        fwd_ms, lo, spread = timed(lambda: hip.softmin(eps, x, y, h, p=1, flags=flags), args.launches, args.warmup, args.budget_ms)
        print(f"hip.softmin p=1     D={D:4d} N=M={n:8d}         {fwd_ms:10.3f} ms (min {lo:10.3f}, spread {spread:5.1%})", flush=True)
        for V in args.widths:
            S = features(n, V, g, dev)
            Sb = S[None].contiguous()
            med, lo, spread = timed(lambda: hip.plan_apply_p1_raw(xb, yb, hb, Sb, eps, 0, want_softmin=True), args.launches, args.warmup,
                                    args.budget_ms)
            line = (f"glhip_plan_apply_p1 D={D:4d} N=M={n:8d} V={V:4d}  {med:10.3f} ms (min {lo:10.3f}, spread {spread:5.1%})"
                    f"  = {med / fwd_ms:6.2f} forwards")
            if args.legacy:
                logs = [(S[:, v].clamp_min(0).log(), (-S[:, v]).clamp_min(0).log()) for v in range(V)]

                def loop():
                    out = torch.empty(n, V, device=dev)
                    for v, (lp, ln) in enumerate(logs):
                        out[:, v] = ((-hip.softmin(eps, x, y, h + lp, p=1, flags=flags) / eps).exp()
                                     - (-hip.softmin(eps, x, y, h + ln, p=1, flags=flags) / eps).exp())
                    return out
                lmed, llo, lspread = timed(loop, args.launches, 1, args.budget_ms)
                line += f";  loop of {2 * V} reductions {lmed:10.3f} ms (min {llo:10.3f}, spread {lspread:5.1%}) = {lmed / med:6.2f} products"
            print(line, flush=True)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=int, choices=[1, 2], default=2, help="the cost: 2 (|x - y|^2 / 2, as ever) or 1 (|x - y|: glhip_plan_apply_p1)")
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--big", type=int, default=0, help="one more V = 32 product at this N = M (1e6), 3 calls")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--widths", type=int, nargs="*", default=[1, 2, 3, 32, 128])
    ap.add_argument("--legacy", action="store_true", help="log-domain path: 2 V forward reductions per product")
    ap.add_argument("--dims", type=int, nargs="*", default=None, help="cloud dimensions (default: 3, as ever); eps = 0.1 D / 3 from D = 4 on")
    ap.add_argument("--budget-ms", type=float, default=0.0, help="fewer calls (at least 3) for products longer than this / --launches")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.legacy and os.environ.get("GEOMLOSS_HIP_LIB"):      # an older library: bind what it exports
        old = ctypes.CDLL(os.environ["GEOMLOSS_HIP_LIB"])
        for name in [k for k in hip.SIGNATURES if not hasattr(old, k)]:
            print(f"# {name}: not exported by {os.environ['GEOMLOSS_HIP_LIB']}, not bound")
            del hip.SIGNATURES[name]
    lib = hip.load_library()
    if args.legacy:
        hip.plan_apply_applies = lambda *a, **k: False
        hip.plan_apply_nd_applies = lambda *a, **k: False
    if args.p == 1:
        run_p1(args, lib, dev)
        return
    if args.dims is not None:
        run_dims(args, lib, dev)
        return
    mode = ("log-domain path (2 V forward reductions)" if args.legacy
            else "glhip_plan_apply (1 forward reduction + 1 application) from 3 columns on, log-domain path below")
    print(f"# libgeomloss_hip {lib.glhip_version()}; {mode}; D = 3, float32; median (min, spread) of {args.launches} calls after "
          f"{args.warmup} (N = M = --big: 3 after 1); {torch.cuda.get_device_name(0)}")

    def run(n, widths, launches, warmup):
        g = torch.Generator().manual_seed(n)
        x, y = torch.rand(n, 3, generator=g).to(dev), torch.rand(n, 3, generator=g).to(dev)
        res = ot.solve_sample(x, y, reg=0.05**2 * 2, max_iter=5)
        op = res.plan_operator
        for V in widths:
            S = features(n, V, g, dev)
            med, lo, spread = timed(lambda: op @ S, launches, warmup)
            print(f"plan_operator @ S   N=M={n:8d} V={V:4d}  {med:10.3f} ms (min {lo:10.3f}, spread {spread:5.1%})", flush=True)
        if args.legacy:
            return
        eps = 0.05**2
        xb, yb = x[None].contiguous(), y[None].contiguous()
        hb = (torch.randn(1, n, generator=g) * 2).to(dev)
        fwd = hip.softmin_fwd_raw(xb, yb, hb, eps, 2, None, 0)
        med, lo, spread = timed(lambda: hip.softmin_fwd_raw(xb, yb, hb, eps, 2, None, 0), launches, warmup)
        print(f"glhip_softmin_fwd   N=M={n:8d}         {med:10.3f} ms (min {lo:10.3f}, spread {spread:5.1%})", flush=True)
        for V in widths:
            S = features(n, V, g, dev)[None].contiguous()
            med, lo, spread = timed(lambda: hip.plan_apply_raw(xb, yb, hb, fwd, S, eps, 0), launches, warmup)
            print(f"glhip_plan_apply    N=M={n:8d} V={V:4d}  {med:10.3f} ms (min {lo:10.3f}, spread {spread:5.1%})", flush=True)

    run(args.n, args.widths, args.launches, args.warmup)
    if args.big:
        run(args.big, [32], 3, 1)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
