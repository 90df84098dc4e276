"""GPU box: the distance reductions for clouds of 17 <= D <= 4095 — p = 1 soft-min, fused half-step, laplacian and energy products —
timed with HIP events: the one-thread-per-row kernel of glhip_generic.h (flag off: the launches of version 130) against the
matrix-core kernel of glhip_dist_xk.h (``GLHIP_FLAG_XK_DIST``), both from ONE library and alternated in one process, next to a p = 2
bf16 x 3 soft-min of the same shape as a yardstick.  float32 clouds, N = M = --n (default 1e5), eps = 0.05 (p = 1),
blur = 0.2 sqrt(D / 3), D in --dims (default 32 64 128 256).

    python tools/dist_xk_bench.py [--n 100000] [--dims 32 64 128 256] [--rounds 3] [--warmup 1]
                                  [--loss-n 20000] [--loss-dims 64] [--check-rows 256]

Per dimension: --warmup calls of every launch, then --rounds rounds of all launches, each call between two events; medians, minima
and the spread (max - min) / median.  With the flag off the half-step is the composition ``hip.sinkhorn_step`` makes there: a soft-min
launch and torch arithmetic.  Before they are timed, both routes are compared with the float64 oracle on --check-rows rows of the
same inputs (soft-min: max|out - ref|; products, weights of mixed sign: max|out - ref| / max|ref_abs|, ref_abs the product of |v|).
Then the online ``SamplesLoss("sinkhorn", p=1)`` and ``SamplesLoss("energy")`` forward at N = M = --loss-n with the switch of
``GEOMLOSS_HIP_XK_DIST`` (``sinkhorn_samples._XK_DIST``, ``kernel_samples._XK_DIST``) on and off, alternated the same way.
No ratio is asserted."""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from geomloss_amd import SamplesLoss, hip, kernel_samples, sinkhorn_samples  # noqa: E402
from oracle import oracle_torch64 as o64  # noqa: E402

EPS1, DAMPING = 0.05, 0.8


def one_call(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(launches, rounds, warmup):
    for _ in range(warmup):
        for _, fn in launches:
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in launches}
    for _ in range(rounds):
        for name, fn in launches:
            ms[name].append(one_call(fn))
    return ms


def report(tag, name, t, pairs):
    med, lo = statistics.median(t), min(t)
    print(f"  {tag:>5} {name:34s} {med:10.3f} {lo:10.3f} {(max(t) - lo) / med:7.1%} {pairs / (med * 1e-3):10.3e}", flush=True)
    return med, (max(t) - lo)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--dims", type=int, nargs="*", default=[32, 64, 128, 256])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--loss-n", type=int, default=20000)
    ap.add_argument("--loss-dims", type=int, nargs="*", default=[64])
    ap.add_argument("--check-rows", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dist_xk_bench: no GPU — nothing is timed without one")
    dev = torch.device("cuda:0")
    lib = hip.load_library()
    XKD = hip.FLAG_XK_DIST
    n = args.n
    print(f"# libgeomloss_hip {lib.glhip_version()}; float32 clouds; N = M = {n}; one process, launches alternated; "
          f"median (min, spread) of {args.rounds} calls after {args.warmup}; {torch.cuda.get_device_name(0)}")
    print(f"# {'D':>4s} {'launch':34s} {'ms':>10s} {'min':>10s} {'spread':>7s} {'pairs/s':>10s}")
    for D in args.dims:
        blur, eps2 = 0.2 * math.sqrt(D / 3), 0.05**2 * D / 3
        g = torch.Generator().manual_seed(n + D)
        x, y = torch.rand(n, D, generator=g).to(dev), (torch.rand(n, D, generator=g) * 0.8 + 0.1).to(dev)
        h = torch.randn(n, generator=g).to(dev)
        v = (torch.randn(n, generator=g) / n).to(dev)
        pot, prev = (0.05 * torch.randn(n, generator=g)).to(dev), torch.randn(n, generator=g).to(dev)
        assert hip.softmin_fwd_family(1, n, n, D, 1, hip.F32, XKD) == hip.FAMILY_DIST and hip.softmin_fwd_family(1, n, n, D, 1, hip.F32, 0) == hip.FAMILY_GENERIC
        for kind in ("laplacian", "energy"):
            assert hip.kernel_conv_fwd_family(kind, 1, n, n, D, hip.F32, XKD) == hip.FAMILY_DIST
            assert hip.kernel_conv_fwd_family(kind, 1, n, n, D, hip.F32, 0) == hip.FAMILY_GENERIC
        assert hip.half_step_applies(D, 1, XKD) and not hip.half_step_applies(D, 1, 0)
        launches = []
        for tag, fl in (("flag off", 0), ("XK_DIST", XKD)):
            launches += [
                (f"soft-min p=1 {tag}", lambda fl=fl: hip.softmin(EPS1, x, y, h, p=1, flags=fl)),
                (f"half-step p=1 {tag}", lambda fl=fl: hip.sinkhorn_step(EPS1, x, y, h, pot, prev, DAMPING, p=1, flags=fl)),
                (f"laplacian {tag}", lambda fl=fl: hip.kernel_conv("laplacian", x, y, v, blur, flags=fl)),
                (f"energy {tag}", lambda fl=fl: hip.kernel_conv("energy", x, y, v, blur, flags=fl)),
            ]
        launches.append(("soft-min p=2 bf16x3 (yardstick)", lambda: hip.softmin(eps2, x, y, h, p=2)))
        # accuracy of both routes on a sample of rows, against float64
        rows = np.linspace(0, n - 1, min(args.check_rows, n)).astype(np.int64)
        xs = x[torch.from_numpy(rows).to(dev)].contiguous()
        x64, y64 = xs.double(), y.double()
        ref = o64.softmin(EPS1, x64, y64, h.double(), 1, device=dev)
        errs = {"soft-min": [float(np.abs(hip.softmin(EPS1, xs, y, h, p=1, flags=fl).cpu().numpy() - ref).max()) for fl in (0, XKD)]}
        fmax = max(1.0, float(np.abs(ref).max()))
        for kind in ("laplacian", "energy"):
            kref, kabs = o64.kconv(kind, x64, y64, v.double(), blur, device=dev), o64.kconv(kind, x64, y64, v.double().abs(), blur, device=dev)
            errs[kind] = [float(np.abs(hip.kernel_conv(kind, xs, y, v, blur, flags=fl).cpu().numpy() - kref).max() / np.abs(kabs).max()) for fl in (0, XKD)]
        del x64, y64
        ms = alternate(launches, args.rounds, args.warmup)
        med = {name: report(D, name, ms[name], float(n) * n) for name, _ in launches}
        for op in ("soft-min p=1", "half-step p=1", "laplacian", "energy"):
            a, b = med[f"{op} flag off"], med[f"{op} XK_DIST"]
            print(f"  {D:5d} {op}: flag off / XK_DIST = {a[0] / b[0]:.2f} (spread of flag off {a[1]:.3f} ms, gain {a[0] - b[0]:.3f} ms); "
                  f"XK_DIST / p=2 yardstick = {b[0] / med[launches[-1][0]][0]:.2f}", flush=True)
        print(f"  {D:5d} error on {len(rows)} rows against float64 (flag off, XK_DIST): soft-min max|out - ref| {errs['soft-min'][0]:.3e}, {errs['soft-min'][1]:.3e} "
              f"(2e-6 max(1, |f|) = {2e-6 * fmax:.3e}); laplacian / |v| product {errs['laplacian'][0]:.3e}, {errs['laplacian'][1]:.3e}; "
              f"energy {errs['energy'][0]:.3e}, {errs['energy'][1]:.3e}", flush=True)
        del x, y, h, v, pot, prev
    n = args.loss_n
    if args.loss_dims:
        print(f"# online SamplesLoss forward (no gradient), N = M = {n}; _XK_DIST (GEOMLOSS_HIP_XK_DIST) on / off, alternated")
    for D in args.loss_dims:
        g = torch.Generator().manual_seed(n + D)
        x, y = torch.rand(n, D, generator=g).to(dev), (torch.rand(n, D, generator=g) * 0.8 + 0.1).to(dev)
        for name, loss_fn in (("sinkhorn p=1", SamplesLoss("sinkhorn", p=1, blur=0.3, backend="online")), ("energy", SamplesLoss("energy", backend="online"))):
            last = {}

            def run(on):
                sinkhorn_samples._XK_DIST = kernel_samples._XK_DIST = on
                with torch.no_grad():
                    last[on] = float(loss_fn(x, y))

            launches = [(f"SamplesLoss {name} off", lambda: run(False)), (f"SamplesLoss {name} on", lambda: run(True))]
            ms = alternate(launches, args.rounds, args.warmup)
            sinkhorn_samples._XK_DIST = kernel_samples._XK_DIST = True
            med = {nm: report(D, nm, ms[nm], float(2 * n) * (2 * n)) for nm, _ in launches}
            a, b = med[launches[0][0]], med[launches[1][0]]
            print(f"  {D:5d} {name}: off / on = {a[0] / b[0]:.2f} (spread of off {a[1]:.3f} ms, gain {a[0] - b[0]:.3f} ms); loss {last[True]!r} / {last[False]!r}", flush=True)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
