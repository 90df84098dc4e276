"""GPU box: the gaussian kernel gradient for clouds of 17 <= D <= 4095, timed with HIP events — the one-thread-per-row kernel of
glhip_generic.h (flag off: the launches of version 129) against the matrix-core gradient (``GLHIP_FLAG_XK_GRAD``,
glhip_gauss_grad_xk.h), both from ONE library and alternated in one process, next to the gaussian product alone.  float32 clouds,
N = M = --n (default 1e5), blur = 0.3 sqrt(D / 3), column weights of mixed sign, D in --dims (default 32 64 128 256).

    python tools/gauss_grad_bench.py [--n 100000] [--dims 32 64 128 256] [--rounds 3] [--warmup 1] [--f16x2]
                                     [--loss-n 50000] [--loss-dims 64 128] [--check-rows 256]

Per dimension: --warmup calls of every launch, then --rounds rounds of (product, bwd_x flag off, bwd_x flag on, product + bwd_x flag off
— what a product-and-gradient costs without the flag, where ``glhip_kernel_conv_fwd_grad`` refuses D > 16 —, fwd_grad flag on), each
call between two events; medians, minima and the spread (max - min) / median.  Before they are timed, both routes are compared with
the float64 oracle on --check-rows rows of the same inputs: max|out - ref| / max|ref_abs|, ref_abs the float64 gradient for |v|, |g|.
Then ``SamplesLoss("gaussian", backend="online")`` forward + backward at N = M = --loss-n with the switch of
``GEOMLOSS_HIP_XK_GRAD`` (``kernel_samples._XK_GRAD``) on and off, alternated the same way.  No ratio is asserted."""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from geomloss_amd import SamplesLoss, hip, kernel_samples  # noqa: E402
from oracle import oracle_torch64 as o64  # noqa: E402


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
    ap.add_argument("--f16x2", action="store_true", help="exponents of the matrix-core launches from f16 x 2 pieces")
    ap.add_argument("--loss-n", type=int, default=50000)
    ap.add_argument("--loss-dims", type=int, nargs="*", default=[64, 128])
    ap.add_argument("--check-rows", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gauss_grad_bench: no GPU — nothing is timed without one")
    dev = torch.device("cuda:0")
    lib = hip.load_library()
    base = hip.FLAG_F16X2 if args.f16x2 else 0
    XK = base | hip.FLAG_XK_GRAD
    G = hip.GAUSSIAN
    n = args.n
    print(f"# libgeomloss_hip {lib.glhip_version()}; float32 clouds; N = M = {n}; flags {base}; one process, launches alternated; "
          f"median (min, spread) of {args.rounds} calls after {args.warmup}; {torch.cuda.get_device_name(0)}")
    print(f"# {'D':>4s} {'launch':34s} {'ms':>10s} {'min':>10s} {'spread':>7s} {'pairs/s':>10s}")
    for D in args.dims:
        blur = 0.3 * math.sqrt(D / 3)
        g = torch.Generator().manual_seed(n + D)
        x, y = torch.rand(1, n, D, generator=g).to(dev), torch.rand(1, n, D, generator=g).to(dev)
        v = (torch.randn(1, n, generator=g) / n).to(dev)
        go = torch.randn(1, n, generator=g).to(dev)
        assert hip.kernel_conv_grad_uses_xk(G, 1, n, n, D, flags=XK) == 1 and hip.kernel_conv_grad_uses_xk(G, 1, n, n, D, flags=base) == 0
        launches = [
            ("glhip_kernel_conv_fwd", lambda: hip.kernel_conv_fwd_raw(G, x, y, v, blur, None, base)),
            ("glhip_kernel_conv_bwd_x flag off", lambda: hip.kernel_conv_bwd_x_raw(G, x, y, v, go, blur, None, base)),
            ("glhip_kernel_conv_bwd_x XK_GRAD", lambda: hip.kernel_conv_bwd_x_raw(G, x, y, v, go, blur, None, XK)),
            ("fwd + bwd_x flag off", lambda: (hip.kernel_conv_fwd_raw(G, x, y, v, blur, None, base),
                                              hip.kernel_conv_bwd_x_raw(G, x, y, v, go, blur, None, base))),
            ("glhip_kernel_conv_fwd_grad XK_GRAD", lambda: hip.kernel_conv_fwd_grad_raw(G, x, y, v, blur, None, XK)),
        ]
        # accuracy of both routes on a sample of rows, against float64
        rows = np.linspace(0, n - 1, min(args.check_rows, n)).astype(np.int64)
        rt = torch.from_numpy(rows).to(dev)
        xs, gs = x[:, rt].contiguous(), go[:, rt].contiguous()
        x64, y64, v64, g64 = (t[0].double() for t in (xs, y, v, gs))
        ref = o64.kconv_grad_x("gaussian", x64, y64, v64, g64, blur, device=dev)
        ref_abs = o64.kconv_grad_x("gaussian", x64, y64, v64.abs(), g64.abs(), blur, device=dev)
        scale = np.abs(ref_abs).max()
        errs = [float(np.abs(hip.kernel_conv_bwd_x_raw(G, xs, y, v, gs, blur, None, fl)[0].cpu().numpy() - ref).max() / scale) for fl in (base, XK)]
        del x64, y64, v64, g64
        ms = alternate(launches, args.rounds, args.warmup)
        med = {name: report(D, name, ms[name], float(n) * n) for name, _ in launches}
        f, a, b, fa, fb = (med[name][0] for name, _ in launches)
        passes = (D + 63) // 64
        print(f"  {D:5d} bwd_x flag off / XK_GRAD = {a / b:.2f} (spread of flag off {med[launches[1][0]][1]:.3f} ms, gain {a - b:.3f} ms); "
              f"(fwd + bwd_x) flag off / fwd_grad XK_GRAD = {fa / fb:.2f}; XK_GRAD / product = {b / f:.2f} ({passes} pass{'es' if passes > 1 else ''}: "
              f"{b / f / passes:.2f} per pass)", flush=True)
        print(f"  {D:5d} error of bwd_x on {len(rows)} rows against float64, max|out - ref| / max|ref_abs|: flag off {errs[0]:.3e}, XK_GRAD {errs[1]:.3e} "
              f"(signed sums cancel {scale / np.abs(ref).max():.1f}x)", flush=True)
        del x, y, v, go
    n = args.loss_n
    if args.loss_dims:
        print(f"# SamplesLoss('gaussian', backend='online') forward + backward, N = M = {n}, gradients in x and y; kernel_samples._XK_GRAD "
              f"(GEOMLOSS_HIP_XK_GRAD) on / off, alternated")
    for D in args.loss_dims:
        blur = 0.3 * math.sqrt(D / 3)
        g = torch.Generator().manual_seed(n + D)
        x, y = torch.rand(n, D, generator=g).to(dev), (torch.rand(n, D, generator=g) * 0.8 + 0.1).to(dev)
        loss_fn = SamplesLoss("gaussian", blur=blur, backend="online")
        last = {}

        def run(on):
            kernel_samples._XK_GRAD = on
            xt, yt = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
            L = loss_fn(xt, yt)
            grads = torch.autograd.grad(L, [xt, yt])
            last[on] = (float(L.detach()), grads)

        launches = [("SamplesLoss XK_GRAD off", lambda: run(False)), ("SamplesLoss XK_GRAD on", lambda: run(True))]
        ms = alternate(launches, args.rounds, args.warmup)
        kernel_samples._XK_GRAD = True
        med = {name: report(D, name, ms[name], float(2 * n) * (2 * n)) for name, _ in launches}
        diff = max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(last[True][1], last[False][1]))
        a, b = med[launches[0][0]], med[launches[1][0]]
        print(f"  {D:5d} off / on = {a[0] / b[0]:.2f} (spread of off {a[1]:.3f} ms, gain {a[0] - b[0]:.3f} ms); loss {last[True][0]!r} / {last[False][0]!r}; "
              f"the gradients differ by {diff:.2e} of the largest entry", flush=True)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
