"""GPU box: the row gradients of the distance reductions for clouds of 17 <= D <= 4095 — p = 1 soft-min, laplacian and energy kernels —
timed with HIP events: the one-thread-per-row kernel of glhip_generic.h (flag off: the launches of version 131) against the
matrix-core kernel of glhip_dist_grad_xk.h (``GLHIP_FLAG_XK_DIST_GRAD``), both from ONE library and alternated in one process, next to
the forward reduction of the same shape under ``GLHIP_FLAG_XK_DIST`` as a yardstick.  float32 clouds, N = M = --n (default 1e5),
eps = 0.3 (p = 1), blur = 0.2 sqrt(D / 3), D in --dims (default 32 64 128 256).

    python tools/dist_grad_xk_bench.py [--n 100000] [--dims 32 64 128 256] [--rounds 3] [--warmup 1]
                                       [--loss-n 20000] [--loss-dims 64] [--check-rows 256]

Per dimension: --warmup calls of every launch, then --rounds rounds of all launches, each call between two events; medians, minima
and the spread (max - min) / median.  "product + gradient" is ``glhip_kernel_conv_fwd_grad`` with the flag on and, with it off, what the
Python layer does without a fused kernel: ``glhip_kernel_conv_fwd`` (under ``GLHIP_FLAG_XK_DIST``) and ``glhip_kernel_conv_bwd_x``.  Before
they are timed, both routes are compared with the float64 oracle on --check-rows rows of the same inputs (relative to the largest entry
of the reference; products: weights of mixed sign, relative to the gradient under |v|).  Then the online ``SamplesLoss("sinkhorn", p=1)``,
``("laplacian")`` and ``("energy")``, forward + backward, at N = M = --loss-n with the switch of ``GEOMLOSS_HIP_XK_GRAD``
(``sinkhorn_samples._XK_GRAD``, ``kernel_samples._XK_GRAD``) on and off, alternated the same way.  No ratio is asserted."""
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

EPS1 = 0.3
KINDS = ("laplacian", "energy")


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
    print(f"  {tag:>5} {name:42s} {med:10.3f} {lo:10.3f} {(max(t) - lo) / med:7.1%} {pairs / (med * 1e-3):10.3e}", flush=True)
    return med, (max(t) - lo)


def relerr(a, ref, scale=None):
    return float(np.abs(a - ref).max() / np.abs(ref if scale is None else scale).max())


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
        sys.exit("dist_grad_xk_bench: no GPU — nothing is timed without one")
    dev = torch.device("cuda:0")
    lib = hip.load_library()
    XDG, XKD = hip.FLAG_XK_DIST_GRAD, hip.FLAG_XK_DIST
    n = args.n
    print(f"# libgeomloss_hip {lib.glhip_version()}; float32 clouds; N = M = {n}; {lib.glhip_dist_grad_pass_width()} coordinates per pass; one process, "
          f"launches alternated; median (min, spread) of {args.rounds} calls after {args.warmup}; {torch.cuda.get_device_name(0)}")
    print(f"# {'D':>4s} {'launch':42s} {'ms':>10s} {'min':>10s} {'spread':>7s} {'pairs/s':>10s}")
    for D in args.dims:
        blur = 0.2 * math.sqrt(D / 3)
        gen = torch.Generator().manual_seed(n + D)
        x, y = torch.rand(1, n, D, generator=gen).to(dev), (torch.rand(1, n, D, generator=gen) * 0.8 + 0.1).to(dev)
        h = torch.randn(1, n, generator=gen).to(dev)
        v = (torch.randn(1, n, generator=gen) / n).to(dev)
        g = torch.randn(1, n, generator=gen).to(dev)
        for op in ("softmin_p1",) + KINDS:
            assert hip.dist_grad_uses_xk(op, 1, n, n, D, hip.F32, XDG) == 1 and hip.dist_grad_uses_xk(op, 1, n, n, D, hip.F32, 0) == 0
        fwd = hip.softmin_fwd_raw(x, y, h, EPS1, 1, None, XKD)
        code = hip.KERNEL_KINDS
        launches = []
        for tag, fl in (("flag off", 0), ("XK_DIST_GRAD", XDG)):
            launches.append((f"soft-min p=1 gradient {tag}", lambda fl=fl: hip.softmin_bwd_x_raw(x, y, h, fwd, g, EPS1, 1, None, fl)))
            for kind in KINDS:
                launches.append((f"{kind} gradient {tag}", lambda fl=fl, kind=kind: hip.kernel_conv_bwd_x_raw(code[kind], x, y, v, g, blur, None, fl)))
        for kind in KINDS:
            launches.append((f"{kind} product + gradient flag off", lambda kind=kind: (hip.kernel_conv_fwd_raw(code[kind], x, y, v, blur, None, XKD),
                                                                                       hip.kernel_conv_bwd_x_raw(code[kind], x, y, v, g, blur, None, 0))))
            launches.append((f"{kind} product + gradient XK_DIST_GRAD", lambda kind=kind: hip.kernel_conv_fwd_grad_raw(code[kind], x, y, v, blur, None, XDG)))
        launches.append(("soft-min p=1 forward (XK_DIST)", lambda: hip.softmin_fwd_raw(x, y, h, EPS1, 1, None, XKD)))
        for kind in KINDS:
            launches.append((f"{kind} forward (XK_DIST)", lambda kind=kind: hip.kernel_conv_fwd_raw(code[kind], x, y, v, blur, None, XKD)))
        # accuracy of both routes on a sample of rows, against float64
        rows = torch.from_numpy(np.linspace(0, n - 1, min(args.check_rows, n)).astype(np.int64)).to(dev)
        xs, gs, fs = x[:, rows].contiguous(), g[:, rows].contiguous(), fwd[:, rows].contiguous()
        x64, y64 = xs[0].double(), y[0].double()
        ref = o64.softmin_grad_x(EPS1, x64, y64, h[0].double(), gs[0].double(), 1, device=dev)
        errs = {"soft-min p=1": [relerr(hip.softmin_bwd_x_raw(xs, y, h, fs, gs, EPS1, 1, None, fl)[0].cpu().numpy(), ref) for fl in (0, XDG)]}
        for kind in KINDS:
            kref = o64.kconv_grad_x(kind, x64, y64, v[0].double(), gs[0].double(), blur, device=dev)
            kabs = o64.kconv_grad_x(kind, x64, y64, v[0].double().abs(), gs[0].double(), blur, device=dev)
            errs[kind] = [relerr(hip.kernel_conv_bwd_x_raw(code[kind], xs, y, v, gs, blur, None, fl)[0].cpu().numpy(), kref, kabs) for fl in (0, XDG)]
        del x64, y64
        ms = alternate(launches, args.rounds, args.warmup)
        med = {name: report(D, name, ms[name], float(n) * n) for name, _ in launches}
        for op in ("soft-min p=1", "laplacian", "energy"):
            a, b, f = med[f"{op} gradient flag off"], med[f"{op} gradient XK_DIST_GRAD"], med[f"{op} forward (XK_DIST)"]
            print(f"  {D:5d} {op} gradient: flag off / XK_DIST_GRAD = {a[0] / b[0]:.2f} (spread of flag off {a[1]:.3f} ms, gain {a[0] - b[0]:.3f} ms); "
                  f"XK_DIST_GRAD / forward = {b[0] / f[0]:.2f}, flag off / forward = {a[0] / f[0]:.2f}", flush=True)
        for kind in KINDS:
            a, b, f = med[f"{kind} product + gradient flag off"], med[f"{kind} product + gradient XK_DIST_GRAD"], med[f"{kind} forward (XK_DIST)"]
            print(f"  {D:5d} {kind} product + gradient: flag off / XK_DIST_GRAD = {a[0] / b[0]:.2f} (spread of flag off {a[1]:.3f} ms, gain {a[0] - b[0]:.3f} ms); "
                  f"XK_DIST_GRAD / forward = {b[0] / f[0]:.2f}", flush=True)
        print(f"  {D:5d} relative error on {rows.numel()} rows against float64 (flag off, XK_DIST_GRAD): soft-min p=1 {errs['soft-min p=1'][0]:.3e}, {errs['soft-min p=1'][1]:.3e}; "
              f"laplacian / |v| gradient {errs['laplacian'][0]:.3e}, {errs['laplacian'][1]:.3e}; energy {errs['energy'][0]:.3e}, {errs['energy'][1]:.3e}", flush=True)
        del x, y, h, v, g, fwd
    n = args.loss_n
    if args.loss_dims:
        print(f"# online SamplesLoss forward + backward (dL/dx), N = M = {n}; _XK_GRAD (GEOMLOSS_HIP_XK_GRAD) on / off, alternated")
    for D in args.loss_dims:
        gen = torch.Generator().manual_seed(n + D)
        x, y = torch.rand(n, D, generator=gen).to(dev), (torch.rand(n, D, generator=gen) * 0.8 + 0.1).to(dev)
        for name, loss_fn in (("sinkhorn p=1", SamplesLoss("sinkhorn", p=1, blur=0.3, backend="online")),
                              ("laplacian", SamplesLoss("laplacian", blur=0.5, backend="online")), ("energy", SamplesLoss("energy", backend="online"))):
            last = {}

            def run(on):
                sinkhorn_samples._XK_GRAD = kernel_samples._XK_GRAD = on
                xg = x.clone().requires_grad_(True)
                L = loss_fn(xg, y)
                (gx,) = torch.autograd.grad(L, [xg])
                last[on] = (float(L.detach()), gx)

            launches = [(f"SamplesLoss {name} fwd+bwd off", lambda: run(False)), (f"SamplesLoss {name} fwd+bwd on", lambda: run(True))]
            ms = alternate(launches, args.rounds, args.warmup)
            sinkhorn_samples._XK_GRAD = kernel_samples._XK_GRAD = True
            med = {nm: report(D, nm, ms[nm], float(2 * n) * (2 * n)) for nm, _ in launches}
            a, b = med[launches[0][0]], med[launches[1][0]]
            diff = float((last[True][1] - last[False][1]).abs().max() / last[False][1].abs().max())
            print(f"  {D:5d} {name}: off / on = {a[0] / b[0]:.2f} (spread of off {a[1]:.3f} ms, gain {a[0] - b[0]:.3f} ms); loss {last[True][0]!r} / {last[False][0]!r}; "
                  f"max|dL/dx on - off| / max|dL/dx| = {diff:.2e}", flush=True)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
