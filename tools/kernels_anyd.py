"""GPU box: raw launches of the reductions for clouds of dimension D > 16 (csrc/glhip_softmin_xk.h, csrc/glhip_generic.h), timed with
HIP events: soft-min forward at D in {16, 32, 64, 128, 256} with flags 0 and GLHIP_FLAG_F16X2, gaussian product at D = 64, soft-min
gradient at D = 64 and 128; N = M = 2e5, float32.  Medians over --launches launches after --warmup warm-up launches.

    python tools/kernels_anyd.py                                   # the build in the tree
    GEOMLOSS_HIP_LIB=/path/to/another/libgeomloss_hip.so python tools/kernels_anyd.py      # another build of the same C-ABI (A/B)
    python tools/kernels_anyd.py --trace                           # two launches of each, no timing: the workload for rocprofv3

One line per reduction: median and min in ms, pairs per second, and for the forward the family the library reports (where it can)."""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from geomloss_amd import hip  # noqa: E402

FAMILIES = {0: "valu", 1: "x32", 2: "xd", 3: "xk", 4: "dist", 5: "generic"}


def timed(fn, launches, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dims", type=int, nargs="*", default=[16, 32, 64, 128, 256])
    ap.add_argument("--trace", action="store_true", help="two launches of each reduction, no timing")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    path = os.environ.get("GEOMLOSS_HIP_LIB")
    if path:      # an older build of the same C-ABI predates the host-side queries: bind what it exports
        old = ctypes.CDLL(path)
        for name in [k for k in hip.SIGNATURES if k.endswith("_family") and not hasattr(old, k)]:
            del hip.SIGNATURES[name]
    lib = hip.load_library()
    n = args.n
    launches, warmup = (2, 0) if args.trace else (args.launches, args.warmup)
    print(f"# libgeomloss_hip {lib.glhip_version()} ({os.environ.get('GEOMLOSS_HIP_LIB', 'tree build')}); N = M = {n}, float32; "
          f"median (min) of {launches} launches after {warmup}; {torch.cuda.get_device_name(0)}")

    def report(name, D, flags, fn):
        med, lo = timed(fn, launches, warmup)
        fam = ""
        if name == "softmin fwd" and hasattr(lib, "glhip_softmin_fwd_family"):
            fam = "  family: " + FAMILIES.get(lib.glhip_softmin_fwd_family(1, n, n, D, 2, hip.F32, flags, 0), "?")
        print(f"{name:18s} D={D:4d} flags={flags:4d}  {med:9.3f} ms (min {lo:9.3f})  {n * n / med / 1e9:8.3f}e12 pairs/s{fam}", flush=True)

    for D in args.dims:
        g = torch.Generator().manual_seed(D)
        x = torch.rand(1, n, D, generator=g).to(dev)
        y = torch.rand(1, n, D, generator=g).to(dev)
        h = (torch.randn(1, n, generator=g) * 2).to(dev)
        eps = 0.05**2 * D / 3
        for flags in (0, hip.FLAG_F16X2):
            report("softmin fwd", D, flags, lambda: hip.softmin_fwd_raw(x, y, h, eps, 2, None, flags))
        if D == 64:
            v = (torch.rand(1, n, generator=g) / n).to(dev)
            report("gaussian product", D, 0, lambda: hip.kernel_conv_fwd_raw(hip.GAUSSIAN, x, y, v, 0.05 * (D / 3) ** 0.5, None, 0))
        if D in (64, 128):
            out = hip.softmin_fwd_raw(x, y, h, eps, 2)
            go = torch.ones(1, n, device=dev)
            try:
                report("softmin bwd_x", D, 0, lambda: hip.softmin_bwd_x_raw(x, y, h, out, go, eps, 2, None, 0))
            except NotImplementedError as e:      # an older build: no gradient beyond D = 64
                print(f"softmin bwd_x      D={D:4d}: {e}")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
