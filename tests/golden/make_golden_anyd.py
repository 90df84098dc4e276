"""Generates tests/golden/reference_anyd_<case>.npz: the REFERENCE implementation (jeanfeydy/geomloss 0.3.1, mounted read-only at
/root/reference) on clouds of dimension D > 16, ``SamplesLoss(backend="tensorized")`` in float64 on the CPU.  Run once in the build
container:

    python tests/golden/make_golden_anyd.py

Inputs are drawn in float32 (what the kernels see) and handed to the reference as float64.  The `reference_` prefix keeps the files
out of ``conftest.golden_cases()``; tests/test_anyd_golden.py (oracles) and tests/test_anyd_kernels_gpu.py (kernels) read them.
Only this script reads /root/reference.
"""

import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, "/root/reference/src")
import geomloss  # noqa: E402  (the reference)

assert geomloss.__version__ == "0.3.1"
OUT = os.path.dirname(os.path.abspath(__file__))
N, M = 300, 400

CASES = {
    # name: (loss, D, seed)
    "sinkhorn_d32": ("sinkhorn", 32, 41),
    "sinkhorn_d128": ("sinkhorn", 128, 42),
    "gaussian_d128": ("gaussian", 128, 43),
}


def main():
    torch.set_num_threads(4)
    for name, (loss, D, seed) in CASES.items():
        g = torch.Generator().manual_seed(seed)
        x = torch.rand(N, D, generator=g)
        y = torch.rand(M, D, generator=g) * 0.9 + 0.05
        a = torch.rand(N, generator=g) + 0.1
        b = torch.rand(M, generator=g) + 0.1
        a, b = (a / a.sum()).float(), (b / b.sum()).float()
        kw = dict(loss=loss, blur=0.3 * math.sqrt(D / 3))
        if loss == "sinkhorn":
            kw.update(p=2, scaling=0.5)
        xd, yd, ad, bd = x.double().requires_grad_(True), y.double(), a.double().requires_grad_(True), b.double()
        L = geomloss.SamplesLoss(backend="tensorized", **kw)(ad, xd, bd, yd)
        gx, ga = torch.autograd.grad(L, [xd, ad])
        F, G = geomloss.SamplesLoss(backend="tensorized", potentials=True, **kw)(ad.detach(), xd.detach(), bd, yd)
        np.savez_compressed(os.path.join(OUT, f"reference_anyd_{name}.npz"), x=x.numpy(), y=y.numpy(), a=a.numpy(), b=b.numpy(),
                            kwargs=repr(kw), loss_f64=L.detach().numpy(), gx_f64=gx.numpy(), ga_f64=ga.numpy(), F_f64=F.detach().numpy(),
                            G_f64=G.detach().numpy())
        print(name, "loss f64", float(L))


if __name__ == "__main__":
    main()
