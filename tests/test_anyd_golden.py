"""Pins the CPU oracles to the reference in dimension D > 16: tests/golden/reference_anyd_*.npz were produced by jeanfeydy/geomloss
0.3.1 (tensorized backend, float64) — see tests/golden/make_golden_anyd.py.  CPU only; the kernels meet the same fixtures in
tests/test_anyd_kernels_gpu.py."""

import numpy as np
import pytest
import torch

from conftest import load_golden, relerr
from oracle import oracle_np, oracle_torch64

CPU = torch.device("cpu")
CASES = ["sinkhorn_d32", "sinkhorn_d128", "gaussian_d128"]


def _load(name):
    rec = load_golden("reference_anyd_" + name)
    kw = dict(rec["kwargs"])
    return rec, kw.pop("loss"), kw


@pytest.mark.parametrize("name", CASES)
def test_fixtures_are_what_the_generator_describes(name):
    rec, loss, kw = _load(name)
    D = int(name.rsplit("_d", 1)[1])
    assert rec["x"].shape == (300, D) and rec["y"].shape == (400, D) and rec["x"].dtype == np.float32
    assert abs(rec["a"].sum() - 1) < 1e-5 and rec["a"].std() > 0 and abs(kw["blur"] - 0.3 * np.sqrt(D / 3)) < 1e-12
    assert rec["gx_f64"].shape == (300, D) and rec["F_f64"].size == 300 and rec["G_f64"].size == 400


@pytest.mark.parametrize("name", CASES)
def test_numpy_oracle_matches_reference_f64(name):
    rec, loss, kw = _load(name)
    a, x, b, y = rec["a"], rec["x"], rec["b"], rec["y"]
    if loss == "sinkhorn":
        L, gx, ga = oracle_np.sinkhorn_loss_and_grad(x, y, a, b, **kw)
        F, G = oracle_np.sinkhorn_loss(x, y, a, b, potentials=True, **kw)
        assert relerr(ga, rec["ga_f64"]) < 1e-7
    else:
        L = oracle_np.kernel_loss(loss, x, y, a, b, blur=kw["blur"])
        gx = oracle_np.kernel_loss_grad_x(loss, x, y, a, b, blur=kw["blur"])
        F, G = oracle_np.kernel_loss(loss, x, y, a, b, blur=kw["blur"], potentials=True)
    assert relerr(L, rec["loss_f64"]) < 1e-8
    assert relerr(gx, rec["gx_f64"]) < 1e-7
    assert relerr(F, rec["F_f64"]) < 1e-7 and relerr(G, rec["G_f64"]) < 1e-7


@pytest.mark.parametrize("name", CASES)
def test_chunked_f64_oracle_matches_reference_f64(name):
    rec, loss, kw = _load(name)
    a, x, b, y = rec["a"], rec["x"], rec["b"], rec["y"]
    if loss == "sinkhorn":
        L, gx, ga = oracle_torch64.sinkhorn_loss(x, y, a, b, grad=True, device=CPU, **kw)
        F, G = oracle_torch64.sinkhorn_loss(x, y, a, b, potentials=True, device=CPU, **kw)
    else:
        L, gx, ga = oracle_torch64.kernel_loss(loss, x, y, a, b, blur=kw["blur"], grad=True, device=CPU)
        F, G = oracle_torch64.kernel_loss(loss, x, y, a, b, blur=kw["blur"], potentials=True, device=CPU)
    assert relerr(L, rec["loss_f64"]) < 1e-8
    assert relerr(gx, rec["gx_f64"]) < 1e-7 and relerr(ga, rec["ga_f64"]) < 1e-7
    assert relerr(F, rec["F_f64"]) < 1e-7 and relerr(G, rec["G_f64"]) < 1e-7
