"""Host-only check of the split arithmetic of the plan-application kernel (tools/plan_apply_model.py restates the two f16 pieces, the
three kept piece products and the per-tile column scales of geomloss_amd/csrc/glhip_plan_apply.h): on the inputs of the GPU parity and feature-range tests
(tests/test_plan_apply_gpu.py) the matrix product alone — exact float64 plan weights rounded to fp32, then split — stays within 1e-6
of max_i sum_j w_ij |feat_jv| in every feature column: 1/20 of the GPU bar of 2e-5, which therefore remains a statement about the
exponents."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import plan_apply_model as pam  # noqa: E402

SHAPES = [(300, 257, 3, 1), (1030, 1100, 2, 33), (200, 300, 1, 32), (64, 8, 3, 5), (1, 1, 3, 3), (5, 3000, 2, 70), (130, 600, 8, 40),
          (97, 513, 16, 31), (257, 300, 5, 129)]


def _eps(D):
    return 0.01 if D <= 3 else 0.1 * D / 3


def test_pieces_and_scales():
    rng = np.random.default_rng(0)
    v = (rng.standard_normal(4096) * 3000.0).astype(np.float32)
    hi, lo = pam.split2(v)
    assert (np.abs(v - (hi + lo)) <= np.maximum(2.0 ** -23 * np.abs(v), 2.0 ** -25)).all()      # glhip_klayout.h: split2_h
    m = (rng.standard_normal(4096) * 10.0 ** rng.integers(-25, 25, 4096)).astype(np.float32)
    scaled = np.abs(m).astype(np.float64) * np.ldexp(1.0, pam.scale_exponent(np.abs(m)) - 127)
    assert ((scaled >= 2.0 ** 14) & (scaled < 2.0 ** 15)).all()                                  # inside the clamp (|f| > 2^-99): the tile maximum lands in [2^14, 2^15)


@pytest.mark.parametrize("N,M,D,V", SHAPES)
def test_matrix_part_on_the_parity_inputs(N, M, D, V):
    x, y, h = pam._clouds(N + M + D, N, M, D)
    feat = np.random.default_rng(V).standard_normal((M, V)).astype(np.float32)
    err = pam.matrix_part_error(pam.weights(x, y, h, _eps(D)), feat, 64 if V % 128 > 64 or V >= 128 else 128)
    print(f"N={N} M={M} D={D} V={V}: worst column {err.max():.2e}")
    assert err.max() <= 1e-6


@pytest.mark.parametrize("eps", [0.01, 0.0025])
def test_matrix_part_on_the_feature_range_inputs(eps):
    N, M, D = 300, 257, 3
    x, y, h = pam._clouds(0, N, M, D)
    rng = np.random.default_rng(1)
    feat = rng.standard_normal((M, 6)).astype(np.float32)
    feat[:, 0] *= 1e12
    feat[:, 1] *= 1e-12
    feat[:, 3] = 0.0
    feat[:, 4] = 2.5
    feat[:, 5] = np.abs(feat[:, 5])
    w = pam.weights(x, y, h, eps)
    err = pam.matrix_part_error(w, feat)
    print(f"eps={eps}: per column {err}")
    assert pam.matrix_part_error(w, feat, 64).max() <= 1e-6
    assert err.max() <= 1e-6
    out = pam.product(w, feat)
    assert (out[:, 3] == 0.0).all()
