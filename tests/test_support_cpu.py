"""Host-side checks of the two helper modules next to the tests, tests/prune_support.py and tests/cloud_support.py, on CPU tensors: the
acceptance rule ``close`` accepts and refuses what it says, ``clouds`` is the formula it replaces with and without its ``offset``,
``covered`` reads an interval record, ``law`` draws x, y and the noise of h in that order."""
import math

import numpy as np
import pytest
import torch

import cloud_support as cs
import prune_support as ps

NAN, INF = math.nan, math.inf


def _refuses(a, b, diam2, **kw):
    with pytest.raises(AssertionError):
        ps.close(torch.tensor(a), torch.tensor(b), diam2, **kw)


def test_close_compares_the_special_values():
    v = [1.0, NAN, INF, -INF, 2.0]
    assert ps.close(torch.tensor(v), torch.tensor(v), 3.0) == (0.0, 4e-7 * 3.0 + 2e-6 * 2.0)
    _refuses(v, [NAN, 1.0, INF, -INF, 2.0], 3.0)            # a NaN moved
    _refuses(v, [1.0, NAN, -INF, -INF, 2.0], 3.0)           # +inf against -inf
    _refuses(v, [1.0, NAN, INF, INF, 2.0], 3.0)
    _refuses(v, [1.0, NAN, 3e38, -INF, 2.0], 3.0)           # an infinity against a large finite value
    _refuses([1.0, NAN, 3e38, -INF, 2.0], v, 3.0)


def test_close_holds_the_bound():
    b = torch.tensor([1.0, -2.0, 0.5, 4.0])
    bound = 4e-7 * 3.0 + 2e-6 * 4.0                          # 9.2e-6: between 77 and 78 float32 ulp of 1.0
    assert 77 * 2.0**-23 < bound < 78 * 2.0**-23
    below, above = b.clone(), b.clone()
    below[0] = 1.0 + 77 * 2.0**-23
    above[0] = 1.0 + 78 * 2.0**-23
    assert ps.close(below, b, 3.0) == (77 * 2.0**-23, bound)
    with pytest.raises(AssertionError):
        ps.close(above, b, 3.0)


def test_close_without_a_finite_entry():
    v = torch.tensor([NAN, INF, -INF, NAN])
    assert ps.close(v, v.clone(), 3.0) is None
    _refuses(v.tolist(), v.tolist(), 3.0, require_finite=True)
    assert ps.close(torch.tensor([NAN, 1.0]), torch.tensor([NAN, 1.0]), 3.0, require_finite=True) == (0.0, 4e-7 * 3.0 + 2e-6)


def test_clouds_is_its_formula_and_a_zero_offset_changes_no_bit():
    seed = 3
    a, b = cs.clouds(seed, 5, 7, 3), cs.clouds(seed, 5, 7, 3, offset=0.0)
    rng = np.random.default_rng(seed)
    x = rng.random((5, 3)).astype(np.float32)
    y = (rng.random((7, 3)) * 0.8 + 0.1).astype(np.float32)
    h = rng.standard_normal(7).astype(np.float32)
    for got, again, want in zip(a, b, (x, y, h)):
        assert got.dtype == again.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(again.view(np.uint32), want.view(np.uint32))
    moved = cs.clouds(seed, 5, 7, 3, offset=100.0)
    assert moved[0].dtype == np.float32 and np.array_equal(moved[0], x + np.float32(100.0)) and np.array_equal(moved[2], h)
    xb, yb, hb = cs.clouds(seed, 5, 7, 3, B=2)
    assert xb.shape == (2, 5, 3) and yb.shape == (2, 7, 3) and hb.shape == (2, 7)


def test_covered_reads_the_non_empty_intervals():
    assert ps.pm.BLOCK == 256
    rec = {"intervals": np.array([[[256, 700], [900, 900]]], np.int32)}      # one slab: columns 256 .. 699, and an empty slot
    assert np.array_equal(ps.covered(rec, 0, 5), [False, True, True, False, False])


def test_law_draws_x_then_y_then_the_noise(monkeypatch):
    monkeypatch.setattr(ps, "DEV", torch.device("cpu"))
    seed = 5
    for D, dtype, noise in ((3, torch.float32, 0.01), (2, torch.bfloat16, 0.01), (3, torch.float32, 0.001)):
        kw = {} if D == 3 and noise == 0.01 else dict(D=D, dtype=dtype, noise=noise)
        x, y, h = ps.law(8, 9, seed, **kw)
        g = torch.Generator().manual_seed(seed)
        x0 = torch.rand(1, 8, D, generator=g)
        y0 = torch.rand(1, 9, D, generator=g)
        h0 = torch.full((1, 9), -math.log(9)) + noise * torch.randn(1, 9, generator=g) / (0.05**2)
        assert x.shape == (1, 8, D) and y.shape == (1, 9, D) and h.shape == (1, 9)
        assert x.dtype == y.dtype == dtype and h.dtype == torch.float32
        assert torch.equal(x, x0.to(dtype)) and torch.equal(y, y0.to(dtype)) and torch.equal(h, h0)
        assert x.is_contiguous() and y.is_contiguous() and h.is_contiguous()
