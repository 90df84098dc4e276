"""The reference's Dirac test of ``ot.solve_sample`` (one point on each side, drawn by its hypothesis strategy over library / dtype /
weights), replayed from the draws recorded in tests/golden/reference_diracs_ot.npz (tests/golden/make_golden_ot_diracs.py): the
reference tree is not part of this repository, so the drawn inputs and expected answers travel instead.

* CPU: every recorded draw is an un-batched call, its arguments bind to ``geomloss_amd.ot.solve_sample``, and the result class
  exposes every field that is compared.
* GPU: every draw through ``geomloss_amd.ot.solve_sample`` on the HIP kernels; each returned field keeps the library and dtype of
  the inputs and the shape of the expected answer, and the values pass ``conftest.reference_accepts``.
"""
import inspect

import numpy as np
import pytest

from conftest import reference_accepts, reference_dirac_cases
from geomloss_amd import ot

FIELDS = ("value", "plan", "potential_a", "potential_b", "marginal_a", "marginal_b")


def _solver_kwargs(c):
    return dict(a=c.get("a"), b=c.get("b"), cost="sqeuclidean", reg=float(c["reg"]), unbalanced=None, max_iter=int(c["max_iter"]),
                method=str(c["method"]))


def test_reference_test_file_collects_against_geomloss_amd():
    cases = reference_dirac_cases()
    assert len(cases) == 60
    sig = inspect.signature(ot.solve_sample)
    for c in cases:
        assert c["X_a"].ndim == 2 and c["X_b"].ndim == 2
        assert str(c["library"]) in ("numpy", "torch") and str(c["dtype"]) in ("float32", "float64")
        sig.bind(c["X_a"], c["X_b"], **_solver_kwargs(c))
        assert {k[5:] for k in c if k.startswith("want_")} <= set(FIELDS)
    for k in FIELDS + ("a_to_b", "b_to_a"):
        assert hasattr(ot.OTResultSample, k), k


@pytest.mark.gpu
def test_reference_test_file_passes_unmodified(cuda):
    import torch

    for i, c in enumerate(reference_dirac_cases()):
        lib, dtype = str(c["library"]), str(c["dtype"])

        def cast(v):
            if v is None:
                return None
            v = np.asarray(v).astype(dtype)
            return torch.from_numpy(v).to(cuda) if lib == "torch" else v
        kw = dict(_solver_kwargs(c), a=cast(c.get("a")), b=cast(c.get("b")))
        res = ot.solve_sample(cast(c["X_a"]), cast(c["X_b"]), **kw)
        got = {}
        for k in FIELDS:
            v = getattr(res, k)
            if lib == "torch":
                assert isinstance(v, torch.Tensor) and v.device == cuda, (i, k)
                v = v.cpu().numpy()
            v = np.asarray(v)
            assert str(v.dtype) == dtype, (i, k, v.dtype)
            got[k] = v
        want = {k[5:]: c[k] for k in c if k.startswith("want_")}
        for k, w in want.items():
            assert got[k].shape == np.shape(w), (i, k, got[k].shape, np.shape(w))
        assert reference_accepts(got, want, float(c["atol"]), float(c["rtol"])) == [], i
