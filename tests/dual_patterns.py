"""Dual vectors built to make a row's running maximum arrive late, grow often or never arrive, for the kernels that carry weighted sums
(tests/test_hostile_duals_gpu.py), with the host-side checks that they do what they are for (tests/test_dual_patterns_cpu.py).

NumPy only.  Every pattern is a valid input of the C-ABI: finite values and -inf, no NaN, no +inf.  The clouds and temperatures are those
of the parity tests of the entry points, imported where they are used (``clouds``)."""
import numpy as np

ONE_HOT = ("late", "stairs")
SPREAD = ("ramp", "descent", "twin", "lead_void", "tail_void", "half_void", "floors")
VOIDS = ("lead_void", "tail_void", "half_void")
F64_ONLY = ("stairs600", "stairs400")
SHAPES = ((300, 300), (130, 5000))      # unsplit; with column splits
CONFIGS = ((3, 2), (5, 2), (8, 2), (16, 2), (24, 2), (70, 2), (3, 1), (8, 1), (33, 1))      # (D, p): every cloud the GPU test takes a one-hot row's column from
GROUP = 32


def _stairs(M, step, width, cliff, spike):
    h = (np.arange(M) // width * float(step)).astype(np.float32)
    h[M // 2:] -= cliff
    h[M - 3] = spike
    return h


def patterns(M, rng):
    """name -> float32 dual vector of length M."""
    j = np.arange(M)
    normal = lambda: rng.standard_normal(M).astype(np.float32)      # noqa: E731
    out = {}
    out["late"] = np.full(M, -50.0, np.float32)
    out["late"][M - 1] = 80.0
    out["stairs"] = _stairs(M, 48.0, 64, 3000.0, 5000.0)      # the stress vector of test_softmin_lazy_max_and_infinities
    R = min(256, M)
    out["ramp"] = np.zeros(M, np.float32)
    out["ramp"][M - R:] = np.arange(R, dtype=np.float32)
    out["descent"] = (-0.25 * j).astype(np.float32)
    out["twin"] = np.full(M, -50.0, np.float32)
    out["twin"][[3, M - 2]] = 80.0
    out["lead_void"] = normal()
    out["lead_void"][:160] = -np.inf      # more than one 128-column tile plus a group
    out["tail_void"] = normal()
    out["tail_void"][M - 160:] = -np.inf
    out["half_void"] = normal()
    out["half_void"][:M // 2] = -np.inf      # whole column splits without mass at the split shape
    out["floors"] = normal()
    out["floors"][0::3] = -100000.0      # the reference's two stand-ins for log(0)
    out["floors"][1::3] = -10000.0
    out["stairs600"] = _stairs(M, 600.0, 100, 30000.0, 50000.0)      # float64 kernels only: every step is past the e^500 threshold
    out["stairs400"] = _stairs(M, 400.0, 100, 30000.0, 50000.0)      # terms between e^0 and e^500 above the lazy maximum, then a rescale
    for name, h in out.items():
        assert h.dtype == np.float32 and h.shape == (M,) and not np.isnan(h).any() and not np.isposinf(h).any(), name
    return out


def feature_patterns(M, V, rng):
    """Standard normal (M, V) float32 with, where it has them: column 0 spanning 24 decades along j with random signs, column 1 times
    1e12, column 2 times 1e-12, column 3 zero, column 4 constant 2.5."""
    feat = rng.standard_normal((M, V))
    sign = np.where(rng.random(M) < 0.5, -1.0, 1.0)
    if V > 0:
        feat[:, 0] = 10.0 ** (np.arange(M) / M * 24 - 12) * sign
    if V > 1:
        feat[:, 1] *= 1e12
    if V > 2:
        feat[:, 2] *= 1e-12
    if V > 3:
        feat[:, 3] = 0.0
    if V > 4:
        feat[:, 4] = 2.5
    return feat.astype(np.float32)


def clouds(D, p, N, M):
    """(x, y, eps): the clouds and temperature of the entry points' own parity tests at this dimension — p = 2:
    tests/test_plan_apply_gpu.py (D <= 16) / tests/test_plan_apply_nd_gpu.py; p = 1: tests/test_plan_apply_p1_gpu.py."""
    if p == 2:
        if D <= 16:
            from test_plan_apply_gpu import _clouds, _eps
        else:
            from test_plan_apply_nd_gpu import _clouds, _eps
        x, y, _ = _clouds(N + M + D, N, M, D)
    else:
        from test_plan_apply_p1_gpu import _eps, _law
        x, y, _ = _law(np.random.default_rng(N + M + D), N, M, D)
    return x, y, float(_eps(D))


def log_weights(x, y, h, eps, p):
    """float64 (N, M): h_j - C_ij / eps with C = |x - y|^2 / 2 (p = 2) or sqrt(max(|x - y|^2, 1e-8)) (p = 1), on explicit differences."""
    x, y, h = (np.asarray(t, np.float64) for t in (x, y, h))
    E = np.empty((x.shape[0], y.shape[0]))
    rows = max(1, int(4e6 // max(1, y.size)))
    for i0 in range(0, x.shape[0], rows):
        diff = x[i0:i0 + rows, None, :] - y[None, :, :]
        d2 = (diff * diff).sum(-1)
        E[i0:i0 + rows] = h[None, :] - (0.5 * d2 if p == 2 else np.sqrt(np.maximum(d2, 1e-8))) / eps
    return E


def relative_weights(E):
    """exp(E - rowmax) in float64; a row without mass is all zero."""
    m = E.max(1, keepdims=True)
    return np.exp(E - np.where(np.isfinite(m), m, 0.0))


def reference(E, feat):
    """float64: (row-normalised weights @ feat, log of the row sums); ``feat`` (M, V), or a callable (j0, j1) -> (N, j1 - j0, V) for
    features that depend on the row (the unit directions of a p = 1 gradient)."""
    m = E.max(1)
    m = np.where(np.isfinite(m), m, 0.0)
    W = np.exp(E - m[:, None])
    s = W.sum(1)
    if callable(feat):
        out = sum(np.einsum("nj,njv->nv", W[:, j0:j0 + 256], feat(j0, min(j0 + 256, E.shape[1]))) for j0 in range(0, E.shape[1], 256))
    else:
        out = W @ np.asarray(feat, np.float64)
    with np.errstate(divide="ignore"):
        return out / np.where(s > 0, s, 1.0)[:, None], m + np.log(s)


def plan_model(E, feat, rescale=True, group=GROUP):
    """float64 model of the accumulation the plan half of the matrix-core kernels performs (glhip_plan_apply.h): the columns go in groups
    of ``group``; a group's weights are 2^(u - m) against the running maximum m of the row, which takes the group in first; when m grows
    the running sums are brought to the new m.  ``rescale=False`` leaves that step out: what a kernel computes whose rescale is broken.
    Returns (out, log of the row sums, how many groups made m grow per row)."""
    U = np.asarray(E, np.float64) * np.log2(np.e)
    N, M = U.shape
    m, s, acc, grew = np.full(N, -np.inf), np.zeros(N), None, np.zeros((N, (M + group - 1) // group), bool)
    for k, j0 in enumerate(range(0, M, group)):
        u = U[:, j0:j0 + group]
        mg = np.maximum(m, u.max(1))
        grew[:, k] = mg > m
        with np.errstate(invalid="ignore"):
            f = np.where(np.isfinite(m), np.exp2(m - mg), 0.0)
            w = np.where(np.isfinite(mg)[:, None], np.exp2(u - mg[:, None]), 0.0)
        fj = feat(j0, min(j0 + group, M)) if callable(feat) else None
        part = np.einsum("nj,njv->nv", w, fj) if callable(feat) else w @ np.asarray(feat[j0:j0 + group], np.float64)
        if acc is None:
            acc = np.zeros_like(part)
        if rescale:
            s, acc = s * f, acc * f[:, None]
        s, acc, m = s + w.sum(1), acc + part, mg
    with np.errstate(divide="ignore"):
        return acc / np.where(s > 0, s, 1.0)[:, None], (np.where(np.isfinite(m), m, 0.0) + np.log2(s)) / np.log2(np.e), grew


# The flat bounds the GPU test asserts, each from the parity test of its entry point (none is set here)
PLAN_BOUND = 2e-5           # per-column _worst: test_parity of tests/test_plan_apply_gpu.py, test_plan_apply_nd_gpu.py, test_plan_apply_p1_gpu.py
PLAN_MASS_BOUND = 1e-4      # |mass - 1|: the same tests
# Split against unsplit, the one comparison of a kernel with itself: only where the entry point's own split test states a bound for it.
SPLIT_BOUND = {
    "plan xd": 2e-6,        # tests/test_plan_apply_gpu.py::test_column_splits_and_long_reductions (agree)
    "plan p1": 2e-5,        # tests/test_plan_apply_p1_gpu.py::test_column_splits (between <= BOUND)
    "grad p2 xk": 2e-5,     # tests/test_softmin_grad_xk_gpu.py::test_column_splits (among the runs), FLAG_XK_GRAD
    "grad p1 xk": 1e-5,     # tests/test_dist_grad_xk_gpu.py::test_column_splits (2 x BOUND), FLAG_XK_DIST_GRAD
}
# (tests/test_plan_apply_nd_gpu.py::test_column_splits prints that figure and asserts none, and the gradient kernels of D <= 16 and the
# one-thread-per-row kernels are held against the oracle alone in their split tests: every variant of those routes is compared with float64 here,
# none with another)
F64_VALUE_BOUND, F64_GRAD_BOUND = 1e-12, 1e-11      # tests/test_f64_gpu.py::test_f64_softmin_and_gradient_vs_c_oracle


def grad_bound(D, p=2):
    """relerr of the soft-min gradient: 2e-5 for D <= 16 (tests/test_hip_kernels.py::test_softmin_bwd_vs_oracle, tests/test_xd_kernels_gpu.py::
    test_softmin_gradient_transposed_kernel); 5e-6 beyond (tests/test_softmin_grad_xk_gpu.py::_bound, tests/test_dist_grad_xk_gpu.py::BOUND)."""
    return 2e-5 if D <= 16 else 5e-6


def p1_value_bound(ref, D):
    """|out - ref| of the p = 1 soft-min: 2e-6 max(1, |ref|max) for D <= 16 (tests/test_hip_kernels.py, the dense distance reductions),
    12 times that beyond (tests/test_dist_xk_gpu.py::_sbound, tests/test_plan_apply_p1_gpu.py::_sbound)."""
    fin = np.asarray(ref)[np.isfinite(ref)]
    return (1 if D <= 16 else 12) * 2e-6 * max(1.0, float(np.abs(fin).max()) if fin.size else 1.0)
