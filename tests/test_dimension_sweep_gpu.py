"""Every compiled (D <= 16) and run-time (17 <= D <= 4095) dimension of the HIP kernels against float64.

One function per entry point; each loops over D = 1..130 (all sixteen compiled dimensions, both sides of the 16 | 17 hand-over, every
residue of the 24-slot group, the MFMA count and the 6-MFMA stage of ``glhip_softmin_xk.h`` on both K layouts through the fourth
f16 x 2 stage edge 126 | 127) and, where the entry point's limit is 4095, over D = 255, 256, 257, 1024, 4095 at the unbatched shape.

Inputs, one law for every entry point, ``rng = default_rng(D)``: per-coordinate scales ``s = 0.5 + 0.5 rng.random(D)`` (coordinates are
not exchangeable: a wrong slot pairing changes the result), ``x = rng.random((N, D)) s``, ``y = (0.8 rng.random((M, D)) + 0.1) s``,
``h = rng.standard_normal(M)``, all float32; diam^2 <= D, so the suite's bounds apply with D put into their formulas.  Shapes:
(N, M) = (70, 150) unbatched (a partial row block, two column tiles with a partial last one, a partial last group of 32) and
B = 2, (N, M) = (33, 40) (the per-item strides b N D).

References are float64 only: ``oracle.oracle_c`` where it covers the operation (its gradients keep 64 accumulators: D > 64 gradients
come from ``oracle.oracle_torch64`` on the host), the float64 restatements of tests/test_plan_apply_gpu.py (``_ref``, ``_worst``) and
tests/test_argmin_gpu.py (``cost64``, ``tol_of``, the criterion of ``judge``) for the rest.  No HIP kernel is compared with another.

The sweep has no tolerance of its own: every bound is the bound of the existing test of that entry point (named beside it), at the
temperature that test states its bound for.  Before a launch the library's own host-side predicates must name the expected kernel
family.  Once per D, on the host alone, each function checks that it has teeth: the float64 result computed WITHOUT the last coordinate
differs from the full one by at least ``TEETH`` x the bound in use (the power of ten is stated beside each function; the host parts
are the ``_host_*`` functions, which need no GPU).  Violations are collected as (D, variant, error / bound) and asserted once, at
the end; the worst ratio per layout and the wall time are printed (``pytest -s``; profiles/dimension_sweep.txt)."""
import functools
import math
import time

import numpy as np
import pytest
import torch

from cloud_support import tol as _tol
from conftest import relerr
from geomloss_amd import hip
from oracle import oracle_c
from oracle import oracle_torch64 as o64

pytestmark = pytest.mark.gpu

H2, NS, XK = hip.FLAG_F16X2, hip.FLAG_NO_SPLIT, hip.FLAG_XK_GRAD
DIMS = list(range(1, 131))
BIG = [255, 256, 257, 1024, 4095]
N1, M1 = 70, 150              # unbatched
B2, N2, M2 = 2, 33, 40        # batched
CPU = torch.device("cpu")


def _t(a, dev):
    return torch.tensor(np.asarray(a, dtype=np.float32)).to(dev)      # a copy: the cached clouds are read-only


@functools.lru_cache(maxsize=None)
def _case(D):
    """The clouds of dimension D: (x, y, h) unbatched and (xb, yb, hb) batched, same scales, one generator."""
    rng = np.random.default_rng(D)
    s = 0.5 + 0.5 * rng.random(D)
    x = (rng.random((N1, D)) * s).astype(np.float32)
    y = ((rng.random((M1, D)) * 0.8 + 0.1) * s).astype(np.float32)
    h = rng.standard_normal(M1).astype(np.float32)
    xb = (rng.random((B2, N2, D)) * s).astype(np.float32)
    yb = ((rng.random((B2, M2, D)) * 0.8 + 0.1) * s).astype(np.float32)
    hb = rng.standard_normal((B2, M2)).astype(np.float32)
    for a in (x, y, h, xb, yb, hb):
        a.setflags(write=False)
    return x, y, h, xb, yb, hb


def _items(D, big=False):
    """The 2-D problems of dimension D: [(tag, x, y, h)], the unbatched one first, then the items of the batch."""
    x, y, h, xb, yb, hb = _case(D)
    return [("u", x, y, h)] + ([] if big else [(f"b{b}", xb[b], yb[b], hb[b]) for b in range(B2)])


def _launches(D, dev, big=False):
    """[(tags, (x, y, h) on the device)]: the unbatched launch and the batched one; ``tags`` index the references."""
    x, y, h, xb, yb, hb = _case(D)
    out = [(("u",), tuple(_t(a, dev) for a in (x, y, h)))]
    if not big:
        out.append((tuple(f"b{b}" for b in range(B2)), tuple(_t(a, dev) for a in (xb, yb, hb))))
    return out


def _rows(t, tags):
    """A launch's output as one NumPy array per tag."""
    a = t.detach().cpu().numpy()
    return [a] if len(tags) == 1 else [a[b] for b in range(len(tags))]


def _drop(*clouds):
    return tuple(np.ascontiguousarray(c[..., :-1]) for c in clouds)


def _eps2(D):
    return 0.05**2 * D / 3                          # the suite's small p = 2 temperature


def _blur(D):
    return 0.2 * math.sqrt(D / 3)


def _layout(flags):
    return "f16x2" if flags & H2 else "bf16x3"


class _Report:
    """Collects (D, variant, error / bound) of every check of a function, fails once at the end with all of them."""

    def __init__(self, name):
        self.name, self.bad, self.worst, self.weak, self.t0, self.n = name, [], {}, [], time.perf_counter(), 0

    def add(self, D, variant, err, bound, layout="-", strict=True):
        """``strict``: the source test asserts ``err < bound``; otherwise ``err <= bound``."""
        ratio = float(err) / float(bound) if np.isfinite(err) else math.inf
        self.n += 1
        if ratio > self.worst.get(layout, (-1.0,))[0]:
            self.worst[layout] = (ratio, D, variant)
        if not (err < bound if strict else err <= bound):
            self.bad.append((D, variant, float(f"{ratio:.3g}")))

    def teeth(self, D, what, moved, factor):
        """``moved``: how far dropping the last coordinate moves the float64 reference, in units of the bound (smallest over the items)."""
        if D >= 2 and not moved >= factor:
            self.weak.append((D, what, float(f"{moved:.3g}")))

    def failures(self):
        for layout, (ratio, D, variant) in sorted(self.worst.items()):
            print(f"sweep {self.name} [{layout}]: worst error / bound {ratio:.3f} at D = {D} ({variant})")
        print(f"sweep {self.name}: {self.n} checks, {time.perf_counter() - self.t0:.1f} s")
        out = []
        if self.weak:
            out.append(f"{self.name}: the reference moves by less than the stated multiple of the bound (D, what, moved / bound): {self.weak}")
        if self.bad:
            out.append(f"{self.name}: {len(self.bad)} of {self.n} checks above their bound (D, variant, error / bound): {self.bad}")
        return out


def _finish(*reports):
    msgs = [m for r in reports for m in r.failures()]
    assert not msgs, "\n".join(msgs)


def _p2_family(D):
    return (hip.FAMILY_X32, hip.FAMILY_VALU) if D <= 3 else (hip.FAMILY_XD,) if D <= 16 else (hip.FAMILY_XK,)


def _shapes(big=False):
    return [(1, N1, M1)] if big else [(1, N1, M1), (B2, N2, M2)]


# ---- 1. hip.softmin, p = 2 -------------------------------------------------------------------------------------------------------
TEETH_SOFTMIN, TEETH_SOFTMIN_BIG = 100, 10      # D <= 130 (>= 950 on the host); the five large dimensions (>= 22): the bound grows like D, one coordinate does not


@functools.lru_cache(maxsize=None)
def _host_softmin(D):
    eps, refs, moved = _eps2(D), {}, math.inf
    for tag, x, y, h in _items(D, D in BIG):
        refs[tag] = oracle_c.softmin(eps, x, y, h, 2)
        if D >= 2:
            moved = min(moved, np.abs(oracle_c.softmin(eps, *_drop(x, y), h, 2) - refs[tag]).max() / _tol(refs[tag], D))
    return refs, moved


def test_softmin_p2(cuda):
    rep = _Report("softmin p=2")
    for D in DIMS + BIG:
        big, eps = D in BIG, _eps2(D)
        refs, moved = _host_softmin(D)
        rep.teeth(D, "softmin", moved, TEETH_SOFTMIN_BIG if big else TEETH_SOFTMIN)
        for flags in (0, NS, H2, H2 | NS):
            for B, N, M in _shapes(big):
                assert hip.softmin_fwd_family(B, N, M, D, 2, hip.F32, flags) in _p2_family(D), (D, flags)
            for tags, (x, y, h) in _launches(D, cuda, big):
                for tag, out in zip(tags, _rows(hip.softmin(eps, x, y, h, p=2, flags=flags), tags)):
                    rep.add(D, f"flags={flags} {tag}", np.abs(out - refs[tag]).max(), _tol(refs[tag], D), _layout(flags))     # _tol
    _finish(rep)


# ---- 2. hip.sinkhorn_step, p = 2 -------------------------------------------------------------------------------------------------
TEETH_STEP, TEETH_STEP_BIG = 100, 1      # D <= 130 (>= 388: half the soft-min's, the step averages with prev); the large dimensions (>= 9)
DAMPING = 0.8


def _step_extras(D, tag, N, M):
    rng = np.random.default_rng([D, 2, len(tag) + ord(tag[-1])])
    return (rng.standard_normal(M) * 0.05).astype(np.float32), rng.standard_normal(N).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _host_step(D, p=2):
    """float64: soft-min of logw (first half-step) and of logw + pot / eps (averaged half-step), per item."""
    eps, refs, moved = (_eps2(D) if p == 2 else 0.05), {}, math.inf
    for tag, x, y, h in _items(D, D in BIG):
        pot, prev = _step_extras(D, tag, x.shape[0], y.shape[0])
        hh = h.astype(np.float64) + pot.astype(np.float64) / eps
        first, soft = oracle_c.softmin(eps, x, y, h, p), oracle_c.softmin(eps, x, y, hh, p)
        refs[tag] = (DAMPING * first, soft, 0.5 * (prev.astype(np.float64) + DAMPING * soft), pot, prev)
        if D >= 2:
            bound = _tol(soft, D) if p == 2 else 2e-6 * max(1.0, np.abs(soft).max())
            moved = min(moved, 0.5 * DAMPING * np.abs(oracle_c.softmin(eps, *_drop(x, y), hh, p) - soft).max() / bound)
    return refs, moved


def test_sinkhorn_step_p2(cuda):
    rep = _Report("sinkhorn_step p=2")
    for D in DIMS + BIG:
        big, eps = D in BIG, _eps2(D)
        refs, moved = _host_step(D)
        rep.teeth(D, "half-step", moved, TEETH_STEP_BIG if big else TEETH_STEP)
        for flags in (0, H2):
            assert hip.half_step_applies(D, 2, flags), D
            for B, N, M in _shapes(big):
                assert hip.softmin_fwd_family(B, N, M, D, 2, hip.F32, flags) in _p2_family(D), (D, flags)
            for tags, (x, y, h) in _launches(D, cuda, big):
                pot = _t(np.stack([refs[t][3] for t in tags]), cuda).reshape(h.shape)
                prev = _t(np.stack([refs[t][4] for t in tags]), cuda).reshape(x.shape[:-1])
                first = _rows(hip.sinkhorn_step(eps, x, y, h, None, None, DAMPING, flags=flags), tags)
                fused = _rows(hip.sinkhorn_step(eps, x, y, h, pot, prev, DAMPING, flags=flags), tags)
                for tag, a, b in zip(tags, first, fused):
                    r1, soft, want = refs[tag][:3]
                    # test_anyd_kernels_gpu.py::test_softmin_batched_bf16_and_fused_step: _tol of the soft-min behind the step
                    rep.add(D, f"first flags={flags} {tag}", np.abs(a - r1).max(), _tol(r1, D), _layout(flags))
                    rep.add(D, f"fused flags={flags} {tag}", np.abs(b - want).max(), _tol(soft, D), _layout(flags))
    _finish(rep)


# ---- 3. hip.softmin and the fused half-step, p = 1 -------------------------------------------------------------------------------
TEETH_P1 = 100           # >= 347 on the host
P1_DIMS = list(range(1, 71))      # D <= 16: the distance kernels (D <= 3: explicit differences); 17..70: glhip_generic.h, chunks of 16 coordinates
EPS1 = 0.05                       # the eps of test_distance_reductions_xd_vs_oracle


def _p1_family(D):
    return (hip.FAMILY_VALU,) if D <= 3 else (hip.FAMILY_DIST,) if D <= 16 else (hip.FAMILY_GENERIC,)


def _p1_bound(ref, D):
    if D <= 3:
        return 4e-7 * D + 2e-6 * np.abs(ref).max()                      # tests/test_hip_kernels.py::test_softmin_fwd_vs_oracle
    # test_distance_reductions_xd_vs_oracle: 2e-6 max(1, |f|) on the MFMA distance kernel, 12 x that on the generic kernel
    return (1 if D <= 16 else 12) * 2e-6 * max(1.0, np.abs(ref).max())


@functools.lru_cache(maxsize=None)
def _host_p1(D):
    refs, moved = {}, math.inf
    step, _ = _host_step(D, 1)
    for tag, x, y, h in _items(D):
        refs[tag] = (oracle_c.softmin(EPS1, x, y, h, 1),) + step[tag]
        if D >= 2:
            moved = min(moved, np.abs(oracle_c.softmin(EPS1, *_drop(x, y), h, 1) - refs[tag][0]).max() / _p1_bound(refs[tag][0], D))
    return refs, moved


def test_softmin_p1_and_half_step(cuda):
    rep = _Report("softmin p=1")
    for D in P1_DIMS:
        refs, moved = _host_p1(D)
        rep.teeth(D, "softmin p=1", moved, TEETH_P1)
        assert hip.half_step_applies(D, 1) == (D <= 16), D
        for flags in (0, NS):
            for B, N, M in _shapes():
                assert hip.softmin_fwd_family(B, N, M, D, 1, hip.F32, flags) in _p1_family(D), (D, flags)
            for tags, (x, y, h) in _launches(D, cuda):
                pot = _t(np.stack([refs[t][4] for t in tags]), cuda).reshape(h.shape)
                prev = _t(np.stack([refs[t][5] for t in tags]), cuda).reshape(x.shape[:-1])
                f = _rows(hip.softmin(EPS1, x, y, h, p=1, flags=flags), tags)
                fused = _rows(hip.sinkhorn_step(EPS1, x, y, h, pot, prev, DAMPING, p=1, flags=flags), tags)
                for tag, a, b in zip(tags, f, fused):
                    ref, _, soft, want = refs[tag][:4]
                    rep.add(D, f"softmin flags={flags} {tag}", np.abs(a - ref).max(), _p1_bound(ref, D))
                    rep.add(D, f"half-step flags={flags} {tag}", np.abs(b - want).max(), _p1_bound(soft, D))
    _finish(rep)


# ---- 4. hip.kernel_conv ----------------------------------------------------------------------------------------------------------
# on the host, smallest over D: gaussian 805 up to D = 130 and 34 at the large dimensions; laplacian 270; energy 126 (D = 69, where the
# generic kernel's bound is 12 x wider)
TEETH_KCONV, TEETH_KCONV_BIG = 100, 10
KINDS = ("gaussian", "laplacian", "energy")


def _weights(h):
    return (np.abs(h) / h.shape[-1]).astype(np.float32)      # positive weights, as the block-sparse tests of the suite: relerr means something


def _kconv_family(kind, D):
    if kind == "gaussian":
        return _p2_family(D)
    return (hip.FAMILY_VALU,) if D <= 3 else (hip.FAMILY_DIST,) if D <= 16 else (hip.FAMILY_GENERIC,)


def _kconv_bound(kind, D, ref, absref, blur):
    """Absolute bound on |out - ref|."""
    if kind == "gaussian":      # test_xd_kernels_gpu.py / test_anyd_kernels_gpu.py::test_gaussian_product_vs_oracle, test_hip_kernels.py::test_kernel_conv_vs_oracle
        return 3e-6 * np.abs(ref).max() + 2.4e-7 * D / blur**2 * np.abs(absref).max()
    if D <= 3:
        return 3e-6 * np.abs(ref).max()                                # test_hip_kernels.py::test_kernel_conv_vs_oracle
    return (1 if D <= 16 else 12) * 5e-6 * np.abs(ref).max()           # test_distance_reductions_xd_vs_oracle (relerr; 12 x on the generic kernel)


def _kconv_dims(kind):
    return DIMS + BIG if kind == "gaussian" else P1_DIMS


@functools.lru_cache(maxsize=None)
def _host_kconv(kind, D):
    blur, refs, moved = _blur(D), {}, math.inf
    for tag, x, y, h in _items(D, D in BIG):
        v = _weights(h)
        ref = oracle_c.kconv(kind, x, y, v, blur)
        refs[tag] = (ref, _kconv_bound(kind, D, ref, ref, blur))      # v >= 0: the product of |v| is the product itself
        if D >= 2:
            moved = min(moved, np.abs(oracle_c.kconv(kind, *_drop(x, y), v, blur) - ref).max() / refs[tag][1])
    return refs, moved


def test_kernel_products(cuda):
    rep = _Report("kernel_conv")
    for kind in KINDS:
        for D in _kconv_dims(kind):
            big, blur = D in BIG, _blur(D)
            refs, moved = _host_kconv(kind, D)
            rep.teeth(D, kind, moved, TEETH_KCONV_BIG if big else TEETH_KCONV)
            for flags in ((0, NS, H2) if kind == "gaussian" else (0, NS)):
                for B, N, M in _shapes(big):
                    assert hip.kernel_conv_fwd_family(kind, B, N, M, D, hip.F32, flags) in _kconv_family(kind, D), (kind, D, flags)
                for tags, (x, y, h) in _launches(D, cuda, big):
                    v = h.abs() / h.shape[-1]
                    for tag, out in zip(tags, _rows(hip.kernel_conv(kind, x, y, v, blur, flags=flags), tags)):
                        rep.add(D, f"{kind} flags={flags} {tag}", np.abs(out - refs[tag][0]).max(), refs[tag][1], f"{kind} {_layout(flags)}")
    _finish(rep)


# ---- 5. first-order gradients in x through autograd ------------------------------------------------------------------------------
# measured on the first D - 1 coordinates of the gradient.  On the host, smallest over D: soft-min p = 2 121 (D = 130) and 5.7 at the
# large dimensions; soft-min p = 1 1330; kernel products 496
TEETH_GRAD, TEETH_GRAD_BIG = 100, 1


def _grad64(fn_c, fn_64, D, *args):
    """oracle_c keeps 64 accumulators per row: beyond, the same closed form from oracle_torch64 in float64 on the host."""
    return fn_c(*args) if D <= 64 else fn_64(*args, device=CPU)


def _gvec(D, tag, N):
    return np.random.default_rng([D, 5, len(tag) + ord(tag[-1])]).standard_normal(N).astype(np.float32)


def _softmin_grad_setups(D, p):
    """[(name, eps, flags, bound)]: each bound at the temperature its test states it for."""
    if p == 2:
        if D <= 3:        # test_hip_kernels.py::test_softmin_bwd_vs_oracle
            return [("p2", 0.01, (0, H2), 2e-5)]
        if D <= 16:       # test_xd_kernels_gpu.py::test_softmin_gradient_transposed_kernel
            return [("p2", 0.1 * D / 3, (0, NS, H2, H2 | NS), 2e-5)]
        # the generic gradient kernel: test_anyd_kernels_gpu.py::test_softmin_gradient_any_dimension (flat 5e-6 for D <= 128);
        # FLAG_XK_GRAD: test_softmin_grad_xk_gpu.py::test_parity (5e-6, and max(5e-6, 4 e_ref) for D > 64, applied below)
        return ([("p2", 0.3, (0,), 5e-6)] if D <= 130 else []) + [("p2xk", 0.1 * D / 3, (XK, XK | H2), 5e-6)]
    if D <= 3:            # test_hip_kernels.py::test_softmin_bwd_vs_oracle
        return [("p1", 0.01, (0,), 2e-5)]
    if D <= 16:           # test_xd_kernels_gpu.py::test_distance_reductions_xd_vs_oracle
        return [("p1", EPS1, (0, NS), 3e-5)]
    return [("p1", 0.3, (0,), 5e-6)]      # test_anyd_kernels_gpu.py::test_softmin_gradient_any_dimension


@functools.lru_cache(maxsize=None)
def _host_softmin_grad(D, p):
    refs, moved = {}, math.inf
    for name, eps, _, bound in _softmin_grad_setups(D, p):
        for tag, x, y, h in _items(D, D in BIG):
            g = _gvec(D, tag, x.shape[0])
            ref = _grad64(oracle_c.softmin_grad_x, o64.softmin_grad_x, D, eps, x, y, h, g, p)
            refs[name, tag] = (ref, g)
            if D >= 2:
                less = _grad64(oracle_c.softmin_grad_x, o64.softmin_grad_x, D - 1, eps, *_drop(x, y), h, g, p)
                moved = min(moved, relerr(less, ref[:, :-1]) / bound)
    return refs, moved


def _f32_error(dev, x, y, h, g, eps, ref):
    """test_softmin_grad_xk_gpu.py::_f32_error: the same gradient in plain float32 torch (expanded cost, softmax, one product)."""
    xt, yt, ht, gt = (_t(a, dev) for a in (x, y, h, g))
    C = (xt * xt).sum(1)[:, None] - 2.0 * xt @ yt.t() + (yt * yt).sum(1)[None, :]
    out = gt[:, None] * (xt - torch.softmax(ht[None, :] - C / (2.0 * eps), dim=1) @ yt)
    return relerr(out.cpu().numpy(), ref)


def _softmin_gradients(cuda, p, dims, name):
    rep = _Report(name)
    for D in dims:
        big = D in BIG
        refs, moved = _host_softmin_grad(D, p)
        rep.teeth(D, f"softmin p={p} gradient", moved, TEETH_GRAD_BIG if big else TEETH_GRAD)
        items = {tag: (x, y, h) for tag, x, y, h in _items(D, big)}
        for setup, eps, flagset, bound in _softmin_grad_setups(D, p):
            for flags in flagset:
                for B, N, M in _shapes(big):
                    assert hip.softmin_fwd_family(B, N, M, D, p, hip.F32, flags) in (_p2_family(D) if p == 2 else _p1_family(D)), (D, flags)
                    assert hip.softmin_bwd_x_uses_plan(B, N, M, D, p=p, flags=flags) == int(bool(flags & XK) and D >= 17), (D, flags)
                for tags, (x, y, h) in _launches(D, cuda, big):
                    xt = x.clone().requires_grad_(True)
                    g = _t(np.stack([refs[setup, t][1] for t in tags]), cuda).reshape(x.shape[:-1])
                    (gx,) = torch.autograd.grad(hip.softmin(eps, xt, y, h, p=p, flags=flags), [xt], grad_outputs=g)
                    for tag, out in zip(tags, _rows(gx, tags)):
                        ref = refs[setup, tag][0]
                        err, bd = relerr(out, ref), bound
                        if setup == "p2xk" and D > 64 and err >= bd:      # test_parity's rule for D > 64: four times plain float32 torch
                            bd = max(bd, 4.0 * _f32_error(cuda, *items[tag], refs[setup, tag][1], eps, ref))
                        rep.add(D, f"{setup} flags={flags} {tag}", err, bd, _layout(flags) + (" xk" if flags & XK else ""), strict=setup != "p2xk")
    return rep


def _kconv_grad_bound(kind, D):
    if D >= 17:
        return 5e-6               # test_anyd_kernels_gpu.py::test_kernel_gradient_any_dimension
    if kind == "gaussian":
        return 1e-4               # test_hip_kernels.py::test_kernel_conv_grads_vs_oracle (D <= 3), test_gaussian_gradient_and_one_pass_transposed_kernel
    return 5e-6 if D <= 3 else 3e-5      # test_kernel_conv_grads_vs_oracle; test_distance_reductions_xd_vs_oracle


@functools.lru_cache(maxsize=None)
def _host_kconv_grad(kind, D):
    blur, refs, moved = _blur(D), {}, math.inf
    for tag, x, y, h in _items(D):
        v, g = _weights(h), _gvec(D, tag, x.shape[0])
        ref = _grad64(oracle_c.kconv_grad_x, o64.kconv_grad_x, D, kind, x, y, v, g, blur)
        refs[tag] = (ref, g)
        if D >= 2:
            less = _grad64(oracle_c.kconv_grad_x, o64.kconv_grad_x, D - 1, kind, *_drop(x, y), v, g, blur)
            moved = min(moved, relerr(less, ref[:, :-1]) / _kconv_grad_bound(kind, D))
    return refs, moved


def _kernel_product_gradients(cuda):
    rep = _Report("kernel_conv gradient")
    fusion = hip.kernel_grad_fusion()
    try:
        for kind in KINDS:
            for D in P1_DIMS:
                blur, bound = _blur(D), _kconv_grad_bound(kind, D)
                refs, moved = _host_kconv_grad(kind, D)
                rep.teeth(D, f"{kind} gradient", moved, TEETH_GRAD)
                for fuse in ((True, False) if D <= 16 else (fusion,)):
                    hip.set_kernel_grad_fusion(fuse)
                    for flags in ((0, H2) if kind == "gaussian" and D <= 16 else (0,)):
                        for B, N, M in _shapes():
                            assert hip.kernel_conv_fwd_family(kind, B, N, M, D, hip.F32, flags) in _kconv_family(kind, D), (kind, D, flags)
                        for tags, (x, y, h) in _launches(D, cuda):
                            xt = x.clone().requires_grad_(True)
                            g = _t(np.stack([refs[t][1] for t in tags]), cuda).reshape(x.shape[:-1])
                            (gx,) = torch.autograd.grad(hip.kernel_conv(kind, xt, y, h.abs() / h.shape[-1], blur, flags=flags), [xt], grad_outputs=g)
                            for tag, out in zip(tags, _rows(gx, tags)):
                                rep.add(D, f"{kind} fuse={fuse} flags={flags} {tag}", relerr(out, refs[tag][0]), bound, f"{kind} {_layout(flags)}")
    finally:
        hip.set_kernel_grad_fusion(fusion)
    return rep


def test_gradients(cuda):
    _finish(_softmin_gradients(cuda, 2, DIMS + BIG, "softmin p=2 gradient"), _softmin_gradients(cuda, 1, P1_DIMS, "softmin p=1 gradient"),
            _kernel_product_gradients(cuda))


# ---- 6. hip.softmin_fwd_grad_raw -------------------------------------------------------------------------------------------------
TEETH_VALUE_GRAD = 100      # >= 615 on the host
XD_DIMS = list(range(1, 17))


@functools.lru_cache(maxsize=None)
def _host_value_grad(D):
    eps, refs, moved = 0.05 * D / 3, {}, math.inf      # the eps of test_softmin_value_and_gradient_transposed_kernel
    for tag, x, y, h in _items(D):
        one = np.ones(x.shape[0], np.float32)
        ref, refg = oracle_c.softmin(eps, x, y, h, 2), oracle_c.softmin_grad_x(eps, x, y, h, one, 2)
        refs[tag] = (ref, refg)
        if D >= 2:
            xs, ys = _drop(x, y)
            moved = min(moved, np.abs(oracle_c.softmin(eps, xs, ys, h, 2) - ref).max() / (_tol(ref, D) + 4e-7 * 3 * eps),
                        relerr(oracle_c.softmin_grad_x(eps, xs, ys, h, one, 2), refg[:, :-1]) / 3e-5)
    return refs, moved


def test_softmin_value_and_gradient(cuda):
    rep = _Report("softmin_fwd_grad")
    for D in XD_DIMS:
        eps = 0.05 * D / 3
        refs, moved = _host_value_grad(D)
        rep.teeth(D, "value + gradient", moved, TEETH_VALUE_GRAD)
        rng = np.random.default_rng([D, 6])
        for flags in (0, H2):
            for B, N, M in _shapes():
                assert hip.softmin_fwd_family(B, N, M, D, 2, hip.F32, flags) in _p2_family(D), (D, flags)
            for tags, (x, y, h) in _launches(D, cuda):
                xb, yb, hb = (t if len(tags) > 1 else t[None].contiguous() for t in (x, y, h))
                ref = np.stack([refs[t][0] for t in tags])
                for margin in (1e-3 * eps, 3 * eps):      # guess = truth +- margin
                    guess = _t(ref + margin * (2 * rng.random(ref.shape) - 1), cuda)
                    out, unit = hip.softmin_fwd_grad_raw(xb, yb, hb, guess.contiguous(), 1.0001 * margin + 1e-7, eps, flags=flags)
                    for tag, a, u in zip(tags, out.cpu().numpy(), unit.cpu().numpy()):
                        r, rg = refs[tag]
                        # D >= 4: test_softmin_value_and_gradient_transposed_kernel; D <= 3: test_hip_kernels.py::test_softmin_value_and_gradient_in_one_pass
                        vb = _tol(r, D) + 4e-7 * margin if D >= 4 else 4e-7 * D + 3e-6 * np.abs(r).max()
                        rep.add(D, f"value flags={flags} margin={margin:.2g} {tag}", np.abs(a - r).max(), vb, _layout(flags))
                        rep.add(D, f"gradient flags={flags} margin={margin:.2g} {tag}", relerr(u, rg), 2e-5 if D >= 4 else 3e-5, _layout(flags))
    _finish(rep)


# ---- 7. hip.sinkhorn_iter4 and hip.sinkhorn_extrapolate4 -------------------------------------------------------------------------
TEETH_ITER4 = 100        # >= 4200 on the host
DAMP4 = 0.9


def _iter4_bound(ref, D, p, extrapolate=False):
    # tests/test_hip_kernels.py::test_iter4_equals_four_fused_steps / test_extrapolate4_equals_four_softmins, their anchors to oracle_c
    return 4e-7 * D + 2e-6 * np.abs(ref).max() + (1e-5 if (p == 1 and extrapolate) else 0.0)


def _measure(rng, n):
    return np.log(rng.random(n) + 0.1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _host_iter4(D, p):
    """Per item: log-weights, old potentials, and the float64 results of the initialisation and of one averaged iteration: four
    oracle soft-mins each (f_ba, g_ab, f_aa, g_bb)."""
    eps, refs, moved = (_eps2(D) if p == 2 else EPS1), {}, math.inf
    for tag, x, y, _ in _items(D):
        rng = np.random.default_rng([D, 7, len(tag) + ord(tag[-1])])
        N, M = x.shape[0], y.shape[0]
        al, bl = _measure(rng, N), _measure(rng, M)
        old = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in (N, M, N, M)]      # f_ba, g_ab, f_aa, g_bb
        sm = lambda r, c, lw, pot=None: oracle_c.softmin(eps, r, c, lw.astype(np.float64) + (0 if pot is None else pot.astype(np.float64) / eps), p)  # noqa: E731
        init = [DAMP4 * s for s in (sm(x, y, bl), sm(y, x, al), sm(x, x, al), sm(y, y, bl))]
        soft = [sm(x, y, bl, old[1]), sm(y, x, al, old[0]), sm(x, x, al, old[2]), sm(y, y, bl, old[3])]
        new = [0.5 * (o.astype(np.float64) + DAMP4 * s) for o, s in zip(old, soft)]
        refs[tag] = (al, bl, old, init, soft, new)
        if D >= 2:
            xs, ys = _drop(x, y)
            less = DAMP4 * oracle_c.softmin(eps, xs, ys, bl, p)
            moved = min(moved, np.abs(less - init[0]).max() / _iter4_bound(init[0], D, p))
    return refs, moved


def _stack(refs, tags, pick, dev):
    return _t(np.stack([pick(refs[t]) for t in tags]), dev)


def _sinkhorn_iter4(cuda):
    rep = _Report("sinkhorn_iter4")
    for p, flagset in ((2, (0, H2)), (1, (0,))):
        for D in XD_DIMS:
            eps = _eps2(D) if p == 2 else EPS1
            refs, moved = _host_iter4(D, p)
            rep.teeth(D, f"iter4 p={p}", moved, TEETH_ITER4)
            for flags in flagset:
                assert hip.fused_step_applies(D, p, flags), (D, p)
                for B, N, M in _shapes():
                    assert hip.softmin_fwd_family(B, N, M, D, p, hip.F32, flags) in (_p2_family(D) if p == 2 else _p1_family(D)), (D, p, flags)
                for tags, (x, y, _) in _launches(D, cuda):
                    sh = (lambda t: t) if len(tags) > 1 else (lambda t: t[0])
                    al, bl = sh(_stack(refs, tags, lambda r: r[0], cuda)), sh(_stack(refs, tags, lambda r: r[1], cuda))
                    old = tuple(sh(_stack(refs, tags, lambda r, k=k: r[2][k], cuda)) for k in range(4))
                    init = hip.sinkhorn_iter4(eps, x, y, al, bl, None, DAMP4, True, flags=flags, p=p)
                    new = hip.sinkhorn_iter4(eps, x, y, al, bl, old, DAMP4, True, flags=flags, p=p)
                    assert len(init) == 4 and len(new) == 4
                    for k in range(4):
                        for tag, a, b in zip(tags, _rows(init[k], tags), _rows(new[k], tags)):
                            _, _, _, ri, rs, rn = refs[tag]
                            lay = f"p={p} {_layout(flags)}"
                            rep.add(D, f"init[{k}] p={p} flags={flags} {tag}", np.abs(a - ri[k]).max(), _iter4_bound(ri[k], D, p), lay)
                            rep.add(D, f"new[{k}] p={p} flags={flags} {tag}", np.abs(b - rn[k]).max(), _iter4_bound(rs[k], D, p), lay)
    return rep


NC, MC = 17, 20          # coarse clouds of the batched launch


def _extrapolate_clouds(D):
    """{tag: (x, y, xc, yc)}: the unbatched fine clouds against item 0 of the batch as coarse clouds (33 and 40 points); the items of the
    batch as fine clouds against 17 and 20 points cut from the unbatched clouds."""
    x, y, _, xb, yb, _ = _case(D)
    out = {"u": (x, y, xb[0], yb[0])}
    for b in range(B2):
        out[f"b{b}"] = (xb[b], yb[b], x[b * NC:(b + 1) * NC], y[b * MC:(b + 1) * MC])
    return out


@functools.lru_cache(maxsize=None)
def _host_extrapolate4(D, p):
    """Per item: coarse log-weights (one massless coarse cluster), coarse potentials, and the four float64 soft-mins of the jump."""
    eps, refs, moved = (_eps2(D) if p == 2 else EPS1), {}, math.inf
    sm = lambda r, c, lw, pot: DAMP4 * oracle_c.softmin(eps, r, c, lw.astype(np.float64) + pot.astype(np.float64) / eps, p)  # noqa: E731
    for tag, (x, y, xc, yc) in _extrapolate_clouds(D).items():
        rng = np.random.default_rng([D, 8, len(tag) + ord(tag[-1])])
        al, bl = _measure(rng, xc.shape[0]), _measure(rng, yc.shape[0])
        bl[0] = -100000.0
        pots = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in (xc.shape[0], yc.shape[0], xc.shape[0], yc.shape[0])]
        want = [sm(x, yc, bl, pots[1]), sm(y, xc, al, pots[0]), sm(x, xc, al, pots[2]), sm(y, yc, bl, pots[3])]
        refs[tag] = (al, bl, pots, want)
        if D >= 2:
            moved = min(moved, np.abs(sm(*_drop(x, yc), bl, pots[1]) - want[0]).max() / _iter4_bound(want[0], D, p, True))
    return refs, moved


def test_sinkhorn_iter4_and_extrapolate4(cuda):
    rep = _Report("sinkhorn_extrapolate4")
    for p, flagset in ((2, (0, H2)), (1, (0,))):
        for D in XD_DIMS:
            eps = _eps2(D) if p == 2 else EPS1
            refs, moved = _host_extrapolate4(D, p)
            rep.teeth(D, f"extrapolate4 p={p}", moved, TEETH_ITER4)
            clouds = _extrapolate_clouds(D)
            for flags in flagset:
                assert hip.fused_step_applies(D, p, flags), (D, p)
                for tags in (("u",), tuple(f"b{b}" for b in range(B2))):
                    sh = (lambda t: t) if len(tags) > 1 else (lambda t: t[0])
                    x, y, xc, yc = (sh(_t(np.stack([clouds[t][k] for t in tags]), cuda)) for k in range(4))
                    for rows, cols in ((x, yc), (y, xc), (x, xc), (y, yc)):
                        assert hip.softmin_fwd_family(len(tags), rows.shape[-2], cols.shape[-2], D, p, hip.F32, flags) in (
                            _p2_family(D) if p == 2 else _p1_family(D)), (D, p, flags)
                    al, bl = sh(_stack(refs, tags, lambda r: r[0], cuda)), sh(_stack(refs, tags, lambda r: r[1], cuda))
                    pots = [sh(_stack(refs, tags, lambda r, k=k: r[2][k], cuda)) for k in range(4)]
                    got = hip.sinkhorn_extrapolate4(eps, x, y, xc, yc, al, bl, pots, DAMP4, flags=flags, p=p)
                    assert len(got) == 4
                    for k in range(4):
                        for tag, a in zip(tags, _rows(got[k], tags)):
                            want = refs[tag][3][k]
                            rep.add(D, f"out[{k}] p={p} flags={flags} {tag}", np.abs(a - want).max(), _iter4_bound(want, D, p, True), f"p={p} {_layout(flags)}")
    _finish(_sinkhorn_iter4(cuda), rep)


# ---- 8. hip.plan_apply (D <= 16) and hip.plan_apply_nd (D >= 17) -----------------------------------------------------------------
# the plan at eps = 0.1 D / 3 is far less sensitive to one coordinate than a potential at eps = 0.05^2 D / 3.  On the host, smallest
# over D: 266 up to D = 16, 22 up to D = 130, 1.2 at D = 4095
TEETH_PLAN, TEETH_PLAN_BIG = 10, 1
VS = (5, 33)


def _plan_eps(D):
    return 0.01 if D <= 3 else 0.1 * D / 3      # tests/test_plan_apply_gpu.py / test_plan_apply_nd_gpu.py::_eps: what their 2e-5 is stated for


def _plan_ref(x, y, h, eps, feat):
    """tests/test_plan_apply_gpu.py::_ref in float64: W = exp(E - max E), out = (W / sum W) @ feat."""
    x, y, h, feat = (np.asarray(t, dtype=np.float64) for t in (x, y, h, feat))
    E = h[None, :] - ((x * x).sum(1)[:, None] - 2.0 * x @ y.T + (y * y).sum(1)[None, :]) / (2.0 * eps)
    W = np.exp(E - E.max(1, keepdims=True))
    return (W / W.sum(1, keepdims=True)) @ feat


def _plan_worst(out, ref, feat):
    """tests/test_plan_apply_gpu.py::_worst: max over columns of max_i |out - ref| / max_j |feat_j|."""
    return float((np.abs(out - ref) / np.abs(feat).max(0)).max())


def _features(D, tag, M, V):
    return np.random.default_rng([D, 9, V, len(tag) + ord(tag[-1])]).standard_normal((M, V)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _host_plan(D):
    eps, refs, moved = _plan_eps(D), {}, math.inf
    for tag, x, y, h in _items(D, D in BIG):
        for V in VS:
            feat = _features(D, tag, y.shape[0], V)
            refs[tag, V] = (feat, _plan_ref(x, y, h, eps, feat))
            if D >= 2:
                moved = min(moved, _plan_worst(_plan_ref(*_drop(x, y), h, eps, feat), refs[tag, V][1], feat) / 2e-5)
    return refs, moved


def _plan_f32_error(dev, x, y, h, eps, feat, ref):
    """test_plan_apply_nd_gpu.py::_torch_f32_error: the same product in plain float32 torch."""
    xt, yt, ht, ft = (_t(a, dev) for a in (x, y, h, feat))
    C = (xt * xt).sum(1)[:, None] - 2.0 * xt @ yt.t() + (yt * yt).sum(1)[None, :]
    return _plan_worst((torch.softmax(ht[None, :] - C / (2.0 * eps), dim=1) @ ft).cpu().numpy(), ref, feat)


def test_plan_apply(cuda):
    rep = _Report("plan_apply")
    for D in DIMS + BIG:
        big, eps = D in BIG, _plan_eps(D)
        refs, moved = _host_plan(D)
        rep.teeth(D, "plan application", moved, TEETH_PLAN_BIG if big else TEETH_PLAN)
        raw = hip.plan_apply_raw if D <= 16 else hip.plan_apply_nd_raw
        items = {tag: (x, y, h) for tag, x, y, h in _items(D, big)}
        for flags in (0, NS, H2, H2 | NS):
            for V in VS:
                for B, N, M in _shapes(big):
                    assert hip.plan_apply_nd_family(B, N, M, D, V, flags=flags) == (hip.FAMILY_XD if D <= 16 else hip.FAMILY_XK), (D, V, flags)
                for tags, (x, y, h) in _launches(D, cuda, big):
                    xb, yb, hb = (t if len(tags) > 1 else t[None] for t in (x, y, h))
                    fb = _stack(refs, [(t, V) for t in tags], lambda r: r[0], cuda)
                    fwd = hip.softmin_fwd_raw(xb, yb, hb, eps, 2, None, flags)
                    out, mass = raw(xb, yb, hb, fwd, fb, eps, flags, want_mass=True)
                    for tag, o, m in zip(tags, out.cpu().numpy(), mass.cpu().numpy()):
                        feat, ref = refs[tag, V]
                        err, bound = _plan_worst(o, ref, feat), 2e-5      # test_parity of the two plan files
                        if D > 64 and err > bound:      # test_plan_apply_nd_gpu.py::test_parity: four times what plain float32 makes of the same product
                            bound = max(bound, 4.0 * _plan_f32_error(cuda, *items[tag], eps, feat, ref))
                        rep.add(D, f"V={V} flags={flags} {tag}", err if np.isfinite(o).all() else math.inf, bound, _layout(flags), strict=False)
                        rep.add(D, f"mass V={V} flags={flags} {tag}", np.abs(m - 1.0).max(), 1e-4, _layout(flags) + " mass", strict=False)
    _finish(rep)


# ---- 9. hip.argmin ---------------------------------------------------------------------------------------------------------------
# the bound grows like D (D + max |g|) while one coordinate moves a cost by <= 1 / 2: on the host the row minimum without the last
# coordinate differs from the full one by >= 2400 tol up to D = 16, 182 up to D = 70 and 71 at D = 121
TEETH_ARGMIN = 10


def _argmin_tol(D, gmax):
    return 2.0 * ((6 + 6 * D + 15) // 16 + 5) * 2.0**-24 * (D + gmax)      # tests/test_argmin_gpu.py::tol_of


def _cost64(x, y, g=None):
    """tests/test_argmin_gpu.py::cost64: |x_i - y_j|^2 / 2 - g_j in float64 from explicit differences."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    C = np.zeros((x.shape[0], y.shape[0]))
    for d in range(x.shape[1]):
        C += (x[:, d, None] - y[None, :, d]) ** 2
    C *= 0.5
    return C if g is None else C - np.asarray(g, np.float64)[None, :]


@functools.lru_cache(maxsize=None)
def _host_argmin(D):
    refs, moved = {}, math.inf
    for tag, x, y, h in _items(D):
        g = (0.1 * h).astype(np.float32)      # g = 0.1 * standard normal
        for gs, gv in ((0, None), (1, g)):
            C = _cost64(x, y, gv)
            tol = _argmin_tol(D, float(np.abs(g).max()) if gs else 0.0)
            refs[tag, gs] = (C, tol, g)
            if D >= 2:
                moved = min(moved, np.abs(_cost64(*_drop(x, y), gv).min(1) - C.min(1)).max() / tol)
    return refs, moved


def test_argmin(cuda):
    rep = _Report("argmin")
    for D in DIMS:
        refs, moved = _host_argmin(D)
        rep.teeth(D, "argmin", moved, TEETH_ARGMIN)
        for B, N, M in _shapes():
            assert hip.argmin_supported(B, N, M, D), D
        for tags, (x, y, h) in _launches(D, cuda):
            for gs in (0, 1):
                g = _t(np.stack([refs[t, gs][2] for t in tags]), cuda).reshape(h.shape) if gs else None
                idx, val = hip.argmin(x, y, g, return_value=True)
                for tag, i, v in zip(tags, _rows(idx, tags), _rows(val, tags)):
                    C, tol, _ = refs[tag, gs]
                    i = i.astype(np.int64)
                    if i.min() < 0 or i.max() >= C.shape[1]:
                        rep.add(D, f"index range g={gs} {tag}", math.inf, tol)
                        continue
                    cmin = C.min(1)      # the criterion of tests/test_argmin_gpu.py::judge
                    rep.add(D, f"cost excess g={gs} {tag}", (C[np.arange(C.shape[0]), i] - cmin).max(), tol, "excess", strict=False)
                    rep.add(D, f"value g={gs} {tag}", np.abs(v.astype(np.float64) - cmin).max(), tol, "value", strict=False)
    _finish(rep)
