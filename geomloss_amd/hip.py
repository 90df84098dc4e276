"""ctypes binding of ``libgeomloss_hip.so`` (C-ABI: ``include/glhip.h``) and the autograd
functions built on it.

This module is the only place where Python touches the HIP kernels.  It plays the role that
``pykeops.torch`` plays for the reference (``generic_logsumexp`` at
``_legacy/sinkhorn_samples.py:322-334,432-442``; ``LazyTensor @ v`` at
``_legacy/kernel_samples.py:128-137``).  There is no fallback: if the shared library is missing or
a tensor is not on a GPU, the call raises.

Three leaves live in private modules and are re-exported here, so that everybody else keeps writing ``hip.NAME``: the mirror of
``include/glhip.h`` with the loader (``_glhip.py``), the permutation cache's key and container (``_perm_cache.py``), the hipGraph cache
and ``settle_host`` (``_graphs.py``).  What reads or calls a name that tests replace on this module stays here.
"""

import ctypes
import os
import warnings

import torch
from torch.autograd.function import once_differentiable

from . import _glhip
from ._glhip import *  # noqa: F401,F403  (FLAG_*, FAMILY_*, kinds, dtype codes, *_MAX_DIM, SIGNATURES, LIB_PATH, load_library, bind, ...)
from ._glhip import _HERE, _RANGES, _SINCE, _TAIL, _c_double, _c_float, _c_int, _c_long, _c_size, _check, _vp  # noqa: F401
from ._graphs import GraphCache, settle_host  # noqa: F401
from ._perm_cache import PERM_CACHE_ENTRIES, _PermCache, perm_cache_key  # noqa: F401


def __getattr__(name):
    if name == "_lib":      # the loaded library, or None before the first load_library(): state of _glhip, read through
        return _glhip._lib
    if name == "ARGKMIN_MAX_K":      # the largest k of argkmin: the library's own limit (glhip_argkmin_max_k), read when asked for
        return int(load_library().glhip_argkmin_max_k())
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _points(t, name, allow_f64=False):
    """Point clouds go to the kernels as contiguous fp32 or bf16 — or, from the four entry points that have double-precision kernels
    (``allow_f64``: soft-min, its gradient, kernel product, its gradient), as fp64; every other float type is widened / narrowed
    to fp32.  float64 clouds keep their dtype there — the reference's matrix-free backends do (``_legacy/sinkhorn_samples.py:229-290``)
    — and run on ``glhip_*_f64`` (any D; no matrix cores, ~20x slower than fp32: cast to fp32 for speed).  The fp32-only entry points
    (one-launch iteration, one-pass value + gradient, hard C-transform) never see an fp64 buffer: a launch with dtype code F32 on
    doubles would read garbage silently (round-4 advice)."""
    if not t.is_cuda:
        raise RuntimeError(
            f"geomloss_amd: '{name}' lives on {t.device}; the HIP backends ('online', 'multiscale') need GPU tensors. "
            "Use backend='tensorized' for CPU tensors."
        )
    if t.dtype not in ((torch.float32, torch.bfloat16, torch.float64) if allow_f64 else (torch.float32, torch.bfloat16)):
        t = t.float()
    return t.contiguous()


def is_f64(t):
    return t.dtype == torch.float64


def _dtype_code(t):
    return BF16 if t.dtype == torch.bfloat16 else F32


def _f32(t):
    return t.detach().float().contiguous()


def _acc_dtype(points):
    """dtype of dual vectors, weights, gradients and outputs next to clouds of this dtype: fp64 with fp64 clouds, fp32 otherwise."""
    return torch.float64 if points.dtype == torch.float64 else torch.float32


def _vec(t, points):
    """A per-point vector (dual values, weights, gradients) in the accumulation dtype of the clouds it goes with."""
    return t.detach().to(_acc_dtype(points)).contiguous()


class BlockRanges:
    """Block-sparse reduction pattern in the KeOps convention (see ``include/glhip.h``), both orientations.

    Stands in for the 6-tuple returned by ``pykeops.torch.cluster.from_matrix``
    (``_legacy/sinkhorn_samples.py:515``); ``.t()`` is ``swap_axes`` (``:529``).
    """

    def __init__(self, ranges_i, slices_i, redranges_j, ranges_j, slices_j, redranges_i, small_i=False, small_j=False):
        self.ranges_i, self.slices_i, self.redranges_j = ranges_i, slices_i, redranges_j
        self.ranges_j, self.slices_j, self.redranges_i = ranges_j, slices_j, redranges_i
        # launch hints (GLHIP_FLAG_SMALL_ROW_BLOCKS): the pairs of this orientation / of the transposed one sit in row blocks of
        # up to 64 points.  Set by whoever knows the block sizes (sinkhorn_samples.kernel_truncation); results do not depend on them.
        self.small_i, self.small_j = bool(small_i), bool(small_j)

    def t(self):
        return BlockRanges(self.ranges_j, self.slices_j, self.redranges_i,
                           self.ranges_i, self.slices_i, self.redranges_j, self.small_j, self.small_i)

    def launch_flags(self):
        return FLAG_SMALL_ROW_BLOCKS if self.small_i else 0

    def c_args(self):
        n = int(self.ranges_i.shape[0])
        return [ctypes.c_void_p(self.ranges_i.data_ptr()), ctypes.c_void_p(self.slices_i.data_ptr()),
                ctypes.c_void_p(self.redranges_j.data_ptr()), n]


_NO_RANGES = [None, None, None, 0]


def _range_flags(flags, ranges):
    return int(flags) | (0 if ranges is None else ranges.launch_flags())


def _range_args(ranges, B):
    if ranges is None:
        return _NO_RANGES
    if B != 1:
        raise NotImplementedError("Block-sparse reductions are only implemented for a single (un-batched) problem.")
    return ranges.c_args()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _scratch(nbytes, device):
    """A scratch buffer of ``nbytes`` bytes (torch's caching allocator makes this a free-list lookup) as ``(tensor | None, [pointer | None,
    nbytes])``: the tensor keeps the bytes alive until the launch is queued, the list is the workspace pair of the C-ABI."""
    if nbytes == 0:
        return None, [None, 0]
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws, [ctypes.c_void_p(ws.data_ptr()), nbytes]


def _workspace(lib, x, B, N, M, D, ranges):
    """Scratch buffer for column splits."""
    n_ranges = 0 if ranges is None else int(ranges.ranges_i.shape[0])
    return _scratch(int(lib.glhip_workspace_bytes(B, N, M, D, n_ranges)), x.device)


def _iter4_scratch(lib, x, B, rows, cols, D):
    """Scratch buffer of the launches that run four reductions side by side (iteration, annealing, extrapolation): four times that of one
    dense reduction of ``rows`` x ``cols``."""
    return _scratch(4 * int(lib.glhip_workspace_bytes(B, rows, cols, D, 0)), x.device)


# the part of ENV_FLAGS that reaches those launches
_ITER4_ENV_MASK = FLAG_NO_SPLIT | FLAG_F16X2


def _as_batched(x, y, s):
    """(N,D),(M,D),(M,) -> (1,N,D),(1,M,D),(1,M); batched inputs pass through.  The per-column vector follows the clouds' accumulation
    dtype (fp64 next to fp64 clouds)."""
    if s.dtype != _acc_dtype(x):
        s = s.to(_acc_dtype(x))
    if x.dim() == 2:
        return x.unsqueeze(0), y.unsqueeze(0), s.reshape(1, -1), False
    return x, y, s.reshape(x.shape[0], -1), True


def _clouds(x, y, s, allow_f64=False, detach=False):
    """The inputs of a launch over the clouds x (N,D)|(B,N,D) and y (M,D)|(B,M,D): ``(xb, yb, sb, batched)`` with a batch axis, both clouds
    as the kernels read them (:func:`_points`) in ONE dtype, x's.  ``s``: the per-column vector as the caller has converted it."""
    if detach:
        x, y = x.detach(), y.detach()
    xb, yb, sb, batched = _as_batched(_points(x, "x", allow_f64), _points(y, "y", allow_f64), s)
    if yb.dtype != xb.dtype:
        yb = yb.to(xb.dtype)
    return xb, yb, sb, batched


def _kind(kind):
    return KERNEL_KINDS[kind] if isinstance(kind, str) else int(kind)


def _blur(blur):
    return 1.0 if blur is None else float(blur)


def _dist_flags(flags, ranges, applies):
    """``flags`` of a distance-type launch — ``applies``: the caller's own condition (p = 1 soft-min / half-step, laplacian / energy
    product of D <= 3) — with the word on squared distances from the matrix cores: the row blocks of a block-sparse launch are voxel
    clusters already (FLAG_MFMA_DIST); big dense launches sort themselves inside the library unless told not to (FLAG_NO_SORT)."""
    if applies and not (flags & (FLAG_NO_MFMA | FLAG_DIRECT)):
        if not _dist_on_mfma:
            return flags | FLAG_NO_SORT
        if ranges is not None:
            return flags | FLAG_MFMA_DIST
    return flags


# ----------------------------------------------------------------------------------------------
#  reused permutations of the sorted p = 2 call
# ----------------------------------------------------------------------------------------------

_perm_cache = _PermCache()


def perm_cache_enabled():
    return os.environ.get("GEOMLOSS_HIP_PERM_CACHE", "1") != "0"


def forget_permutations():
    """Drops every cached permutation (see :class:`_PermCache`); the hit / miss counters stay."""
    _perm_cache.clear()


def perm_cache_stats():
    """(hits, misses, live entries) of the permutation cache."""
    return _perm_cache.hits, _perm_cache.misses, len(_perm_cache.entries)


def softmin_perm_applies(B, N, M, D, p=2, dtype=F32, flags=0, n_ranges=0):
    """Whether ``glhip_softmin_fwd`` / ``glhip_sinkhorn_step`` of this shape is the sorted p = 2 call, the one whose permutations can be
    reused: the library's own predicate (``glhip_softmin_perm_applies``), host arithmetic only.  1 / 0, or ``ValueError``."""
    return _route_predicate("glhip_softmin_perm_applies", (B, N, M, D, p, dtype, flags, n_ranges),
                            f"B {B}, N {N}, M {M}, D {D}, p {p}, dtype {dtype}, n_ranges {n_ranges}")


def stable_clouds(x, y, p=2):
    """For the drivers, before a loop of soft-min calls on the clouds x (N,D), y (M,D): where those calls are the sorted p = 2 call and
    a cloud would be converted or copied by EVERY call (``_points``: a dtype the kernels do not read, a non-contiguous layout), the
    conversion is made once here — differentiably, so gradients reach the caller's tensor — and the calls of the loop see one storage
    and reuse its permutation.  Everything else comes back as it is (mixed dtypes too: each call converts the columns to its rows')."""
    if not (p == 2 and x.is_cuda and x.dim() == 2 and y.dim() == 2 and perm_cache_enabled()):
        return x, y
    lib = load_library()
    N, M, D = x.shape[0], y.shape[0], x.shape[1]
    if not hasattr(lib, "glhip_softmin_perm_applies") or (lib.glhip_softmin_perm_applies(1, N, M, D, 2, F32, 0, 0) != 1
                                                           and lib.glhip_softmin_perm_applies(1, M, N, D, 2, F32, 0, 0) != 1):
        return x, y

    def once(t):
        if t.dtype not in (torch.float32, torch.bfloat16, torch.float64):
            t = t.float()
        return t if t.is_contiguous() else t.contiguous()

    return once(x), once(y)


def _perm_plan(lib, x, y, p, ranges, flags):
    """The permutation arguments of one ``glhip_sinkhorn_step_perm`` call on the clouds x (1,N,D), y (1,M,D), or None where the call
    takes none (not the sorted p = 2 call, cache off, a capturing stream, a library without the entry point).  Returns
    ``([perm_x, perm_y, perm_flags], commit)``; ``commit()`` keeps the exported permutations once the call has been queued."""
    if not perm_cache_enabled() or not hasattr(lib, "glhip_softmin_perm_applies"):
        return None
    B, N, D = x.shape
    M = y.shape[1]
    n_ranges = 0 if ranges is None else int(ranges.ranges_i.shape[0])
    if lib.glhip_softmin_perm_applies(B, N, M, D, int(p), _dtype_code(x), _range_flags(flags, ranges), n_ranges) != 1:
        return None
    if torch.cuda.is_current_stream_capturing():
        return None
    stream = torch.cuda.current_stream(x.device).cuda_stream
    kx, ky = perm_cache_key(x, stream), perm_cache_key(y, stream)
    if kx is None or ky is None:
        return None
    px = _perm_cache.lookup(kx)
    fresh = []
    bits = 0
    if px is None:
        px = torch.empty(N, dtype=torch.int32, device=x.device)
        fresh.append((kx, x, px))
    else:
        bits |= PERM_HINT_X
    if ky == kx:      # one cloud on both sides: the x side is prepared first, the y side reads what it wrote
        py = px
        with _perm_cache.lock:
            _perm_cache.hits += 1
        bits |= PERM_HINT_Y
    else:
        py = _perm_cache.lookup(ky)
        if py is None:
            py = torch.empty(M, dtype=torch.int32, device=x.device)
            fresh.append((ky, y, py))
        else:
            bits |= PERM_HINT_Y

    def commit():
        for k, t, perm in fresh:
            _perm_cache.store(k, t, perm)

    return [ctypes.c_void_p(px.data_ptr()), ctypes.c_void_p(py.data_ptr()), bits], commit


# ----------------------------------------------------------------------------------------------
#  raw launches
# ----------------------------------------------------------------------------------------------

def _softmin_step(step, x, y, h, pot, prev, eps, damping, p, ranges, flags):
    """The launch of the soft-min (``step`` False; pot = prev = None, damping = 1) and of the half-step: one body here as in the library,
    where ``glhip_softmin_fwd`` is the step with those arguments (``softmin_step`` of csrc/glhip_api.hip).  Each keeps the entry point
    of its name — ``glhip_last_error`` texts carry it — except that the sorted p = 2 call of either goes through
    ``glhip_sinkhorn_step_perm`` and reuses the permutations of its clouds from call to call (:class:`_PermCache`)."""
    lib = load_library()
    B, N, D = x.shape
    M = y.shape[1]
    f64 = is_f64(x)
    out = torch.empty((B, N), dtype=torch.float64 if f64 else torch.float32, device=x.device)
    perm = None
    with torch.cuda.device(x.device):
        if f64:      # every array double (glhip_*_f64): no dtype code, no workspace, no flags, no permutations
            entry = lib.glhip_sinkhorn_step_f64 if step else lib.glhip_softmin_fwd_f64
            tail = (*_range_args(ranges, B), _stream(x))
        else:
            ws, ws_args = _workspace(lib, x, B, N, M, D, ranges)
            perm = _perm_plan(lib, x, y, p, ranges, flags)
            entry = lib.glhip_sinkhorn_step_perm if perm is not None else lib.glhip_sinkhorn_step if step else lib.glhip_softmin_fwd
            tail = (_dtype_code(x), *_range_args(ranges, B), *ws_args, _range_flags(flags, ranges), _stream(x),
                    *(() if perm is None else perm[0]))
        if step or perm is not None:
            rc = entry(x.data_ptr(), y.data_ptr(), h.data_ptr(), _ptr(pot), _ptr(prev), out.data_ptr(), B, N, M, D,
                       float(eps), float(damping), int(p), *tail)
        else:
            rc = entry(x.data_ptr(), y.data_ptr(), h.data_ptr(), out.data_ptr(), B, N, M, D, float(eps), int(p), *tail)
    _check(rc, lib)
    if perm is not None:
        perm[1]()
    return out


def softmin_fwd_raw(x, y, h, eps, p=2, ranges=None, flags=0):
    """x (B,N,D), y (B,M,D) fp32|bf16|fp64 contiguous CUDA; h (B,M) fp32 (fp64 next to fp64 clouds) -> (B,N) of h's dtype."""
    return _softmin_step(False, x, y, h, None, None, eps, 1.0, p, ranges, flags)


def sinkhorn_step_raw(x, y, logw, pot, prev, eps, damping, p=2, ranges=None, flags=0):
    """Fused half-step: (prev + damping * softmin(eps, C(x,y), logw + pot/eps)) / 2, or damping * softmin(...) if prev is None."""
    return _softmin_step(True, x, y, logw, pot, prev, eps, damping, p, ranges, flags)


def _launch(stem, x, ranges, out_shape, head, dims, scalars, flags, routes=None, workspace=True):
    """One reduction with a float32 / bfloat16 entry point ``<stem>`` and a float64 one ``<stem>_f64`` (softmin_bwd_x, kernel_conv_fwd,
    kernel_conv_bwd_x).  Both take ``head`` (what stands before the output), the output, ``dims`` = (B, N, M, D), ``scalars``, the ranges
    and the stream; ``<stem>`` alone takes the dtype code before the ranges and the workspace and ``flags`` after them.  That workspace is
    :func:`_workspace`'s, or with ``routes`` (a gradient launch) :func:`_grad_workspace`'s.  Returns the output, allocated here in the
    clouds' accumulation dtype."""
    lib = load_library()
    f64 = is_f64(x)
    out = torch.empty(out_shape, dtype=torch.float64 if f64 else torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        if f64:
            rc = getattr(lib, stem + "_f64")(*head, out.data_ptr(), *dims, *scalars, *_range_args(ranges, dims[0]), _stream(x))
        else:
            ws, ws_args = (_workspace(lib, x, *dims, ranges) if routes is None
                           else _grad_workspace(lib, x, *dims, ranges, flags, workspace, routes))
            rc = getattr(lib, stem)(*head, out.data_ptr(), *dims, *scalars, _dtype_code(x), *_range_args(ranges, dims[0]), *ws_args,
                                    int(flags), _stream(x))
    _check(rc, lib)
    return out


def sinkhorn_iter4_raw(x, y, a_log, b_log, pots, eps, damping, debias=True, flags=0, p=2):
    """The 4 (or 2) simultaneous updates of one Sinkhorn iteration in one launch.

    x (B,N,D), y (B,M,D); a_log (B,N), b_log (B,M); ``pots`` = None (initialisation) or the old potentials
    ``(f_ba, g_ab, f_aa, g_bb)`` / ``(f_ba, g_ab)`` as (B,N) / (B,M) fp32.  Returns the new ones, same arity."""
    lib = load_library()
    B, N, D = x.shape
    M = y.shape[1]
    first = pots is None
    outs = [torch.empty((B, n), dtype=torch.float32, device=x.device) for n in ((N, M, N, M) if debias else (N, M))]
    old = [None] * 4 if first else list(pots) + [None] * (4 - len(pots))
    new = outs + [None] * (4 - len(outs))
    with torch.cuda.device(x.device):
        ws, ws_args = _iter4_scratch(lib, x, B, max(N, M), max(N, M), D)
        rc = lib.glhip_sinkhorn_iter4(x.data_ptr(), y.data_ptr(), a_log.data_ptr(), b_log.data_ptr(),
                                      *[_ptr(t) for t in old], *[_ptr(t) for t in new], B, N, M, D, float(eps), float(damping),
                                      int(p), _dtype_code(x), int(first), *ws_args, int(flags), _stream(x))
    _check(rc, lib)
    return tuple(outs)


def sinkhorn_extrapolate4_raw(x, y, xc, yc, a_log_c, b_log_c, pots, eps, damping, flags=0, p=2):
    """The coarse-to-fine jump in one launch (``glhip_sinkhorn_extrapolate4``): fine clouds x (B,N,D), y (B,M,D), coarse clouds
    xc (B,Nc,D), yc (B,Mc,D) with log-weights a_log_c (B,Nc), b_log_c (B,Mc) and potentials ``pots`` = (f_ba, g_ab, f_aa, g_bb) /
    (f_ba, g_ab) on the coarse clouds.  Returns the potentials on the fine clouds, same arity."""
    lib = load_library()
    B, N, D = x.shape
    M, Nc, Mc = y.shape[1], xc.shape[1], yc.shape[1]
    debias = len(pots) == 4
    outs = [torch.empty((B, n), dtype=torch.float32, device=x.device) for n in ((N, M, N, M) if debias else (N, M))]
    old = [t.data_ptr() for t in pots] + [None] * (4 - len(pots))
    new = [t.data_ptr() for t in outs] + [None] * (4 - len(outs))
    with torch.cuda.device(x.device):
        ws, ws_args = _iter4_scratch(lib, x, B, max(N, M), max(Nc, Mc), D)     # rows: fine clouds, columns: coarse ones
        rc = lib.glhip_sinkhorn_extrapolate4(x.data_ptr(), y.data_ptr(), xc.data_ptr(), yc.data_ptr(), a_log_c.data_ptr(), b_log_c.data_ptr(),
                                             *old, *new, B, N, M, Nc, Mc, D, float(eps), float(damping), int(p), _dtype_code(x),
                                             *ws_args, int(flags), _stream(x))
    _check(rc, lib)
    return tuple(outs)


def _route_predicate(name, args, shown, no_kernel=None):
    """One of the library's route and family predicates (host arithmetic, no GPU): its answer >= 0, or ``ValueError`` for arguments the
    entry point rejects.  ``no_kernel``: the text of the ``NotImplementedError`` for -2 where the predicate tells that apart."""
    r = int(getattr(load_library(), name)(*(int(a) for a in args)))
    if r == -2 and no_kernel is not None:
        raise NotImplementedError(no_kernel)
    if r < 0:
        raise ValueError(f"{name}: bad argument ({shown})")
    return r


def softmin_bwd_x_uses_plan(B, N, M, D, p=2, dtype=F32, flags=0, n_ranges=0):
    """Whether ``glhip_softmin_bwd_x`` runs the matrix-core gradient of 17 <= D <= 4095 for this launch (``FLAG_XK_GRAD``): the
    library's own predicate (host arithmetic, no GPU).  1 / 0, or ``ValueError`` for arguments the entry point rejects."""
    return _route_predicate("glhip_softmin_bwd_x_uses_plan", (B, N, M, D, p, dtype, flags, n_ranges),
                            f"B {B}, N {N}, M {M}, D {D}, p {p}, dtype {dtype}, n_ranges {n_ranges}")


def dist_grad_uses_xk(op, B, N, M, D, dtype=F32, flags=0, n_ranges=0):
    """Whether ``glhip_softmin_bwd_x`` with p = 1 (``op`` "softmin_p1") resp. ``glhip_kernel_conv_bwd_x`` / ``glhip_kernel_conv_fwd_grad``
    (``op`` "laplacian" / "energy", or a kernel kind code) run the matrix-core distance gradient of 17 <= D <= 4095 for this launch
    (``FLAG_XK_DIST_GRAD``): the library's own predicate (host arithmetic, no GPU).  1 / 0, or ``ValueError`` for bad arguments."""
    return _route_predicate("glhip_dist_grad_uses_xk", (DIST_GRAD_OPS.get(op, op), B, N, M, D, dtype, flags, n_ranges),
                            f"op {op}, B {B}, N {N}, M {M}, D {D}, dtype {dtype}, n_ranges {n_ranges}")


def kernel_conv_grad_uses_xk(kind, B, N, M, D, dtype=F32, flags=0, n_ranges=0):
    """Whether ``glhip_kernel_conv_bwd_x`` / ``glhip_kernel_conv_fwd_grad`` run the matrix-core gaussian gradient of 17 <= D <= 4095 for
    this launch (``FLAG_XK_GRAD``): the library's own predicate (host arithmetic, no GPU); ``kind``: a name or a code.  1 / 0, or
    ``ValueError`` for arguments the entry points reject."""
    return _route_predicate("glhip_kernel_conv_grad_uses_xk", (KERNEL_KINDS.get(kind, kind), B, N, M, D, dtype, flags, n_ranges),
                            f"kind {kind}, B {B}, N {N}, M {M}, D {D}, dtype {dtype}, n_ranges {n_ranges}")


def _grad_workspace(lib, x, B, N, M, D, ranges, flags, workspace, routes):
    """The workspace of a gradient launch.  ``routes``: the matrix-core routes of 17 <= D <= 4095 the entry point has, in the order it asks
    them, as (predicate name, its arguments before the dtype, sizing call name).  The first route whose predicate — the library's own —
    takes the launch sizes its split partials itself; every other launch takes ``glhip_workspace_bytes``."""
    n_ranges = 0 if ranges is None else int(ranges.ranges_i.shape[0])
    for uses, args, sizing in routes:
        if getattr(lib, uses)(*args, _dtype_code(x), int(flags), n_ranges) == 1:
            return _scratch(int(getattr(lib, sizing)(B, N, M, D, int(flags))) if workspace else 0, x.device)
    if workspace:
        return _workspace(lib, x, B, N, M, D, ranges)
    return _scratch(0, x.device)


def softmin_bwd_x_raw(x, y, h, out, grad_out, eps, p=2, ranges=None, flags=0, workspace=True):
    """``workspace=False``: launch without one (no column splits) — tests only."""
    B, N, D = x.shape
    M = y.shape[1]
    routes = [("glhip_softmin_bwd_x_uses_plan", (B, N, M, D, int(p)), "glhip_softmin_bwd_x_workspace_bytes")]
    if int(p) == 1:
        routes.append(("glhip_dist_grad_uses_xk", (DIST_GRAD_OPS["softmin_p1"], B, N, M, D), "glhip_dist_grad_workspace_bytes"))
    return _launch("glhip_softmin_bwd_x", x, ranges, (B, N, D), (x.data_ptr(), y.data_ptr(), h.data_ptr(), out.data_ptr(), grad_out.data_ptr()),
                   (B, N, M, D), (float(eps), int(p)), flags, routes, workspace)


def _plan_apply_call(entry, x, y, h, fwd, feat, eps, flags, want_mass, p, ranges, workspace):
    """``glhip_plan_apply`` (D <= 16) or ``glhip_plan_apply_nd`` (D <= 4095) with its own workspace sizing call."""
    lib = load_library()
    B, N, D = x.shape
    M, V = y.shape[1], feat.shape[2]
    if is_f64(x):
        raise NotImplementedError(f"{entry}: float64 clouds are not supported (cast to float32)")
    if tuple(feat.shape[:2]) != (B, M) or tuple(h.shape) != (B, M) or tuple(fwd.shape) != (B, N):
        raise ValueError(f"{entry}: expected h {(B, M)}, fwd {(B, N)}, feat {(B, M, 'V')}; got {tuple(h.shape)}, "
                         f"{tuple(fwd.shape)}, {tuple(feat.shape)}")
    out = torch.empty((B, N, V), dtype=torch.float32, device=x.device)
    mass = torch.empty((B, N), dtype=torch.float32, device=x.device) if want_mass else None
    with torch.cuda.device(x.device):
        ws, ws_args = _scratch(int(getattr(lib, entry + "_workspace_bytes")(B, N, M, D, V)) if workspace else 0, x.device)
        rc = getattr(lib, entry)(x.data_ptr(), y.data_ptr(), h.data_ptr(), fwd.data_ptr(), feat.data_ptr(), out.data_ptr(),
                                 _ptr(mass), B, N, M, D, V, float(eps), int(p), _dtype_code(x),
                                 *_range_args(ranges, B), *ws_args, int(flags), _stream(x))
    _check(rc, lib)
    return (out, mass) if want_mass else out


def plan_apply_raw(x, y, h, fwd, feat, eps, flags=0, want_mass=False, p=2, ranges=None, workspace=True):
    """The plan of a p = 2 soft-min applied to features (``glhip_plan_apply``, D <= 16 — this contract stays; any D <= 4095:
    :func:`plan_apply_nd_raw`): x (B,N,D), y (B,M,D) fp32|bf16, h (B,M), fwd (B,N) the
    saved soft-min, feat (B,M,V) fp32 -> (B,N,V) fp32 row-normalised averages [, (B,N) recomputed row masses].  ``workspace=False``
    passes no workspace: the launch runs without column splits (same results up to summation order)."""
    return _plan_apply_call("glhip_plan_apply", x, y, h, fwd, feat, eps, flags, want_mass, p, ranges, workspace)


def plan_apply_nd_raw(x, y, h, fwd, feat, eps, flags=0, want_mass=False, p=2, ranges=None, workspace=True):
    """:func:`plan_apply_raw` for any D <= PLAN_MAX_DIM (``glhip_plan_apply_nd``): D <= 16 is the very launch of ``glhip_plan_apply``,
    17 <= D <= 4095 the K-chunked kernel of glhip_plan_apply_xk.h."""
    return _plan_apply_call("glhip_plan_apply_nd", x, y, h, fwd, feat, eps, flags, want_mass, p, ranges, workspace)


def plan_apply_p1_raw(xb, yb, hb, fb, eps, flags=0, want_softmin=False, workspace=True):
    """The plan of a p = 1 soft-min applied to features (``glhip_plan_apply_p1``, any D <= PLAN_P1_MAX_DIM): xb (B,N,D), yb (B,M,D)
    fp32|bf16, hb (B,M), fb (B,M,V) fp32 -> (B,N,V) fp32 row-normalised averages [, (B,N) the soft-min computed on the side].  The kernel
    normalises itself: no saved forward value comes in.  ``workspace=False`` passes no workspace: the launch runs without column splits
    (same results up to summation order)."""
    lib = load_library()
    B, N, D = xb.shape
    M, V = yb.shape[1], fb.shape[2]
    if is_f64(xb):
        raise NotImplementedError("glhip_plan_apply_p1: float64 clouds are not supported (cast to float32)")
    if tuple(fb.shape[:2]) != (B, M) or tuple(hb.shape) != (B, M):
        raise ValueError(f"glhip_plan_apply_p1: expected h {(B, M)}, feat {(B, M, 'V')}; got {tuple(hb.shape)}, {tuple(fb.shape)}")
    out = torch.empty((B, N, V), dtype=torch.float32, device=xb.device)
    soft = torch.empty((B, N), dtype=torch.float32, device=xb.device) if want_softmin else None
    with torch.cuda.device(xb.device):
        ws, ws_args = _scratch(int(lib.glhip_plan_apply_p1_workspace_bytes(B, N, M, D, V)) if workspace else 0, xb.device)
        rc = lib.glhip_plan_apply_p1(xb.data_ptr(), yb.data_ptr(), hb.data_ptr(), fb.data_ptr(), out.data_ptr(), _ptr(soft),
                                     B, N, M, D, V, float(eps), _dtype_code(xb), *_NO_RANGES, *ws_args, int(flags), _stream(xb))
    _check(rc, lib)
    return (out, soft) if want_softmin else out


def plan_bilinear_raw(xb, yb, hb, fwd, rowfeat, colfeat, eps, flags=0, p=2, ranges=None, workspace=True):
    """The plan of a p = 2 soft-min contracted with the per-pair weight ``<rowfeat_i, colfeat_j>`` (``glhip_plan_bilinear``, any
    D, K <= PLAN_BILINEAR_MAX_DIM): xb (B,N,D), yb (B,M,D) fp32|bf16, hb (B,M), fwd (B,N) the saved soft-min, rowfeat (B,N,K),
    colfeat (B,M,K) fp32 -> out (B,N,D), wsum (B,N) fp32.  ``workspace=False`` passes no workspace: the launch runs without column
    splits (same results up to summation order)."""
    lib = load_library()
    B, N, D = xb.shape
    M, K = yb.shape[1], rowfeat.shape[2]
    if is_f64(xb):
        raise NotImplementedError("glhip_plan_bilinear: float64 clouds are not supported (cast to float32)")
    if (tuple(rowfeat.shape) != (B, N, K) or tuple(colfeat.shape) != (B, M, K) or tuple(hb.shape) != (B, M) or tuple(fwd.shape) != (B, N)
            or tuple(yb.shape) != (B, M, D)):
        raise ValueError(f"glhip_plan_bilinear: expected y {(B, M, D)}, h {(B, M)}, fwd {(B, N)}, rowfeat {(B, N, 'K')}, colfeat {(B, M, 'K')}; got "
                         f"{tuple(yb.shape)}, {tuple(hb.shape)}, {tuple(fwd.shape)}, {tuple(rowfeat.shape)}, {tuple(colfeat.shape)}")
    out = torch.empty((B, N, D), dtype=torch.float32, device=xb.device)
    wsum = torch.empty((B, N), dtype=torch.float32, device=xb.device)
    with torch.cuda.device(xb.device):
        ws, ws_args = _scratch(int(lib.glhip_plan_bilinear_workspace_bytes(B, N, M, D, K)) if workspace else 0, xb.device)
        rc = lib.glhip_plan_bilinear(xb.data_ptr(), yb.data_ptr(), hb.data_ptr(), fwd.data_ptr(), rowfeat.data_ptr(), colfeat.data_ptr(),
                                     out.data_ptr(), wsum.data_ptr(), B, N, M, D, K, float(eps), int(p), _dtype_code(xb),
                                     *_range_args(ranges, B), *ws_args, int(flags), _stream(xb))
    _check(rc, lib)
    return out, wsum


def softmin_fwd_grad_raw(x, y, h, guess, margin, eps, ranges=None, flags=0):
    """Soft-min and d out_i / d x_i in one reduction, given a guess within ``margin`` of the answer (``glhip_softmin_fwd_grad``;
    p = 2, D <= 16) -> (B,N), (B,N,D)."""
    lib = load_library()
    B, N, D = x.shape
    M = y.shape[1]
    out = torch.empty((B, N), dtype=torch.float32, device=x.device)
    gu = torch.empty((B, N, D), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        ws, ws_args = _workspace(lib, x, B, N, M, D, ranges)
        rc = lib.glhip_softmin_fwd_grad(x.data_ptr(), y.data_ptr(), h.data_ptr(), guess.data_ptr(), float(margin), out.data_ptr(),
                                        gu.data_ptr(), B, N, M, D, float(eps), 2, _dtype_code(x), *_range_args(ranges, B), *ws_args,
                                        int(flags), _stream(x))
    _check(rc, lib)
    return out, gu


def kernel_conv_fwd_raw(kind, x, y, v, blur, ranges=None, flags=0):
    B, N, D = x.shape
    M = y.shape[1]
    return _launch("glhip_kernel_conv_fwd", x, ranges, (B, N), (int(kind), x.data_ptr(), y.data_ptr(), v.data_ptr()),
                   (B, N, M, D), (float(blur),), flags)


def _conv_grad_routes(kind, B, N, M, D):
    """The matrix-core routes of ``glhip_kernel_conv_bwd_x`` / ``glhip_kernel_conv_fwd_grad`` (``_grad_workspace``): the gaussian gradient, then
    the distance gradient of the laplacian and energy kernels (their ops are their kind codes)."""
    routes = [("glhip_kernel_conv_grad_uses_xk", (int(kind), B, N, M, D), "glhip_kernel_conv_grad_workspace_bytes")]
    if int(kind) in (LAPLACIAN, ENERGY):
        routes.append(("glhip_dist_grad_uses_xk", (int(kind), B, N, M, D), "glhip_dist_grad_workspace_bytes"))
    return routes


def kernel_conv_bwd_x_raw(kind, x, y, v, g, blur, ranges=None, flags=0, workspace=True):
    """``workspace=False``: launch without one (no column splits) — tests only."""
    B, N, D = x.shape
    M = y.shape[1]
    return _launch("glhip_kernel_conv_bwd_x", x, ranges, (B, N, D), (int(kind), x.data_ptr(), y.data_ptr(), v.data_ptr(), g.data_ptr()),
                   (B, N, M, D), (float(blur),), flags, _conv_grad_routes(kind, B, N, M, D), workspace)


def kernel_conv_fwd_grad_raw(kind, x, y, v, blur, ranges=None, flags=0, workspace=True):
    """out = K v and d out_i / d x_i in one pass (``glhip_kernel_conv_fwd_grad``: every kernel at D <= 3, the gaussian kernel at
    D <= 16, and at 17 <= D <= 4095 under ``FLAG_XK_GRAD``; the laplacian and energy kernels at 17 <= D <= 4095 under
    ``FLAG_XK_DIST_GRAD``) -> (B,N), (B,N,D).  ``workspace=False``: launch without one (no column
    splits) — tests only."""
    lib = load_library()
    B, N, D = x.shape
    M = y.shape[1]
    out = torch.empty((B, N), dtype=torch.float32, device=x.device)
    gu = torch.empty((B, N, D), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        ws, ws_args = _grad_workspace(lib, x, B, N, M, D, ranges, flags, workspace, _conv_grad_routes(kind, B, N, M, D))
        rc = lib.glhip_kernel_conv_fwd_grad(int(kind), x.data_ptr(), y.data_ptr(), v.data_ptr(), out.data_ptr(), gu.data_ptr(),
                                            B, N, M, D, float(blur), _dtype_code(x), *_range_args(ranges, B), *ws_args,
                                            int(flags), _stream(x))
    _check(rc, lib)
    return out, gu


def softmin_dense_fwd_raw(C, h, eps):
    lib = load_library()
    B, N, M = C.shape
    out = torch.empty((B, N), dtype=torch.float32, device=C.device)
    with torch.cuda.device(C.device):
        rc = lib.glhip_softmin_dense_fwd(C.data_ptr(), h.data_ptr(), out.data_ptr(), B, N, M, float(eps), _stream(C))
    _check(rc, lib)
    return out


def read_back(*tensors):
    """ONE host round trip for several small device tensors (cluster counts, kept-pair counts): their values as lists of ints."""
    same = all(t.dtype == tensors[0].dtype for t in tensors)      # (int32 cluster counts, int64 pair counts: no conversion launches)
    flat = torch.cat([t.reshape(-1) if same else t.reshape(-1).to(torch.int64) for t in tensors]).tolist()
    out, o = [], 0
    for t in tensors:
        out.append([int(v) for v in flat[o:o + t.numel()]])
        o += t.numel()
    return out


def grid_cluster_raw(x, weights, voxel, pre_div=1.0, gather=True, defer=False):
    """Voxel clustering on the device (``glhip_grid_cluster``).  x (N,D) fp32|bf16 contiguous CUDA, weights (N,) fp32 or None.

    Returns ``(perm, x_sorted, w_sorted, ranges, centroids, weights_c)``: ``perm`` (N,) int32; ``x_sorted`` / ``w_sorted`` the
    cloud in cluster order (None without ``gather``); ``ranges`` (C,2) int32, ``centroids`` (C,D) fp32 of ``x / pre_div``,
    ``weights_c`` (C,) fp32.  One host read-back (the cluster count) sizes the outputs — with ``defer`` the launch is queued and
    ``(count tensor, finish)`` comes back instead: the caller reads the counts of several clusterings in one round trip
    (:func:`read_back`) and calls ``finish(count values)`` for the tuple above.  The count tensor holds 8 integers, ``{C, overflow,
    qmin[3], qmax[3]}``: the voxel bounds of the cloud travel in the same round trip (:func:`voxel_extent`)."""
    lib = load_library()
    N, D = x.shape
    dev = x.device
    with torch.cuda.device(dev):
        perm = torch.empty(N, dtype=torch.int32, device=dev)
        x_sorted = torch.empty_like(x) if gather else None
        w_sorted = torch.empty(N, dtype=torch.float32, device=dev) if gather else None
        ranges = torch.empty((N, 2), dtype=torch.int32, device=dev)
        cents = torch.empty((N, D), dtype=torch.float32, device=dev)
        w_c = torch.empty(N, dtype=torch.float32, device=dev)
        count = torch.empty(8, dtype=torch.int32, device=dev)        # {C, overflow, qmin[3], qmax[3]}
        nbytes = int(lib.glhip_cluster_workspace_bytes(N, D))
        ws, (ws_ptr, _) = _scratch(max(nbytes, 1), dev)
        rc = lib.glhip_grid_cluster(x.data_ptr(), _ptr(weights), N, D, _dtype_code(x), float(pre_div), float(voxel), perm.data_ptr(),
                                    _ptr(x_sorted), _ptr(w_sorted), ranges.data_ptr(), cents.data_ptr(), w_c.data_ptr(),
                                    count.data_ptr(), ws_ptr, nbytes, _stream(x))
    _check(rc, lib)

    def finish(values):
        C, overflow = values[:2]
        if overflow:
            raise ValueError("geomloss_amd: the voxel grid has more than 2^21 cells along an axis; use a larger cluster_scale.")
        return perm, x_sorted, w_sorted, ranges[:C], cents[:C], w_c[:C]
    if defer:
        return count, finish
    return finish(read_back(count)[0])      # the one host round trip


def voxel_extent(count_values, voxel, pre_div=1.0):
    """Upper bound of the diagonal of the joint bounding box of the clouds whose ``glhip_grid_cluster`` count values (8 integers
    each, same ``voxel`` and ``pre_div``) are given: every cloud lies in [qmin, qmax + 1) voxels along each axis."""
    live = [v for v in count_values if v[0] > 0]
    if not live:
        return 0.0
    side = [(max(v[5 + d] for v in live) + 1 - min(v[2 + d] for v in live)) * float(voxel) * float(pre_div) for d in range(3)]
    return float(sum(s * s for s in side) ** 0.5)


# intervals: up to here the worst-case buffers (2 x 32 MB of address space the kernels touch the used part of) are cheaper than the
# counting pass (two more launches of 25 us per pattern) and its host round trip.  The ~2000 x 2000 clusters of the reference's
# voxel rule need 2e6: with 2^20 every pattern of a two-scale loss was counted first — three synchronisations and 0.3 ms of a
# 6.2-ms loss at N = 1e5 (round 5).
_RANGES_WORST_CASE_MAX = 1 << 22


def _worst_case_intervals(dev):
    """Largest worst-case interval count served without the counting pass: 2^22 = 2 x 32 MB of address space per pattern, of which
    the kernels touch the used part.  (A cap relative to the device's memory was tried after the round-5 advice:
    ``torch.cuda.get_device_properties`` costs ~110 ms on its first call — the whole first-call budget of a two-scale loss — and
    ``mem_get_info`` a driver round trip per pattern; the buffers are transient and come from torch's caching allocator.)"""
    return _RANGES_WORST_CASE_MAX


def block_ranges_raw(kind, rows, cols, f, g, ranges_rows, ranges_cols, thr, p=2, symmetric=False):
    """Keep rule on cluster pairs -> :class:`BlockRanges` (``glhip_block_ranges``).

    The interval buffers are sized for the worst case (every other cluster kept: Cr * ceil(Cc / 2)) while that is small —
    no host round trip — and from the counting pass (``glhip_block_ranges_count``, one read-back of two integers) beyond:
    the worst case is quadratic in the number of clusters, the real count is not."""
    lib = load_library()
    Cr, D = rows.shape
    Cc = cols.shape[0]
    dev = rows.device
    with torch.cuda.device(dev):
        # symmetric (rows is cols, f is g: the caller's word): the transposed pattern is the same arrays — one orientation is built
        symmetric = bool(symmetric) and Cr == Cc
        slices_r = torch.empty(Cr, dtype=torch.int32, device=dev)
        slices_c = None if symmetric else torch.empty(Cc, dtype=torch.int32, device=dev)
        head = (int(kind), rows.data_ptr(), cols.data_ptr(), _ptr(f), _ptr(g), Cr, Cc, D, int(p), float(thr),
                ranges_rows.data_ptr(), ranges_cols.data_ptr())
        cap = max(Cr * ((Cc + 1) // 2), Cc * ((Cr + 1) // 2), 1)
        if cap > _worst_case_intervals(dev):
            totals = torch.empty(2, dtype=torch.int32, device=dev)
            _check(lib.glhip_block_ranges_count(*head, slices_r.data_ptr(), (slices_r if symmetric else slices_c).data_ptr(), totals.data_ptr(),
                                                _stream(rows)), lib)
            counts = [int(v) for v in totals.tolist()]                   # the one host round trip of the big case
            if min(counts) < 0:      # int32 totals: a kept pattern of >= 2^31 intervals wraps around
                raise ValueError("geomloss_amd: the block-sparse pattern has more than 2^31 column intervals; use a larger cluster_scale.")
            cap = max(max(counts), 1)
            counted = True
        else:
            counted = False
        red_c = torch.empty((cap, 2), dtype=torch.int32, device=dev)
        red_r = None if symmetric else torch.empty((cap, 2), dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)          # set by the kernel if an interval did not fit `cap`
        rc = lib.glhip_block_ranges(*head, slices_r.data_ptr(), red_c.data_ptr(), _ptr(slices_c), _ptr(red_r), cap,
                                    status.data_ptr(), _stream(rows))
    _check(rc, lib)
    # worst-case buffers cannot overflow; counted ones could only if the two passes disagreed: the host is already in step with
    # the stream there (it read the totals), so the check costs one more small read-back and nothing is dropped silently
    if counted and int(status.item()) != 0:
        raise RuntimeError("geomloss_amd: glhip_block_ranges wrote more intervals than its counting pass announced.")
    if symmetric:
        return BlockRanges(ranges_rows, slices_r, red_c, ranges_rows, slices_r, red_c)
    return BlockRanges(ranges_rows, slices_r, red_c, ranges_cols, slices_c, red_r)


# ----------------------------------------------------------------------------------------------
#  the elementwise front and back end of a small Sinkhorn loss as one launch each (glhip_log_weights, glhip_sinkhorn_cost)
# ----------------------------------------------------------------------------------------------

_SMALL_ENDS_MAX = 32768      # points per measure up to which the one-workgroup-per-item cost kernel beats torch's tree of reductions


def small_ends_apply(*tensors):
    """fp32 CUDA vectors of at most _SMALL_ENDS_MAX entries per batch item, library present: the regime where a loss is bound by the
    host's launch rate (a 2000-point loss: 26 launches, 9 of them soft-mins)."""
    return (library_available() and all(t is None or (t.is_cuda and t.dtype == torch.float32 and t.shape[-1] <= _SMALL_ENDS_MAX)
                                        for t in tensors))


_BBOX_MAX_POINTS = 16384      # one workgroup: beyond, the latency of its serial sweep exceeds the two torch reductions it replaces


def bounding_box_applies(x, y):
    """(n, D) contiguous fp32 / bf16 CUDA clouds of one dtype, D <= 16, at most _BBOX_MAX_POINTS points together."""
    return (library_available() and x.is_cuda and y.is_cuda and x.device == y.device and x.dtype == y.dtype
            and x.dtype in (torch.float32, torch.bfloat16) and x.dim() == 2 and y.dim() == 2 and x.shape[1] == y.shape[1] <= 16
            and x.is_contiguous() and y.is_contiguous() and 0 < x.shape[0] + y.shape[0] <= _BBOX_MAX_POINTS and _SMALL_ENDS_MAX > 0)


def bounding_box(x, y):
    """(mins, maxs) of the coordinates of x and y together, fp32 (D,) each: ``glhip_bounding_box``, one launch."""
    lib = load_library()
    D = x.shape[1]
    out = torch.empty(2 * D, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib.glhip_bounding_box(x.data_ptr(), x.shape[0], y.data_ptr(), y.shape[0], D, _dtype_code(x), out.data_ptr(), _stream(x)), lib)
    return out[:D], out[D:]


def log_weights_raw(ws):
    """[log(w) with log(0) -> -100000 for w in ws] (up to 4 fp32 CUDA vectors of any shape) in ONE launch."""
    lib = load_library()
    ws = [w.detach().contiguous() for w in ws]
    outs = [torch.empty_like(w) for w in ws]
    k = len(ws)
    arr_w = (ctypes.c_void_p * k)(*[w.data_ptr() for w in ws])
    arr_o = (ctypes.c_void_p * k)(*[o.data_ptr() for o in outs])
    arr_n = (ctypes.c_long * k)(*[w.numel() for w in ws])
    with torch.cuda.device(ws[0].device):
        _check(lib.glhip_log_weights(arr_w, arr_o, arr_n, k, _stream(ws[0])), lib)
    return outs


def _cost_raw(a, f_ba, f_aa, b, g_ab, g_bb, B, N, M):
    lib = load_library()
    c = lambda t: None if t is None else t.detach().contiguous()  # noqa: E731
    a, f_ba, f_aa, b, g_ab, g_bb = (c(t) for t in (a, f_ba, f_aa, b, g_ab, g_bb))
    out = torch.empty(B, dtype=torch.float32, device=f_ba.device)
    with torch.cuda.device(f_ba.device):
        _check(lib.glhip_sinkhorn_cost(_ptr(a), _ptr(f_ba), _ptr(f_aa), _ptr(b), _ptr(g_ab), _ptr(g_bb), out.data_ptr(), B, N, M,
                                       int(a.numel() == B * N), int(b.numel() == B * M), _stream(f_ba)), lib)
    return out


class _SinkhornCost(torch.autograd.Function):
    """<a, f_ba - f_aa> + <b, g_ab - g_bb> per batch item as one launch (``sinkhorn_cost``, balanced; f_aa = g_bb = None: no
    debiasing).  The backward pass is written with differentiable torch operations of the inputs — the loss formula is bilinear —
    so that gradients of any order flow as they do through the seven torch operations it replaces."""

    @staticmethod
    def forward(ctx, batch, a, f_ba, f_aa, b, g_ab, g_bb):
        B = f_ba.shape[0] if batch else 1
        N, M = f_ba.shape[-1], g_ab.shape[-1]
        ctx.batch = batch
        ctx.save_for_backward(a, f_ba, f_aa, b, g_ab, g_bb)
        out = _cost_raw(a, f_ba, f_aa, b, g_ab, g_bb, B, N, M)
        return out if batch else out.reshape(())

    @staticmethod
    def backward(ctx, g):
        a, f_ba, f_aa, b, g_ab, g_bb = ctx.saved_tensors
        gg = g.reshape(-1, 1) if ctx.batch else g
        need = ctx.needs_input_grad
        like = lambda v, t: v.reshape(t.shape) if v.numel() == t.numel() else v.sum(0).reshape(t.shape)  # noqa: E731  (weights shared by the batch)
        ga = like(gg * (f_ba - f_aa if f_aa is not None else f_ba), a) if need[1] else None
        gb = like(gg * (g_ab - g_bb if g_bb is not None else g_ab), b) if need[4] else None
        wa = (gg * a).expand_as(f_ba) if (need[2] or need[3]) else None
        wb = (gg * b).expand_as(g_ab) if (need[5] or need[6]) else None
        return (None, ga, wa if need[2] else None, (-wa if (need[3] and f_aa is not None) else None), gb, wb if need[5] else None,
                (-wb if (need[6] and g_bb is not None) else None))


def sinkhorn_cost_fused(a, f_ba, f_aa, b, g_ab, g_bb, batch):
    return _SinkhornCost.apply(bool(batch), a, f_ba, f_aa, b, g_ab, g_bb)


def kept_pairs_raw(kind, rows, cols, f, g, ranges_rows, ranges_cols, thr, p=2, defer=False):
    """``(kept pairs of points, sum of squared row-cluster sizes, sum of squared column-cluster sizes)`` for the keep rule of
    :func:`block_ranges_raw` (``glhip_block_ranges_kept_pairs``; same arguments): one launch and one 24-byte read-back, no intervals
    built.  ``defer``: the (3,) int64 device tensor instead, for a shared :func:`read_back`."""
    lib = load_library()
    Cr, D = rows.shape
    with torch.cuda.device(rows.device):
        kept = torch.empty(3, dtype=torch.int64, device=rows.device)
        _check(lib.glhip_block_ranges_kept_pairs(int(kind), rows.data_ptr(), cols.data_ptr(), _ptr(f), _ptr(g), Cr, cols.shape[0], D, int(p),
                                                 float(thr), ranges_rows.data_ptr(), ranges_cols.data_ptr(), kept.data_ptr(),
                                                 _stream(rows)), lib)
    return kept if defer else tuple(read_back(kept)[0])


# ----------------------------------------------------------------------------------------------
#  distance-type reductions on the matrix cores (GLHIP_FLAG_MFMA_DIST): compact row blocks for dense launches
# ----------------------------------------------------------------------------------------------

# p = 1 soft-min / laplacian / energy: large dense launches are voxel-sorted first, so that every row block of the launch is
# spatially compact — the condition under which the squared distance may come from the MFMA (glhip_dist_x32.h)
_dist_on_mfma = os.environ.get("GEOMLOSS_HIP_MFMA_DIST", "1") != "0"
_DIST_MIN_ROWS, _DIST_MIN_PAIRS, _DIST_ROWS_PER_VOXEL, _DIST_COL_CHUNKS = 65536, 5e8, 256, 8
_DIST_SLAB = 256          # rows per row block of a compact-rows plan = the row tile of the distance kernel (8 wavefronts x 32 rows)


def set_distance_on_mfma(enabled):
    global _dist_on_mfma
    _dist_on_mfma = bool(enabled)


def _voxel_for(x, rows_per_voxel):
    """Voxel edge that puts ~rows_per_voxel points in an occupied voxel, from the bounding box of the (N, D) cloud."""
    N, D = x.shape
    # reduce along the contiguous axis of a (D, N) copy: torch's reduction over dim 0 of a row-major (N, 3) tensor runs at 25 GB/s
    # (0.8 ms for the two of them at 1e6 points, as long as the voxel sort they prepare)
    lo, hi = torch.aminmax(x.detach().float().t().contiguous(), dim=1)
    ext = [float(e) for e in (hi - lo).tolist()]
    live = [e for e in ext if e > 1e-6 * max(max(ext), 1e-30)]                     # axes the cloud really extends along
    vol = 1.0
    for e in live:
        vol *= e
    # never more than 2^20 voxels along an axis
    return max((vol * rows_per_voxel / N) ** (1.0 / max(len(live), 1)), max(ext) / (1 << 20), 1e-30)


def _serpentine(perm, xs, ranges, cents, voxel):
    """Re-orders the voxel clusters of a lexicographically voxel-sorted cloud along a boustrophedon path (the scan direction of
    every axis flips each time the path index of the axes before it advances), so that voxels that follow each other in memory
    are always face neighbours in space.  ANY run of consecutive rows of the result is then spatially compact — which is what
    lets the callers cut the rows into equal slabs instead of one (unevenly filled) block per voxel.
    perm (N,) int64, xs (N,D) sorted cloud, ranges (C,2), cents (C,D) -> (perm, xs) in the new order."""
    q = torch.floor(cents.float() / voxel).long()
    q = q - q.amin(0)
    ext = q.amax(0) + 1
    path = torch.zeros_like(q[:, 0])
    for a in range(q.shape[1]):
        c = torch.where(path % 2 == 1, ext[a] - 1 - q[:, a], q[:, a])
        path = path * ext[a] + c
    order = torch.argsort(path)
    sizes = (ranges[:, 1] - ranges[:, 0]).long()[order]
    starts = ranges[:, 0].long()[order]
    offs = torch.cumsum(sizes, 0) - sizes                                   # first row of every cluster in the new order
    # output_size: spares repeat_interleave the host round trip it would otherwise make to learn sum(sizes)
    idx = torch.repeat_interleave(starts - offs, sizes, output_size=xs.shape[0]) + torch.arange(xs.shape[0], device=xs.device)
    return perm[idx], xs[idx]


def compact_order(x, rows_per_voxel=None):
    """(perm, x[perm]): the cloud x (N,D) voxel-sorted (``glhip_grid_cluster``, ~rows_per_voxel points per voxel) with the voxels
    chained along the boustrophedon path of :func:`_serpentine` — any run of consecutive rows is spatially compact."""
    voxel = _voxel_for(x, _DIST_ROWS_PER_VOXEL if rows_per_voxel is None else rows_per_voxel)
    perm, xs, _, ranges, cents, _ = grid_cluster_raw(x.contiguous(), None, voxel)
    return _serpentine(perm.long(), xs, ranges, cents, voxel)


def autosort_applies(x, y, ranges=None, flags=0):
    """Whether a dense distance-type launch (p = 1 soft-min / half-step, laplacian / energy product) over these clouds sorts them
    inside the library (``csrc/glhip_autosort.h``: voxel sort along a boustrophedon path into the workspace, distances on the matrix
    cores over slabs of 256 compact rows, results back in the caller's order).  Until round 5 this was a Python-side plan
    (``_CompactRows``); it lives behind the C-ABI now, so a caller of ``glhip_softmin_fwd(p=1)`` gets it too.  Shapes and flags
    only: no device work."""
    B = 1 if x.dim() == 2 else x.shape[0]
    N, M, D = x.shape[-2], y.shape[-2], x.shape[-1]
    flags = int(flags) | ENV_FLAGS
    return not (not _dist_on_mfma or ranges is not None or B != 1 or D > 3 or N < _DIST_MIN_ROWS or is_f64(x)
                or float(N) * M < _DIST_MIN_PAIRS or (flags & (FLAG_NO_MFMA | FLAG_DIRECT | FLAG_NO_SORT)))


# ----------------------------------------------------------------------------------------------
#  autograd functions
# ----------------------------------------------------------------------------------------------

def _plan_moments(xb, yb, hb, out, eps, ranges, flags):
    """S_i = sum_j P_ij u_j u_j^T (B,N,D,D) and the centre c (B,1,D), u_j = y_j - c, for the plan P_ij = exp(h_j - |x_i - y_j|^2 / (2 eps)
    + out_i / eps) of a p = 2 soft-min — from the EXISTING gradient reduction (``glhip_softmin_bwd_x``), on augmented clouds:
    x' = (x, 0), y' = (y, t q_j), h' = h + t^2 |q_j|^2 / (2 eps) leave every P_ij unchanged (the extra squared distance cancels
    against the shift of h), and the extra components of sum_j P_ij (x'_i - y'_j) are -t sum_j P_ij q_j: any average of column
    features q_j under the plan, here q = the D (D + 1) / 2 products u_a u_b.  t = sqrt(eps) / max |q| keeps the shift of h of
    order one; D + features <= 16 per call keeps the matrix-core kernels."""
    B, N, D = xb.shape
    xf, yf = xb.float(), yb.float()
    c = yf.mean(1, keepdim=True)
    u = yf - c
    ia, ib = torch.triu_indices(D, D, device=xb.device)
    q = u[..., ia] * u[..., ib]                                    # (B, M, K)
    K = q.shape[-1]
    t = (eps ** 0.5) / q.abs().amax().clamp_min(1e-30)             # device scalar: no host round trip
    chunk = (XD_MAX_DIM - D) if D <= XD_MAX_DIM - 4 else 8
    ones = torch.ones((B, N), dtype=torch.float32, device=xb.device)
    mom = torch.empty((B, N, K), dtype=torch.float32, device=xb.device)
    flags = int(flags) & ~(FLAG_F16X2 | FLAG_MFMA_DIST)
    for k0 in range(0, K, chunk):
        qa = q[..., k0:k0 + chunk] * t
        ya = torch.cat([yf, qa], -1).contiguous()
        xa = torch.cat([xf, torch.zeros((B, N, qa.shape[-1]), dtype=torch.float32, device=xb.device)], -1).contiguous()
        ha = (hb.float() + (qa * qa).sum(-1) / (2.0 * eps)).contiguous()
        r = softmin_bwd_x_raw(xa, ya, ha, out, ones, eps, 2, ranges, flags)
        mom[..., k0:k0 + chunk] = r[..., D:] / (-t)
    S = torch.empty((B, N, D, D), dtype=torch.float32, device=xb.device)
    S[..., ia, ib] = mom
    S[..., ib, ia] = mom
    return S, c


class _SoftminBwdX(torch.autograd.Function):
    """G_i = g_i d f_i / d x_i, the backward pass of the soft-min as a differentiable operation of (x, g): what
    ``torch.autograd.grad(..., create_graph=True)`` records (KeOps' `Grad` of `_legacy/sinkhorn_samples.py:322-334`
    is differentiable again, `_legacy/sinkhorn_divergence.py:612-623` leaves autograd on for that).  y and h carry no gradient:
    the Sinkhorn loop detaches them.

    p = 2: d f_i / d x_i = x_i - ybar_i with ybar_i = sum_j P_ij y_j, so for a cotangent V (B,N,D)
        d<V, G> / d g_i = V_i . (x_i - ybar_i)
        d<V, G> / d x_i = g_i [ V_i - Cov_i V_i / eps ],   Cov_i = sum_j P_ij y_j y_j^T - ybar_i ybar_i^T
    (d P_ij / d x_i = P_ij (y_j - ybar_i) / eps).  The second moments come from :func:`_plan_moments`: one or a few more calls of
    the gradient kernel, O(N + M) memory at any size.  p = 1: the Hessian of |x - y| makes the column features depend on the row;
    d / d g is served, d / d x raises (``backend="tensorized"`` is differentiable to any order)."""

    @staticmethod
    def forward(ctx, x, g, yb, hb, out, eps, p, ranges, flags):
        xb = _points(x.detach(), "x", True)
        ones = torch.ones_like(out)
        unit = softmin_bwd_x_raw(xb, yb, hb, out, ones, eps, p, ranges, flags)       # d f_i / d x_i
        ctx.save_for_backward(xb, g.detach(), yb, hb, out, unit)
        ctx.cfg = (eps, p, ranges, flags, x.dtype, g.dtype)
        return (g.detach().to(unit.dtype).unsqueeze(-1) * unit).to(x.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, V):
        xb, g, yb, hb, out, unit = ctx.saved_tensors
        eps, p, ranges, flags, xdtype, gdtype = ctx.cfg
        V = V.reshape(unit.shape).to(unit.dtype)
        grad_g = (V * unit).sum(-1).to(gdtype) if ctx.needs_input_grad[1] else None
        grad_x = None
        if ctx.needs_input_grad[0]:
            if p != 2 or is_f64(xb):
                raise NotImplementedError(
                    "geomloss_amd: second-order derivatives with respect to the points are implemented for the p = 2 HIP soft-min "
                    "on float32 / bfloat16 clouds; use backend='tensorized' (differentiable to any order) for p = 1 or float64.")
            S, c = _plan_moments(xb, yb, hb, out, eps, ranges, flags)
            ubar = (xb.float() - c) - unit                                           # sum_j P_ij (y_j - c)
            cov_v = torch.einsum("bnde,bne->bnd", S, V) - ubar * (ubar * V).sum(-1, keepdim=True)
            grad_x = (g.to(unit.dtype).unsqueeze(-1) * (V - cov_v / eps)).to(xdtype)
        return grad_x, grad_g, None, None, None, None, None, None, None


def _bwd_x(x, g, yb, hb, out, eps, p, ranges, flags):
    """g_i d f_i / d x_i (B,N,D): one reduction — or, while autograd records the backward pass (``create_graph=True``), the
    differentiable node above.  ``x``: the (B,N,D) view of the tensor the caller differentiates."""
    if torch.is_grad_enabled() and (x.requires_grad or g.requires_grad):
        return _SoftminBwdX.apply(x, g, yb, hb, out, eps, p, ranges, flags)
    return softmin_bwd_x_raw(_points(x.detach(), "x", True), yb, hb, out, g.detach().to(out.dtype).contiguous(), eps, p, ranges, flags)


class _Softmin(torch.autograd.Function):
    """f_i = -eps log sum_j exp(h_j - C(x_i,y_j)/eps); differentiable in x only, like the reference's call sites."""

    @staticmethod
    def forward(ctx, x, y, h, eps, p, ranges, flags):
        xb, yb, hb, batched = _clouds(x, y, h.detach().contiguous(), allow_f64=True)
        flags = _dist_flags(flags, ranges, p == 1 and not is_f64(xb))
        out = softmin_fwd_raw(xb, yb, hb, eps, p, ranges, flags)
        ctx.save_for_backward(x, yb, hb, out)         # (x itself: under create_graph the backward pass is differentiated through it)
        ctx.cfg = (eps, p, ranges, flags, xb.shape)
        return out if batched else out.view(-1)

    @staticmethod
    def backward(ctx, grad_out):      # differentiable once more under create_graph=True (_SoftminBwdX)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            raise NotImplementedError(
                "geomloss_amd: the HIP soft-min is differentiable with respect to its first point cloud only "
                "(the Sinkhorn loop detaches the second cloud and the dual vector)."
            )
        x, yb, hb, out = ctx.saved_tensors
        eps, p, ranges, flags, bshape = ctx.cfg
        gx = _bwd_x(x.reshape(bshape), grad_out.reshape(out.shape), yb, hb, out, eps, p, ranges, flags)
        return gx.reshape(x.shape).to(x.dtype), None, None, None, None, None, None


class _SoftminValueGrad(torch.autograd.Function):
    """The soft-min together with its x-gradient from ONE reduction, for callers that can bound the answer (the last update of
    the Sinkhorn loop): forward runs ``glhip_softmin_fwd_grad`` and keeps d out_i / d x_i, backward is an elementwise product."""

    @staticmethod
    def forward(ctx, x, y, h, eps, guess, margin, ranges, flags):
        xb, yb, hb, batched = _clouds(x, y, _f32(h))
        out, unit = softmin_fwd_grad_raw(xb, yb, hb, _f32(guess).reshape(hb.shape[0], -1), margin, eps, ranges, flags)
        ctx.unit, ctx.cfg = unit, (x.shape, x.dtype, eps, ranges, flags)
        ctx.save_for_backward(x, yb, hb, out)         # for a backward pass that is differentiated again (create_graph=True)
        return out if batched else out.view(-1)

    @staticmethod
    def backward(ctx, grad_out):
        xshape, xdtype, eps, ranges, flags = ctx.cfg
        g = grad_out.reshape(ctx.unit.shape[0], -1)
        x, yb, hb, out = ctx.saved_tensors
        if torch.is_grad_enabled() and (x.requires_grad or g.requires_grad):
            gx = _SoftminBwdX.apply(x.reshape(ctx.unit.shape), g, yb, hb, out, eps, 2, ranges, flags)
        else:
            gx = g.float().unsqueeze(-1) * ctx.unit
        return gx.reshape(xshape).to(xdtype), None, None, None, None, None, None, None


_VALUE_GRAD_MIN_PAIRS = 5e8
_VALUE_GRAD_MAX_MARGIN = 25.0       # in units of eps: the weights stay >= exp(-50) of the largest one


def softmin_value_and_grad(eps, x, y, h, guess, margin, ranges=None, flags=0):
    """``softmin(eps, x, y, h)`` (differentiable in x) from one reduction instead of a forward and a backward one, or None when that
    does not apply: x needs no gradient, p = 2 / D <= 16 kernels only, launches too small to pay for the host check of ``margin``
    (a device scalar: sup |h - h_previous| * eps), or a margin beyond 25 eps (the loop has not converged: use the two passes)."""
    if (not (torch.is_grad_enabled() and x.requires_grad) or x.shape[-1] > XD_MAX_DIM or is_f64(x)
            or (int(flags) | ENV_FLAGS) & (FLAG_NO_MFMA | FLAG_DIRECT)):
        return None
    rows, cols = x.shape[-2], y.shape[-2]
    B = 1 if x.dim() == 2 else x.shape[0]
    if float(B) * rows * cols < _VALUE_GRAD_MIN_PAIRS:
        return None
    m = float(margin)                       # the one host round trip of this path
    if not (m >= 0.0) or m > _VALUE_GRAD_MAX_MARGIN * eps:
        return None
    guess = torch.nan_to_num(guess.detach().float(), nan=0.0, posinf=0.0, neginf=0.0)     # rows without columns: any finite guess
    return _SoftminValueGrad.apply(x, y.detach(), h.detach(), float(eps), guess, m * 1.0001 + 1e-12, ranges, int(flags) | ENV_FLAGS)


def sinkhorn_iter4(eps, x, y, a_log, b_log, pots, damping, debias=True, flags=0, p=2):
    """One whole iteration of the symmetric Sinkhorn loop on the GPU, non-differentiable (dense, p = 1 or 2, D <= 16).

    x: (N,D)|(B,N,D), y: (M,D)|(B,M,D); a_log: (N,)|(1,N)|(B,N), b_log likewise; ``pots`` None (initial potentials)
    or the old ``(f_ba, g_ab, f_aa, g_bb)`` / ``(f_ba, g_ab)``.  Returns the new potentials, shaped like a_log / b_log."""
    xb, yb, bl, _ = _clouds(x, y, _f32(b_log), detach=True)
    B = xb.shape[0]
    al = _f32(a_log).reshape(B, -1)
    old = None if pots is None else tuple(_f32(t).reshape(B, -1) for t in pots)
    new = sinkhorn_iter4_raw(xb, yb, al, bl, old, eps, damping, debias, int(flags) | (ENV_FLAGS & _ITER4_ENV_MASK), p)
    shapes = (a_log.shape, b_log.shape, a_log.shape, b_log.shape)
    return tuple(t.view(sh) for t, sh in zip(new, shapes))


def sinkhorn_extrapolate4(eps, x, y, xc, yc, a_log_c, b_log_c, pots, damping, flags=0, p=2):
    """Coarse-to-fine jump of the two-scale loop on the GPU, non-differentiable: every potential of ``pots`` — (f_ba, g_ab, f_aa, g_bb)
    or (f_ba, g_ab), living on the coarse clouds xc (Nc,D), yc (Mc,D) — carried to the fine clouds x (N,D), y (M,D) by one soft-min
    against the coarse measure each, in ONE launch (dense, p = 1 or 2, D <= 16).  Batched (B,.,D) clouds alike."""
    pts = [_points(t.detach(), n) for t, n in ((x, "x"), (y, "y"), (xc, "xc"), (yc, "yc"))]
    if any(t.dtype != pts[0].dtype for t in pts):
        pts = [t.to(pts[0].dtype) for t in pts]
    batched = pts[0].dim() == 3
    xb, yb, xcb, ycb = (t if batched else t[None] for t in pts)
    B = xb.shape[0]
    row = lambda t: _f32(t).reshape(B, -1)      # noqa: E731
    outs = sinkhorn_extrapolate4_raw(xb, yb, xcb, ycb, row(a_log_c), row(b_log_c), tuple(row(t) for t in pots), eps, damping,
                                     int(flags) | (ENV_FLAGS & _ITER4_ENV_MASK), p)
    return outs if batched else tuple(t.view(-1) for t in outs)


class Iter4Plan:
    """Everything about a run of ``glhip_sinkhorn_iter4`` calls that does not change from one iteration to the next:
    validated contiguous inputs, the scratch buffer, two sets of output buffers (an iteration reads the potentials the
    previous one wrote, and outputs may not alias inputs).  At N ~ 1e3 the per-call Python work (checks, allocations,
    device guard) costs more than the kernels; the plan leaves one ctypes call per iteration."""

    def __init__(self, x, y, a_log, b_log, debias=True, flags=0, p=2):
        self.lib = load_library()
        self.p = int(p)
        xb, yb, bl, _ = _clouds(x, y, _f32(b_log), detach=True)
        self.x, self.y, self.b_log = xb, yb, bl
        B, N, D = xb.shape
        M = yb.shape[1]
        self.a_log = _f32(a_log).reshape(B, -1)
        self.dims = (B, N, M, D)
        self.debias = debias
        self.flags = int(flags) | (ENV_FLAGS & _ITER4_ENV_MASK)
        self.shapes = (a_log.shape, b_log.shape, a_log.shape, b_log.shape)[: 4 if debias else 2]
        sizes = (N, M, N, M)[: 4 if debias else 2]
        dev = xb.device
        self.device = dev
        with torch.cuda.device(dev):
            self.ws, self.ws_args = _iter4_scratch(self.lib, xb, B, max(N, M), max(N, M), D)
            self.sets = []
            for _ in range(2):
                flat = torch.empty(B * sum(sizes), dtype=torch.float32, device=dev)
                bufs, o = [], 0
                for n in sizes:
                    bufs.append(flat[o:o + B * n].view(B, n))
                    o += B * n
                self.sets.append(bufs)
        self.shaped = [tuple(t.view(sh) for t, sh in zip(bufs, self.shapes)) for bufs in self.sets]     # what run / anneal hand out
        self.turn = 0
        self.extra_flags = 0      # per-call flags of the owner (GLHIP_FLAG_F16X2 where the temperature allows: sinkhorn_samples._HipSoftmin)
        self.fixed = (xb.data_ptr(), yb.data_ptr(), self.a_log.data_ptr(), bl.data_ptr())
        self.dtype = _dtype_code(xb)

    def run(self, eps, damping, pots, last=False):
        """pots None: initial potentials.  Otherwise the averaged update, or with ``last`` the plain, non-averaged
        update ``damping * softmin(eps, C, logw + pot/eps)`` written to fresh tensors (the differentiable step)."""
        B, N, M, D = self.dims
        if last:      # fresh tensors, in the shapes of the log-weights (same element counts as (B, N) / (B, M))
            outs = shaped = tuple(torch.empty(sh, dtype=torch.float32, device=self.device) for sh in self.shapes)
        else:
            outs, shaped = self.sets[self.turn], self.shaped[self.turn]
            self.turn ^= 1
        if pots is None:
            old = (None, None, None, None)
        else:
            old = tuple(t.data_ptr() if (t.dtype is torch.float32 and t.is_contiguous()) else None for t in pots)
            if None in old:   # unusual inputs: normalise (keeps them alive until the launch is queued)
                pots = tuple(_f32(t).reshape(B, -1) for t in pots)
                old = tuple(t.data_ptr() for t in pots)
            old = old + (None,) * (4 - len(old))
        new = tuple(t.data_ptr() for t in outs) + (None,) * (4 - len(outs))
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self.lib.glhip_sinkhorn_iter4(*self.fixed, *old, *new, B, N, M, D, float(eps), float(damping), self.p, self.dtype,
                                           1 if pots is None else (2 if last else 0), *self.ws_args, self.flags | self.extra_flags, stream)
        _check(rc, self.lib)
        return shaped

    def anneal(self, eps_list, dampings, f16x2_min_eps=float("inf")):
        """The initialisation at ``eps_list[0]`` and one averaged iteration per temperature, queued by ONE library call
        (``glhip_sinkhorn_anneal``) into the plan's two buffer sets.  Returns ``(final potentials, inputs of the last iteration)``,
        both shaped like the log-weights; the next :meth:`run` writes over the latter.  GLHIP_FLAG_F16X2 (with the plan's other
        flags) applies to the temperatures >= ``f16x2_min_eps``."""
        B, N, M, D = self.dims
        n = len(eps_list)
        ptrs = ctypes.c_void_p * 4
        sets = [ptrs(*([t.data_ptr() for t in bufs] + [None] * (4 - len(bufs)))) for bufs in self.sets]
        farr = ctypes.c_float * n
        stream = torch.cuda.current_stream(self.device).cuda_stream
        flags, min_eps = self.flags, min(float(f16x2_min_eps), 3.0e38)
        if flags & FLAG_F16X2:           # forced for every launch through the environment (GEOMLOSS_HIP_FLAGS)
            min_eps = 0.0
        elif min_eps < 3.0e38:
            flags |= FLAG_F16X2
        rc = self.lib.glhip_sinkhorn_anneal(*self.fixed, sets[0], sets[1], B, N, M, D, farr(*[float(e) for e in eps_list]),
                                            farr(*[float(d) for d in dampings]), n, self.p, self.dtype,
                                            *self.ws_args, flags, min_eps, stream)
        _check(rc, self.lib)
        self.turn = (n + 1) % 2          # the set the final potentials are NOT in
        return self.shaped[n % 2], self.shaped[(n + 1) % 2]


class _Last4(torch.autograd.Function):
    """The non-averaged last update of the loop (sinkhorn_divergence.py:612-623) for all potentials at once: one forward
    launch (``glhip_sinkhorn_iter4``, first = 2); differentiable in the row cloud of each cost (x for f_ba / f_aa, y for
    g_ab / g_bb), exactly like the four separate soft-mins it replaces."""

    @staticmethod
    def forward(ctx, x, y, plan, eps, damping, *pots):
        outs = plan.run(eps, damping, tuple(p.detach() for p in pots), last=True)
        ctx.plan, ctx.cfg, ctx.extra_flags = plan, (eps, damping, x.shape, x.dtype, y.shape, y.dtype), plan.extra_flags
        ctx.save_for_backward(x, y, *(p.detach() for p in pots), *outs)
        return outs

    @staticmethod
    def backward(ctx, *grads):        # differentiable once more under create_graph=True (_SoftminBwdX)
        plan = ctx.plan
        eps, damping, xshape, xdtype, yshape, ydtype = ctx.cfg
        B = plan.dims[0]
        x_in, y_in = ctx.saved_tensors[:2]
        saved = ctx.saved_tensors[2:]
        k = len(saved) // 2
        pots, outs = saved[:k], saved[k:]
        # (rows, columns, log-weights of the columns, potential carried by the columns) of each reduction
        specs = [(x_in, plan.y, plan.b_log, pots[1]), (y_in, plan.x, plan.a_log, pots[0])]
        if k == 4:
            specs += [(x_in, plan.x, plan.a_log, pots[2]), (y_in, plan.y, plan.b_log, pots[3])]
        gx = gy = None
        for i, (rows, cols, logw, pot) in enumerate(specs):
            g = grads[i]
            if g is None or not ctx.needs_input_grad[i % 2]:
                continue
            with torch.no_grad():      # (only for the reductions that take a gradient: a loss differentiated in x alone uses 2 of the 4 —
                # the other two cost 6 launches of a launch-bound backward pass, round 6)
                h_i = logw + pot.reshape(B, -1) * (1.0 / eps)
                val_i = (outs[i].reshape(B, -1) * (1.0 / damping)).contiguous()      # the soft-min values themselves
            gr = _bwd_x(rows.reshape(B, -1, rows.shape[-1]), g.reshape(B, -1) * damping, cols, h_i, val_i, eps, plan.p, None,
                        plan.flags | ctx.extra_flags).float()
            if i % 2 == 0:
                gx = gr if gx is None else gx + gr
            else:
                gy = gr if gy is None else gy + gr
        gx = None if gx is None else gx.reshape(xshape).to(xdtype)
        gy = None if gy is None else gy.reshape(yshape).to(ydtype)
        return (gx, gy, None, None, None) + (None,) * k


def sinkhorn_last4(plan, x, y, eps, damping, pots):
    """Differentiable last update through an :class:`Iter4Plan`; returns the new potentials shaped like the old ones."""
    if not (torch.is_grad_enabled() and (x.requires_grad or y.requires_grad)):      # nothing to differentiate: no autograd node
        return plan.run(float(eps), float(damping), tuple(p.detach() for p in pots), last=True)
    return _Last4.apply(x, y, plan, float(eps), float(damping), *pots)        # (Iter4Plan.run hands them out in those shapes)


# kernel-selection knobs for A/B runs (tuning through the environment only): a GLHIP_FLAG_* bitmask
ENV_FLAGS = int(os.environ.get("GEOMLOSS_HIP_FLAGS", "0"))


def softmin(eps, x, y, h, p=2, ranges=None, flags=0):
    """Soft-C-transform on the GPU.  x: (N,D)|(B,N,D), y: (M,D)|(B,M,D), h: (M,)|(B,M) -> (N,)|(B,N) fp32."""
    return _Softmin.apply(x, y, h, float(eps), int(p), ranges, int(flags) | ENV_FLAGS)


def plan_apply_applies(x, p=2, ranges=None):
    """Whether :func:`plan_apply` serves clouds like ``x``: p = 2, dense, D <= XD_MAX_DIM, float32 / bfloat16 compute."""
    return p == 2 and ranges is None and x.shape[-1] <= XD_MAX_DIM and x.dtype != torch.float64


def plan_apply_nd_applies(x, p=2, ranges=None):
    """Whether :func:`plan_apply_nd` serves clouds like ``x``: p = 2, dense, D <= PLAN_MAX_DIM, float32 / bfloat16 compute."""
    return p == 2 and ranges is None and x.shape[-1] <= PLAN_MAX_DIM and x.dtype != torch.float64


def plan_apply_nd_family(B, N, M, D, V, p=2, dtype=torch.float32, flags=0, n_ranges=0):
    """The kernel family (FAMILY_XD for D <= 16, FAMILY_XK for 17 <= D <= PLAN_MAX_DIM) that ``glhip_plan_apply_nd`` selects: the
    predicate the launch itself evaluates, host arithmetic only.  Raises ``NotImplementedError`` for valid requests without a
    kernel and ``ValueError`` for what the entry point rejects."""
    code = {torch.float32: F32, torch.bfloat16: BF16}.get(dtype, -1)
    return _route_predicate("glhip_plan_apply_nd_family", (B, N, M, D, V, p, code, flags, n_ranges),
                            f"B {B}, N {N}, M {M}, D {D}, V {V}, p {p}, dtype {dtype}, flags {flags}, n_ranges {n_ranges}",
                            no_kernel=f"glhip_plan_apply_nd: no kernel for p = {p}, D = {D}, n_ranges = {n_ranges}")


def _plan_apply(name, raw, max_dim, eps, x, y, h, feat, fwd, flags, p, ranges):
    D = x.shape[-1]
    if x.dtype == torch.float64 or y.dtype == torch.float64:
        raise NotImplementedError(f"geomloss_amd.hip.{name}: float64 clouds are not supported (cast to float32)")
    if p != 2 or D > max_dim or ranges is not None:
        raise NotImplementedError(f"geomloss_amd.hip.{name}: only p = 2, D <= {max_dim}, dense plans (got p = {p}, D = {D}, "
                                  f"ranges {'given' if ranges is not None else 'None'})")
    batched = x.dim() == 3
    lead = tuple(y.shape[:-1])
    vector = feat.dim() == len(lead)
    if tuple(feat.shape[:len(lead)]) != lead or feat.dim() not in (len(lead), len(lead) + 1):
        raise ValueError(f"geomloss_amd.hip.{name}: expected features of shape {lead} or {lead + ('V',)}, got {tuple(feat.shape)}")
    with torch.no_grad():
        xb, yb, hb, _ = _clouds(x, y, _f32(h), detach=True)
        B, M = yb.shape[0], yb.shape[1]
        fb = _f32(feat).to(xb.device).reshape(B, M, -1)
        flags = int(flags) | ENV_FLAGS
        fwd_b = softmin_fwd_raw(xb, yb, hb, eps, 2, None, flags) if fwd is None else _f32(fwd).reshape(B, -1)
        out = raw(xb, yb, hb, fwd_b, fb, float(eps), flags)
    if not batched:
        out = out[0]
    return out[..., 0] if vector else out


def plan_apply(eps, x, y, h, feat, fwd=None, flags=0, p=2, ranges=None):
    """Row-normalised application of the plan of a p = 2 soft-min to a feature matrix on the matrix cores (``glhip_plan_apply``):

        out[i, v] = sum_j w_ij feat[j, v] / sum_j w_ij,     w_ij = exp(h_j - |x_i - y_j|^2 / (2 eps) + fwd_i / eps)

    x: (N,D)|(B,N,D), y: (M,D)|(B,M,D), h: (M,)|(B,M), feat: (M,V)|(B,M,V)|(M,) -> (N,V)|(B,N,V)|(N,) fp32.  ``fwd`` is
    ``softmin(eps, x, y, h)`` for the same arguments; it is computed here when not given.  The unnormalised product is
    ``exp(-fwd / eps)[..., None] * out``.  Cost: one sweep over the N x M pairs per pass, each worth about four soft-min reductions
    whatever it carries; a pass takes up to 128 feature columns for D <= 4, 64 for 5 <= D <= 11 and 32 beyond, and a remainder of
    a single column is a whole pass: V = 129 at D = 3 costs two.  Inside the kernel the weights are taken relative to the largest one
    of their row, and ``out`` is divided by the recomputed row sum: ``fwd`` only centres the exponents (an error of a few units of
    ``eps`` in it costs no accuracy in ``out``; it must be close enough for the exponents to stay in range), and one-hot plan rows
    return their features bit for bit where two f16 pieces hold them (within 1.5 x 2^-23 of the column's largest entry otherwise:
    include/glhip.h); the features of a column with ``h = -inf`` are staged as 0.  NOT an autograd function: it runs under ``torch.no_grad()`` and returns a tensor without
    ``grad_fn``.  float64 clouds, p = 1, D > 16 and block-sparse ranges raise ``NotImplementedError``; :func:`plan_apply_nd` is the
    same function for any D <= PLAN_MAX_DIM = 4095."""
    return _plan_apply("plan_apply", plan_apply_raw, XD_MAX_DIM, eps, x, y, h, feat, fwd, flags, p, ranges)


def plan_apply_nd(eps, x, y, h, feat, fwd=None, flags=0, p=2, ranges=None):
    """:func:`plan_apply` for clouds of any dimension D <= PLAN_MAX_DIM = 4095 (``glhip_plan_apply_nd``).  D <= 16 runs the very
    launch of :func:`plan_apply`; for 17 <= D <= 4095 the exponent blocks come from the K-chunked kernel of the forward reduction
    of these dimensions (glhip_plan_apply_xk.h) and a pass carries up to 64 feature columns.  Same shapes, same semantics
    (row-normalised, one-hot rows bit for bit, rows without mass give 0), not an autograd function.  float64 clouds, p = 1,
    D > 4095 and block-sparse ranges raise ``NotImplementedError``."""
    return _plan_apply("plan_apply_nd", plan_apply_nd_raw, PLAN_MAX_DIM, eps, x, y, h, feat, fwd, flags, p, ranges)


def plan_apply_p1_applies(x, ranges=None):
    """Whether :func:`plan_apply_p1` serves clouds like ``x``: dense, D <= PLAN_P1_MAX_DIM, float32 / bfloat16 compute."""
    return ranges is None and 1 <= x.shape[-1] <= PLAN_P1_MAX_DIM and x.dtype != torch.float64


def plan_apply_p1(eps, x, y, h, feat, flags=0, want_softmin=False, ranges=None):
    """Row-normalised application of the plan of a p = 1 soft-min to a feature matrix on the matrix cores (``glhip_plan_apply_p1``,
    glhip_dist_plan_xk.h), for clouds of any dimension D <= PLAN_P1_MAX_DIM = 4095:

        out[i, v] = sum_j w_ij feat[j, v] / sum_j w_ij,     w_ij = exp(h_j - |x_i - y_j| / eps)

    with the distance clamped from below as in ``utils.distances``.  Shapes as :func:`plan_apply_nd`: x: (N,D)|(B,N,D), y: (M,D)|(B,M,D),
    h: (M,)|(B,M), feat: (M,V)|(B,M,V)|(M,) -> (N,V)|(B,N,V)|(N,) fp32.  The kernel normalises itself, so there is no ``fwd`` argument;
    ``want_softmin=True`` also returns ``softmin(eps, x, y, h, p=1)`` as the kernel has computed it on the side, (N,)|(B,N): the
    unnormalised product is ``exp(-softmin / eps)[..., None] * out``.  One sweep over the N x M pairs per pass of
    ``glhip_plan_apply_p1_pass_width()`` feature columns; a remainder is a pass of its own.  One-hot plan rows return their features bit
    for bit, rows without mass give 0 (soft-min +inf), results are bit-identical run to run.  NOT an autograd function: it runs under
    ``torch.no_grad()`` and returns tensors without ``grad_fn``.  float64 clouds, D > 4095 and block-sparse ranges raise
    ``NotImplementedError``."""
    D = x.shape[-1]
    if x.dtype == torch.float64 or y.dtype == torch.float64:
        raise NotImplementedError("geomloss_amd.hip.plan_apply_p1: float64 clouds are not supported (cast to float32)")
    if D > PLAN_P1_MAX_DIM or ranges is not None:
        raise NotImplementedError(f"geomloss_amd.hip.plan_apply_p1: only D <= {PLAN_P1_MAX_DIM}, dense plans (got D = {D}, "
                                  f"ranges {'given' if ranges is not None else 'None'})")
    batched = x.dim() == 3
    lead = tuple(y.shape[:-1])
    vector = feat.dim() == len(lead)
    if tuple(feat.shape[:len(lead)]) != lead or feat.dim() not in (len(lead), len(lead) + 1):
        raise ValueError(f"geomloss_amd.hip.plan_apply_p1: expected features of shape {lead} or {lead + ('V',)}, got {tuple(feat.shape)}")
    with torch.no_grad():
        xb, yb, hb, _ = _clouds(x, y, _f32(h), detach=True)
        B, M = yb.shape[0], yb.shape[1]
        fb = _f32(feat).to(xb.device).reshape(B, M, -1)
        res = plan_apply_p1_raw(xb, yb, hb, fb, float(eps), int(flags) | ENV_FLAGS, want_softmin)
    out, soft = res if want_softmin else (res, None)
    if not batched:
        out = out[0]
        soft = None if soft is None else soft[0]
    out = out[..., 0] if vector else out
    return (out, soft) if want_softmin else out


def plan_bilinear_applies(x, ranges=None):
    """Whether :func:`plan_bilinear` serves clouds like ``x``: dense, D <= PLAN_BILINEAR_MAX_DIM, float32 / bfloat16 compute (p = 2 only)."""
    return ranges is None and 1 <= x.shape[-1] <= PLAN_BILINEAR_MAX_DIM and x.dtype != torch.float64


def plan_bilinear(eps, x, y, h, rowfeat, colfeat, fwd=None, flags=0, p=2, ranges=None):
    """The plan of a p = 2 soft-min contracted with a bilinear per-pair weight on the matrix cores (``glhip_plan_bilinear``,
    glhip_plan_bilinear_xk.h), for clouds of any dimension D <= PLAN_BILINEAR_MAX_DIM = 4095 and K <= 4095 features:

        pi_ij = w_ij / sum_j w_ij,    w_ij = exp(h_j - |x_i - y_j|^2 / (2 eps) + fwd_i / eps),    tau_ij = <rowfeat_i, colfeat_j>
        out[i, :] = sum_j pi_ij tau_ij (y_j - x_i)            wsum[i] = sum_j pi_ij tau_ij

    x: (N,D)|(B,N,D), y: (M,D)|(B,M,D), h: (M,)|(B,M), rowfeat: (N,K)|(B,N,K), colfeat: (M,K)|(B,M,K) -> ``(out, wsum)`` of shapes
    (N,D)|(B,N,D) and (N,)|(B,N), fp32.  ``fwd`` is ``softmin(eps, x, y, h)`` for the same arguments; it is computed here by one
    soft-min when not given, and only centres the exponents (the kernel divides by the row mass it recomputes).  This is the one
    reduction behind the gradients of ``P @ S`` and of the barycentric map (``geomloss_amd.transport``).  One sweep over the pairs per 32
    coordinates; every sweep evaluates the exponents and tau on the matrix cores.  Features of any finite magnitude are safe: the
    product is scaled per row.  Rows without mass give 0, a column with ``h = -inf`` weighs exactly 0, results are bit-identical run
    to run.  NOT an autograd function itself: it runs under ``torch.no_grad()`` and returns tensors without ``grad_fn``.  float64
    clouds, p != 2, block-sparse ranges and D or K > 4095 raise ``NotImplementedError``; mismatched shapes raise ``ValueError``."""
    D = x.shape[-1]
    if x.dtype == torch.float64 or y.dtype == torch.float64:
        raise NotImplementedError("geomloss_amd.hip.plan_bilinear: float64 clouds are not supported (cast to float32)")
    lead_x, lead_y = tuple(x.shape[:-1]), tuple(y.shape[:-1])
    if (x.dim() not in (2, 3) or y.dim() != x.dim() or y.shape[-1] != D or rowfeat.dim() != x.dim() or colfeat.dim() != x.dim()
            or tuple(rowfeat.shape[:-1]) != lead_x or tuple(colfeat.shape[:-1]) != lead_y or rowfeat.shape[-1] != colfeat.shape[-1]
            or tuple(h.shape) != lead_y or (fwd is not None and tuple(fwd.shape) != lead_x)):
        raise ValueError(f"geomloss_amd.hip.plan_bilinear: expected y {lead_y[:-1] + ('M', D)}, h {lead_y}, rowfeat {lead_x + ('K',)}, "
                         f"colfeat {lead_y + ('K',)}, fwd {lead_x}; got {tuple(y.shape)}, {tuple(h.shape)}, {tuple(rowfeat.shape)}, "
                         f"{tuple(colfeat.shape)}, {None if fwd is None else tuple(fwd.shape)}")
    K = rowfeat.shape[-1]
    if p != 2 or D > PLAN_BILINEAR_MAX_DIM or K > PLAN_BILINEAR_MAX_DIM or ranges is not None:
        raise NotImplementedError(f"geomloss_amd.hip.plan_bilinear: only p = 2, D and K <= {PLAN_BILINEAR_MAX_DIM}, dense plans (got p = {p}, "
                                  f"D = {D}, K = {K}, ranges {'given' if ranges is not None else 'None'})")
    batched = x.dim() == 3
    with torch.no_grad():
        xb, yb, hb, _ = _clouds(x, y, _f32(h), detach=True)
        B, N, M = xb.shape[0], xb.shape[1], yb.shape[1]
        rf = _f32(rowfeat).to(xb.device).reshape(B, N, K).contiguous()
        cf = _f32(colfeat).to(xb.device).reshape(B, M, K).contiguous()
        flags = int(flags) | ENV_FLAGS
        fwd_b = softmin_fwd_raw(xb, yb, hb, eps, 2, None, flags) if fwd is None else _f32(fwd).reshape(B, -1).contiguous()
        out, wsum = plan_bilinear_raw(xb, yb, hb.contiguous(), fwd_b, rf, cf, float(eps), flags)
    return (out, wsum) if batched else (out[0], wsum[0])


def fused_step_applies(D, p=2, flags=0, sparse=False):
    """Whether one of the kernels of D <= XD_MAX_DIM = 16 serves ``glhip_sinkhorn_step`` for clouds of dimension D (always False
    beyond: the fused half-step of 17 <= D <= 4095 is a different kernel — ask :func:`half_step_applies`, which the drivers do, for
    "is the half-step ONE launch"): every operator for D <= 3; for 4 <= D <= XD_MAX_DIM
    the matrix-core kernels — p = 2 (glhip_softmin_xd.h), and since round 5 p = 1 on DENSE launches (glhip_dist_xd.h; ``sparse``:
    the launch carries block-sparse ranges) — which GLHIP_FLAG_NO_MFMA / GLHIP_FLAG_DIRECT switch off: the generic-dimension
    kernel those flags fall back to has no fused half-step."""
    if D <= 3:
        return True
    if D > XD_MAX_DIM or ((int(flags) | ENV_FLAGS) & (FLAG_NO_MFMA | FLAG_DIRECT)):
        return False
    return p == 2 or (p == 1 and not sparse)


def half_step_applies(D, p=2, flags=0, sparse=False):
    """Whether :func:`sinkhorn_step` runs as ONE ``glhip_sinkhorn_step`` launch: wherever :func:`fused_step_applies` (the kernels of
    D <= 16), and for p = 2 clouds of 17 <= D <= MFMA_FWD_MAX_DIM on the K-chunked matrix-core kernel (glhip_softmin_xk.h), which
    GLHIP_FLAG_NO_MFMA / GLHIP_FLAG_DIRECT switch off like the others; under ``FLAG_XK_DIST`` also for p = 1 clouds of
    17 <= D <= DIST_XK_MAX_DIM on DENSE launches (glhip_dist_xk.h), with the same two flags switching it off."""
    if fused_step_applies(D, p, flags, sparse):
        return True
    flags = int(flags) | ENV_FLAGS
    if flags & (FLAG_NO_MFMA | FLAG_DIRECT):
        return False
    if p == 1:
        return bool(flags & FLAG_XK_DIST) and not sparse and XD_MAX_DIM < D <= DIST_XK_MAX_DIM
    return p == 2 and XD_MAX_DIM < D <= MFMA_FWD_MAX_DIM


def softmin_fwd_family(B, N, M, D, p=2, dtype=F32, flags=0, n_ranges=0):
    """The kernel family (FAMILY_*) ``glhip_softmin_fwd`` / ``glhip_sinkhorn_step`` select for a launch of this shape: the library's own
    predicate (``glhip_softmin_fwd_family``), host arithmetic only — no device is touched."""
    return _route_predicate("glhip_softmin_fwd_family", (B, N, M, D, p, dtype, flags, n_ranges),
                            f"B {B}, N {N}, M {M}, D {D}, p {p}, dtype {dtype}, n_ranges {n_ranges}")


def kernel_conv_fwd_family(kind, B, N, M, D, dtype=F32, flags=0, n_ranges=0):
    """The same for the kernel products of ``glhip_kernel_conv_fwd`` (``glhip_kernel_conv_fwd_family``); ``kind``: a name or a code."""
    return _route_predicate("glhip_kernel_conv_fwd_family", (KERNEL_KINDS.get(kind, kind), B, N, M, D, dtype, flags, n_ranges),
                            f"kind {kind}, B {B}, N {N}, M {M}, D {D}, dtype {dtype}, n_ranges {n_ranges}")


def sinkhorn_step(eps, x, y, logw, pot, prev, damping, p=2, ranges=None, flags=0):
    """One non-differentiable half-step of the Sinkhorn loop on the GPU: (prev + damping * softmin(eps, C, logw + pot/eps)) / 2,
    or damping * softmin(...) when prev is None — ONE launch where :func:`half_step_applies`, the soft-min kernel followed by
    torch arithmetic elsewhere (p = 1 in D > 16 without ``FLAG_XK_DIST``, D > 4095, block-sparse p = 1 in D > 3, D > 3 under GLHIP_FLAG_NO_MFMA / GLHIP_FLAG_DIRECT).

    x: (N,D)|(B,N,D), y: (M,D)|(B,M,D); logw, pot: (M,)|(B,M) (pot may be None); prev: (N,)|(B,N) or None.
    Returns fp32 (N,)|(B,N).  Used by the drivers inside the no-grad part of ``sinkhorn_loop``."""
    if is_f64(x) and p in (1, 2):      # float64 clouds: the fused double-precision half-step (any D, dense / batched / block-sparse)
        xb, yb, lw, batched = _clouds(x, y, logw.detach().double().contiguous(), allow_f64=True, detach=True)
        B = xb.shape[0]
        pt = None if pot is None else pot.detach().double().contiguous().reshape(B, -1)
        pv = None if prev is None else prev.detach().double().contiguous().reshape(B, -1)
        out = sinkhorn_step_raw(xb, yb, lw, pt, pv, eps, damping, p, ranges, 0)
        return out if batched else out.view(-1)
    if not half_step_applies(x.shape[-1], p, flags, ranges is not None) or is_f64(x):
        with torch.no_grad():
            h = _vec(logw, x) if pot is None else _vec(logw, x) + _vec(pot, x).reshape(logw.shape) / eps
            ft = damping * softmin(eps, x.detach(), y.detach(), h, p=p, ranges=ranges, flags=flags)
            return ft if prev is None else 0.5 * (_vec(prev, x).reshape(ft.shape) + ft)
    xb, yb, lw, batched = _clouds(x, y, _f32(logw), detach=True)
    B = xb.shape[0]
    pt = None if pot is None else _f32(pot).reshape(B, -1)
    pv = None if prev is None else _f32(prev).reshape(B, -1)
    flags = _dist_flags(int(flags) | ENV_FLAGS, ranges, p == 1)
    out = sinkhorn_step_raw(xb, yb, lw, pt, pv, eps, damping, p, ranges, flags)
    return out if batched else out.view(-1)


# Gaussian reductions on the kernels that centre every workgroup on its own first row (the gradient kernels and the products of
# their family, glhip_wsum_mfma.h): the exponent -|x - y|^2 / 2 blur^2 is assembled on the matrix cores from terms of size
# |x - c| |y - c| / blur^2, and its float32 accumulation leaves a relative error of that size x 2^-24 in the kernel value — a
# common bias of -1.6e-5 on every term of a norm at blur = .05 in the unit cube when the rows of a workgroup are scattered over
# the cloud.  With the rows in compact order (256 neighbours per workgroup) |x - c| is the size of a voxel and the bias drops to
# -1.2e-6 (profiles/r03_upper_triangle.txt).  Large dense launches only: the sort costs ~1 ms at 1e6 points.
_GAUSS_SORT_MIN_PAIRS = 1e11


def _gauss_compact_rows(kind, xb, M, ranges, flags):
    """(perm, rows in compact order) for a big dense gaussian launch of the per-workgroup-centre kernels, or None."""
    B, N, D = xb.shape
    if (kind != GAUSSIAN or ranges is not None or B != 1 or D > 3 or is_f64(xb) or float(N) * M < _GAUSS_SORT_MIN_PAIRS
            or (flags & (FLAG_NO_MFMA | FLAG_DIRECT))):
        return None
    perm, xs = compact_order(xb[0])
    return perm, xs.unsqueeze(0).contiguous()


def _unsort_rows(perm, t):
    """(1, N, ...) in sorted row order -> original order."""
    out = torch.empty_like(t)
    out[0, perm] = t[0]
    return out


class _KernelConv(torch.autograd.Function):
    """out_i = sum_j k(x_i,y_j) v_j, differentiable in x, y and v."""

    @staticmethod
    def forward(ctx, kind, x, y, v, blur, ranges, flags, x_grad=True):
        # x_grad: needs_input_grad says True for a leaf that requires gradients even under no_grad, where nothing will be asked for
        xb, yb, vb, batched, out, unit = _KernelConv.product(kind, x, y, v, blur, ranges, flags, x_grad and ctx.needs_input_grad[1])
        ctx.unit = unit
        ctx.save_for_backward(xb, yb, vb, x, y, v)      # x, y, v themselves: the differentiable backward (create_graph) needs their history
        ctx.cfg = (kind, blur, ranges, flags, x.shape, y.shape, v.shape, x.dtype, y.dtype, v.dtype)
        return out if batched else out.view(-1)

    @staticmethod
    def product(kind, x, y, v, blur, ranges, flags, want_unit):
        """The launch behind forward: (xb, yb, vb, batched, out (B,N), unit (B,N,D) | None); unit_i = d out_i / d x_i when
        ``want_unit`` and a product-and-gradient kernel exists for this kind and dimension."""
        xb, yb, vb, batched = _clouds(x, y, v.detach().contiguous(), allow_f64=True)
        if is_f64(xb):      # double precision: the plain product kernel, no plans, no fused gradient
            return xb, yb, vb, batched, kernel_conv_fwd_raw(kind, xb, yb, vb, blur, ranges, flags), None
        # When x requires gradients, the product and its row gradient come out of ONE reduction: the gradient kernel
        # carries one more accumulator, the product itself.  The backward pass is then elementwise.
        # (D <= 3: every kernel; 4 <= D <= 16: the gaussian kernel on the matrix cores; 17 <= D <= 4095: the gaussian kernel where
        # the caller asked for the matrix-core gradient, FLAG_XK_GRAD; the laplacian and energy kernels there under FLAG_XK_DIST_GRAD)
        launch = (xb.shape[0], xb.shape[1], yb.shape[1], xb.shape[2], _dtype_code(xb), int(flags), 0 if ranges is None else int(ranges.ranges_i.shape[0]))
        fused = (_fuse_kernel_grad and want_unit
                 and (xb.shape[-1] <= 3 or (kind == GAUSSIAN and xb.shape[-1] <= XD_MAX_DIM and not (flags & FLAG_NO_MFMA))
                      or load_library().glhip_kernel_conv_grad_uses_xk(int(kind), *launch) == 1
                      or (int(kind) in (LAPLACIAN, ENERGY) and load_library().glhip_dist_grad_uses_xk(int(kind), *launch) == 1)))
        # laplacian / energy: squared distances from the matrix cores wherever the row blocks are spatially compact — the voxel
        # clusters of the multiscale backend as they are, large dense launches after the voxel sort the library does itself
        # (csrc/glhip_autosort.h) — for the product, the product + gradient and (GRAD_FAMILY) the companion products of a norm alike
        fl = _dist_flags(flags, ranges, kind != GAUSSIAN and xb.shape[-1] <= 3)
        rows = None
        X, Y, V, R = xb, yb, vb, ranges
        if fused or (flags & FLAG_GRAD_FAMILY):      # gaussian: the kernels with one centre per workgroup
            rows = _gauss_compact_rows(kind, xb, yb.shape[1], ranges, flags)
            if rows is not None:
                X = rows[1]
        if fused:
            out, unit = kernel_conv_fwd_grad_raw(kind, X, Y, V, blur, R, fl)
        else:
            out, unit = kernel_conv_fwd_raw(kind, X, Y, V, blur, R, fl), None
        if rows is not None:
            out, unit = _unsort_rows(rows[0], out), (None if unit is None else _unsort_rows(rows[0], unit))
        return xb, yb, vb, batched, out, unit

    @staticmethod
    def _differentiable_backward(ctx, grad_out):
        """backward under ``create_graph=True``: the three gradients written with differentiable operations, so that autograd can
        go through them once more (KeOps' symbolic ``Grad`` composes the same way: ``_legacy/kernel_samples.py:43-54``).  Gaussian
        kernel, dense: with s = 1 / blur^2 and k = exp(-s |x - y|^2 / 2),
            d/dx_i = -s g_i [ x_i (K v)_i - (K (v y))_i ],   d/dy_j = s v_j [ (K^T (g x))_j - y_j (K^T g)_j ],   d/dv = K^T g
        — D + 1 kernel products per cloud instead of one gradient reduction, each of them this very autograd function."""
        kind, blur, ranges, flags = ctx.cfg[:4]
        x, y, v = ctx.saved_tensors[3:]
        g = grad_out.reshape(x.shape[:-1])
        v = v.reshape(y.shape[:-1])
        s = 1.0 / (blur * blur)
        conv = lambda rows, cols, w: kernel_conv(kind, rows, cols, w, blur, None, flags & ~FLAG_GRAD_FAMILY)   # noqa: E731
        D = x.shape[-1]
        gx = gy = gv = None
        if ctx.needs_input_grad[1]:
            Kvy = torch.stack([conv(x, y, v * y[..., d]) for d in range(D)], dim=-1)
            gx = (-s) * g.unsqueeze(-1) * (x * conv(x, y, v).unsqueeze(-1) - Kvy)
        if ctx.needs_input_grad[2]:
            Kgx = torch.stack([conv(y, x, g * x[..., d]) for d in range(D)], dim=-1)
            gy = s * v.unsqueeze(-1) * (Kgx - y * conv(y, x, g).unsqueeze(-1))
        if ctx.needs_input_grad[3]:
            gv = conv(y, x, g)
        return None, gx, gy, gv, None, None, None, None

    @staticmethod
    def backward(ctx, grad_out):
        # create_graph=True: somebody may differentiate this gradient.  Dense gaussian products: the differentiable form; laplacian /
        # energy / block-sparse ones: the one-reduction gradients below, marked once-differentiable (autograd raises if a second
        # derivative is really taken through them; backend="tensorized" is differentiable to any order)
        if torch.is_grad_enabled() and ctx.cfg[0] == GAUSSIAN and ctx.cfg[2] is None:
            return _KernelConv._differentiable_backward(ctx, grad_out)
        return _KernelConv._backward_once(ctx, grad_out)

    @staticmethod
    @once_differentiable
    def _backward_once(ctx, grad_out):
        xb, yb, vb = ctx.saved_tensors[:3]
        kind, blur, ranges, flags, xs, ys, vs, xdt, ydt, vdt = ctx.cfg
        g = grad_out.reshape(xb.shape[0], -1).to(vb.dtype).contiguous()
        rt = None if ranges is None else ranges.t()
        gx = gy = gv = None
        if ctx.needs_input_grad[1]:
            if ctx.unit is not None:
                gx = (g.unsqueeze(-1) * ctx.unit).reshape(xs).to(xdt)
            else:
                gx = _KernelConv._row_gradient(kind, xb, yb, vb, g, blur, ranges, flags).reshape(xs).to(xdt)
        if ctx.needs_input_grad[2]:
            gy = _KernelConv._row_gradient(kind, yb, xb, g, vb, blur, rt, flags).reshape(ys).to(ydt)
        if ctx.needs_input_grad[3]:
            rows = _gauss_compact_rows(kind, yb, xb.shape[1], rt, flags) if (flags & FLAG_GRAD_FAMILY) else None
            if rows is not None:
                gv = _unsort_rows(rows[0], kernel_conv_fwd_raw(kind, rows[1], xb, g, blur, rt, flags))
            else:
                gv = kernel_conv_fwd_raw(kind, yb, xb, g, blur, rt, flags)
            gv = gv.reshape(vs).to(vdt)
        return None, gx, gy, gv, None, None, None, None

    @staticmethod
    def _row_gradient(kind, rows_pts, cols_pts, v, g, blur, ranges, flags):
        """d/d rows of sum_i g_i sum_j k(rows_i, cols_j) v_j (g per row, v per column), big gaussian launches in compact row order."""
        rows = _gauss_compact_rows(kind, rows_pts, cols_pts.shape[1], ranges, flags)
        if rows is None:
            return kernel_conv_bwd_x_raw(kind, rows_pts, cols_pts, v, g, blur, ranges, flags)
        perm, X = rows
        return _unsort_rows(perm, kernel_conv_bwd_x_raw(kind, X, cols_pts, v, g[:, perm].contiguous(), blur, ranges, flags))


# product + row gradient in one pass when x requires gradients (set_kernel_grad_fusion(False): always two reductions)
_fuse_kernel_grad = True


def set_kernel_grad_fusion(enabled):
    global _fuse_kernel_grad
    _fuse_kernel_grad = bool(enabled)


def kernel_grad_fusion():
    return _fuse_kernel_grad


def kernel_conv(kind, x, y, v, blur=0.05, ranges=None, flags=0):
    """Kernel-matrix x vector product on the GPU; ``kind`` is a name or a GLHIP_* code."""
    return _KernelConv.apply(_kind(kind), x, y, v, _blur(blur), ranges, int(flags) | ENV_FLAGS, torch.is_grad_enabled() and x.requires_grad)


def kernel_conv_with_unit(kind, x, y, v, blur, want_unit, flags=0):
    """No autograd: ``(K v, d (K v)_i / d x_i | None)`` from one reduction where a product-and-gradient kernel exists (the building
    block of kernel_samples._UnionNorm); shapes follow x: (N,), (N,D) or (B,N), (B,N,D)."""
    with torch.no_grad():
        _, _, _, batched, out, unit = _KernelConv.product(_kind(kind), x, y, v, _blur(blur), None, int(flags) | ENV_FLAGS, want_unit)
    if not batched:
        out, unit = out.view(-1), (None if unit is None else unit.view(-1, unit.shape[-1]))
    return out, unit


def kernel_conv_row_gradient(kind, x, y, v, g, blur, flags=0):
    """No autograd: d/dx of sum_i g_i (K v)_i as one gradient reduction (``glhip_kernel_conv_bwd_x``), shaped like x."""
    with torch.no_grad():
        xb, yb, vb, _ = _clouds(x, y, v.detach().contiguous(), allow_f64=True)
        gb = _vec(g, xb).reshape(xb.shape[0], -1)
        return _KernelConv._row_gradient(_kind(kind), xb, yb, vb, gb, _blur(blur), None, int(flags) | ENV_FLAGS).reshape(x.shape)


class _SoftminDense(torch.autograd.Function):
    """Row-wise soft-min of an explicit cost matrix (the tensorized backend on GPU tensors)."""

    @staticmethod
    def forward(ctx, C, h, eps):
        Cb, hb = C.float().contiguous(), h.float().contiguous()
        out = softmin_dense_fwd_raw(Cb, hb, eps)
        ctx.save_for_backward(Cb, hb, out)
        ctx.eps = eps
        ctx.dtypes = (C.dtype, h.dtype)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        Cb, hb, out = ctx.saved_tensors
        eps = ctx.eps
        # d out_i / d C_ij = P_ij,  d out_i / d h_j = -eps P_ij,  P = softmax_j(h_j - C_ij/eps)
        P = torch.exp(hb[:, None, :] - Cb / eps + (out / eps)[:, :, None]) * grad_out[:, :, None]
        gC = P.to(ctx.dtypes[0]) if ctx.needs_input_grad[0] else None
        gh = (-eps * P.sum(1)).to(ctx.dtypes[1]) if ctx.needs_input_grad[1] else None
        return gC, gh, None


def softmin_dense(eps, C, h):
    return _SoftminDense.apply(C, h, float(eps))


class _LseLines(torch.autograd.Function):
    """out[..., i] = log sum_j exp(h[..., j] - c(i, j)) along the last axis of a contiguous fp32 tensor, c the (scaled)
    squared or absolute distance between grid samples i/N and j/N (``include/glhip.h``); differentiable in h."""

    @staticmethod
    def forward(ctx, h, eps, p):
        if not h.is_cuda:
            raise RuntimeError("geomloss_amd: the grid soft-min runs on the HIP kernels only; move the images to a GPU.")
        hc = h.detach().float().contiguous()
        N = hc.shape[-1]
        R = hc.numel() // max(N, 1)
        out = torch.empty_like(hc)
        lib = load_library()
        with torch.cuda.device(hc.device):
            rc = lib.glhip_lse_lines_fwd(hc.data_ptr(), out.data_ptr(), R, N, float(eps), int(p), _stream(hc))
        _check(rc, lib)
        ctx.save_for_backward(hc, out)
        ctx.cfg = (float(eps), int(p), h.dtype)
        return out.to(h.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        hc, out = ctx.saved_tensors
        eps, p, dtype = ctx.cfg
        g = grad_out.float().contiguous()
        gh = torch.empty_like(hc)
        N = hc.shape[-1]
        lib = load_library()
        with torch.cuda.device(hc.device):
            rc = lib.glhip_lse_lines_bwd(hc.data_ptr(), out.data_ptr(), g.data_ptr(), gh.data_ptr(), hc.numel() // max(N, 1), N,
                                         eps, p, _stream(hc))
        _check(rc, lib)
        return gh.to(dtype), None, None


def cmin(x, y, g, p=2, ranges=None, flags=0):
    """Hard C-transform on the GPU: min_j [C(x_i, y_j) - g_j], C = |x-y|^2/2 (p = 2) or |x-y| (p = 1); not differentiable.
    x: (N,D)|(B,N,D), y: (M,D)|(B,M,D), g: (M,)|(B,M) -> (N,)|(B,N) fp32."""
    lib = load_library()
    xb, yb, gb, batched = _clouds(x, y, _f32(g), detach=True)
    B, N, D = xb.shape
    M = yb.shape[1]
    out = torch.empty((B, N), dtype=torch.float32, device=xb.device)
    with torch.cuda.device(xb.device):
        ws, ws_args = _workspace(lib, xb, B, N, M, D, ranges)
        rc = lib.glhip_cmin_fwd(xb.data_ptr(), yb.data_ptr(), gb.data_ptr(), out.data_ptr(), B, N, M, D, int(p), _dtype_code(xb),
                                *_range_args(ranges, B), *ws_args, int(flags) | ENV_FLAGS, _stream(xb))
    _check(rc, lib)
    return out if batched else out.view(-1)


def argmin_supported(B, N, M, D, p=2, dtype=F32, n_ranges=0):
    """Whether ``glhip_argmin`` serves a launch of this shape (p = 2, dense, 1 <= D <= ARGMIN_MAX_DIM, fp32 / bf16 clouds): the
    predicate the launch itself evaluates (``glhip_argmin_supported``), host arithmetic only — no device is touched.  Raises
    ``ValueError`` for what the entry point rejects (negative sizes, D < 1, a bad p or dtype)."""
    return bool(_route_predicate("glhip_argmin_supported", (B, N, M, D, p, dtype, n_ranges),
                                 f"B {B}, N {N}, M {M}, D {D}, p {p}, dtype {dtype}, n_ranges {n_ranges}"))


def argmin(x, y, g=None, return_value=False, flags=0, p=2):
    """Arg-reduction on the matrix cores (``glhip_argmin``): ``argmin_j [|x_i - y_j|^2 / 2 - g_j]`` — the nearest column for
    ``g = None``, what KeOps' ``generic_argmin("SqDist(x,y)", ...)`` returns in the reference's K-means recipe; the column a plan row
    sends most of its mass to for g = dual potential + eps log weight.
    x: (N,D)|(B,N,D), y: (M,D)|(B,M,D), g: (M,)|(B,M)|None -> int32 (N,)|(B,N); with ``return_value`` also the fp32 minima.
    Ties go to the smallest index; ``g_j = -inf`` excludes column j; a row without an admissible column (M = 0, every g = -inf) gets
    index -1 and value +inf.  Not recorded by autograd.  float64 clouds, p != 2 and D > ARGMIN_MAX_DIM = 4095 raise
    ``NotImplementedError``; block-sparse ranges and p = 1 are out of scope; k > 1 neighbours: :func:`argkmin`."""
    if x.dtype == torch.float64 or y.dtype == torch.float64:
        raise NotImplementedError("geomloss_amd.hip.argmin: float64 clouds are not supported (cast to float32)")
    D = x.shape[-1]
    if p != 2 or D > ARGMIN_MAX_DIM:
        raise NotImplementedError(f"geomloss_amd.hip.argmin: only p = 2, D <= {ARGMIN_MAX_DIM} (got p = {p}, D = {D})")
    lib = load_library()
    with torch.no_grad():
        # (g may be None or empty: a placeholder goes with the clouds, g is checked against them and reshaped below)
        xb, yb, _, batched = _clouds(x, y, torch.empty(x.shape[0] if x.dim() == 3 else 1, dtype=torch.float32, device=x.device), detach=True)
        if g is not None and g.numel() != yb.numel() // max(D, 1):
            raise ValueError(f"geomloss_amd.hip.argmin: expected one dual value per column, {tuple(y.shape[:-1])}, got {tuple(g.shape)}")
        gb = None if g is None else _f32(g).to(xb.device).reshape(yb.shape[:2])
        if yb.shape[0] != xb.shape[0] or yb.shape[2] != D:
            raise ValueError(f"geomloss_amd.hip.argmin: clouds of shapes {tuple(x.shape)} and {tuple(y.shape)} do not go together")
        B, N, _ = xb.shape
        M = yb.shape[1]
        index = torch.empty((B, N), dtype=torch.int32, device=xb.device)
        value = torch.empty((B, N), dtype=torch.float32, device=xb.device) if return_value else None
        with torch.cuda.device(xb.device):
            ws, ws_args = _scratch(int(lib.glhip_argmin_workspace_bytes(B, N, M, D)), xb.device)
            rc = lib.glhip_argmin(xb.data_ptr(), yb.data_ptr(), _ptr(gb), index.data_ptr(), _ptr(value), B, N, M, D, int(p), _dtype_code(xb),
                                  *_NO_RANGES, *ws_args, int(flags) | ENV_FLAGS, _stream(xb))
        _check(rc, lib)
    if not batched:
        index = index.view(-1)
        value = value.view(-1) if return_value else None
    return (index, value) if return_value else index


def argkmin_supported(B, N, M, D, k, p=2, dtype=F32, n_ranges=0):
    """Whether ``glhip_argkmin`` serves a launch of this shape (p = 2, dense, 1 <= D <= ARGMIN_MAX_DIM, 1 <= k <= ARGKMIN_MAX_K, fp32 /
    bf16 clouds): the predicate the launch itself evaluates (``glhip_argkmin_supported``), host arithmetic only — no device is touched.
    Raises ``ValueError`` for what the entry point rejects (negative sizes, D < 1, k < 1, a bad p or dtype)."""
    return bool(_route_predicate("glhip_argkmin_supported", (B, N, M, D, k, p, dtype, n_ranges),
                                 f"B {B}, N {N}, M {M}, D {D}, k {k}, p {p}, dtype {dtype}, n_ranges {n_ranges}"))


def argkmin(x, y, k, g=None, return_value=False, flags=0, p=2):
    """Top-k arg-reduction on the matrix cores (``glhip_argkmin``): for every row the ``k`` columns of the smallest
    ``|x_i - y_j|^2 / 2 - g_j``, best first — the k nearest columns for ``g = None``, what KeOps' ``LazyTensor.argKmin(k, dim=1)`` of
    ``SqDist`` returns (``Kmin_argKmin`` with ``return_value``: the squared distance is twice the value); the k columns a plan row sends
    most of its mass to for g = dual potential + eps log weight.
    x: (N,D)|(B,N,D), y: (M,D)|(B,M,D), g: (M,)|(B,M)|None -> int32 (N,k)|(B,N,k); with ``return_value`` also the fp32 costs.
    Entries are sorted by (cost ascending, index ascending) on the kernel's float32 exponents: the first k' < k columns are what a call
    with k' returns, ``k = 1`` is :func:`argmin`, bit for bit both, whatever the launch.  ``g_j = -inf`` excludes column j; ranks a row
    has no admissible column for (M < k, masks, M = 0) get index -1 and value +inf.  Not recorded by autograd.  float64 clouds, p != 2,
    D > ARGMIN_MAX_DIM = 4095 and k > ARGKMIN_MAX_K raise ``NotImplementedError``, k < 1 ``ValueError``; block-sparse ranges and p = 1
    are out of scope."""
    if x.dtype == torch.float64 or y.dtype == torch.float64:
        raise NotImplementedError("geomloss_amd.hip.argkmin: float64 clouds are not supported (cast to float32)")
    D = x.shape[-1]
    k = int(k)
    if k < 1:
        raise ValueError(f"geomloss_amd.hip.argkmin: k must be at least 1, got {k}")
    lib = load_library()
    max_k = int(lib.glhip_argkmin_max_k())
    if p != 2 or D > ARGMIN_MAX_DIM or k > max_k:
        raise NotImplementedError(f"geomloss_amd.hip.argkmin: only p = 2, D <= {ARGMIN_MAX_DIM}, k <= {max_k} (got p = {p}, D = {D}, k = {k})")
    with torch.no_grad():
        # (g may be None or empty: a placeholder goes with the clouds, g is checked against them and reshaped below)
        xb, yb, _, batched = _clouds(x, y, torch.empty(x.shape[0] if x.dim() == 3 else 1, dtype=torch.float32, device=x.device), detach=True)
        if g is not None and g.numel() != yb.numel() // max(D, 1):
            raise ValueError(f"geomloss_amd.hip.argkmin: expected one dual value per column, {tuple(y.shape[:-1])}, got {tuple(g.shape)}")
        gb = None if g is None else _f32(g).to(xb.device).reshape(yb.shape[:2])
        if yb.shape[0] != xb.shape[0] or yb.shape[2] != D:
            raise ValueError(f"geomloss_amd.hip.argkmin: clouds of shapes {tuple(x.shape)} and {tuple(y.shape)} do not go together")
        B, N, _ = xb.shape
        M = yb.shape[1]
        index = torch.empty((B, N, k), dtype=torch.int32, device=xb.device)
        value = torch.empty((B, N, k), dtype=torch.float32, device=xb.device) if return_value else None
        with torch.cuda.device(xb.device):
            ws, ws_args = _scratch(int(lib.glhip_argkmin_workspace_bytes(B, N, M, D, k)), xb.device)
            rc = lib.glhip_argkmin(xb.data_ptr(), yb.data_ptr(), _ptr(gb), index.data_ptr(), _ptr(value), B, N, M, D, k, int(p), _dtype_code(xb),
                                   *_NO_RANGES, *ws_args, int(flags) | ENV_FLAGS, _stream(xb))
        _check(rc, lib)
    if not batched:
        index = index.view(N, k)
        value = value.view(N, k) if return_value else None
    return (index, value) if return_value else index


def max_lines(g, step, p=2):
    """out[..., i] = max_j [g[..., j] - c(i, j)] along the last axis, c = (step (i-j))^2 (p = 2) or step |i-j| (p = 1)."""
    if not g.is_cuda:
        raise RuntimeError("geomloss_amd: the grid C-transform runs on the HIP kernels only; move the arrays to a GPU.")
    gc = g.detach().float().contiguous()
    N = gc.shape[-1]
    out = torch.empty_like(gc)
    lib = load_library()
    with torch.cuda.device(gc.device):
        rc = lib.glhip_max_lines_fwd(gc.data_ptr(), out.data_ptr(), gc.numel() // max(N, 1), N, float(step), int(p), _stream(gc))
    _check(rc, lib)
    return out.to(g.dtype)


def lse_lines(h, eps, p=2):
    return _LseLines.apply(h, float(eps), int(p))
