"""Using the transport plan behind the dual potentials of the legacy API.

``F, G = SamplesLoss("sinkhorn", p=2, blur=blur, potentials=True, debias=False)(a, x, b, y)`` describes the entropic plan

    P_ij = a_i b_j exp((F_i + G_j - |x_i - y_j|^2 / 2) / blur^2)

without ever forming it.  The functions below push features through that plan — labels, colours, the barycentric map — with one
soft-min reduction and one matrix-core application of the plan (:func:`geomloss_amd.hip.plan_apply_nd`), at any N, M the solver
itself handles.  GPU tensors only, like the ``online`` backend; p = 2, float32 / bfloat16 clouds of dimension D <= 4095: D <= 16 on
the kernel with resident operands (up to 128 feature columns per pass), 17 <= D <= 4095 — principal components, embeddings — on the
K-chunked kernel (64 per pass); beyond, ``NotImplementedError``.

Autograd (p = 2): :func:`apply_plan` (plain and ``transpose=True``) and :func:`barycentric_map` are ``torch.autograd.Function`` s when
grad mode is on and one of ``x, y, F, G, feat`` requires grad, so that ``|T(x) - target|^2`` or a feature-matching term ``P @ S`` can sit
in a loss.  For a cotangent ``Gb`` of ``P @ S`` the plan is contracted with the per-pair weight ``tau_ij = <Gb_i, S_j>``,

    dL/dx_i = (1/eps) sum_j P_ij tau_ij (y_j - x_i),        dL/dG_j = (1/eps) sum_i P_ij tau_ij,

by ONE matrix-core reduction per side (:func:`geomloss_amd.hip.plan_bilinear`, glhip_plan_bilinear_xk.h) instead of the ``V D``
feature columns that composing it from :func:`geomloss_amd.hip.plan_apply_nd` would take.  Only the reductions that the requested
gradients need are launched; gradients come back in the dtype of their input; the backward pass is once-differentiable.  The functions
reach the kernels through ``hip.softmin``, ``hip.plan_apply_nd`` and ``hip.plan_bilinear`` alone, looked up at call time.  When no input
requires grad, or under ``torch.no_grad()``, the calls run exactly as before: same launches, same bits, no ``grad_fn``.  Not
differentiable here: the weights ``a`` / ``b`` (detached), ``p = 1`` (no ``grad_fn``), block-sparse ranges, float64 clouds, second
derivatives, ``hip.softmin`` with respect to ``y`` / ``h``, ``OTResultSample.plan_operator``, :func:`plan_argmax` and :func:`plan_topk`.

``p=1`` (:func:`apply_plan`, :func:`barycentric_map`): the plan of ``SamplesLoss("sinkhorn", p=1, ...)``,

    P_ij = a_i b_j exp((F_i + G_j - |x_i - y_j|) / blur),

through ONE launch of :func:`geomloss_amd.hip.plan_apply_p1` per product, which normalises itself and returns the row sums' soft-min on
the side: one kernel for every dimension 1 <= D <= 4095, 64 feature columns per pass.  Measured at N = M = 2e5 on an MI355X
(profiles/dist_plan_xk.txt): a product of V = 3 / 32 / 128 columns costs 5.4 / 5.5 / 13.2 p = 1 soft-min reductions at D = 3,
1.7 / 1.7 / 3.8 at D = 32 and 1.4 / 1.4 / 2.9 at D = 128 — less than the 2 V reductions of the log-domain loop at every measured
(D, V), narrowly so at D = 3, V = 3 (the loop: 1.1x the product).

:func:`plan_argmax` gives the hard correspondence instead of an average: the column that receives most of a row's mass, one
arg-reduction (:func:`geomloss_amd.hip.argmin`), same clouds and dimensions.  :func:`plan_topk` gives the k heaviest entries of
every row with their weights — a sparse plan — from one top-k arg-reduction (:func:`geomloss_amd.hip.argkmin`).
"""

import math

import torch

from . import hip

__all__ = ["apply_plan", "barycentric_map", "plan_argmax", "plan_topk"]


def _log_weights(w, like, count):
    """log of the weights (uniform when ``w`` is None) with the shape of ``like``; zero weights become -inf, i.e. no mass."""
    if w is None:
        return torch.full_like(like, -math.log(count))
    return w.detach().to(like.dtype).reshape(like.shape).log()


def _eps(blur, p):
    """The temperature ``blur ** p`` of the plan; only the costs |x - y| (p = 1) and |x - y|^2 / 2 (p = 2) have kernels here."""
    if p not in (1, 2):
        raise ValueError(f"geomloss_amd.transport: p must be 1 or 2, got {p!r}")
    return float(blur) ** p


def _wants_grad(*tensors):
    """Whether a call is recorded: grad mode is on and one of the differentiable inputs asks for a gradient."""
    return torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in tensors)


def _like(grad, ref):
    """A gradient in the dtype and shape of the input it belongs to."""
    return grad.to(ref.dtype).reshape(ref.shape)


def _plan_p2(x, y, F, G, feat, eps, a, b):
    """``P @ feat`` for p = 2 with what its backward pass reuses: ``(out, h, fwd, rows)``.  Runs without a graph, through
    ``hip.softmin`` and ``hip.plan_apply_nd`` looked up at call time."""
    with torch.no_grad():
        N, M = x.shape[-2], y.shape[-2]
        Ff = F.detach().float().reshape(x.shape[:-1])
        Gf = G.detach().float().reshape(y.shape[:-1])
        h = _log_weights(b, Gf, M) + Gf / eps
        fwd = hip.softmin(eps, x.detach(), y.detach(), h)              # sum_j b_j exp((G_j - C_ij) / eps) = exp(-fwd_i / eps)
        avg = hip.plan_apply_nd(eps, x, y, h, feat, fwd=fwd)
        rows = (_log_weights(a, Ff, N) + (Ff - fwd) / eps).exp()       # sum_j P_ij
        return (rows * avg if avg.dim() == rows.dim() else rows.unsqueeze(-1) * avg), h, fwd, rows


class _ApplyPlan(torch.autograd.Function):
    """``out = P @ feat`` (p = 2) with gradients for x, y, F, G and feat; the weights a, b are constants.  With the cotangent Gb,
    tau_ij = <Gb_i, feat_j>, rows_i = sum_j P_ij, cols_j = sum_i P_ij and bil = :func:`geomloss_amd.hip.plan_bilinear`::

        (o,  w)  = bil(x, y, h;  Gb,   feat)          dx = rows / eps * o          dF = <Gb, out> / eps
        (oT, wT) = bil(y, x, hT; feat, Gb)            dy = cols / eps * oT         dG = cols / eps * wT
        dfeat = P^T @ Gb                              (the transposed application, ``hip.plan_apply_nd``)

    Only the reductions that ``ctx.needs_input_grad`` asks for are launched: at most one transposed soft-min, one transposed
    application and two bilinear reductions next to the saved soft-min of the forward pass."""

    @staticmethod
    def forward(ctx, x, y, F, G, feat, eps, a, b):
        out, h, fwd, rows = _plan_p2(x, y, F, G, feat, eps, a, b)
        ctx.save_for_backward(x, y, F, G, feat, a, b, h, fwd, rows, out)
        ctx.eps = eps
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, y, F, G, feat, a, b, h, fwd, rows, out = ctx.saved_tensors
        eps = ctx.eps
        need_x, need_y, need_F, need_G, need_feat = ctx.needs_input_grad[:5]
        vector = feat.dim() == y.dim() - 1
        Gb = grad_out.detach().float()
        S = feat.detach().float()
        if vector:
            Gb, S, out = Gb.unsqueeze(-1), S.unsqueeze(-1), out.unsqueeze(-1)
        dx = dy = dF = dG = dfeat = None
        if need_x:
            o, _ = hip.plan_bilinear(eps, x, y, h, Gb, S, fwd=fwd)
            dx = _like((rows / eps).unsqueeze(-1) * o, x)
        if need_F:
            dF = _like((Gb * out).sum(-1) / eps, F)
        if need_y or need_G or need_feat:
            Ff = F.detach().float().reshape(x.shape[:-1])
            Gf = G.detach().float().reshape(y.shape[:-1])
            hT = _log_weights(a, Ff, x.shape[-2]) + Ff / eps
            fwdT = hip.softmin(eps, y.detach(), x.detach(), hT)        # sum_i a_i exp((F_i - C_ij) / eps) = exp(-fwdT_j / eps)
            cols = (_log_weights(b, Gf, y.shape[-2]) + (Gf - fwdT) / eps).exp()
            if need_y or need_G:
                oT, wT = hip.plan_bilinear(eps, y, x, hT, S, Gb, fwd=fwdT)
                if need_y:
                    dy = _like((cols / eps).unsqueeze(-1) * oT, y)
                if need_G:
                    dG = _like(cols / eps * wT, G)
            if need_feat:
                dS = cols.unsqueeze(-1) * hip.plan_apply_nd(eps, y, x, hT, Gb, fwd=fwdT)
                dfeat = _like(dS[..., 0] if vector else dS, feat)
        return dx, dy, dF, dG, dfeat, None, None, None


def _map_p2(x, y, G, eps, b, want_fwd):
    """The barycentric map for p = 2, ``(T, h, fwd)``; without ``want_fwd`` the application computes the soft-min itself."""
    with torch.no_grad():
        Gf = G.detach().float().reshape(y.shape[:-1])
        h = _log_weights(b, Gf, y.shape[-2]) + Gf / eps
        fwd = hip.softmin(eps, x.detach(), y.detach(), h) if want_fwd else None
        return hip.plan_apply_nd(eps, x, y, h, y.detach().float(), fwd=fwd), h, fwd


class _BarycentricMap(torch.autograd.Function):
    """``T = pi @ y`` (p = 2), pi the row-normalised plan, with gradients for x, y and G (none for F: the map does not depend on it;
    the weights b are constants).  With the cotangent Gd, cbar = mean_j y_j, colsum_j = sum_i pi_ij::

        A  = [Gd, -<Gd, T - cbar>],   Sf = [y - cbar, 1]          so that tau_ij = <A_i, Sf_j> = <Gd_i, y_j - T_i>
        (o,  w)  = bil(x, y, h;       A,  Sf)                     dx = (o + (x - T) w) / eps
        (oT, wT) = bil(y, x, fwd/eps; Sf, A)                      dy = pi^T Gd + colsum / eps * oT        dG = colsum / eps * wT"""

    @staticmethod
    def forward(ctx, x, y, G, eps, b):
        T, h, fwd = _map_p2(x, y, G, eps, b, True)
        ctx.save_for_backward(x, y, G, h, fwd, T)
        ctx.eps = eps
        return T

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, y, G, h, fwd, T = ctx.saved_tensors
        eps = ctx.eps
        need_x, need_y, need_G = ctx.needs_input_grad[:3]
        Gd = grad_out.detach().float()
        yf = y.detach().float()
        cbar = yf.mean(-2, keepdim=True)
        A = torch.cat([Gd, -(Gd * (T - cbar)).sum(-1, keepdim=True)], -1)
        Sf = torch.cat([yf - cbar, torch.ones_like(yf[..., :1])], -1)
        dx = dy = dG = None
        if need_x:
            o, w = hip.plan_bilinear(eps, x, y, h, A, Sf, fwd=fwd)
            dx = _like((o + (x.detach().float() - T) * w.unsqueeze(-1)) / eps, x)
        if need_y or need_G:
            hT = fwd / eps
            fwdT = hip.softmin(eps, y.detach(), x.detach(), hT)        # colsum_j = exp(h_j - fwdT_j / eps)
            colsum = (h - fwdT / eps).exp()
            oT, wT = hip.plan_bilinear(eps, y, x, hT, Sf, A, fwd=fwdT)
            if need_y:
                direct = colsum.unsqueeze(-1) * hip.plan_apply_nd(eps, y, x, hT, Gd, fwd=fwdT)
                dy = _like(direct + (colsum / eps).unsqueeze(-1) * oT, y)
            if need_G:
                dG = _like(colsum / eps * wT, G)
        return dx, dy, dG, None, None


def apply_plan(x, y, F, G, feat, blur, a=None, b=None, transpose=False, p=2):
    """``sum_j P_ij feat_j`` for the plan of the potentials ``F`` (N,)|(B,N), ``G`` (M,)|(B,M) on the clouds ``x`` (N,D)|(B,N,D),
    ``y`` (M,D)|(B,M,D) with weights ``a``, ``b`` (uniform by default): feat (M,V)|(B,M,V)|(M,) -> (N,V)|(B,N,V)|(N,) fp32.
    ``transpose=True`` applies the transposed plan instead: ``sum_i P_ij feat_i`` for feat on the rows, (N,V) -> (M,V).
    ``p=1``: the plan of the cost |x_i - y_j| at temperature ``blur`` — ONE launch (:func:`geomloss_amd.hip.plan_apply_p1`), which
    returns the row sums' soft-min next to the average.  Any other ``p`` than 1 or 2 raises ``ValueError``.

    Autograd (``p=2`` only): when grad mode is on and one of ``x, y, F, G, feat`` requires grad, the result carries a ``grad_fn`` and
    ``.backward()`` fills the gradients of those five, each in the dtype of its input, through
    :func:`geomloss_amd.hip.plan_bilinear` (at most two launches of it, one transposed soft-min and one transposed application; only
    what the requested gradients need).  The weights ``a``, ``b`` are detached: no gradient flows to them.  The backward pass is
    once-differentiable: no second derivatives.  Otherwise — and always for ``p=1`` — the call runs as before and returns a tensor
    without ``grad_fn``."""
    if transpose:
        return apply_plan(y, x, G, F, feat, blur, a=b, b=a, p=p)
    eps = _eps(blur, p)
    if p == 2:
        if _wants_grad(x, y, F, G, feat):
            return _ApplyPlan.apply(x, y, F, G, feat, eps, a, b)
        return _plan_p2(x, y, F, G, feat, eps, a, b)[0]
    with torch.no_grad():
        N, M = x.shape[-2], y.shape[-2]
        Ff = F.detach().float().reshape(x.shape[:-1])
        Gf = G.detach().float().reshape(y.shape[:-1])
        h = _log_weights(b, Gf, M) + Gf / eps
        avg, fwd = hip.plan_apply_p1(eps, x, y, h, feat, want_softmin=True)      # sum_j b_j exp((G_j - C_ij) / eps) = exp(-fwd_i / eps)
        rows = (_log_weights(a, Ff, N) + (Ff - fwd) / eps).exp()                  # sum_j P_ij
        return rows * avg if avg.dim() == rows.dim() else rows.unsqueeze(-1) * avg


def barycentric_map(x, y, F, G, blur, b=None, p=2):
    """``T(x_i) = sum_j P_ij y_j / sum_j P_ij`` (N,D)|(B,N,D) fp32: where the plan sends each x_i on average.  The row-normalised
    average does not depend on ``a`` or ``F`` (they scale a whole row); ``F`` is accepted so that the call reads like
    :func:`apply_plan`.  ``p`` as there.

    Autograd (``p=2`` only): when grad mode is on and one of ``x, y, G`` requires grad, the result carries a ``grad_fn`` and
    ``(barycentric_map(x, y, F, G, blur) - target).pow(2).sum().backward()`` fills ``x.grad``, ``y.grad`` and ``G.grad`` in the dtype
    of each input (``F`` gets none: the map does not depend on it), for clouds of any dimension D <= 4095, through
    :func:`geomloss_amd.hip.plan_bilinear` with D + 1 features.  ``b`` is detached; the backward pass is once-differentiable.
    Otherwise — and always for ``p=1`` — the call runs as before and returns a tensor without ``grad_fn``."""
    eps = _eps(blur, p)
    if p == 2:
        if _wants_grad(x, y, G):
            return _BarycentricMap.apply(x, y, G, eps, b)
        return _map_p2(x, y, G, eps, b, False)[0]
    with torch.no_grad():
        Gf = G.detach().float().reshape(y.shape[:-1])
        h = _log_weights(b, Gf, y.shape[-2]) + Gf / eps
        return hip.plan_apply_p1(eps, x, y, h, y.detach().float())


def plan_argmax(x, y, F, G, blur, b=None):
    """``argmax_j P_ij`` int32 (N,)|(B,N): the column that receives most of the mass of row i — a hard correspondence where
    :func:`barycentric_map` gives an average.  It is ``argmin_j [|x_i - y_j|^2 / 2 - G_j - blur^2 log b_j]``
    (:func:`geomloss_amd.hip.argmin`); columns of zero weight are never returned, ties go to the smallest index.  Like the
    barycentric map it does not depend on ``a`` or ``F``; ``F`` is accepted so that the call reads like :func:`apply_plan`."""
    eps = float(blur) ** 2
    with torch.no_grad():
        Gf = G.detach().float().reshape(y.shape[:-1])
        return hip.argmin(x, y, Gf + eps * _log_weights(b, Gf, y.shape[-2]))


def plan_topk(x, y, F, G, blur, k, a=None, b=None, p=2):
    """The ``k`` heaviest entries of every row of the plan: ``(index, weight)``, int32 and fp32 (N,k)|(B,N,k), heaviest first, with
    ``weight[i, r] = P[i, index[i, r]]``.  One top-k arg-reduction (:func:`geomloss_amd.hip.argkmin`) of
    ``|x_i - y_j|^2 / 2 - G_j - blur^2 log b_j``, whose values give the weights as ``a_i exp((F_i - value_ir) / blur^2)``: nothing of
    size N x M is stored.  Columns of zero weight are never returned; a row with fewer than k columns of positive weight has index -1 and
    weight 0 in its last ranks; equal entries come in ascending column order.  1 <= k <= ``hip.ARGKMIN_MAX_K``; ``p=1`` raises
    ``NotImplementedError`` (the arg-reduction has the squared cost only).

    As a sparse matrix (unbatched, every rank filled)::

        rows = torch.arange(N, device=index.device).repeat_interleave(k)
        P_k = torch.sparse_coo_tensor(torch.stack((rows, index.reshape(-1).long())), weight.reshape(-1), (N, M))

    and the share of every row's mass that its k entries keep (``fwd`` is the soft-min :func:`apply_plan` starts from)::

        fwd = hip.softmin(blur**2, x, y, G / blur**2 + b.log())
        share = weight.sum(-1) / (a * ((F - fwd) / blur**2).exp())
    """
    if p != 2:
        raise NotImplementedError(f"geomloss_amd.transport.plan_topk: only the plans of p = 2 (got p = {p!r})")
    eps = float(blur) ** 2
    with torch.no_grad():
        Ff = F.detach().float().reshape(x.shape[:-1])
        Gf = G.detach().float().reshape(y.shape[:-1])
        index, value = hip.argkmin(x, y, k, Gf + eps * _log_weights(b, Gf, y.shape[-2]), return_value=True)
        la = _log_weights(a, Ff, x.shape[-2]).to(value.device)
        weight = (la.unsqueeze(-1) + (Ff.to(value.device).unsqueeze(-1) - value) / eps).exp()
        return index, torch.where(index >= 0, weight, torch.zeros_like(weight))
