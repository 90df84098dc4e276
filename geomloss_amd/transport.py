"""Using the transport plan behind the dual potentials of the legacy API.

``F, G = SamplesLoss("sinkhorn", p=2, blur=blur, potentials=True, debias=False)(a, x, b, y)`` describes the entropic plan

    P_ij = a_i b_j exp((F_i + G_j - |x_i - y_j|^2 / 2) / blur^2)

without ever forming it.  The functions below push features through that plan — labels, colours, the barycentric map — with one
soft-min reduction and one matrix-core application of the plan (:func:`geomloss_amd.hip.plan_apply_nd`), at any N, M the solver
itself handles.  GPU tensors only, like the ``online`` backend; p = 2, float32 / bfloat16 clouds of dimension D <= 4095: D <= 16 on
the kernel with resident operands (up to 128 feature columns per pass), 17 <= D <= 4095 — principal components, embeddings — on the
K-chunked kernel (64 per pass); beyond, ``NotImplementedError``.  Nothing here is recorded by autograd.

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


def apply_plan(x, y, F, G, feat, blur, a=None, b=None, transpose=False, p=2):
    """``sum_j P_ij feat_j`` for the plan of the potentials ``F`` (N,)|(B,N), ``G`` (M,)|(B,M) on the clouds ``x`` (N,D)|(B,N,D),
    ``y`` (M,D)|(B,M,D) with weights ``a``, ``b`` (uniform by default): feat (M,V)|(B,M,V)|(M,) -> (N,V)|(B,N,V)|(N,) fp32.
    ``transpose=True`` applies the transposed plan instead: ``sum_i P_ij feat_i`` for feat on the rows, (N,V) -> (M,V).
    ``p=1``: the plan of the cost |x_i - y_j| at temperature ``blur`` — ONE launch (:func:`geomloss_amd.hip.plan_apply_p1`), which
    returns the row sums' soft-min next to the average.  Any other ``p`` than 1 or 2 raises ``ValueError``."""
    if transpose:
        return apply_plan(y, x, G, F, feat, blur, a=b, b=a, p=p)
    eps = _eps(blur, p)
    with torch.no_grad():
        N, M = x.shape[-2], y.shape[-2]
        Ff = F.detach().float().reshape(x.shape[:-1])
        Gf = G.detach().float().reshape(y.shape[:-1])
        h = _log_weights(b, Gf, M) + Gf / eps
        if p == 1:
            avg, fwd = hip.plan_apply_p1(eps, x, y, h, feat, want_softmin=True)      # sum_j b_j exp((G_j - C_ij) / eps) = exp(-fwd_i / eps)
            rows = (_log_weights(a, Ff, N) + (Ff - fwd) / eps).exp()                  # sum_j P_ij
            return rows * avg if avg.dim() == rows.dim() else rows.unsqueeze(-1) * avg
        fwd = hip.softmin(eps, x.detach(), y.detach(), h)              # sum_j b_j exp((G_j - C_ij) / eps) = exp(-fwd_i / eps)
        avg = hip.plan_apply_nd(eps, x, y, h, feat, fwd=fwd)
        rows = (_log_weights(a, Ff, N) + (Ff - fwd) / eps).exp()       # sum_j P_ij
        return rows * avg if avg.dim() == rows.dim() else rows.unsqueeze(-1) * avg


def barycentric_map(x, y, F, G, blur, b=None, p=2):
    """``T(x_i) = sum_j P_ij y_j / sum_j P_ij`` (N,D)|(B,N,D) fp32: where the plan sends each x_i on average.  The row-normalised
    average does not depend on ``a`` or ``F`` (they scale a whole row); ``F`` is accepted so that the call reads like
    :func:`apply_plan`.  ``p`` as there."""
    eps = _eps(blur, p)
    with torch.no_grad():
        Gf = G.detach().float().reshape(y.shape[:-1])
        h = _log_weights(b, Gf, y.shape[-2]) + Gf / eps
        if p == 1:
            return hip.plan_apply_p1(eps, x, y, h, y.detach().float())
        return hip.plan_apply_nd(eps, x, y, h, y.detach().float())


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
