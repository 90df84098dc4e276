"""What the tests of ``hip.plan_bilinear`` and of the autograd functions of ``geomloss_amd.transport`` share: the float64 reference of the
primitive and its error measure, dense float64 torch versions of ``apply_plan`` / ``barycentric_map`` for autograd oracles, and dense
float32 CPU stand-ins with the signatures of ``hip.softmin``, ``hip.plan_apply_nd`` and ``hip.plan_bilinear``.  A plain module; the
clouds come from ``cloud_support``."""
import numpy as np
import torch

from cloud_support import clouds  # noqa: F401  (re-exported: the tests draw their clouds here)


def _sq_half(x, y):
    """|x_i - y_j|^2 / 2 on explicit differences, (..., N, M)."""
    return ((x.unsqueeze(-2) - y.unsqueeze(-3)) ** 2).sum(-1) / 2


# ---- the primitive -------------------------------------------------------------------------------------------------------------------

def bilinear_ref(x, y, h, eps, rowfeat, colfeat, budget=2e7):
    """float64, explicit differences, row-chunked: ``(out, wsum, unsigned_out, unsigned_w)`` for unbatched NumPy inputs, with
    unsigned_out[i, d] = sum_j pi_ij |tau_ij| |y_j[d] - x_i[d]| and unsigned_w[i] = sum_j pi_ij |tau_ij|.  Rows without mass give 0."""
    x, y, h, rf, cf = (torch.as_tensor(np.asarray(t), dtype=torch.float64) for t in (x, y, h, rowfeat, colfeat))
    N, D = x.shape
    M = y.shape[0]
    rows = max(1, int(budget // max(1, M * D)))
    out, wsum, uo, uw = torch.zeros(N, D, dtype=torch.float64), torch.zeros(N, dtype=torch.float64), torch.zeros(N, D, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    for i0 in range(0, N, rows):
        xi = x[i0:i0 + rows]
        diff = y.unsqueeze(0) - xi.unsqueeze(1)                        # (r, M, D)
        E = h.unsqueeze(0) - (diff ** 2).sum(-1) / (2 * eps)
        m = E.max(1, keepdim=True).values
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        W = (E - m).exp()
        s = W.sum(1, keepdim=True)
        pi = W / torch.where(s > 0, s, torch.ones_like(s))
        tau = rf[i0:i0 + rows] @ cf.T
        q = torch.where(pi > 0, pi * tau, torch.zeros_like(pi))        # a column without mass weighs 0 whatever it holds
        out[i0:i0 + rows] = (q.unsqueeze(-1) * diff).sum(1)
        wsum[i0:i0 + rows] = q.sum(1)
        uo[i0:i0 + rows] = (q.abs().unsqueeze(-1) * diff.abs()).sum(1)
        uw[i0:i0 + rows] = q.abs().sum(1)
    return out.numpy(), wsum.numpy(), uo.numpy(), uw.numpy()


def bilinear_dense(x, y, h, eps, rowfeat, colfeat, dtype=torch.float32):
    """The same expression in plain dense torch arithmetic of ``dtype`` — expanded squared distances, a soft-max, two matrix products:
    the yardstick e32 of the parity tests.  Unbatched or batched tensors / arrays -> (out, wsum) tensors."""
    x, y, h, rf, cf = (torch.as_tensor(np.asarray(t)).to(dtype) for t in (x, y, h, rowfeat, colfeat))
    E = h.unsqueeze(-2) - ((x * x).sum(-1).unsqueeze(-1) - 2 * x @ y.transpose(-1, -2) + (y * y).sum(-1).unsqueeze(-2)) / (2 * eps)
    m = E.max(-1, keepdim=True).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    W = (E - m).exp()
    s = W.sum(-1, keepdim=True)
    pi = W / torch.where(s > 0, s, torch.ones_like(s))
    q = torch.where(pi > 0, pi * (rf @ cf.transpose(-1, -2)), torch.zeros_like(pi))
    wsum = q.sum(-1)
    return q @ y - x * wsum.unsqueeze(-1), wsum


def bilinear_errors(out, wsum, ref):
    """The error measure of the primitive, relative to the unsigned sums: ``(max |out - ref| / max_{i,d} unsigned_out,
    max |wsum - ref| / max_i unsigned_w)``; ``ref`` = what :func:`bilinear_ref` returns."""
    ro, rw, uo, uw = ref
    out, wsum = np.asarray(out, np.float64), np.asarray(wsum, np.float64)
    return (float(np.abs(out - ro).max() / max(uo.max(), 1e-300)), float(np.abs(wsum - rw).max() / max(uw.max(), 1e-300)))


# ---- dense float64 torch versions, for autograd oracles ----------------------------------------------------------------------------

def _weights(w, like, count):
    return torch.full_like(like, 1.0 / count) if w is None else w.to(like.dtype).reshape(like.shape)


def dense_plan(x, y, F, G, eps, a=None, b=None):
    """P_ij = a_i b_j exp((F_i + G_j - |x_i - y_j|^2 / 2) / eps), (..., N, M), differentiable in x, y, F, G."""
    F, G = F.reshape(x.shape[:-1]), G.reshape(y.shape[:-1])
    a, b = _weights(a, F, x.shape[-2]), _weights(b, G, y.shape[-2])
    return a.unsqueeze(-1) * b.unsqueeze(-2) * ((F.unsqueeze(-1) + G.unsqueeze(-2) - _sq_half(x, y)) / eps).exp()


def dense_apply_plan(x, y, F, G, feat, eps, a=None, b=None, transpose=False):
    P = dense_plan(x, y, F, G, eps, a, b)
    if transpose:
        P = P.transpose(-1, -2)
    return (P @ feat.unsqueeze(-1))[..., 0] if feat.dim() == P.dim() - 1 else P @ feat


def dense_barycentric_map(x, y, G, eps, b=None):
    P = dense_plan(x, y, torch.zeros_like(x[..., 0]), G, eps, None, b)
    return (P / P.sum(-1, keepdim=True)) @ y


# ---- dense float32 CPU stand-ins for the three entry points the autograd functions reach -------------------------------------------

class DenseHip:
    """``softmin``, ``plan_apply_nd`` and ``plan_bilinear`` with the signatures of ``geomloss_amd.hip``, in dense float32 torch on
    whatever device the inputs live on, without a graph; ``calls`` counts them by name."""

    def __init__(self):
        self.calls = {"softmin": 0, "plan_apply_nd": 0, "plan_bilinear": 0}

    @staticmethod
    def _exponents(eps, x, y, h):
        return h.float().unsqueeze(-2) - _sq_half(x.float(), y.float()) / eps

    def softmin(self, eps, x, y, h, p=2, ranges=None, flags=0):
        assert p == 2 and ranges is None
        self.calls["softmin"] += 1
        with torch.no_grad():
            return -eps * torch.logsumexp(self._exponents(eps, x, y, h), -1)

    def plan_apply_nd(self, eps, x, y, h, feat, fwd=None, flags=0, p=2, ranges=None):
        assert p == 2 and ranges is None
        self.calls["plan_apply_nd"] += 1
        with torch.no_grad():
            pi = torch.softmax(self._exponents(eps, x, y, h), -1)
            f = feat.detach().float()
            return (pi @ f.unsqueeze(-1))[..., 0] if f.dim() == pi.dim() - 1 else pi @ f

    def plan_bilinear(self, eps, x, y, h, rowfeat, colfeat, fwd=None, flags=0, p=2, ranges=None):
        assert p == 2 and ranges is None
        self.calls["plan_bilinear"] += 1
        with torch.no_grad():
            x, y = x.detach().float(), y.detach().float()
            q = torch.softmax(self._exponents(eps, x, y, h), -1) * (rowfeat.detach().float() @ colfeat.detach().float().transpose(-1, -2))
            diff = y.unsqueeze(-3) - x.unsqueeze(-2)
            return (q.unsqueeze(-1) * diff).sum(-2), q.sum(-1)

    def install(self, monkeypatch):
        from geomloss_amd import hip
        for name in self.calls:
            monkeypatch.setattr(hip, name, getattr(self, name))
        return self
