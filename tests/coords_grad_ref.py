"""Yardstick of the adjoints of compose and invert, independent of the package: float64 torch restatements whose autograd is the
reference gradient.

compose_ref is the plain four-term bilinear formula with torch.clamp for the clip and the cell index i0 = min(floor(r), n - 2) as
a detached index tensor.  It has NO `where` on zero weights: the forward's "a tap of weight exactly 0 is not read" is a NaN rule of
the forward, and a `where` would zero the derivative at every integer position.  invert_ift_ref is one Newton step from the
detached inverse G with a detached Jacobian, G - J^-1 (F(G) - q): its value is G (up to the solver's residual) and its autograd
is the implicit-function gradient of F(G[q]) = q.  tests/test_coords_grad_cpu.py anchors compose_ref's forward on
coords_ref.compose before it holds the library against these."""
import torch


def _axis(v, n):
    r = torch.clamp(v, 0.0, float(n - 1))
    i0 = torch.clamp(torch.floor(r.detach()), max=float(n - 2)).long()
    t = r - i0.to(r.dtype)
    return i0, 1.0 - t, t


def _corners(a, i0, j0):
    return a[i0, j0], a[i0, j0 + 1], a[i0 + 1, j0], a[i0 + 1, j0 + 1]


def compose_ref(outer, inner):
    """C[i, j] = outer(inner[i, j]): outer [aH, aW, 2] (aH, aW >= 2), inner [oH, oW, 2] finite; float64; differentiable in both"""
    a, b = outer.double(), inner.double()
    i0, wr0, wr1 = _axis(b[..., 0], a.shape[0])
    j0, wc0, wc1 = _axis(b[..., 1], a.shape[1])
    p00, p01, p10, p11 = _corners(a, i0, j0)
    return wr0[..., None] * (wc0[..., None] * p00 + wc1[..., None] * p01) + wr1[..., None] * (wc0[..., None] * p10 + wc1[..., None] * p11)


def jacobian(outer, pos):
    """(Jr, Jc) = (dC/drow, dC/dcol) [oH, oW, 2] each, of the bilinear patch of `outer` at the positions `pos`"""
    a, b = outer.double(), pos.double()
    i0, wr0, wr1 = _axis(b[..., 0], a.shape[0])
    j0, wc0, wc1 = _axis(b[..., 1], a.shape[1])
    p00, p01, p10, p11 = _corners(a, i0, j0)
    return wc0[..., None] * (p10 - p00) + wc1[..., None] * (p11 - p01), wr0[..., None] * (p01 - p00) + wr1[..., None] * (p11 - p10)


def invert_ift_ref(F, G, origin=(0, 0)):
    """One Newton step from the detached inverse G [H, W, 2] (finite) of F [fH, fW, 2]: differentiable in F; d/dF is the
    implicit-function gradient"""
    G = G.detach().double()
    H, W = G.shape[:2]
    ii = torch.arange(H, dtype=torch.float64, device=G.device) + origin[0]
    jj = torch.arange(W, dtype=torch.float64, device=G.device) + origin[1]
    q = torch.stack(torch.meshgrid(ii, jj, indexing="ij"), dim=-1)
    Jr, Jc = jacobian(F.detach(), G)
    det = Jr[..., 0] * Jc[..., 1] - Jr[..., 1] * Jc[..., 0]
    e = compose_ref(F, G) - q
    step_r = (e[..., 0] * Jc[..., 1] - Jc[..., 0] * e[..., 1]) / det
    step_c = (Jr[..., 0] * e[..., 1] - Jr[..., 1] * e[..., 0]) / det
    return G - torch.stack([step_r, step_c], dim=-1)
