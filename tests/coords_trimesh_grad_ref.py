"""An independent restatement of what coords.from_triangles interpolates, for the tests of its adjoint.  It imports
nothing of the library: given the WINNING-FACE plane of a forward (the face index of every pixel, -1 in a hole) it restates the
interpolation of the attribute in torch float64 on the CPU -- barycentrics from the three edge functions, affine or
perspective-correct with w -- and takes the gradients of sum(u * grad_out) over the covered pixels by autograd.  Visibility is
fixed: the plane is data, so coverage and the depth test get no gradient, which is the adjoint's contract."""
import numpy as np
import torch


def _edge(P, Q, q):
    """(Q - P) x (q - P) in (row, col)"""
    return (Q[:, 1] - P[:, 1]) * (q[:, 0] - P[:, 0]) - (Q[:, 0] - P[:, 0]) * (q[:, 1] - P[:, 1])


def interpolate(face_plane, pos, attr, faces, attr_faces=None, w=None, origin=(0, 0)):
    """-> (u [n, 2], rows, cols): the attribute at the n covered pixels of face_plane [oH, oW] (int64, -1 = hole), in row-major
    order; pos, attr (and w) are float64 torch tensors, which may require grad"""
    plane = torch.as_tensor(np.asarray(face_plane).astype(np.int64))
    rows, cols = torch.nonzero(plane >= 0, as_tuple=True)
    f = plane[rows, cols]
    fc = torch.as_tensor(np.asarray(faces).astype(np.int64))
    af = fc if attr_faces is None else torch.as_tensor(np.asarray(attr_faces).astype(np.int64))
    q = torch.stack([(rows + int(origin[0])).double(), (cols + int(origin[1])).double()], dim=1)
    A, B, C = pos[fc[f, 0]], pos[fc[f, 1]], pos[fc[f, 2]]
    area2 = _edge(A, B, C)
    lb, lc = _edge(C, A, q) / area2, _edge(A, B, q) / area2
    lam = torch.stack([1.0 - lb - lc, lb, lc], dim=1)
    a = torch.stack([attr[af[f, 0]], attr[af[f, 1]], attr[af[f, 2]]], dim=1)          # [n, 3, 2]
    if w is not None:
        lam = lam / torch.stack([w[fc[f, 0]], w[fc[f, 1]], w[fc[f, 2]]], dim=1)
        lam = lam / lam.sum(dim=1, keepdim=True)
    return (lam[:, :, None] * a).sum(dim=1), rows, cols


def gradients(face_plane, pos, attr, faces, grad_out, attr_faces=None, w=None, origin=(0, 0)):
    """-> (grad_attr [Va, 2], grad_pos [V, 2], grad_w [V] or None) as float64 numpy arrays: d sum(u * grad_out) / d operand, grad_out
    [oH, oW, 2] read at covered pixels only (it may hold NaN in the holes)"""
    P = torch.tensor(np.asarray(pos, dtype=np.float64), requires_grad=True)
    Aq = torch.tensor(np.asarray(attr, dtype=np.float64), requires_grad=True)
    Wq = None if w is None else torch.tensor(np.asarray(w, dtype=np.float64), requires_grad=True)
    u, rows, cols = interpolate(face_plane, P, Aq, faces, attr_faces, Wq, origin)
    g = torch.as_tensor(np.asarray(grad_out, dtype=np.float64))[rows, cols]
    if u.shape[0] == 0:
        return np.zeros(Aq.shape), np.zeros(P.shape), None if Wq is None else np.zeros(Wq.shape)
    (u * g).sum().backward()
    zero = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy().copy()
    return zero(Aq), zero(P), None if Wq is None else zero(Wq)


def within(got, ref):
    """(largest |got - ref|, the family's bound 1e-9 * max(max |ref|, 1))"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max()) if got.size else 0.0, 1e-9 * max(float(np.abs(ref).max()) if ref.size else 0.0, 1.0)
