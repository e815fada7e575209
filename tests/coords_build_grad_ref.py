"""Yardstick of the adjoint of the model builders, independent of the package: float64 torch restatements of the three models of
csrc/lerf_coords_models.h (homography, radial, brown) as functions of their parameter VECTOR, and of coords.brown_params as a
function of the camera operands.  Their autograd is the reference gradient; their forward is anchored on the library's host forward
by tests/test_coords_build_grad_cpu.py before anything is held against them.  Every function takes one parameter set ([n]) or a
batch ([B, n]) and returns [oH, oW, 2] or [B, oH, oW, 2].

`cases` are the parameter sets both suites use, and `denominators` what the tests assert about them: every divisor of every entry
stays away from zero over the maps tested, so the models are smooth there and central differences are meaningful."""
import numpy as np
import torch

N_PARAMS = {"homography": 9, "radial": 8, "brown": 21}
M_ISC = np.array([[2.05, 0.12, 15.0], [-0.08, 1.95, 40.0], [1.5e-5, -1.0e-5, 1.0]])          # BASELINE config 4
RADIAL_IN_HW, RADIAL_K, RADIAL_CENTRE = (40, 64), (-0.18, 0.03), (19.3, 30.9)
BROWN_K = np.array([[61.5, 0.0, 25.25], [0.0, 58.75, 17.5], [0.0, 0.0, 1.0]])
BROWN_NEW_K = np.array([[55.0, 0.0, 27.5], [0.0, 53.0, 16.0], [0.0, 0.0, 1.0]])
BROWN_DIST = np.array([0.11, -0.04, 0.002, -0.003, 0.013, 0.02, -0.007, 0.001])            # all eight non-zero, small


def rotation(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    return np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ \
        np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])


BROWN_R = rotation(0.02, -0.03, 0.01)


def radial_params(in_hw, out_hw, k1, k2, centre):
    """cr, cc, no, ni, hr, hc, k1, k2 of coords.radial (the scalars of the WHOLE output out_hw)"""
    (H, W), (oH, oW) = in_hw, out_hw
    return np.array([centre[0], centre[1], np.hypot(oH, oW) / 2.0, np.hypot(H, W) / 2.0, (oH - 1) / 2.0, (oW - 1) / 2.0, k1, k2])


def brown_params_np(K, dist, R, new_K):
    return np.concatenate([np.linalg.inv(new_K @ R).reshape(9), [K[0, 0], K[1, 1], K[0, 2], K[1, 2]], dist])


def cases(full_hw):
    """{model: float64 parameter vector}; radial's geometry scalars are those of a whole output of full_hw"""
    return {"homography": np.linalg.inv(M_ISC).reshape(9),
            "radial": radial_params(RADIAL_IN_HW, full_hw, RADIAL_K[0], RADIAL_K[1], RADIAL_CENTRE),
            "brown": brown_params_np(BROWN_K, BROWN_DIST, BROWN_R, BROWN_NEW_K)}


def _grid(p, hw, origin):
    ii = torch.arange(hw[0], dtype=torch.float64, device=p.device) + float(origin[0])
    jj = torch.arange(hw[1], dtype=torch.float64, device=p.device) + float(origin[1])
    return torch.meshgrid(ii, jj, indexing="ij")


def _project(m, x, y):
    X = m[0] * x + m[1] * y + m[2]
    Y = m[3] * x + m[4] * y + m[5]
    Wh = m[6] * x + m[7] * y + m[8]
    return X / Wh, Y / Wh, Wh


def _one(model, p, hw, origin, mask=None):
    """(map [oH, oW, 2], the divisors of its entries as a list of tensors) of ONE parameter set.  mask [oH, oW] bool: those entries
    are evaluated at the first unmasked pixel instead of their own (a `where` on the RESULT would still send 0 * inf = NaN back
    through a division by zero), so the caller can leave them out of a loss"""
    y, x = _grid(p, hw, origin)
    if mask is not None:
        keep = (~mask).nonzero()[0]
        y, x = torch.where(mask, y[keep[0], keep[1]], y), torch.where(mask, x[keep[0], keep[1]], x)
    if model == "homography":
        col, row, Wh = _project(p, x, y)
        return torch.stack([row, col], dim=-1), [Wh]
    if model == "radial":
        cr, cc, no, ni, hr, hc, k1, k2 = p
        ur, uc = (y - hr) / no, (x - hc) / no
        r2 = ur * ur + uc * uc
        f = 1 + k1 * r2 + k2 * r2 * r2
        return torch.stack([cr + ur * f * ni, cc + uc * f * ni], dim=-1), [no.expand(hw)]
    assert model == "brown", model
    u, v, Wh = _project(p[:9], x, y)
    fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 = p[9:]
    r2 = u * u + v * v
    den = 1 + r2 * (k4 + r2 * (k5 + r2 * k6))
    rad = (1 + r2 * (k1 + r2 * (k2 + r2 * k3))) / den
    xd = u * rad + 2 * p1 * u * v + p2 * (r2 + 2 * u * u)
    yd = v * rad + p1 * (r2 + 2 * v * v) + 2 * p2 * u * v
    return torch.stack([fy * yd + cy, fx * xd + cx], dim=-1), [Wh, den]


def model_map(model, params, hw, origin=(0, 0), mask=None):
    """the map of `model`: params float64 tensor [n] -> [oH, oW, 2], [B, n] -> [B, oH, oW, 2]; differentiable in params.  mask
    (bool, the map's shape without its last axis): entries evaluated elsewhere, see _one"""
    p = params.double()
    if p.ndim == 1:
        return _one(model, p, hw, origin, mask)[0]
    return torch.stack([_one(model, q, hw, origin, None if mask is None else mask[b])[0] for b, q in enumerate(p)])


def denominators(model, params, hw, origin=(0, 0)):
    """min |divisor| over every entry of the map of ONE parameter set (numpy in, float out)"""
    with torch.no_grad():
        return min(float(d.abs().min()) for d in _one(model, torch.from_numpy(np.asarray(params, np.float64)), hw, origin)[1])


def brown_params_ref(K, dist, R, new_K):
    """coords.brown_params in torch ops: inv(new_K . R)[9], fx, fy, cx, cy, dist padded to 8 -> [21] (or [B, 21] when any operand
    carries a leading B); differentiable in all four"""
    K, dist, R, new_K = (t.double() for t in (K, dist, R, new_K))
    B = max([t.shape[0] for t, nd in ((K, 3), (dist, 2), (R, 3), (new_K, 3)) if t.ndim == nd] + [0])
    lead = (B,) if B else ()
    K, R, new_K = (t.expand(lead + (3, 3)) for t in (K, R, new_K))
    dist = dist.expand(lead + (dist.shape[-1],))
    minv = torch.linalg.inv(new_K @ R)
    pad = torch.zeros(lead + (8 - dist.shape[-1],), dtype=torch.float64, device=dist.device)
    cam = torch.stack([K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2]], dim=-1)
    return torch.cat([minv.reshape(lead + (9,)), cam, dist, pad], dim=-1)


def params_grad_ref(model, params, g, hw, origin=(0, 0), mask=None):
    """grad_params by autograd of the restatement (numpy in and out); mask [.., oH, oW] bool: entries left out of the loss (their
    upstream gradient is ignored, whatever it holds)"""
    p = torch.from_numpy(np.asarray(params, np.float64)).requires_grad_(True)
    w = torch.from_numpy(np.asarray(g, np.float64))
    if mask is not None:
        mask = torch.from_numpy(np.asarray(mask, bool))
        w = torch.where(mask[..., None], torch.zeros((), dtype=torch.float64), w)
    gp, = torch.autograd.grad((model_map(model, p, hw, origin, mask) * w).sum(), p)
    return gp.numpy()
