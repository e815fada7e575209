"""Yardstick of the fisheye and equirectangular map models, independent of the package: numpy and torch float64 restatements of the
two models of csrc/lerf_coords_models.h as functions of their parameter VECTOR, with np.sqrt / np.arctan / np.arctan2 (torch.sqrt /
torch.atan / torch.atan2) where the library uses its own sqrt_pm / atan_pm / atan2_pm.  The torch forms exist for autograd: their
gradient is the reference of the hand-written backward.  Nothing here imports the library.

    fisheye   p = m[9] (inv(new_K . R)), fx, fy, cx, cy, k1, k2, k3, k4          cv::fisheye::initUndistortRectifyMap, no skew
    equirect  p = m[9] (inv(K_view . R)), sx, sy, cxp, cyp                       a pinhole view of an equirectangular panorama

`cases` are the parameter sets both suites use; `divisors` is what the tests assert about them before a gradient is compared: every
quantity the backward divides by (Wh and r of the fisheye, h of the equirect view) stays away from zero over the map."""
import numpy as np
import torch

N_PARAMS = {"fisheye": 17, "equirect": 13}

FISH_K = np.array([[61.5, 0.0, 25.25], [0.0, 58.75, 17.5], [0.0, 0.0, 1.0]])
FISH_NEW_K = np.array([[35.0, 0.0, 27.5], [0.0, 33.0, 16.0], [0.0, 0.0, 1.0]])
FISH_DIST = np.array([0.05, -0.012, 0.004, -0.0009])
VIEW_K = np.array([[70.0, 0.0, 24.5], [0.0, 66.0, 19.25], [0.0, 0.0, 1.0]])
PANO_HW = (96, 192)


def rotation(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    return np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ \
        np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])


FISH_R = rotation(0.02, -0.03, 0.01)
VIEW_R = rotation(0.3, -0.5, 0.1)


def fisheye_params_np(K, dist4, R=None, new_K=None):
    R = np.eye(3) if R is None else R
    new_K = K if new_K is None else new_K
    return np.concatenate([np.linalg.inv(new_K @ R).reshape(9), [K[0, 0], K[1, 1], K[0, 2], K[1, 2]], dist4])


def pano_scalars(pano_hw):
    Hp, Wp = pano_hw
    return np.array([Wp / (2.0 * np.pi), Hp / np.pi, (Wp - 1) / 2.0, (Hp - 1) / 2.0])


def equirect_params_np(pano_hw, K_view, R=None):
    R = np.eye(3) if R is None else R
    return np.concatenate([np.linalg.inv(K_view @ R).reshape(9), pano_scalars(pano_hw)])


def cases(scale_to=None):
    """{model: float64 parameter vector}.  The fisheye view's new_K is stretched so that a map of scale_to = (H, W) pixels (origin
    included) spans the field of view a 48 x 144 map spans at the plain new_K -- every tile of every size stays in front of the
    camera and inside the lens; the equirect view's K likewise"""
    f = 1.0 if scale_to is None else max(1.0, scale_to[0] / 48.0, scale_to[1] / 144.0)
    return {"fisheye": fisheye_params_np(FISH_K, FISH_DIST, FISH_R, FISH_NEW_K * np.array([[f], [f], [1.0]])),
            "equirect": equirect_params_np(PANO_HW, VIEW_K * np.array([[f], [f], [1.0]]), VIEW_R)}


# ---------------------------------------------------------------------------------------------- numpy
def _grid_np(hw, origin):
    return np.meshgrid(np.arange(hw[0], dtype=np.float64) + origin[0], np.arange(hw[1], dtype=np.float64) + origin[1], indexing="ij")


def model_map_np(model, p, hw, origin=(0, 0)):
    """[oH, oW, 2] float64 of one parameter vector"""
    p = np.asarray(p, np.float64)
    v, u = _grid_np(hw, origin)
    X = p[0] * u + p[1] * v + p[2]
    Y = p[3] * u + p[4] * v + p[5]
    Z = p[6] * u + p[7] * v + p[8]
    with np.errstate(all="ignore"):
        if model == "fisheye":
            fx, fy, cx, cy, k1, k2, k3, k4 = p[9:]
            x, y = X / Z, Y / Z
            r = np.sqrt(x * x + y * y)
            th = np.arctan(r)
            th2 = th * th
            thd = th * (1 + th2 * (k1 + th2 * (k2 + th2 * (k3 + th2 * k4))))
            s = np.where(r == 0, 1.0, thd / np.where(r == 0, 1.0, r))
            out = np.stack([fy * (y * s) + cy, fx * (x * s) + cx], axis=-1)
            out[~(Z > 0)] = np.nan
            return out
        assert model == "equirect", model
        sx, sy, cxp, cyp = p[9:]
        lon = np.arctan2(X, Z)
        lat = np.arctan2(Y, np.sqrt(X * X + Z * Z))
        return np.stack([cyp + sy * lat, cxp + sx * lon], axis=-1)


# ---------------------------------------------------------------------------------------------- torch
def _grid(p, hw, origin):
    ii = torch.arange(hw[0], dtype=torch.float64, device=p.device) + float(origin[0])
    jj = torch.arange(hw[1], dtype=torch.float64, device=p.device) + float(origin[1])
    return torch.meshgrid(ii, jj, indexing="ij")


def _one(model, p, hw, origin):
    """(map [oH, oW, 2], the quantities its backward divides by) of ONE parameter set; smooth entries only (no select: r = 0, h = 0
    and Wh <= 0 are the caller's to keep out)"""
    v, u = _grid(p, hw, origin)
    X = p[0] * u + p[1] * v + p[2]
    Y = p[3] * u + p[4] * v + p[5]
    Z = p[6] * u + p[7] * v + p[8]
    if model == "fisheye":
        fx, fy, cx, cy, k1, k2, k3, k4 = p[9:]
        x, y = X / Z, Y / Z
        r = torch.sqrt(x * x + y * y)
        th = torch.atan(r)
        th2 = th * th
        s = th * (1 + th2 * (k1 + th2 * (k2 + th2 * (k3 + th2 * k4)))) / r
        return torch.stack([fy * (y * s) + cy, fx * (x * s) + cx], dim=-1), [Z, r]
    assert model == "equirect", model
    sx, sy, cxp, cyp = p[9:]
    h = torch.sqrt(X * X + Z * Z)
    return torch.stack([cyp + sy * torch.atan2(Y, h), cxp + sx * torch.atan2(X, Z)], dim=-1), [h]


def model_map(model, params, hw, origin=(0, 0)):
    """params float64 tensor [n] -> [oH, oW, 2], [B, n] -> [B, oH, oW, 2]; differentiable in params"""
    p = params.double()
    if p.ndim == 1:
        return _one(model, p, hw, origin)[0]
    return torch.stack([_one(model, q, hw, origin)[0] for q in p])


def divisors(model, params, hw, origin=(0, 0)):
    """min over the map of ONE parameter set of the quantities the backward divides by: min(Wh) (signed: it must stay positive) and
    min r for the fisheye, min h for the equirect view (numpy in, float out)"""
    with torch.no_grad():
        return min(float(d.min()) for d in _one(model, torch.from_numpy(np.asarray(params, np.float64)), hw, origin)[1])


def params_grad_ref(model, params, g, hw, origin=(0, 0)):
    """grad_params by autograd of the restatement (numpy in and out)"""
    p = torch.from_numpy(np.asarray(params, np.float64)).requires_grad_(True)
    gp, = torch.autograd.grad((model_map(model, p, hw, origin) * torch.from_numpy(np.asarray(g, np.float64))).sum(), p)
    return gp.numpy()


def camera_params_ref(K, dist, R, new_K):
    """coords.fisheye_params in torch ops: inv(new_K . R)[9], fx, fy, cx, cy, dist -> [13 + len(dist)] (or [B, ..] when an operand
    carries a leading B); differentiable in all four"""
    K, dist, R, new_K = (t.double() for t in (K, dist, R, new_K))
    B = max([t.shape[0] for t, nd in ((K, 3), (dist, 2), (R, 3), (new_K, 3)) if t.ndim == nd] + [0])
    lead = (B,) if B else ()
    K, R, new_K = (t.expand(lead + (3, 3)) for t in (K, R, new_K))
    dist = dist.expand(lead + (dist.shape[-1],))
    cam = torch.stack([K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2]], dim=-1)
    return torch.cat([torch.linalg.inv(new_K @ R).reshape(lead + (9,)), cam, dist], dim=-1)


def equirect_params_ref(pano_hw, K_view, R):
    K_view, R = K_view.double(), R.double()
    lead = tuple(K_view.shape[:-2]) if K_view.ndim == 3 else tuple(R.shape[:-2]) if R.ndim == 3 else ()
    minv = torch.linalg.inv(K_view @ R).expand(lead + (3, 3))
    pano = torch.from_numpy(pano_scalars(pano_hw)).to(K_view.device).expand(lead + (4,))
    return torch.cat([minv.reshape(lead + (9,)), pano], dim=-1)
