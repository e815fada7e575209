"""Coordinate-map builders for the remap (ops.RemapGeometry, LerfEngine.remap).

A map is a float64 (or float32) array [oH, oW, 2]; entry (i, j) is (row, col) of the source position of output pixel
(i, j), in the reference's convention: integers are pixel indices, the values are what Warp2dNumpy.get_projected_grid2d
(resize_right/resize_right2d_numpy.py:306-342) holds BEFORE its clip -- the remap clips.  Host numpy: a map is built once per
transform, not per frame -- except from_flow_torch, which builds the map of a flow on the flow's device and keeps it in the
autograd graph (a flow fitted by gradient).
"""
from __future__ import annotations

import numpy as np


def _grid(out_hw):
    oH, oW = int(out_hw[0]), int(out_hw[1])
    if oH < 1 or oW < 1:
        raise ValueError("out_hw must be positive")
    return np.meshgrid(np.arange(oH), np.arange(oW), indexing="ij")


def from_homography(matrix, out_hw, arithmetic="device"):
    """The projected grid of the homographic warp of `matrix` (3 x 3, source -> output like Warp2dNumpy.set_shape's), unclipped,
    float64 [oH, oW, 2]: the reference's get_projected_grid2d (:312-335) -- (col, row, 1) through the inverse matrix, the two
    divisions -- in one of two roundings of the three-term sums:

    "device" (default): every product and sum rounded, left to right, the order of the warp kernels' project_point
        (csrc/lerf_host_geometry.h; the reference's statement "without FMA").  ops.remap_* on this map give what ops.warp_* give
        for the matrix BIT FOR BIT, float64 outputs included.
    "reference": np.dot with the inverse matrix exactly as :327 writes it (and oracle.warp_geometry restates it).  A BLAS
        kernel fuses its multiply-adds, so this grid differs from the device's in the last bit at a few per cent to a third
        of the entries (1e-16 relative): invisible to a byte, visible in the last bits of a float64 output."""
    m = np.asarray(matrix.detach().cpu().numpy() if hasattr(matrix, "detach") else matrix, dtype=np.float64)
    if m.shape != (3, 3):
        raise ValueError("matrix must be 3x3")
    if arithmetic not in ("device", "reference"):
        raise ValueError("arithmetic is 'device' or 'reference'")
    ii, jj = _grid(out_hw)
    oH, oW = ii.shape
    minv = np.linalg.inv(m)                                                                          # :327
    if arithmetic == "reference":
        pts = np.stack([jj.ravel().astype(np.float32), ii.ravel().astype(np.float32)], axis=-1)      # h -> y, w -> x (:325)
        pts = np.concatenate([pts, np.ones([pts.shape[0], 1])], axis=-1)
        g = np.dot(minv, pts.transpose(1, 0)).transpose(1, 0)
        g[:, 0] /= g[:, -1]
        g[:, 1] /= g[:, -1]
        return np.ascontiguousarray(np.stack([g[:, 1].reshape(oH, oW), g[:, 0].reshape(oH, oW)], axis=-1))
    q = minv.reshape(9)
    x, y = jj.astype(np.float64), ii.astype(np.float64)
    X = q[0] * x + q[1] * y + q[2]                               # numpy rounds each elementwise product and sum: project_point's order
    Y = q[3] * x + q[4] * y + q[5]
    Wh = q[6] * x + q[7] * y + q[8]
    return np.ascontiguousarray(np.stack([Y / Wh, X / Wh], axis=-1))


def from_flow(flow):
    """identity + displacement: flow [H, W, 2] = (d_row, d_col) of every output pixel -> float64 [H, W, 2]; from_flow(0 * flow) is
    the identity grid (row i, col j)."""
    f = np.asarray(flow.detach().cpu().numpy() if hasattr(flow, "detach") else flow, dtype=np.float64)
    if f.ndim != 3 or f.shape[2] != 2:
        raise ValueError("flow must be [H, W, 2]")
    ii, jj = _grid(f.shape[:2])
    return np.ascontiguousarray(np.stack([ii + f[..., 0], jj + f[..., 1]], axis=-1))


def from_flow_torch(flow):
    """from_flow with torch ops on the flow's device: flow [H, W, 2] tensor (float32 or float64) -> identity + flow in the flow's
    dtype, same device.  A flow that requires grad stays in the graph, so a remap class that has opted in with enable_backward()
    hands it d loss / d flow (resize_right2d_torch.Remap2dTorch)."""
    import torch
    if not isinstance(flow, torch.Tensor) or flow.ndim != 3 or flow.shape[2] != 2 or not flow.is_floating_point():
        raise ValueError("flow must be a floating-point [H, W, 2] tensor")
    ii = torch.arange(flow.shape[0], dtype=flow.dtype, device=flow.device)
    jj = torch.arange(flow.shape[1], dtype=flow.dtype, device=flow.device)
    grid = torch.stack(torch.meshgrid(ii, jj, indexing="ij"), dim=-1)
    return grid + flow


def radial(in_hw, out_hw, k1, k2=0.0, centre=None):
    """Radial (Brown) lens model about `centre` (row, col of the SOURCE frame; default: its middle): the output pixel at
    normalised offset u from the output's middle reads the source at centre + u (1 + k1 r^2 + k2 r^4) * half-diagonal, r = |u|,
    offsets normalised by the half-diagonal of each frame (so k1 = k2 = 0 is the plain resize between the two sizes).
    float64 [oH, oW, 2]."""
    H, W = int(in_hw[0]), int(in_hw[1])
    ii, jj = _grid(out_hw)
    oH, oW = ii.shape
    cr, cc = ((H - 1) / 2.0, (W - 1) / 2.0) if centre is None else (float(centre[0]), float(centre[1]))
    no = np.hypot(oH, oW) / 2.0
    ni = np.hypot(H, W) / 2.0
    ur = (ii - (oH - 1) / 2.0) / no
    uc = (jj - (oW - 1) / 2.0) / no
    r2 = ur * ur + uc * uc
    f = 1.0 + float(k1) * r2 + float(k2) * r2 * r2
    return np.ascontiguousarray(np.stack([cr + ur * f * ni, cc + uc * f * ni], axis=-1))
