"""Coordinate-map builders for the remap (ops.RemapGeometry, LerfEngine.remap).

A map is a float64 (or float32) array [oH, oW, 2]; entry (i, j) is (row, col) of the source position of output pixel
(i, j), in the reference's convention: integers are pixel indices, the values are what Warp2dNumpy.get_projected_grid2d
(resize_right/resize_right2d_numpy.py:306-342) holds BEFORE its clip -- the remap clips.  Host numpy: a map is built once per
transform, not per frame -- except from_flow_torch, which builds the map of a flow on the flow's device and keeps it in the
autograd graph (a flow fitted by gradient).

With device=<a torch device> the builders write the map ON the device with the kernels of csrc/lerf_coords.hip (one store per
entry, no host array, no upload): from_homography, radial, undistort_rectify, fisheye_undistort_rectify, equirect_view,
from_mesh; from_mesh_torch keeps a control mesh
in the autograd graph through the mesh upsample's adjoint, compose chains two maps into one, and invert / invert_flow solve a
map for its inverse (distort <-> undistort, forward flow -> backward map).  invert_raster / invert_flow_raster invert a map that
FOLDS or TEARS (a forward flow with occlusions, a folded mesh), where Newton's method has no basin to start in: every triangle of
the map is drawn into the frame with a depth test (lerf_coords_invert_raster), the nearest surface wins, a cell
stretched across a disocclusion fills nothing; its result is also the start invert lacks on such a map.  The kernels' arithmetic is
float64 with + - * / only, bit-equal to its host twin (csrc/lerf_coords_models.h); the square root and arc tangents of the
fisheye and equirectangular models are written in those operations too (_lib.coords_math_host), not taken from a math library.

from_homography_torch, radial_torch, undistort_rectify_torch (with brown_params_torch), fisheye_undistort_rectify_torch (with
fisheye_params_torch) and equirect_view_torch are the differentiable twins of the
closed-form builders: their operands are DEVICE tensors (a matrix, lens coefficients, camera matrices -- one set or a leading
batch B, one map per sample in one launch), the map is written by lerf_coords_build_dev from parameters that never leave the
device, and a loss reaches the operands through lerf_coords_build_bwd: direct image alignment, calibration
refinement, a spatial-transformer head.  An entry whose point is not finite (a homography's Wh == 0) contributes nothing to the
gradient -- unlike autograd of the same formulas, which would return NaN.

compose, invert, invert_flow, invert_raster and invert_flow_raster refuse operands that require grad.  The first three have opt-in twins: compose_torch, invert_torch and
invert_flow_torch (device tensors only) run the same forward kernels and keep the maps in the autograd graph through the HIP
adjoints lerf_coords_compose_bwd and lerf_coords_invert_bwd, so a loss reaches a flow or a control mesh through
chained maps: coarse-to-fine refinement (compose_torch(upsampled, residual)), scaling and squaring (compose_torch(phi, phi)),
inverse-consistency losses (invert_torch).  Once differentiable; init, max_iter and tol have no gradient.

reproject turns a DEPTH image and a camera pose into a map (lerf_coords_reproject): pixel (i, j) of one view, lifted by
its depth (or inverse depth) and moved by X_dst = R X_src + t, lands at (row, col) of the other view; with return_depth=True its
depth there comes back too, the plane invert_raster's depth test reads.  Two chains end in a remap:

    remap(img_src, reproject(depth_dst, K_dst, K_src, R, t))                  backward warp: the target's depth reads the source
    m, z = reproject(depth_src, K_src, K_dst, R, t, return_depth=True)
    remap(img_src, invert_raster(m, hw, depth=z, orient=1))                   forward splat: the nearest surface wins, holes stay NaN

reproject_torch (with reproject_params_torch) is the differentiable twin: depth, K_src, K_dst, R and t receive gradients through
lerf_coords_reproject_bwd -- float64, a fixed summation order, an entry that is not valid contributes nothing.

splat is FORWARD warping by summation splatting (lerf_splat): every source pixel is added into the target frame at the
position a forward map gives it, with a normalisation plane for the modes "average", "linear" and "softmax"; splat_torch is the
differentiable twin (lerf_splat_bwd: image, weight and map), the third chain beside reproject's two:
    m, z = reproject_torch(depth_src, K_src, K_dst, R, t, return_depth=True)
    splat_torch(img_src, m, hw, weight=-beta * z, mode="softmax")             forward, soft: the source's own depth, differentiable

from_triangles builds a map from an irregular TRIANGLE MESH (lerf_coords_trimesh): vertex positions in the output
frame, the source position every vertex shows, faces by index, optionally per-corner attributes (attr_faces), a per-vertex depth
(the nearest face wins) and a per-vertex w (perspective-correct interpolation) -- landmark-driven piecewise-affine warps, UV-mapped
meshes, any warp whose control points are not a grid.  invert_raster's watertight inside test and integer-min key over faces of any
size, bit-equal to its host twin; pixels no face covers stay NaN.  grid_faces is invert_raster's own triangulation.
from_triangles_torch is the differentiable twin (lerf_coords_trimesh_bwd): attr, pos and w receive gradients at fixed
visibility, in a fixed order -- bit-equal from run to run.
"""
from __future__ import annotations

import numpy as np


def _grid(out_hw):
    oH, oW = int(out_hw[0]), int(out_hw[1])
    if oH < 1 or oW < 1:
        raise ValueError("out_hw must be positive")
    return np.meshgrid(np.arange(oH), np.arange(oW), indexing="ij")


def _np_dtype(dtype):
    """numpy dtype of a dtype= argument (numpy or torch float32 / float64; None: float64)"""
    name = "float64" if dtype is None else str(dtype).replace("torch.", "").replace("<class 'numpy.", "").replace("'>", "")
    if name not in ("float32", "float64"):
        raise ValueError("dtype is float32 or float64")
    return np.dtype(name)


def _build(model, params, out_hw, dtype, device):
    """the map of a model by the kernels' arithmetic: on `device` by the kernel, or (device None) by its bit-equal host twin"""
    dt = _np_dtype(dtype)
    _grid((out_hw[0], 1)), _grid((1, out_hw[1]))
    if device is None:
        from . import _lib
        return _lib.coords_build_host(model, params, out_hw, dt)
    import torch
    from . import ops
    return ops.coords_build(model, params, out_hw, dtype=getattr(torch, dt.name), device=device)


def from_homography(matrix, out_hw, arithmetic="device", device=None, dtype=None):
    """The projected grid of the homographic warp of `matrix` (3 x 3, source -> output like Warp2dNumpy.set_shape's), unclipped,
    float64 [oH, oW, 2]: the reference's get_projected_grid2d (:312-335) -- (col, row, 1) through the inverse matrix, the two
    divisions -- in one of two roundings of the three-term sums:

    "device" (default): every product and sum rounded, left to right, the order of the warp kernels' project_point
        (csrc/lerf_host_geometry.h; the reference's statement "without FMA").  ops.remap_* on this map give what ops.warp_* give
        for the matrix BIT FOR BIT, float64 outputs included.
    "reference": np.dot with the inverse matrix exactly as :327 writes it (and oracle.warp_geometry restates it).  A BLAS
        kernel fuses its multiply-adds, so this grid differs from the device's in the last bit at a few per cent to a third
        of the entries (1e-16 relative): invisible to a byte, visible in the last bits of a float64 output.

    device: a torch device -> the map is written there by the kernel (lerf_coords_build, the "device" arithmetic; bit-equal to
    the host array) and returned as a tensor; "reference" arithmetic is a host form and is refused with a device.  dtype:
    float64 (default) or float32 (the float64 value rounded once)."""
    m = np.asarray(matrix.detach().cpu().numpy() if hasattr(matrix, "detach") else matrix, dtype=np.float64)
    if m.shape != (3, 3):
        raise ValueError("matrix must be 3x3")
    if arithmetic not in ("device", "reference"):
        raise ValueError("arithmetic is 'device' or 'reference'")
    if device is not None:
        if arithmetic != "device":
            raise ValueError("from_homography on a device computes the 'device' arithmetic; 'reference' is a host form")
        return _build("homography", np.linalg.inv(m).reshape(9), out_hw, dtype, device)
    dt = _np_dtype(dtype)
    ii, jj = _grid(out_hw)
    oH, oW = ii.shape
    minv = np.linalg.inv(m)                                                                          # :327
    if arithmetic == "reference":
        pts = np.stack([jj.ravel().astype(np.float32), ii.ravel().astype(np.float32)], axis=-1)      # h -> y, w -> x (:325)
        pts = np.concatenate([pts, np.ones([pts.shape[0], 1])], axis=-1)
        g = np.dot(minv, pts.transpose(1, 0)).transpose(1, 0)
        g[:, 0] /= g[:, -1]
        g[:, 1] /= g[:, -1]
        return np.ascontiguousarray(np.stack([g[:, 1].reshape(oH, oW), g[:, 0].reshape(oH, oW)], axis=-1)).astype(dt, copy=False)
    q = minv.reshape(9)
    x, y = jj.astype(np.float64), ii.astype(np.float64)
    X = q[0] * x + q[1] * y + q[2]                               # numpy rounds each elementwise product and sum: project_point's order
    Y = q[3] * x + q[4] * y + q[5]
    Wh = q[6] * x + q[7] * y + q[8]
    return np.ascontiguousarray(np.stack([Y / Wh, X / Wh], axis=-1)).astype(dt, copy=False)


def from_flow(flow):
    """identity + displacement: flow [H, W, 2] = (d_row, d_col) of every output pixel -> float64 [H, W, 2]; from_flow(0 * flow) is
    the identity grid (row i, col j).  A batch of flows [B, H, W, 2] -> [B, H, W, 2], one map per sample."""
    f = np.asarray(flow.detach().cpu().numpy() if hasattr(flow, "detach") else flow, dtype=np.float64)
    if f.ndim not in (3, 4) or f.shape[-1] != 2:
        raise ValueError("flow must be [H, W, 2] or [B, H, W, 2]")
    ii, jj = _grid(f.shape[-3:-1])
    return np.ascontiguousarray(np.stack([ii + f[..., 0], jj + f[..., 1]], axis=-1))


def from_flow_torch(flow):
    """from_flow with torch ops on the flow's device: flow [H, W, 2] (or a batch [B, H, W, 2]) tensor (float32 or float64) ->
    identity + flow in the flow's dtype, same device.  A flow that requires grad stays in the graph, so a remap class that has
    opted in with enable_backward() hands it d loss / d flow (resize_right2d_torch.Remap2dTorch)."""
    import torch
    if not isinstance(flow, torch.Tensor) or flow.ndim not in (3, 4) or flow.shape[-1] != 2 or not flow.is_floating_point():
        raise ValueError("flow must be a floating-point [H, W, 2] or [B, H, W, 2] tensor")
    ii = torch.arange(flow.shape[-3], dtype=flow.dtype, device=flow.device)
    jj = torch.arange(flow.shape[-2], dtype=flow.dtype, device=flow.device)
    grid = torch.stack(torch.meshgrid(ii, jj, indexing="ij"), dim=-1)
    return grid + flow


def from_grid_sample(grid, in_hw, align_corners=False):
    """The (row, col) maps of an F.grid_sample grid: grid [B, oH, oW, 2] (or [oH, oW, 2]) of normalised (x, y) in [-1, 1] ->
    maps of the same shape, dtype and device for a source frame of in_hw = (H, W), with torch ops, so a grid that requires grad
    stays in the graph:

        align_corners=True:   row = (y + 1) / 2 * (H - 1)          (-1 and +1 are the centres of the first and last pixel)
        align_corners=False:  row = ((y + 1) * H - 1) / 2          (-1 and +1 are the outer edges: -0.5 and H - 0.5)

    and the columns alike with x and W.  This converts COORDINATES only.  What the remap does with them stays the reference's,
    not grid_sample's: the point is clipped to [0, H] x [0, W], the support, pads, border handling (pad_mode) and the weights'
    normalisation are the warp's -- there is no padding_mode / zeros-outside rule of grid_sample here, and a bilinear remap is
    the reference's bilinear kernel on its own tap set."""
    import torch
    if not isinstance(grid, torch.Tensor) or grid.ndim not in (3, 4) or grid.shape[-1] != 2 or not grid.is_floating_point():
        raise ValueError("grid must be a floating-point [B, oH, oW, 2] (or [oH, oW, 2]) tensor of normalised (x, y)")
    H, W = int(in_hw[0]), int(in_hw[1])
    if H < 1 or W < 1:
        raise ValueError("in_hw must be positive")
    x, y = grid[..., 0], grid[..., 1]
    if align_corners:
        row, col = (y + 1) / 2 * (H - 1), (x + 1) / 2 * (W - 1)
    else:
        row, col = ((y + 1) * H - 1) / 2, ((x + 1) * W - 1) / 2
    return torch.stack([row, col], dim=-1)


def radial(in_hw, out_hw, k1, k2=0.0, centre=None, device=None, dtype=None):
    """Radial (Brown) lens model about `centre` (row, col of the SOURCE frame; default: its middle): the output pixel at
    normalised offset u from the output's middle reads the source at centre + u (1 + k1 r^2 + k2 r^4) * half-diagonal, r = |u|,
    offsets normalised by the half-diagonal of each frame (so k1 = k2 = 0 is the plain resize between the two sizes).
    float64 [oH, oW, 2].  device: a torch device -> built there by the kernel (the same statements in the same order, bit-equal);
    dtype: float64 (default) or float32."""
    H, W = int(in_hw[0]), int(in_hw[1])
    oH, oW = int(out_hw[0]), int(out_hw[1])
    cr, cc = ((H - 1) / 2.0, (W - 1) / 2.0) if centre is None else (float(centre[0]), float(centre[1]))
    no = np.hypot(oH, oW) / 2.0
    ni = np.hypot(H, W) / 2.0
    if device is not None:
        return _build("radial", [cr, cc, no, ni, (oH - 1) / 2.0, (oW - 1) / 2.0, float(k1), float(k2)], out_hw, dtype, device)
    ii, jj = _grid(out_hw)
    ur = (ii - (oH - 1) / 2.0) / no
    uc = (jj - (oW - 1) / 2.0) / no
    r2 = ur * ur + uc * uc
    f = 1.0 + float(k1) * r2 + float(k2) * r2 * r2
    return np.ascontiguousarray(np.stack([cr + ur * f * ni, cc + uc * f * ni], axis=-1)).astype(_np_dtype(dtype), copy=False)


def _host(a, dtype=np.float64):
    return np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=dtype)


def brown_params(K, dist=None, R=None, new_K=None):
    """The 21 parameters of the "brown" model from what cv::initUndistortRectifyMap takes: K (3 x 3 source camera, no skew), dist
    (k1 k2 p1 p2 [k3 [k4 k5 k6]], missing ones 0), R (rectifying rotation, default I), new_K (default K) ->
    inv(new_K . R)[9], fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6."""
    K, R, new_K = _camera(K, R, new_K)
    d = np.zeros(8) if dist is None else _host(dist).reshape(-1)
    if d.size not in (4, 5, 8):
        raise ValueError("dist holds 4, 5 or 8 coefficients (k1 k2 p1 p2 [k3 [k4 k5 k6]])")
    d = np.concatenate([d, np.zeros(8 - d.size)])
    minv = np.linalg.inv(np.dot(new_K, R))
    return np.concatenate([minv.reshape(9), [K[0, 0], K[1, 1], K[0, 2], K[1, 2]], d])


def undistort_rectify(K, dist, R, new_K, out_hw, device=None, dtype=None):
    """The map of cv::initUndistortRectifyMap (pinhole + Brown-Conrady, 4 / 5 / 8 distortion coefficients in OpenCV's order, a
    rectifying rotation R and the new camera matrix new_K; R and new_K may be None = identity / K): output pixel (u = j, v = i)
    goes through inv(new_K . R) to the normalised (x, y), is distorted, and lands at (row, col) = (fy y'' + cy, fx x'' + cx) of
    the source.  [oH, oW, 2], float64 (default) or float32; device None: host numpy through the kernel's host twin, else a
    device tensor written by the kernel -- bit-equal to each other.  remap() of a distorted frame with this map undistorts and
    rectifies it."""
    return _build("brown", brown_params(K, dist, R, new_K), out_hw, dtype, device)


def _camera(K, R, new_K, what="K"):
    """(K, R, new_K) as float64 host arrays, defaults filled in, K checked for skew"""
    K = _host(K)
    if K.shape != (3, 3):
        raise ValueError("%s must be 3x3" % what)
    if K[0, 1] != 0.0 or K[1, 0] != 0.0 or K[2, 0] != 0.0 or K[2, 1] != 0.0 or K[2, 2] != 1.0:
        raise ValueError("%s must be [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] (skew is not supported)" % what)
    R = np.eye(3) if R is None else _host(R)
    new_K = K if new_K is None else _host(new_K)
    if R.shape != (3, 3) or new_K.shape != (3, 3):
        raise ValueError("R and new_K must be 3x3")
    return K, R, new_K


def fisheye_params(K, dist4, R=None, new_K=None):
    """The 17 parameters of the "fisheye" model from what cv::fisheye::initUndistortRectifyMap takes: K (3 x 3 source camera, no
    skew), dist4 (k1 k2 k3 k4 of the equidistant model; None: all 0), R (rectifying rotation, default I), new_K (default K) ->
    inv(new_K . R)[9], fx, fy, cx, cy, k1, k2, k3, k4."""
    K, R, new_K = _camera(K, R, new_K)
    d = np.zeros(4) if dist4 is None else _host(dist4).reshape(-1)
    if d.size != 4:
        raise ValueError("dist holds the 4 coefficients k1 k2 k3 k4 of the fisheye model")
    minv = np.linalg.inv(np.dot(new_K, R))
    return np.concatenate([minv.reshape(9), [K[0, 0], K[1, 1], K[0, 2], K[1, 2]], d])


def fisheye_undistort_rectify(K, dist, R, new_K, out_hw, device=None, dtype=None):
    """The map of cv::fisheye::initUndistortRectifyMap (the equidistant fisheye model, 4 coefficients, a rectifying rotation R and
    the new camera matrix new_K; R and new_K may be None = identity / K, no skew): output pixel (u = j, v = i) of the PINHOLE
    view goes through inv(new_K . R) to the normalised (x, y), r = |(x, y)|, theta = atan(r), theta_d = theta (1 + k1 theta^2 +
    k2 theta^4 + k3 theta^6 + k4 theta^8), and lands at (row, col) = (fy y theta_d / r + cy, fx x theta_d / r + cx) of the fisheye
    frame.  A ray behind the camera (Wh <= 0) has no source: (NaN, NaN), which the remap masks.  [oH, oW, 2], float64 (default) or
    float32; device None: host numpy through the kernel's host twin, else a device tensor written by the kernel -- bit-equal to
    each other: the square root and the arc tangent are the library's own (csrc/lerf_coords_models.h), within 1 ulp of numpy's
    and not equal to them.  remap() of a fisheye frame with this map rectifies it to the pinhole view.  The opposite direction
    needs no model of its own: invert(this map, fisheye_hw) is the map that distorts a pinhole frame into the fisheye's."""
    return _build("fisheye", fisheye_params(K, dist, R, new_K), out_hw, dtype, device)


def equirect_params(pano_hw, K_view, R=None):
    """The 13 parameters of the "equirect" model: a panorama of pano_hw = (Hp, Wp) pixels (pixel centres; longitude -pi .. pi
    over the width, latitude -pi/2 .. pi/2 over the height, rows growing with the view's y), the pinhole view's camera matrix
    K_view (3 x 3, no skew) and its rotation R (view -> panorama axes, default I) ->
    inv(K_view . R)[9], sx = Wp / (2 pi), sy = Hp / pi, cxp = (Wp - 1) / 2, cyp = (Hp - 1) / 2."""
    Hp, Wp = int(pano_hw[0]), int(pano_hw[1])
    if Hp < 1 or Wp < 1:
        raise ValueError("pano_hw must be positive")
    K, R, _ = _camera(K_view, R, None, "K_view")
    minv = np.linalg.inv(np.dot(K, R))
    return np.concatenate([minv.reshape(9), [Wp / (2.0 * np.pi), Hp / np.pi, (Wp - 1) / 2.0, (Hp - 1) / 2.0]])


def equirect_view(pano_hw, K_view, R, out_hw, device=None, dtype=None):
    """The map of a pinhole view of an equirectangular (360 degree) panorama: output pixel (u = j, v = i) is the ray
    d = inv(K_view . R) (u, v, 1), lon = atan2(d.x, d.z), lat = atan2(d.y, |(d.x, d.z)|), and reads the panorama at
    (row, col) = (cyp + sy lat, cxp + sx lon) (equirect_params).  R may be None.  The seam lon = +-pi is an ordinary border: the
    remap clips there, it does not wrap around.  [oH, oW, 2], float64 (default) or float32; device None: the kernel's host twin,
    else a device tensor written by the kernel, bit-equal to each other (the library's own square root and arc tangent, see
    fisheye_undistort_rectify).  remap() of a panorama with this map renders the view; invert(this map, pano_hw) is the map
    that pastes the view back into the panorama's frame (NaN where the view does not reach)."""
    return _build("equirect", equirect_params(pano_hw, K_view, R), out_hw, dtype, device)


def from_mesh(ctrl, out_hw, interp="bilinear", device=None, dtype=None):
    """A control mesh upsampled to a dense map: ctrl [gh, gw, 2] (gh, gw >= 2) holds the absolute source position (row, col) at
    control vertices spread align-corners over the output (vertex a at output row a (oH - 1) / (gh - 1)); interp "bilinear", or
    "bicubic" (Keys A = -0.75 with clamped border taps: F.interpolate(mode="bicubic", align_corners=True)).  device None and a
    host ctrl: host numpy (the kernel's host twin); a torch device, or a ctrl already on one: a device tensor written by the
    kernel.  dtype: the map's, default ctrl's (float64 for anything that is not float32).  A batch of meshes ctrl [B, gh, gw, 2]
    gives [B, oH, oW, 2], one map per sample in ONE launch (lerf_coords_mesh_batched; on the host one call of its host twin), map s
    bit-equal to from_mesh(ctrl[s])."""
    on_dev = getattr(ctrl, "is_cuda", False)
    if device is None and not on_dev:
        from . import _lib
        c = np.asarray(ctrl.detach().numpy() if hasattr(ctrl, "detach") else ctrl)
        if c.dtype not in (np.float32, np.float64):
            c = c.astype(np.float64)
        _grid(out_hw)
        return _lib.coords_mesh_host(c, out_hw, interp, c.dtype if dtype is None else _np_dtype(dtype))
    import torch
    from . import ops
    if not isinstance(ctrl, torch.Tensor):
        c = np.asarray(ctrl)
        ctrl = torch.from_numpy(np.ascontiguousarray(c if c.dtype in (np.float32, np.float64) else c.astype(np.float64)))
    if device is not None:
        ctrl = ctrl.to(device)
    return ops.coords_mesh(ctrl, out_hw, interp, dtype=None if dtype is None else getattr(torch, _np_dtype(dtype).name))


_MESH_FN = None


def _mesh_fn():
    global _MESH_FN
    if _MESH_FN is None:
        import torch
        from . import ops

        class _MeshFn(torch.autograd.Function):
            """map = ops.coords_mesh(ctrl); backward: ops.coords_mesh_bwd in float64, cast to ctrl's dtype; a batch of meshes goes through
            both in one call each"""

            @staticmethod
            def forward(ctx, ctrl, out_hw, interp):
                ctx.interp, ctx.ctrl_hw, ctx.dtype = interp, tuple(ctrl.shape[-3:-1]), ctrl.dtype
                return ops.coords_mesh(ctrl, out_hw, interp)

            @staticmethod
            def backward(ctx, grad):
                g = ops.coords_mesh_bwd(grad.contiguous().double(), ctx.ctrl_hw, ctx.interp)
                return g.to(ctx.dtype), None, None

        _MESH_FN = _MeshFn
    return _MESH_FN


def from_mesh_torch(ctrl, out_hw, interp="bilinear"):
    """from_mesh on ctrl's device, differentiable: ctrl [gh, gw, 2] device tensor (float32 or float64) -> the map in ctrl's
    dtype.  A ctrl that requires grad stays in the graph: a remap class that has opted in with enable_backward() hands it
    d loss / d ctrl through the upsample's adjoint (lerf_coords_mesh_bwd: float64, deterministic, cast to ctrl's dtype).  A batch
    ctrl [B, gh, gw, 2] gives [B, oH, oW, 2] and the gradient [B, gh, gw, 2]: one launch forward (lerf_coords_mesh_batched), one call
    of two launches backward (lerf_coords_mesh_bwd_batched), sample s bit-equal to the single-mesh call."""
    import torch
    if not isinstance(ctrl, torch.Tensor) or ctrl.ndim not in (3, 4) or ctrl.shape[-1] != 2 or not ctrl.is_floating_point() or not ctrl.is_cuda \
            or ctrl.shape[0] < 1:
        raise ValueError("ctrl must be a floating-point [gh, gw, 2] or [B, gh, gw, 2] device tensor")
    if interp not in ("bilinear", "bicubic"):
        raise ValueError("interp is 'bilinear' or 'bicubic'")
    return _mesh_fn().apply(ctrl, (int(out_hw[0]), int(out_hw[1])), interp)


def compose(outer, inner, dtype=None):
    """One map for two chained remaps: C[i, j] = outer(inner[i, j]), the outer map sampled bilinearly at the position the inner
    map holds, so remap(remap(img, outer), inner) and remap(img, compose(outer, inner)) describe the same geometry -- one pass
    through the LUT stages and one interpolation instead of two.  Positions outside the outer map are clipped onto its border;
    a NaN entry of the inner map stays (NaN, NaN).  numpy in -> numpy out (the kernel's host twin); device tensors in -> a
    device tensor; mixed operands are refused.  dtype: default the inner map's.  A batch: inner [B, H, W, 2] with outer
    [B, aH, aW, 2] or one shared [aH, aW, 2] gives [B, H, W, 2] in ONE launch (lerf_coords_compose_batched; on the host one call of its
    host twin).  No autograd: an operand that requires grad (with grad mode on) is refused -- compose_torch is the differentiable
    twin."""
    dev = [bool(getattr(t, "is_cuda", False)) for t in (outer, inner)]
    if dev[0] != dev[1]:
        raise ValueError("compose: both maps on the host or both on one device, not mixed")
    if any(getattr(t, "requires_grad", False) for t in (outer, inner)):
        import torch
        if torch.is_grad_enabled():
            raise ValueError("compose has no autograd: use compose_torch, or detach() the maps (or call it under torch.no_grad())")
    if dev[0]:
        import torch
        from . import ops
        return ops.coords_compose(outer, inner, dtype=None if dtype is None else getattr(torch, _np_dtype(dtype).name))
    from . import _lib
    a, b = (np.asarray(t.detach().numpy() if hasattr(t, "detach") else t) for t in (outer, inner))
    a, b = (t if t.dtype in (np.float32, np.float64) else t.astype(np.float64) for t in (a, b))
    return _lib.coords_compose_host(a, b, b.dtype if dtype is None else _np_dtype(dtype))


def invert(map, in_hw, init=None, max_iter=16, tol=1e-9, dtype=None):
    """The inverse of a map: G [H, W, 2] with in_hw = (H, W) the size of the frame `map` points INTO (and so the shape of the
    inverse); G[i, j] is the position u at which the map, read bilinearly like compose reads its outer map, holds (i, j) -- so
    compose(map, G) is the identity within tol wherever G is not NaN.  A map that distorts gives the map that undistorts; the map of
    a forward flow gives the backward map a remap needs.  Newton's method per entry on the device (lerf_coords_invert: one thread per
    entry, float64), at most max_iter (1..64) passes, stopped when both residuals are <= tol.

    init: a map [H, W, 2] of starting positions -- the analytic inverse of a model (radial(..., -k1) for radial(..., k1)), the
    previous frame's inverse -- for maps far from affine; None: the affine guess through three corners of the map.  An entry is
    (NaN, NaN) where the map does not reach (i, j), where it folds (a singular Jacobian), where the cell read holds a NaN, or where
    max_iter passes did not meet tol; the remap treats a NaN entry as "no source" (mask false).

    numpy in -> numpy out (the kernel's host twin, bit-equal); device tensors in -> a device tensor; mixed map / init is refused.
    dtype: default the map's.  A batch [B, fH, fW, 2] (init [B, H, W, 2] or None) gives [B, H, W, 2] in ONE launch
    (lerf_coords_invert_batched: the sample is the grid's third axis; a wave still runs as long as its slowest lane, a sample as long
    as its slowest wave, and no sample waits for another's).  No autograd: an operand that requires grad (with grad mode on) is
    refused -- invert_torch is the differentiable twin."""
    ops_ = [t for t in (map, init) if t is not None]
    dev = [bool(getattr(t, "is_cuda", False)) for t in ops_]
    if any(d != dev[0] for d in dev):
        raise ValueError("invert: map and init on the host or both on one device, not mixed")
    if any(getattr(t, "requires_grad", False) for t in ops_):
        import torch
        if torch.is_grad_enabled():
            raise ValueError("invert has no autograd: use invert_torch, or detach() the maps (or call it under torch.no_grad())")
    H, W = int(in_hw[0]), int(in_hw[1])
    if H < 1 or W < 1:
        raise ValueError("in_hw must be positive")
    nd = getattr(map, "ndim", None)
    if nd not in (3, 4) or (init is not None and getattr(init, "ndim", None) != nd):
        raise ValueError("invert: map is [fH, fW, 2] or [B, fH, fW, 2], init (if given) [H, W, 2] or [B, H, W, 2] alike")
    if nd == 4 and init is not None and init.shape[0] != map.shape[0]:
        raise ValueError("invert: map and init hold different numbers of maps")
    if dev[0]:
        import torch
        return _invert_maps(map, (H, W), init, max_iter, tol, map.dtype if dtype is None else getattr(torch, _np_dtype(dtype).name))
    a, b = (None if t is None else np.asarray(t.detach().numpy() if hasattr(t, "detach") else t) for t in (map, init))
    a, b = (t if t is None or t.dtype in (np.float32, np.float64) else t.astype(np.float64) for t in (a, b))
    return _invert_maps(a, (H, W), b, max_iter, tol, a.dtype if dtype is None else _np_dtype(dtype))


def _invert_maps(map, hw, init, max_iter, tol, dt):
    """invert of numpy maps by the host twin or of device tensors by the kernel (dt: a numpy or a torch dtype alike): one map, or a
    batch in one call"""
    if getattr(map, "is_cuda", False):
        from . import ops
        return ops.coords_invert(map, hw, init=init, dtype=dt, max_iter=max_iter, tol=tol)
    from . import _lib
    return _lib.coords_invert_host(map, hw, init=init, dtype=dt, max_iter=max_iter, tol=tol)


def invert_flow(flow, init=None, max_iter=16, tol=1e-9):
    """The backward flow of a forward flow: flow [H, W, 2] (or a batch [B, H, W, 2]) = (d_row, d_col) of every pixel, numpy or a
    device tensor -> b = invert(identity + flow, (H, W)) - identity, in the flow's dtype and place, so that the map identity + flow
    read at identity + b is the identity (within tol); NaN where no pixel of the flow lands.  init, max_iter, tol: invert's (init
    is a MAP of starting positions, not a flow).  No autograd (invert_flow_torch is the differentiable twin)."""
    if getattr(flow, "ndim", None) not in (3, 4) or flow.shape[-1] != 2:
        raise ValueError("flow must be [H, W, 2] or [B, H, W, 2]")
    H, W = int(flow.shape[-3]), int(flow.shape[-2])
    if getattr(flow, "is_cuda", False):
        import torch
        if flow.requires_grad and torch.is_grad_enabled():
            raise ValueError("invert has no autograd: use invert_torch, or detach() the maps (or call it under torch.no_grad())")
        ident = from_flow_torch(torch.zeros((H, W, 2), dtype=flow.dtype, device=flow.device))
        return invert(ident + flow.detach(), (H, W), init=init, max_iter=max_iter, tol=tol) - ident
    if getattr(flow, "requires_grad", False):
        import torch
        if torch.is_grad_enabled():
            raise ValueError("invert has no autograd: use invert_torch, or detach() the maps (or call it under torch.no_grad())")
    f = np.asarray(flow.detach().numpy() if hasattr(flow, "detach") else flow)
    f = f if f.dtype in (np.float32, np.float64) else f.astype(np.float64)
    ident = from_flow(np.zeros((H, W, 2))).astype(f.dtype)
    return invert(ident + f, (H, W), init=init, max_iter=max_iter, tol=tol) - ident


def _no_autograd(what, operands):
    if any(getattr(t, "requires_grad", False) for t in operands):
        import torch
        if torch.is_grad_enabled():
            raise ValueError("%s has no autograd: detach() the operands (or call it under torch.no_grad())" % what)


def invert_raster(map, in_hw, depth=None, max_span=16, orient=0, dtype=None):
    """The inverse of a map that FOLDS or TEARS, by rasterisation with a depth test: G [H, W, 2] with in_hw = (H, W) the size of the
    frame `map` points INTO; G[i, j] is the position u at which the map, read as its piecewise-LINEAR interpolant over two triangles
    a cell, holds (i, j).  Every triangle of the map is drawn into the frame (lerf_coords_invert_raster: one thread per cell, one
    64-bit integer atomic min per covered pixel), so nothing depends on a starting guess or on a Jacobian that never vanishes -- what
    invert needs, and why it returns NaN on such maps.

    depth: [fH, fW] (read as float32), the depth of every vertex of the map: where several surfaces land on one pixel the NEAREST
    (smallest depth) wins -- the foreground of an optical flow with occlusions; None: the lowest-numbered triangle.  max_span
    (1..64): a triangle whose box of pixels is wider than this on either axis is a TEAR -- a cell stretched across a disocclusion --
    and fills nothing: the disoccluded area stays (NaN, NaN), which the remap treats as "no source" (mask false).  orient: +1 keeps
    only triangles with the identity's orientation, -1 only the reversed ones, 0 (default) both.

    The result differs from invert's by the difference of the two interpolants (hundredths of a pixel on a smooth map that stretches
    by 1.7), and it is the start Newton's method lacks on a folded map:

        invert(map, in_hw, init=invert_raster(map, in_hw))          a bilinear-exact inverse of a folded map
        remap(img, invert_flow_raster(flow, depth) + identity)      carries a frame forward along its flow

    numpy in -> numpy out (the kernel's host twin, bit-equal); device tensors in -> a device tensor; mixed map / depth is refused.
    dtype: default the map's.  A batch [B, fH, fW, 2] (depth [B, fH, fW] or None) gives [B, H, W, 2] in ONE call of three launches
    (lerf_coords_invert_raster_batched).  The batched call needs one plane of 64-bit keys PER SAMPLE -- 8 bytes per output pixel per
    sample, B * H * W * 8 bytes allocated here for the call (a loop over the samples could reuse one plane; the single launch cannot).
    Bit-equal from run to run.  No autograd: an operand that requires grad (with grad mode on) is refused."""
    ops_ = [t for t in (map, depth) if t is not None]
    dev = [bool(getattr(t, "is_cuda", False)) for t in ops_]
    if any(d != dev[0] for d in dev):
        raise ValueError("invert_raster: map and depth on the host or both on one device, not mixed")
    _no_autograd("invert_raster", ops_)
    H, W = int(in_hw[0]), int(in_hw[1])
    if H < 1 or W < 1:
        raise ValueError("in_hw must be positive")
    nd = getattr(map, "ndim", None)
    if nd not in (3, 4) or (depth is not None and (getattr(depth, "ndim", None) != nd - 1 or tuple(depth.shape) != tuple(map.shape[:-1]))):
        raise ValueError("invert_raster: map is [fH, fW, 2] or [B, fH, fW, 2], depth (if given) [fH, fW] or [B, fH, fW] alike")
    if dev[0]:
        import torch
        from . import ops
        a, d = map.detach(), None if depth is None else depth.detach().to(torch.float32).contiguous()
        dt = a.dtype if dtype is None else getattr(torch, _np_dtype(dtype).name)
        one = ops.coords_invert_raster
    else:
        from . import _lib
        a, d = (None if t is None else np.asarray(t.detach().numpy() if hasattr(t, "detach") else t) for t in (map, depth))
        a = a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)
        d = None if d is None else np.ascontiguousarray(d, dtype=np.float32)
        dt = a.dtype if dtype is None else _np_dtype(dtype)
        one = _lib.coords_invert_raster_host
    return one(a, (H, W), depth=d, dtype=dt, max_span=max_span, orient=orient)          # a batch: one call, B key planes


def invert_flow_raster(flow, depth=None, max_span=16, orient=0):
    """The backward flow of a forward flow WITH OCCLUSIONS: flow [H, W, 2] (or a batch [B, H, W, 2]) = (d_row, d_col) of every pixel,
    numpy or a device tensor -> b = invert_raster(identity + flow, (H, W), depth, max_span, orient) - identity, in the flow's dtype
    and place.  Where a foreground moves over a background the surface with the smaller depth wins; the area it uncovers stays
    NaN (no stretched cell fills it: max_span).  remap(img, invert_flow_raster(flow, depth) + identity) carries a frame forward
    along its flow.  No autograd."""
    if getattr(flow, "ndim", None) not in (3, 4) or flow.shape[-1] != 2:
        raise ValueError("flow must be [H, W, 2] or [B, H, W, 2]")
    H, W = int(flow.shape[-3]), int(flow.shape[-2])
    _no_autograd("invert_flow_raster", [flow])
    if getattr(flow, "is_cuda", False):
        import torch
        ident = from_flow_torch(torch.zeros((H, W, 2), dtype=flow.dtype, device=flow.device))
        return invert_raster(ident + flow.detach(), (H, W), depth, max_span, orient) - ident
    f = np.asarray(flow.detach().numpy() if hasattr(flow, "detach") else flow)
    f = f if f.dtype in (np.float32, np.float64) else f.astype(np.float64)
    ident = from_flow(np.zeros((H, W, 2))).astype(f.dtype)
    return invert_raster(ident + f, (H, W), depth, max_span, orient) - ident


def grid_faces(fH, fW):
    """The triangulation invert_raster draws of a map [fH, fW, 2] (fH, fW >= 2), as faces for from_triangles: int32
    [2 (fH - 1) (fW - 1), 3] indices into the map's vertices in row-major order (vertex (i, j) = i fW + j), in invert_raster's
    numbering and vertex order -- cell (i, j) gives face 2 (i (fW - 1) + j) = (i, j), (i, j + 1), (i + 1, j) and the next face
    = (i + 1, j + 1), (i + 1, j), (i, j + 1).  from_triangles(map.reshape(-1, 2), grid indices, grid_faces(fH, fW), hw) IS
    invert_raster(map, hw), bit for bit."""
    fH, fW = int(fH), int(fW)
    if fH < 2 or fW < 2:
        raise ValueError("grid_faces: fH and fW must be at least 2")
    i, j = np.meshgrid(np.arange(fH - 1, dtype=np.int64), np.arange(fW - 1, dtype=np.int64), indexing="ij")
    v = (i * fW + j).reshape(-1)
    faces = np.stack([np.stack([v, v + 1, v + fW], axis=-1), np.stack([v + fW + 1, v + fW, v + 1], axis=-1)], axis=1).reshape(-1, 3)
    if faces.max() > 0x7fffffff:
        raise ValueError("grid_faces: the vertex indices do not fit int32")
    return faces.astype(np.int32)


def from_triangles(pos, attr, faces, out_hw, attr_faces=None, depth=None, w=None, max_span=0, orient=0, dtype=None, return_depth=False,
                   return_faces=False):
    """An irregular TRIANGLE MESH rasterised into a dense map [oH, oW, 2] for remap: landmark-driven piecewise-affine warps, UV-mapped
    meshes, any warp whose control points are not a grid.  pos [V, 2]: the (row, col) of every vertex in the OUTPUT frame; attr
    [Va, 2]: what the map holds at a vertex, the SOURCE position (row, col); faces [F, 3] integer indices into pos; attr_faces
    [F, 3] indices into attr (None: faces) -- welded positions with per-corner texture coordinates, the OBJ v/vt model.  Inside a
    face the attribute is interpolated affinely in the frame, or perspective-correctly when w [V] (the homogeneous w of every
    vertex) is given; there is no near-plane clipping, a face with a w <= 0 is skipped.  depth [V]: where faces overlap the
    smallest interpolated depth wins the pixel (None, and ties: the lowest face).  Pixels no face covers hold (NaN, NaN), which the
    remap reads as "no source" (mask false).  The inside test is closed and watertight for faces that share an edge BY INDEX.

    max_span: 0 = none, else a face whose box of pixels is wider than this on either axis is skipped (the tear rule of
    invert_raster).  orient +1 / -1 keeps only faces with (B - A) x (C - A) > 0 / < 0 in (row, col), 0 both.  A face with an index
    outside the mesh, a vertex that is not finite, a NaN depth or no area is skipped.  THE SIZE RULE: the (face, tile) items of one
    call are numbered in 32 bits, B * F * b <= 2^32 - 1 with b the 4 x 16 pixel tiles of the frame (or of a box max_span wide) --
    about 33 000 faces into 2160 x 3840 with max_span = 0; a finer mesh passes a max_span.

    numpy in -> numpy out (the kernel's host twin, bit-equal); device tensors in -> a device tensor (lerf_coords_trimesh: fill, count,
    scan, one wave per (face, tile), resolve; no sync); mixed operands are refused.  dtype: the map's, default attr's.  pos (and / or
    attr) [B, V, 2] give [B, oH, oW, 2] in ONE batched call; faces, attr_faces, depth and w are then batched alike or shared.
    return_depth: also the winning depth, float32 [oH, oW], NaN in holes (needs depth); return_faces: also the winning face,
    int64 [oH, oW], -1 in holes -> map, or (map[, depth][, faces]).  Bit-equal from run to run.  No autograd here: an operand that
    requires grad (with grad mode on) is refused -- from_triangles_torch is the differentiable twin (gradients to attr, pos and w at
    fixed visibility)."""
    given = [t for t in (pos, attr, faces, attr_faces, depth, w) if t is not None]
    dev = [bool(getattr(t, "is_cuda", False)) for t in given]
    if any(d != dev[0] for d in dev):
        raise ValueError("from_triangles: every operand on the host or all on one device, not mixed")
    _no_autograd("from_triangles", given)
    H, W = int(out_hw[0]), int(out_hw[1])
    if H < 1 or W < 1:
        raise ValueError("out_hw must be positive")
    if return_depth and depth is None:
        raise ValueError("from_triangles: return_depth needs depth")
    if dev[0]:
        import torch
        from . import ops
        fl = lambda t: t.detach().contiguous() if t.dtype in (torch.float32, torch.float64) else t.detach().to(torch.float64).contiguous()
        f32 = lambda t: None if t is None else t.detach().to(torch.float32).contiguous()
        i32 = lambda t: None if t is None else _int32_indices(t.detach(), torch.int32, lambda x, dt: x.to(dt).contiguous())
        dt = None if dtype is None else getattr(torch, _np_dtype(dtype).name)
        one, hole = ops.coords_trimesh, lambda k: k == -1
        low = lambda k: torch.where(hole(k), k, k & 0xffffffff)
    else:
        from . import _lib
        host = lambda t: np.asarray(t.detach().numpy() if hasattr(t, "detach") else t)
        fl = lambda t: np.ascontiguousarray(host(t) if host(t).dtype in (np.float32, np.float64) else host(t).astype(np.float64))
        f32 = lambda t: None if t is None else np.ascontiguousarray(host(t), dtype=np.float32)
        i32 = lambda t: None if t is None else _int32_indices(host(t), np.int32, lambda x, dt: np.ascontiguousarray(x, dtype=dt))
        dt = None if dtype is None else _np_dtype(dtype)
        one = _lib.coords_trimesh_host
        low = lambda k: np.where(k == np.uint64(2 ** 64 - 1), np.int64(-1), (k & np.uint64(0xffffffff)).astype(np.int64))
    res = one(fl(pos), fl(attr), i32(faces), (H, W), attr_faces=i32(attr_faces), depth=f32(depth), w=None if w is None else fl(w), dtype=dt, max_span=max_span,
              orient=orient, return_keys=bool(return_faces), return_depth=bool(return_depth))
    if not (return_faces or return_depth):
        return res
    m, rest = res[0], list(res[1:])
    k = low(rest.pop(0)) if return_faces else None
    return (m,) + ((rest.pop(0),) if return_depth else ()) + ((k,) if return_faces else ())


def _int32_indices(t, int32, cast):
    """face indices as int32.  An int64 index beyond int32 is clamped to -1 / 2^31 - 1 first, which no mesh holds (V < 2^31): its
    face is skipped like any face with an index outside the mesh, where a plain cast would wrap it into a valid one.  No read-back."""
    name = str(t.dtype).replace("torch.", "")
    if name not in ("int8", "uint8", "int16", "int32", "int64"):
        raise ValueError("from_triangles: faces and attr_faces hold integer indices, not %s" % name)
    return cast(t.clip(-1, 0x7fffffff) if name == "int64" else t, int32)


# ---------------------------------------------------------------------------------------------- differentiable twins
def _compose_dev(outer, inner, tdt):
    """compose on the device: one pair, or a batch (outer [B, aH, aW, 2] or one shared [aH, aW, 2]) in one launch"""
    from . import ops
    return ops.coords_compose(outer, inner, dtype=tdt)


def _deterministic(flag):
    """a twin's `deterministic`: None follows torch.are_deterministic_algorithms_enabled()"""
    import torch
    return bool(torch.are_deterministic_algorithms_enabled()) if flag is None else bool(flag)


def _ordered_kw(ordered):
    """the keyword arguments of an ops scatter: none for the atomic kernel (the call is today's), the cap for the ordered one"""
    return {} if ordered is None else {"deterministic": True, "max_adders": ordered}


_CHAIN_FNS = None


def _chain_fns():
    global _CHAIN_FNS
    if _CHAIN_FNS is None:
        import torch
        from torch.autograd.function import once_differentiable
        from . import ops

        class _ComposeFn(torch.autograd.Function):
            """C = compose(outer, inner); backward: ops.coords_compose_bwd in float64, one launch for the whole batch, a shared outer map's
            gradient summed into one buffer by the scatter's atomics; each gradient cast to its operand's dtype.  ordered (None or
            the cap): the outer gradient by the ordered scatter, a shared outer map's summed sample by sample"""

            @staticmethod
            def forward(ctx, outer, inner, tdt, ordered=None):
                ctx.save_for_backward(outer, inner)
                ctx.ordered = ordered
                return _compose_dev(outer.detach(), inner.detach(), tdt)

            @staticmethod
            @once_differentiable
            def backward(ctx, grad):
                outer, inner = ctx.saved_tensors
                need = (ctx.needs_input_grad[0], ctx.needs_input_grad[1])
                g = grad.contiguous().double()
                ga = torch.zeros(tuple(outer.shape), dtype=torch.float64, device=g.device) if need[0] else None
                gb = torch.zeros(tuple(inner.shape), dtype=torch.float64, device=g.device) if need[1] else None
                ops.coords_compose_bwd(outer, inner, g, ga, gb, need, **_ordered_kw(ctx.ordered))
                return None if ga is None else ga.to(outer.dtype), None if gb is None else gb.to(inner.dtype), None, None

        class _InvertFn(torch.autograd.Function):
            """G = invert(map); backward: ops.coords_invert_bwd in float64 at the saved inverse (the implicit function theorem), cast
            to the map's dtype; init is a constant"""

            @staticmethod
            def forward(ctx, map, init, hw, max_iter, tol, tdt, ordered=None):
                out = _invert_maps(map.detach(), hw, None if init is None else init.detach(), max_iter, tol, tdt)
                ctx.save_for_backward(map, out)
                ctx.ordered = ordered
                return out

            @staticmethod
            @once_differentiable
            def backward(ctx, grad):
                map, out = ctx.saved_tensors
                g = grad.contiguous().double()
                gf = torch.zeros(tuple(map.shape), dtype=torch.float64, device=g.device)
                ops.coords_invert_bwd(map, out, g, gf, **_ordered_kw(ctx.ordered))
                return gf.to(map.dtype), None, None, None, None, None, None

        _CHAIN_FNS = (_ComposeFn, _InvertFn)
    return _CHAIN_FNS


def _device_map(t, what, batch=True):
    """a floating-point device tensor [h, w, 2] (or [B, h, w, 2]) or ValueError"""
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_floating_point():
        raise ValueError("%s must be a floating-point device tensor" % what)
    if t.ndim not in ((3, 4) if batch else (3,)) or t.shape[-1] != 2:
        raise ValueError("%s must be [h, w, 2]%s" % (what, " or [B, h, w, 2]" if batch else ""))
    return t


def compose_torch(outer, inner, dtype=None, deterministic=None, max_adders=4096):
    """compose on the maps' device, differentiable: C[i, j] = outer(inner[i, j]) by the same kernel (bit-equal to compose when
    grad mode is off or no operand requires grad); an operand that requires grad stays in the graph through
    lerf_coords_compose_bwd: the outer map's gradient is the bilinear scatter of the upstream gradient (float64 atomic adds), the
    inner map's is J^T g with the clip's gradient that of torch.clamp (it passes on the border, blocks outside) and the cell held
    constant at integer positions.  Floating-point device tensors only; dtype: C's, default the inner map's; each gradient is
    computed in float64 and cast to its operand's dtype.  A batch: inner [B, H, W, 2] with outer [B, aH, aW, 2] or one shared
    [aH, aW, 2] (its gradient is the sum over the samples) -- ONE launch forward and one backward, whatever B
    (lerf_coords_compose_batched, lerf_coords_compose_bwd_batched).  compose_torch(phi, phi) returns the sum of
    both gradients to phi.  The differentiable path needs an outer map of at least 2 x 2.  Once differentiable.
    deterministic (None: follow torch.are_deterministic_algorithms_enabled(), read at this call): the outer map's gradient by the ORDERED
    scatter (lerf_coords_compose_bwd_ordered) -- summed in the host twin's order, bit-equal from run to run and to
    lerf_coords_compose_bwd_host.  Its backward ends with one 4-byte copy to the host and a synchronisation, and raises LerfError when
    more than max_adders entries add into one element.  One shared outer map in a batch: every sample scatters into a gradient of its
    own, and they are added one after the other, sample 0 first.  The inner map's gradient is the same either way."""
    import torch
    a, b = _device_map(outer, "compose_torch: outer"), _device_map(inner, "compose_torch: inner")
    if a.device != b.device:
        raise ValueError("compose_torch: outer and inner live on different devices")
    if a.ndim == 4 and (b.ndim != 4 or a.shape[0] != b.shape[0]):
        raise ValueError("compose_torch: a batch of outer maps needs a batch of as many inner maps")
    tdt = b.dtype if dtype is None else getattr(torch, _np_dtype(dtype).name)
    if not (torch.is_grad_enabled() and (a.requires_grad or b.requires_grad)):
        return _compose_dev(a.detach(), b.detach(), tdt)
    if a.shape[-3] < 2 or a.shape[-2] < 2:
        raise ValueError("compose_torch: the gradient needs an outer map of at least 2 x 2")
    return _chain_fns()[0].apply(a, b, tdt, int(max_adders) if _deterministic(deterministic) else None)


def invert_torch(map, in_hw, init=None, max_iter=16, tol=1e-9, dtype=None, deterministic=None, max_adders=4096):
    """invert on the map's device, differentiable: the same Newton kernel (bit-equal to invert when grad mode is off or the map
    does not require grad); a map that requires grad stays in the graph through lerf_coords_invert_bwd, the implicit-function
    gradient of map(G[q]) = q at the inverse returned: the bilinear scatter of -J^-T g.  Entries of the inverse that are NaN, cells
    with a NaN corner and folded cells contribute nothing.  init is a constant (no gradient), as are max_iter and tol.
    Floating-point device tensors only; a batch [B, fH, fW, 2] (init [B, H, W, 2]) runs ONE launch forward and one backward
    (lerf_coords_invert_batched, lerf_coords_invert_bwd_batched).  The gradient is
    computed in float64 and cast to the map's dtype.  Once differentiable.
    deterministic (None: follow torch.are_deterministic_algorithms_enabled(), read at this call): the gradient by the ORDERED scatter
    (lerf_coords_invert_bwd_ordered), bit-equal from run to run and to lerf_coords_invert_bwd_host; its backward ends with
    one 4-byte copy to the host and a synchronisation, and raises LerfError when more than max_adders entries add into one element."""
    import torch
    a = _device_map(map, "invert_torch: map")
    H, W = int(in_hw[0]), int(in_hw[1])
    if H < 1 or W < 1:
        raise ValueError("in_hw must be positive")
    if init is not None:
        b = _device_map(init, "invert_torch: init")
        if b.device != a.device:
            raise ValueError("invert_torch: map and init live on different devices")
        if b.ndim != a.ndim or tuple(b.shape[-3:-1]) != (H, W) or (a.ndim == 4 and b.shape[0] != a.shape[0]):
            raise ValueError("invert_torch: init is [H, W, 2], or [B, H, W, 2] for a batch of B maps")
    tdt = a.dtype if dtype is None else getattr(torch, _np_dtype(dtype).name)
    if not (torch.is_grad_enabled() and a.requires_grad):
        return _invert_maps(a.detach(), (H, W), None if init is None else init.detach(), max_iter, tol, tdt)
    return _chain_fns()[1].apply(a, init, (H, W), int(max_iter), float(tol), tdt, int(max_adders) if _deterministic(deterministic) else None)


def invert_flow_torch(flow, init=None, max_iter=16, tol=1e-9, deterministic=None, max_adders=4096):
    """invert_flow on the flow's device, differentiable: b = invert_torch(identity + flow, (H, W)) - identity in the flow's
    dtype; a flow that requires grad receives its gradient through lerf_coords_invert_bwd.  init, max_iter, tol, deterministic,
    max_adders: invert_torch's."""
    import torch
    f = _device_map(flow, "invert_flow_torch: flow")
    H, W = int(f.shape[-3]), int(f.shape[-2])
    ident = from_flow_torch(torch.zeros((H, W, 2), dtype=f.dtype, device=f.device))
    return invert_torch(ident + f, (H, W), init=init, max_iter=max_iter, tol=tol, deterministic=deterministic, max_adders=max_adders) - ident


# ---------------------------------------------------------------------------------------------- differentiable model builders
_BUILD_FN = None


def _build_fn():
    global _BUILD_FN
    if _BUILD_FN is None:
        import torch
        from torch.autograd.function import once_differentiable
        from . import ops

        class _BuildFn(torch.autograd.Function):
            """map = ops.coords_build_params(model, params), params float64 [n] or [B, n] on the device; backward:
            ops.coords_build_bwd, the gradient of EVERY entry of the parameter vector in float64 (autograd carries it on to the
            operands the vector was assembled from, constants drop theirs)"""

            @staticmethod
            def forward(ctx, params, model, out_hw, tdt):
                p = params.detach().contiguous()
                ctx.save_for_backward(p)
                ctx.model = model
                return ops.coords_build_params(model, p, out_hw, dtype=tdt)

            @staticmethod
            @once_differentiable
            def backward(ctx, grad):
                p, = ctx.saved_tensors
                return ops.coords_build_bwd(ctx.model, p, grad.contiguous().double()), None, None, None

        _BUILD_FN = _BuildFn
    return _BUILD_FN


def _build_torch(model, params, out_hw, tdt):
    """the map of float64 device parameters [n] or [B, n] by the kernel; in the autograd graph when they require grad"""
    import torch
    from . import ops
    hw = (int(out_hw[0]), int(out_hw[1]))
    if hw[0] < 1 or hw[1] < 1:
        raise ValueError("out_hw must be positive")
    if torch.is_grad_enabled() and params.requires_grad:
        return _build_fn().apply(params, model, hw, tdt)
    return ops.coords_build_params(model, params.detach(), hw, dtype=tdt)


def _operand(t, what, shapes):
    """a float32 / float64 device tensor whose shape is one of `shapes` or one of them behind a leading B, or ValueError -> B (0: none)"""
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in (torch.float32, torch.float64):
        raise ValueError("%s must be a float32 or float64 device tensor" % what)
    for shp in shapes:
        if tuple(t.shape) == tuple(shp):
            return 0
        if t.ndim == len(shp) + 1 and tuple(t.shape[1:]) == tuple(shp) and t.shape[0] >= 1:
            return int(t.shape[0])
    raise ValueError("%s must be %s, or that behind a leading batch size" % (what, " or ".join(str(list(x)) for x in shapes)))


def _one_batch(what, operands, sizes):
    """the common B of the operands (0: none is batched); all on one device"""
    B = 0
    for t, b in zip(operands, sizes):
        if t.device != operands[0].device:
            raise ValueError("%s: the operands live on different devices" % what)
        if b and B and b != B:
            raise ValueError("%s: the operands hold different numbers of samples (%d and %d)" % (what, B, b))
        B = B or b
    return B


def _map_dtype(dtype, default):
    import torch
    return default if dtype is None else getattr(torch, _np_dtype(dtype).name)


def from_homography_torch(matrix, out_hw, dtype=None):
    """from_homography on the matrix's device, differentiable: matrix [3, 3] (source -> output, as from_homography takes it) or a batch
    [B, 3, 3] device tensor, float32 or float64 -> the map [oH, oW, 2] or [B, oH, oW, 2] (one launch) in the matrix's dtype (or
    `dtype`).  The inverse is torch.linalg.inv(matrix.double()) on the device, differentiated by autograd; its nine entries go
    through the kernel (lerf_coords_build_dev, the "device" arithmetic) and, for a matrix that requires grad, through its HIP
    adjoint lerf_coords_build_bwd: float64, a fixed summation order (bit-equal from run to run), cast to the matrix's dtype.
    The map is bit-equal to from_homography(..., device=) for EQUAL INVERSE ENTRIES -- not necessarily for equal matrices:
    torch.linalg.inv and np.linalg.inv may round the inverse differently.  An entry with Wh == 0 (a point that is not finite)
    contributes nothing to the gradient.  Once differentiable."""
    import torch
    B = _operand(matrix, "from_homography_torch: matrix", [(3, 3)])
    minv = torch.linalg.inv(matrix.double())
    return _build_torch("homography", minv.reshape(((B,) if B else ()) + (9,)), out_hw, _map_dtype(dtype, matrix.dtype))


def radial_torch(in_hw, out_hw, k1, k2=0.0, centre=None, dtype=None):
    """radial on the coefficients' device, differentiable: k1 a 0-d or [B] device tensor (float32 or float64); k2 alike, or a
    number (a constant); centre a device tensor [2] or [B, 2] (row, col of the source), or None = the middle of the source (a
    constant) -> the map [oH, oW, 2], or [B, oH, oW, 2] when any operand carries a B (the others are shared), in k1's dtype (or
    `dtype`).  The geometry scalars (the half-diagonals, the half-extents of the output) are constants: the kernel returns their
    gradient entries and they are dropped.  Bit-equal to radial(..., device=) for the same numbers."""
    import torch
    H, W = int(in_hw[0]), int(in_hw[1])
    oH, oW = int(out_hw[0]), int(out_hw[1])
    what = "radial_torch"
    ops_, sizes = [k1], [_operand(k1, what + ": k1", [()])]
    if isinstance(k2, torch.Tensor):
        ops_.append(k2), sizes.append(_operand(k2, what + ": k2", [()]))
    if centre is not None:
        ops_.append(centre), sizes.append(_operand(centre, what + ": centre", [(2,)]))
    B = _one_batch(what, ops_, sizes)
    lead = (B,) if B else ()
    const = lambda v: torch.full(lead, float(v), dtype=torch.float64, device=k1.device)
    k2t = k2.double().expand(lead) if isinstance(k2, torch.Tensor) else const(k2)
    if centre is None:
        cr, cc = const((H - 1) / 2.0), const((W - 1) / 2.0)
    else:
        c = centre.double().expand(lead + (2,))
        cr, cc = c[..., 0], c[..., 1]
    params = torch.stack([cr, cc, const(np.hypot(oH, oW) / 2.0), const(np.hypot(H, W) / 2.0), const((oH - 1) / 2.0), const((oW - 1) / 2.0),
                          k1.double().expand(lead), k2t], dim=-1)
    return _build_torch("radial", params, (oH, oW), _map_dtype(dtype, k1.dtype))


def brown_params_torch(K, dist=None, R=None, new_K=None):
    """brown_params in torch ops on the operands' device, differentiable in all four: K [3, 3] (no skew), dist [4], [5] or [8]
    (missing coefficients 0; None: all 0), R [3, 3] (None: identity), new_K [3, 3] (None: K), each a float32 / float64 device
    tensor, single or behind a leading B (single operands are shared by the batch) -> float64 [21] or [B, 21]:
    inv(new_K . R) by torch.linalg.inv, fx, fy, cx, cy picked from K, dist padded to 8.  The skew check reads K (one sync)."""
    return _camera_params_torch("brown_params_torch", K, dist, R, new_K, [(4,), (5,), (8,)], 8)


def _camera_params_torch(what, K, dist, R, new_K, dist_shapes, n_dist):
    """inv(new_K . R)[9], fx, fy, cx, cy, dist padded to n_dist -> float64 [13 + n_dist] or [B, 13 + n_dist], in torch ops"""
    import torch
    ops_, sizes = [K], [_operand(K, what + ": K", [(3, 3)])]
    if dist is not None:
        ops_.append(dist), sizes.append(_operand(dist, what + ": dist", dist_shapes))
    for t, name in ((R, "R"), (new_K, "new_K")):
        if t is not None:
            ops_.append(t), sizes.append(_operand(t, "%s: %s" % (what, name), [(3, 3)]))
    B = _one_batch(what, ops_, sizes)
    lead = (B,) if B else ()
    Kd = K.double()
    with torch.no_grad():
        skew = (Kd[..., 0, 1] != 0) | (Kd[..., 1, 0] != 0) | (Kd[..., 2, 0] != 0) | (Kd[..., 2, 1] != 0) | (Kd[..., 2, 2] != 1)
        if bool(skew.any()):
            raise ValueError("K must be [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] (skew is not supported)")
    Rd = torch.eye(3, dtype=torch.float64, device=K.device) if R is None else R.double()
    Nd = Kd if new_K is None else new_K.double()
    minv = torch.linalg.inv(torch.matmul(Nd, Rd)).expand(lead + (3, 3))
    Kd = Kd.expand(lead + (3, 3))
    cam = torch.stack([Kd[..., 0, 0], Kd[..., 1, 1], Kd[..., 0, 2], Kd[..., 1, 2]], dim=-1)
    d = torch.zeros(lead + (n_dist,), dtype=torch.float64, device=K.device) if dist is None else dist.double().expand(lead + (dist.shape[-1],))
    if d.shape[-1] < n_dist:
        d = torch.cat([d, torch.zeros(lead + (n_dist - d.shape[-1],), dtype=torch.float64, device=K.device)], dim=-1)
    return torch.cat([minv.reshape(lead + (9,)), cam, d], dim=-1)


def undistort_rectify_torch(K, dist, R, new_K, out_hw, dtype=None):
    """undistort_rectify on the operands' device, differentiable: the operands of brown_params_torch (device tensors, single or
    behind a leading B; dist, R and new_K may be None) -> the map [oH, oW, 2] or [B, oH, oW, 2] in K's dtype (or `dtype`).  K, dist,
    R and new_K each receive a gradient when they require one: the 21 parameters go through lerf_coords_build_dev and its
    adjoint lerf_coords_build_bwd, the assembly (the 3 x 3 inverse included) through autograd.  Calibration refinement: fit k1 ..
    k6, p1, p2, fx, fy, cx, cy against a rectified target through a remap class that has opted in with enable_backward()."""
    return _build_torch("brown", brown_params_torch(K, dist, R, new_K), out_hw, _map_dtype(dtype, K.dtype))


def fisheye_params_torch(K, dist4=None, R=None, new_K=None):
    """fisheye_params in torch ops on the operands' device, differentiable in all four: K [3, 3] (no skew), dist4 [4] (None: all 0), R
    [3, 3] (None: identity), new_K [3, 3] (None: K), each a float32 / float64 device tensor, single or behind a leading B (single
    operands are shared by the batch) -> float64 [17] or [B, 17].  The skew check reads K (one sync)."""
    return _camera_params_torch("fisheye_params_torch", K, dist4, R, new_K, [(4,)], 4)


def fisheye_undistort_rectify_torch(K, dist, R, new_K, out_hw, dtype=None):
    """fisheye_undistort_rectify on the operands' device, differentiable: the operands of fisheye_params_torch (device tensors,
    single or behind a leading B, one map per sample in one launch; dist, R and new_K may be None) -> the map [oH, oW, 2] or
    [B, oH, oW, 2] in K's dtype (or `dtype`).  K, dist, R and new_K each receive a gradient when they require one: the 17
    parameters go through lerf_coords_build_dev and its adjoint lerf_coords_build_bwd, the assembly (the inverse of new_K . R
    included) through autograd.  An entry behind the camera contributes nothing; at the principal ray the gradient is the
    pinhole's.  invert_torch of this map distorts a pinhole frame."""
    return _build_torch("fisheye", fisheye_params_torch(K, dist, R, new_K), out_hw, _map_dtype(dtype, K.dtype))


def equirect_view_torch(pano_hw, K_view, R, out_hw, dtype=None):
    """equirect_view on the operands' device, differentiable in K_view and R: K_view [3, 3] (no skew) and R [3, 3] (None: identity)
    float32 / float64 device tensors, single or behind a leading B -> the map [oH, oW, 2] or [B, oH, oW, 2] in K_view's dtype (or
    `dtype`).  The panorama's scalars (equirect_params) are constants: the kernel returns their gradient entries and they are
    dropped.  At a pole (d.x = d.z = 0) the matrix receives nothing from that entry.  invert_torch of this map pastes a view
    into the panorama's frame."""
    import torch
    Hp, Wp = int(pano_hw[0]), int(pano_hw[1])
    if Hp < 1 or Wp < 1:
        raise ValueError("pano_hw must be positive")
    cam = _camera_params_torch("equirect_view_torch", K_view, None, R, None, [], 0)          # inv(K_view . R)[9], fx, fy, cx, cy
    pano = torch.tensor([Wp / (2.0 * np.pi), Hp / np.pi, (Wp - 1) / 2.0, (Hp - 1) / 2.0], dtype=torch.float64, device=K_view.device)
    params = torch.cat([cam[..., :9], pano.expand(tuple(cam.shape[:-1]) + (4,))], dim=-1)
    return _build_torch("equirect", params, out_hw, _map_dtype(dtype, K_view.dtype))


# ---------------------------------------------------------------------------------------------- reproject by depth
def _last_row_ok(K_dst):
    return bool(np.all(K_dst[..., 2, 0] == 0.0) and np.all(K_dst[..., 2, 1] == 0.0) and np.all(K_dst[..., 2, 2] == 1.0))


def reproject_params(K_src, K_dst, R=None, t=None):
    """The 12 parameters of reproject from two cameras and a pose: K_src, K_dst (3 x 3 camera matrices; the last row of K_dst must be
    (0, 0, 1), so that the third homogeneous coordinate is the depth in the second view), R (3 x 3, default I) and t (3, default 0) with
    X_dst = R X_src + t -> float64 [12] = (K_dst . R . inv(K_src))[9] row-major, (K_dst . t)[3]; the inverse is np.linalg.inv's.  Any
    operand may carry a leading B (the others are shared) -> [B, 12].  Host numpy."""
    Ks, Kd = _host(K_src), _host(K_dst)
    Rm = np.eye(3) if R is None else _host(R)
    tv = np.zeros(3) if t is None else _host(t)
    for a, name, nd in ((Ks, "K_src", 2), (Kd, "K_dst", 2), (Rm, "R", 2), (tv, "t", 1)):
        if a.ndim not in (nd, nd + 1) or a.shape[-nd:] != (3,) * nd or a.shape[0] < 1:
            raise ValueError("%s must be %s, or that behind a leading batch size" % (name, "3x3" if nd == 2 else "[3]"))
    if not _last_row_ok(Kd):
        raise ValueError("the last row of K_dst must be (0, 0, 1): reproject's third coordinate is the depth in the second view")
    sizes = {a.shape[0] for a, nd in ((Ks, 2), (Kd, 2), (Rm, 2), (tv, 1)) if a.ndim == nd + 1}
    if len(sizes) > 1:
        raise ValueError("the operands hold different numbers of samples")
    m = np.matmul(np.matmul(Kd, Rm), np.linalg.inv(Ks))
    q = np.matmul(Kd, tv[..., None])[..., 0]
    lead = (sizes.pop(),) if sizes else ()
    return np.ascontiguousarray(np.concatenate([np.broadcast_to(m, lead + (3, 3)).reshape(lead + (9,)), np.broadcast_to(q, lead + (3,))], axis=-1))


def reproject_params_torch(K_src, K_dst, R=None, t=None):
    """reproject_params in torch ops on the operands' device, differentiable in all four: K_src, K_dst [3, 3], R [3, 3] (None:
    identity), t [3] (None: 0), each a float32 / float64 device tensor, single or behind a leading B (single operands are shared by
    the batch) -> float64 [12] or [B, 12]: K_dst . R . inv(K_src) by torch.linalg.inv, K_dst . t.  The check of K_dst's last row
    reads it (one sync)."""
    import torch
    what = "reproject_params_torch"
    ops_, sizes = [K_src, K_dst], [_operand(K_src, what + ": K_src", [(3, 3)]), _operand(K_dst, what + ": K_dst", [(3, 3)])]
    if R is not None:
        ops_.append(R), sizes.append(_operand(R, what + ": R", [(3, 3)]))
    if t is not None:
        ops_.append(t), sizes.append(_operand(t, what + ": t", [(3,)]))
    B = _one_batch(what, ops_, sizes)
    lead = (B,) if B else ()
    Kd = K_dst.double()
    with torch.no_grad():
        if bool(((Kd[..., 2, 0] != 0) | (Kd[..., 2, 1] != 0) | (Kd[..., 2, 2] != 1)).any()):
            raise ValueError("the last row of K_dst must be (0, 0, 1): reproject's third coordinate is the depth in the second view")
    KR = Kd if R is None else torch.matmul(Kd, R.double())
    m = torch.matmul(KR, torch.linalg.inv(K_src.double())).expand(lead + (3, 3))
    q = torch.zeros(lead + (3,), dtype=torch.float64, device=K_src.device) if t is None else \
        torch.matmul(Kd, t.double().unsqueeze(-1)).squeeze(-1).expand(lead + (3,))
    return torch.cat([m.reshape(lead + (9,)), q], dim=-1)


def _depth_kind(inverse_depth):
    return "inverse" if inverse_depth else "z"


def reproject(depth, K_src, K_dst, R=None, t=None, inverse_depth=False, dtype=None, return_depth=False):
    """The map that carries a view with a depth per pixel into another view (lerf_coords_reproject): depth [H, W] (or a
    batch [B, H, W], one launch) is the depth z of every pixel of the view of K_src -- or 1 / z with inverse_depth=True, where 0 is
    a point at infinity -- and K_dst, R, t (X_dst = R X_src + t; reproject_params) describe the other view.  -> [H, W, 2] (or
    [B, H, W, 2]), float64 (default) or float32: entry (i, j) is (row, col) of pixel (i, j) in the other view, (NaN, NaN) where the
    depth is not positive (inverse: negative), not finite, or the point lies behind the other camera.  return_depth=True -> (map, zo),
    zo float32 of depth's shape: the depth in the other view (inverse_depth: +inf at infinity), NaN where the map is.

    Two chains end in a remap (names of this module):

        remap(img_src, reproject(depth_dst, K_dst, K_src, R, t))
            BACKWARD warp: the map of the target view (its own depth, the pose target -> source) reads the source frame -- view
            synthesis and the photometric loss of self-supervised depth; every target pixel has one source, occlusions are not seen.
        m, z = reproject(depth_src, K_src, K_dst, R, t, return_depth=True)
        remap(img_src, invert_raster(m, hw, depth=z, orient=1))
            FORWARD splat: the source's own depth carries it into the target view, the rasterising inverse lets the nearest surface
            win where several land on one pixel and leaves the disocclusions NaN (mask false in the remap).

    numpy depth -> numpy (the kernel's host twin); a device tensor -> device tensors written by the kernel, bit-equal to the host's for
    equal parameters.  The cameras and the pose are host values (arrays, lists, host tensors) or, beside a device depth, tensors on its
    device; a device tensor beside a host depth, or a host tensor beside a device depth, is refused.  No autograd: an operand that
    requires grad (with grad mode on) is refused -- reproject_torch is the differentiable twin."""
    cams = [a for a in (K_src, K_dst, R, t) if a is not None]
    on_dev = bool(getattr(depth, "is_cuda", False))
    for a in cams:                                                       # an array or a list has no is_cuda: a host value, taken beside either
        if hasattr(a, "is_cuda") and bool(a.is_cuda) != on_dev:
            raise ValueError("reproject: the depth and the cameras on the host or on one device, not mixed")
    _no_autograd("reproject", [depth] + cams)
    if getattr(depth, "ndim", None) not in (2, 3) or min(depth.shape) < 1:
        raise ValueError("reproject: depth is [H, W] or [B, H, W]")
    p = reproject_params(K_src, K_dst, R, t)
    B = depth.shape[0] if depth.ndim == 3 else 0
    if p.ndim == 2 and B and p.shape[0] != B:
        raise ValueError("reproject: depth and the cameras hold different numbers of samples")
    if B and p.ndim == 1:
        p = np.ascontiguousarray(np.broadcast_to(p, (B, 12)))
    kind, want = _depth_kind(inverse_depth), (True if return_depth else None)
    if on_dev:
        import torch
        from . import ops
        d = depth.detach()
        d = d if d.dtype in (torch.float32, torch.float64) else d.double()
        return ops.coords_reproject(kind, torch.from_numpy(p).to(d.device), d, dtype=getattr(torch, _np_dtype(dtype).name), depth_out=want)
    from . import _lib
    d = np.asarray(depth.detach().numpy() if hasattr(depth, "detach") else depth)
    d = d if d.dtype in (np.float32, np.float64) else d.astype(np.float64)
    return _lib.coords_reproject_host(kind, p, d, _np_dtype(dtype), depth_out=want)


_REPROJECT_FN = None


def _reproject_fn():
    global _REPROJECT_FN
    if _REPROJECT_FN is None:
        import torch
        from torch.autograd.function import once_differentiable
        from . import ops

        class _ReprojectFn(torch.autograd.Function):
            """(map[, zo]) = ops.coords_reproject(params, depth); backward: ops.coords_reproject_bwd in float64, the half that is not
            required skipped; the depth's gradient cast to its dtype, the 12-vector's handed on to autograd"""

            @staticmethod
            def forward(ctx, depth, params, kind, tdt, want_zo):
                d, p = depth.detach().contiguous(), params.detach().contiguous()
                ctx.save_for_backward(d, p)
                ctx.kind, ctx.depth_dtype = kind, depth.dtype
                ctx.set_materialize_grads(False)
                return ops.coords_reproject(kind, p, d, dtype=tdt, depth_out=True if want_zo else None)

            @staticmethod
            @once_differentiable
            def backward(ctx, gmap, gzo=None):
                d, p = ctx.saved_tensors
                need = (ctx.needs_input_grad[0], ctx.needs_input_grad[1])
                if (gmap is None and gzo is None) or not (need[0] or need[1]):
                    return None, None, None, None, None
                lead = tuple(p.shape[:-1]) + tuple(d.shape[-2:])
                gm = torch.zeros(lead + (2,), dtype=torch.float64, device=d.device) if gmap is None else gmap.contiguous().double()
                gz = None if gzo is None else gzo.contiguous().double()
                gd, gp = ops.coords_reproject_bwd(ctx.kind, p, d, gm, gz, need=need)
                if gd is not None and gd.ndim > d.ndim:                  # one depth plane shared by the batch: the sum over the samples
                    gd = gd.sum(0)
                return None if gd is None else gd.to(ctx.depth_dtype), gp, None, None, None

        _REPROJECT_FN = _ReprojectFn
    return _REPROJECT_FN


def reproject_torch(depth, K_src, K_dst, R=None, t=None, inverse_depth=False, dtype=None, return_depth=False):
    """reproject on the operands' device, differentiable: depth [H, W] or [B, H, W] and the operands of reproject_params_torch, all
    float32 / float64 DEVICE tensors (single camera operands are shared by a batch) -> the map (float64, or `dtype`), or (map, zo)
    with return_depth=True.  depth, K_src, K_dst, R and t each receive a gradient when they require one: the map and zo go through
    lerf_coords_reproject and its adjoint lerf_coords_reproject_bwd (float64, a fixed summation order: bit-equal from run to run),
    the 12 parameters' assembly -- the inverse of K_src included -- through autograd.  An entry that is not valid contributes
    nothing, unlike autograd of the same formulas.  The photometric loss of self-supervised depth and ego-motion: a remap class that
    has opted in with enable_backward() hands this map its gradient.  Once differentiable."""
    import torch
    from . import ops
    if not isinstance(depth, torch.Tensor) or not depth.is_cuda or depth.dtype not in (torch.float32, torch.float64):
        raise ValueError("reproject_torch: depth must be a float32 or float64 device tensor")
    if depth.ndim not in (2, 3) or min(depth.shape) < 1:
        raise ValueError("reproject_torch: depth is [H, W] or [B, H, W]")
    params = reproject_params_torch(K_src, K_dst, R, t)
    if params.device != depth.device:
        raise ValueError("reproject_torch: the depth and the cameras live on different devices")
    B = depth.shape[0] if depth.ndim == 3 else 0
    if params.ndim == 2 and B and params.shape[0] != B:
        raise ValueError("reproject_torch: depth and the cameras hold different numbers of samples")
    if B and params.ndim == 1:
        params = params.expand(B, 12)
    kind, tdt = _depth_kind(inverse_depth), _map_dtype(dtype, torch.float64)
    if torch.is_grad_enabled() and (depth.requires_grad or params.requires_grad):
        return _reproject_fn().apply(depth, params, kind, tdt, bool(return_depth))
    return ops.coords_reproject(kind, params.detach().contiguous(), depth.detach(), dtype=tdt, depth_out=True if return_depth else None)


# ---------------------------------------------------------------------------------------------- forward warp by splatting
SPLAT_MODES = ("sum", "average", "linear", "softmax")


def _splat_args(what, src, map, out_hw, weight, mode):
    if mode not in SPLAT_MODES:
        raise ValueError("%s: mode is one of %s, not %r" % (what, ", ".join(SPLAT_MODES), mode))
    if mode == "average" and weight is not None:
        raise ValueError("%s: mode 'average' takes no weight (every pixel counts 1); 'linear' weighs" % what)
    if mode in ("linear", "softmax") and weight is None:
        raise ValueError("%s: mode %r needs a weight" % (what, mode))
    if getattr(src, "ndim", None) not in (3, 4) or min(src.shape) < 1:
        raise ValueError("%s: src is [C, H, W] or [B, C, H, W]" % what)
    lead, hw = tuple(src.shape[:-3]), tuple(src.shape[-2:])
    if getattr(map, "ndim", None) not in (3, 4) or tuple(map.shape[-3:]) != hw + (2,) or (map.ndim == 4 and tuple(map.shape[:1]) != lead):
        raise ValueError("%s: map is [H, W, 2] (shared by the batch) or [B, H, W, 2], H and W the source's" % what)
    if weight is not None and tuple(getattr(weight, "shape", ())) != lead + hw:
        raise ValueError("%s: weight is [H, W], or [B, H, W] beside a batch" % what)
    oH, oW = int(out_hw[0]), int(out_hw[1])
    if oH < 1 or oW < 1:
        raise ValueError("%s: out_hw must be positive" % what)
    return oH, oW


def splat(src, map, out_hw, weight=None, mode="sum", eps=1e-7, return_norm=False, deterministic=False, max_adders=4096):
    """Forward warp by SUMMATION SPLATTING (lerf_splat): every pixel of src [C, H, W] (or a batch [B, C, H, W]) is ADDED
    into the frame out_hw = (oH, oW) at the position map[i, j] = (row, col) gives it -- map [H, W, 2], shared by the batch, or
    [B, H, W, 2]; invert_raster reads a forward map the same way -- spread bilinearly over up to four pixels.  Mass that leaves the frame
    is lost (a tap outside is dropped, not clipped); an entry that is not finite contributes nothing (NaN: "no target").  Where
    invert_raster + remap lets the nearest surface win by a hard test, this sums, and a normalisation plane divides:

        mode        what it returns
        "sum"       the accumulator; weight (src's dtype, [H, W] or [B, H, W]) multiplies every pixel if given
        "average"   weight must be None:  acc / (norm + eps),  norm = the splatted ones
        "linear"    the same quotient with weight as the importance:  splat(weight * src) / (splat(weight) + eps)
        "softmax"   the same with m = exp(weight - max over the sample) as the importance.  The shift cancels in the quotient (up to
                    eps); it keeps exp in range.  weight = -beta * z with z from reproject(..., return_depth=True) is the soft depth
                    test: the nearer surface dominates by exp(-beta * dz).  A NaN weight counts as -inf (m = 0): reproject's z is NaN
                    exactly where its map is.

    return_norm=True -> (out, norm) with norm [oH, oW] (or [B, oH, oW]) the splatted importance; norm == 0 is the hole mask.
    numpy operands -> numpy (the kernel's host twin, row-major order); device tensors -> device tensors written by the kernel (float
    atomic adds: equal from run to run up to the rounding of a reordered sum).  Mixed operands are refused.  The quotient and the exp
    are elementwise array / tensor operations.  float32 / float64 src decides the dtype; the map may be either.  No autograd: an
    operand that requires grad (with grad mode on) is refused -- splat_torch is the differentiable twin.
    deterministic=True (device tensors): the ORDERED scatter (lerf_splat_ordered) -- every output pixel adds its source
    pixels in row-major order, so the accumulator equals the host twin's bit for bit and two runs agree exactly.  It ends with one
    4-byte copy to the host and a synchronisation, and raises LerfError when more than max_adders source pixels add into one output
    pixel (a map that collapses the frame; that pixel would hold NaN).  On numpy operands the flag is accepted and changes nothing: the
    host twin is ordered already."""
    oH, oW = _splat_args("splat", src, map, out_hw, weight, mode)
    ops_ = [t for t in (src, map, weight) if t is not None]
    dev = [bool(getattr(t, "is_cuda", False)) for t in ops_]
    if any(d != dev[0] for d in dev):
        raise ValueError("splat: src, map and weight on the host or all on one device, not mixed")
    _no_autograd("splat", ops_)
    norm = mode != "sum" or bool(return_norm)
    if dev[0]:
        import torch
        from . import ops
        x = src.detach()
        x = x if x.dtype in (torch.float32, torch.float64) else x.double()
        f = map.detach()
        f = f if f.dtype in (torch.float32, torch.float64) else f.double()
        w = None if weight is None else weight.detach().to(x.dtype)
        if mode == "softmax":
            w = _softmax_importance_torch(w)
        acc = ops.splat(x, f, (oH, oW), w, norm, **_ordered_kw(int(max_adders) if deterministic else None))
    else:
        from . import _lib
        x, f, w = (None if t is None else np.asarray(t.detach().numpy() if hasattr(t, "detach") else t) for t in (src, map, weight))
        x = x if x.dtype in (np.float32, np.float64) else x.astype(np.float64)
        f = f if f.dtype in (np.float32, np.float64) else f.astype(np.float64)
        w = None if w is None else w.astype(x.dtype, copy=False)
        if mode == "softmax":
            w = np.where(np.isnan(w), -np.inf, w)
            top = w.max(axis=(-2, -1), keepdims=True)
            w = np.exp(w - np.where(np.isfinite(top), top, 0)).astype(x.dtype, copy=False)
        acc = _lib.splat_host(x, f, (oH, oW), w, norm)
    C = x.shape[-3]
    out = acc[..., :C, :, :]
    if mode != "sum":
        out = out / (acc[..., C:, :, :] + eps)
    return (out, acc[..., C, :, :]) if return_norm else out


def _softmax_importance_torch(w):
    """exp(w - max over the sample); a NaN counts as -inf; in torch ops, so autograd carries it (the max is a constant: it cancels)"""
    import torch
    w = torch.where(torch.isnan(w), torch.full_like(w, float("-inf")), w)
    top = w.detach().amax(dim=(-2, -1), keepdim=True)
    return torch.exp(w - torch.where(torch.isfinite(top), top, torch.zeros_like(top)))


_SPLAT_FN = None


def _splat_fn():
    global _SPLAT_FN
    if _SPLAT_FN is None:
        import torch
        from torch.autograd.function import once_differentiable
        from . import ops

        class _SplatFn(torch.autograd.Function):
            """acc = ops.splat(src, map, weight); backward: ops.splat_bwd, the halves that are not required skipped; the map's
            gradient (float64) cast to the map's dtype"""

            @staticmethod
            def forward(ctx, src, weight, map, hw, norm, ordered=None):
                x, f = src.detach().contiguous(), map.detach()
                m = None if weight is None else weight.detach().contiguous()
                ctx.save_for_backward(x, f, *(() if m is None else (m,)))
                ctx.hw, ctx.norm, ctx.map_dtype = hw, norm, map.dtype
                return ops.splat(x, f, hw, m, norm, **_ordered_kw(ordered))

            @staticmethod
            @once_differentiable
            def backward(ctx, grad):
                x, f = ctx.saved_tensors[:2]
                m = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else None
                need = (ctx.needs_input_grad[0], m is not None and ctx.needs_input_grad[1], ctx.needs_input_grad[2])
                if not any(need):
                    return None, None, None, None, None, None
                gx, gm, gf = ops.splat_bwd(x, f, grad.contiguous().to(x.dtype), m, ctx.norm, need)
                return gx, gm, None if gf is None else gf.to(ctx.map_dtype), None, None, None

        _SPLAT_FN = _SplatFn
    return _SPLAT_FN


_TRIANGLES_FN = None


def _triangles_fn():
    global _TRIANGLES_FN
    if _TRIANGLES_FN is None:
        import torch
        from torch.autograd.function import once_differentiable
        from . import ops

        class _TrianglesFn(torch.autograd.Function):
            """map (, depth_out), keys = ops.coords_trimesh(...); backward: ops.coords_trimesh_bwd at the saved keys in float64, one call
            for the whole batch; an operand the batch shares gains the sum of its per-set gradients; each gradient cast to its
            operand's dtype"""

            @staticmethod
            def forward(ctx, pos, attr, w, faces, attr_faces, depth, hw, tdt, max_span, orient, want_depth, max_adders):
                p, a = pos.detach().contiguous(), attr.detach().contiguous()
                wv = None if w is None else w.detach().contiguous()
                res = ops.coords_trimesh(p, a, faces, hw, attr_faces=attr_faces, depth=depth, w=wv, dtype=tdt, max_span=max_span, orient=orient,
                                         return_keys=True, return_depth=want_depth)
                out, keys = res[0], res[1]
                ctx.save_for_backward(p, a, keys, *(() if wv is None else (wv,)))
                ctx.mesh = (faces, attr_faces, depth, hw, max_span, orient, max_adders)
                ctx.dtypes = (pos.dtype, attr.dtype, None if w is None else w.dtype)
                ctx.mark_non_differentiable(keys)
                if want_depth:
                    ctx.mark_non_differentiable(res[2])
                    return out, keys, res[2]
                return out, keys

            @staticmethod
            @once_differentiable
            def backward(ctx, grad, *unused):
                p, a, keys = ctx.saved_tensors[:3]
                wv = ctx.saved_tensors[3] if len(ctx.saved_tensors) > 3 else None
                faces, attr_faces, depth, hw, max_span, orient, max_adders = ctx.mesh
                need = (ctx.needs_input_grad[1], ctx.needs_input_grad[0], wv is not None and ctx.needs_input_grad[2])
                none = (None,) * 12
                if not any(need):
                    return none
                ga, gp, gw = ops.coords_trimesh_bwd(p, a, faces, hw, keys, grad.detach().to(torch.float64).contiguous(), attr_faces=attr_faces,
                                                    depth=depth, w=wv, max_span=max_span, orient=orient, need=need, max_adders=max_adders)
                batch = keys.dim() == 3

                def fit(g, operand, base, dt):
                    if g is None:
                        return None
                    if batch and operand.dim() == base:          # shared across the batch: the per-set gradients summed, set 0 first
                        total = g[0]
                        for s in range(1, g.shape[0]):
                            total = total + g[s]
                        g = total
                    return g.to(dt)

                return (fit(gp, p, 2, ctx.dtypes[0]), fit(ga, a, 2, ctx.dtypes[1]), fit(gw, wv, 1, ctx.dtypes[2])) + none[3:]

        _TRIANGLES_FN = _TrianglesFn
    return _TRIANGLES_FN


def from_triangles_torch(pos, attr, faces, out_hw, attr_faces=None, depth=None, w=None, max_span=0, orient=0, dtype=None, return_depth=False,
                         return_faces=False, max_adders=4096):
    """from_triangles on the operands' device, DIFFERENTIABLE (lerf_coords_trimesh_bwd): pos [V, 2], attr [Va, 2] and
    w [V] (or None) are float32 / float64 DEVICE tensors, faces / attr_faces integer device tensors, depth [V] a device tensor; the
    rest as from_triangles -> what from_triangles returns, bit for bit.  pos, attr and w each receive a gradient when they require
    one: landmark positions fitted by a photometric loss, refined UVs, the vertices of a projected mesh --

        remap(img, from_triangles_torch(pos, attr, faces, hw))          # through a *Remap2dTorch twin after enable_backward()

    VISIBILITY IS HELD FIXED: every pixel belongs to the face that won it in the forward (the key plane, saved for the backward);
    coverage, edges and the depth test are piecewise constant and give no gradient, as in any rasterise-then-interpolate renderer.
    So depth gets no gradient (a depth that requires grad is refused), the depth and faces results are not differentiable, and a
    NaN the loss puts at a hole reaches nothing.  The backward is a face pass (one workgroup per face reduces its pixels by a fixed
    tree) and a vertex pass (one writer per vertex adds its faces in ascending (face, corner) order): bit-equal from run to run.  It
    ends with one 4-byte copy to the host and a synchronisation, and raises LerfError when more than max_adders drawn face corners
    meet in one vertex.  pos / attr [B, V, 2] run one call forward and one backward; an operand without the B axis is shared and
    gains the sum over the batch.  Gradients are computed in float64 and cast to each operand's dtype.  Once differentiable."""
    import torch
    for t, name in ((pos, "pos"), (attr, "attr"), (w, "w")):
        if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in (torch.float32, torch.float64)):
            raise ValueError("from_triangles_torch: %s must be a float32 or float64 device tensor" % name)
    for t, name in ((faces, "faces"), (attr_faces, "attr_faces"), (depth, "depth")):
        if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda):
            raise ValueError("from_triangles_torch: %s must be a device tensor" % name)
    if any(t is not None and t.device != pos.device for t in (attr, faces, attr_faces, depth, w)):
        raise ValueError("from_triangles_torch: the operands live on different devices")
    if depth is not None and depth.requires_grad and torch.is_grad_enabled():
        raise ValueError("from_triangles_torch: depth gets no gradient -- visibility is held fixed, the depth test is piecewise constant; "
                         "pass depth.detach()")
    H, W = int(out_hw[0]), int(out_hw[1])
    if H < 1 or W < 1:
        raise ValueError("out_hw must be positive")
    if return_depth and depth is None:
        raise ValueError("from_triangles_torch: return_depth needs depth")
    fc = _int32_indices(faces.detach(), torch.int32, lambda x, dt: x.to(dt).contiguous())
    af = None if attr_faces is None else _int32_indices(attr_faces.detach(), torch.int32, lambda x, dt: x.to(dt).contiguous())
    d = None if depth is None else depth.detach().to(torch.float32).contiguous()
    tdt = None if dtype is None else (dtype if isinstance(dtype, torch.dtype) else getattr(torch, _np_dtype(dtype).name))
    res = _triangles_fn().apply(pos, attr, w, fc, af, d, (H, W), tdt, int(max_span), int(orient), bool(return_depth), int(max_adders))
    m, k = res[0], res[1]
    if not (return_faces or return_depth):
        return m
    low = torch.where(k == -1, k, k & 0xffffffff)
    return (m,) + ((res[2],) if return_depth else ()) + ((low,) if return_faces else ())


def splat_torch(src, map, out_hw, weight=None, mode="sum", eps=1e-7, return_norm=False, deterministic=None, max_adders=4096):
    """splat on the operands' device, differentiable: src [C, H, W] or [B, C, H, W], map [H, W, 2] or [B, H, W, 2] and weight ([H, W] or
    [B, H, W], or None), all float32 / float64 DEVICE tensors (weight is cast to src's dtype) -> what splat returns.  src, weight and
    map each receive a gradient when they require one, through lerf_splat_bwd -- a gather with one writer per source pixel, bit-equal
    from run to run; a half that is not required is skipped.  The map's gradient is the derivative of the bilinear cell floor picked
    (one-sided at integer positions); a non-finite entry gets exact zeros.  The modes are built from the one accumulator in torch ops,
    so autograd carries the quotient and the exp.  The third chain beside reproject's two -- the source's own depth, differentiable:

        m, z = reproject_torch(depth_src, K_src, K_dst, R, t, return_depth=True)
        splat_torch(img_src, m, hw, weight=-beta * z, mode="softmax")

    deterministic (None: follow torch.are_deterministic_algorithms_enabled(), read at this call): the forward by the ORDERED scatter
    (lerf_splat_ordered) -- bit-equal from run to run and to lerf_splat_host.  The forward then ends with one 4-byte copy
    to the host and a synchronisation, and raises LerfError when more than max_adders source pixels add into one output pixel.  The
    backward is a gather and was reproducible all along.  Once differentiable."""
    import torch
    oH, oW = _splat_args("splat_torch", src, map, out_hw, weight, mode)
    for t, name in ((src, "src"), (map, "map"), (weight, "weight")):
        if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in (torch.float32, torch.float64)):
            raise ValueError("splat_torch: %s must be a float32 or float64 device tensor" % name)
    if any(t is not None and t.device != src.device for t in (map, weight)):
        raise ValueError("splat_torch: src, map and weight live on different devices")
    w = None if weight is None else weight.to(src.dtype)
    if mode == "softmax":
        w = _softmax_importance_torch(w)
    norm = mode != "sum" or bool(return_norm)
    ordered = int(max_adders) if _deterministic(deterministic) else None
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (src, map, w)):
        acc = _splat_fn().apply(src, w, map, (oH, oW), norm, ordered)
    else:
        from . import ops
        acc = ops.splat(src.detach(), map.detach(), (oH, oW), None if w is None else w.detach(), norm, **_ordered_kw(ordered))
    C = src.shape[-3]
    out = acc[..., :C, :, :]
    if mode != "sum":
        out = out / (acc[..., C:, :, :] + eps)
    return (out, acc[..., C, :, :]) if return_norm else out
