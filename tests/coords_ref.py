"""Yardstick of the coordinate-map builders, independent of the package: float64 numpy restatements of the BROWN camera model, the
mesh upsample (bilinear, bicubic) and compose, written from the formulas of the C ABI's contract (include/lerf_hip.h), and a
float64 torch restatement of the mesh upsample for autograd.

numpy rounds every elementwise product and sum and evaluates left to right as written, so a restatement in the stated order is
bit-equal to the library where the contract says so.  tests/test_coords_cpu.py anchors these restatements on independent
ground (np.dot homographies, coords.radial, F.interpolate) before it holds the library against them."""
import numpy as np

A = -0.75     # Keys coefficient of torch's upsample_bicubic2d


def _ij(out_hw, origin=(0, 0)):
    ii, jj = np.meshgrid(np.arange(out_hw[0]) + origin[0], np.arange(out_hw[1]) + origin[1], indexing="ij")
    return ii.astype(np.float64), jj.astype(np.float64)


def brown(minv, fx, fy, cx, cy, dist, out_hw, origin=(0, 0)):
    """minv: inv(new_K . R) [3, 3]; dist: k1 k2 p1 p2 k3 k4 k5 k6 -> float64 [oH, oW, 2] (row, col)"""
    m = np.asarray(minv, np.float64).reshape(9)
    k1, k2, p1, p2, k3, k4, k5, k6 = (float(v) for v in dist)
    y_, x_ = _ij(out_hw, origin)
    X = m[0] * x_ + m[1] * y_ + m[2]
    Y = m[3] * x_ + m[4] * y_ + m[5]
    Wh = m[6] * x_ + m[7] * y_ + m[8]
    x = X / Wh
    y = Y / Wh
    r2 = x * x + y * y
    rad = (1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1.0 + r2 * (k4 + r2 * (k5 + r2 * k6)))
    xy = x * y
    xd = (x * rad + (2.0 * p1) * xy) + p2 * (r2 + 2.0 * (x * x))
    yd = (y * rad + p1 * (r2 + 2.0 * (y * y))) + (2.0 * p2) * xy
    return np.stack([fy * yd + cy, fx * xd + cx], axis=-1)


def _c1(x):
    return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0


def _c2(x):
    return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A


def mesh_axis(k, n, g, interp, xp=np):
    """taps of output indices k (float64 array) along an axis of n outputs over g vertices: (indices [taps, len(k)] int,
    weights [taps, len(k)])"""
    u = (k * float(g - 1)) / float(n - 1) if n > 1 else k * 0.0
    f = xp.floor(u)
    if interp == "bilinear":
        a0 = xp.clip(f, 0, g - 2)                              # min(floor(u), g - 2); u >= 0
        t = u - a0
        return xp.stack([a0, a0 + 1]), xp.stack([1.0 - t, t])
    t = u - f
    idx = xp.stack([xp.clip(f + d, 0, g - 1) for d in (-1, 0, 1, 2)])
    return idx, xp.stack([_c2(t + 1.0), _c1(t), _c1(1.0 - t), _c2(2.0 - t)])


def mesh(ctrl, out_hw, interp, origin=(0, 0), full_hw=None):
    """ctrl [gh, gw, 2] (float32 is promoted exactly) -> float64 [oH, oW, 2]:
    value = sum_a wr[a] * (sum_b wc[b] * ctrl[a][b]), both sums left to right"""
    c = np.asarray(ctrl).astype(np.float64)
    gh, gw = c.shape[:2]
    fh, fw = out_hw if full_hw is None else full_hw
    ir, wr = mesh_axis(np.arange(out_hw[0], dtype=np.float64) + origin[0], fh, gh, interp)
    ic, wc = mesh_axis(np.arange(out_hw[1], dtype=np.float64) + origin[1], fw, gw, interp)
    ir, ic = ir.astype(np.int64), ic.astype(np.int64)
    v = None
    for a in range(len(ir)):
        s = None
        for b in range(len(ic)):
            term = wc[b][None, :, None] * c[ir[a][:, None], ic[b][None, :]]
            s = term if s is None else s + term
        term = wr[a][:, None, None] * s
        v = term if v is None else v + term
    return v


def mesh_torch(ctrl, out_hw, interp):
    """the same upsample in float64 torch ops on ctrl's device; differentiable in ctrl"""
    import torch
    c = ctrl.double()
    gh, gw = c.shape[:2]
    dev = c.device
    ir, wr = mesh_axis(torch.arange(out_hw[0], dtype=torch.float64, device=dev), out_hw[0], gh, interp, xp=torch)
    ic, wc = mesh_axis(torch.arange(out_hw[1], dtype=torch.float64, device=dev), out_hw[1], gw, interp, xp=torch)
    ir, ic = ir.long(), ic.long()
    v = 0
    for a in range(len(ir)):
        s = 0
        for b in range(len(ic)):
            s = s + wc[b][None, :, None] * c[ir[a][:, None], ic[b][None, :]]
        v = v + wr[a][:, None, None] * s
    return v


def _compose_axis(v, n):
    r = np.where(v >= 0.0, np.minimum(v, float(n - 1)), 0.0)          # the clip onto [0, n - 1]; -inf -> 0, +inf -> n - 1
    i0 = np.minimum(np.floor(r), float(n - 2)) if n > 1 else np.zeros_like(r)
    t = r - i0
    return i0.astype(np.int64), (1.0 - t, t)


def compose(outer, inner):
    """C[i, j] = outer(inner[i, j]), float64 [oH, oW, 2]: bilinear taps of the clipped position; every sum starts at +0.0 and adds
    its counted terms in order, a tap of weight exactly 0 is not counted; a NaN coordinate in `inner` gives (NaN, NaN)"""
    a = np.asarray(outer).astype(np.float64)
    b = np.asarray(inner).astype(np.float64)
    aH, aW = a.shape[:2]
    nan = np.isnan(b[..., 0]) | np.isnan(b[..., 1])
    bb = np.where(nan[..., None], 0.0, b)
    i0, wr = _compose_axis(bb[..., 0], aH)
    j0, wc = _compose_axis(bb[..., 1], aW)
    with np.errstate(invalid="ignore"):
        v = np.zeros(b.shape)
        for da in range(2):
            s = np.zeros(b.shape)
            for db in range(2):
                e = a[np.minimum(i0 + da, aH - 1), np.minimum(j0 + db, aW - 1)]      # the index clamp only keeps numpy in range:
                s = s + np.where((wc[db] != 0.0)[..., None], wc[db][..., None] * e, 0.0)   # such a tap has weight 0
            v = v + np.where((wr[da] != 0.0)[..., None], wr[da][..., None] * s, 0.0)
    v[nan] = np.nan
    return v


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))
