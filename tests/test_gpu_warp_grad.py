"""Autograd through the homographic warps: lerf_warp_bwd (csrc/lerf_warp_bwd.hip) behind the *Warp2dTorch classes
(`_WarpFn`) and the dispatcher ops lerf::warp_gauss / warp_linear / warp_backward.

  1. every g24 case (the reference's own torch warp classes on the CPU, float64 distances, float32 leaves): forward
     to 1e-9, gradients to GRAD_RTOL * max(max|ref|, 1) -- float32 atomics sum in arrival order -- and the same NaNs;
  2. the fixed-weight kinds the reference has only as numpy classes (bilinear, lanczos2/3) by the adjoint identity
     sum G * warp(x) == sum x.grad * x;
  3. an LDS-window case, an LDS-overflow (global-atomic) case and a horizon inside the output, against a float64 torch
     autograd restatement of the warp written from its formulas (`_restated_warp`), on a few output rows;
  4. the dispatcher ops; 5. the C contract (NULL maps, accumulation, rectangles refused, the no-grad path unchanged).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GRAD_RTOL = 2e-5          # test_gpu_train.py's tolerance and scale rule


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def _close(ours, ref):
    ours, ref = np.asarray(ours, np.float64), np.asarray(ref, np.float64)
    assert ours.shape == ref.shape
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(ours), nan), "NaN positions differ (%d vs %d)" % (int(np.isnan(ours).sum()), int(nan.sum()))
    if nan.all():
        return
    scale = max(float(np.max(np.abs(ref[~nan]))), 1.0)
    err = float(np.max(np.abs(ours[~nan] - ref[~nan])))
    assert err <= GRAD_RTOL * scale, "max |ours - ref| = %g > %g" % (err, GRAD_RTOL * scale)


def _classes():
    from lerf_pytorch_amd.resize_right import resize_right2d_torch as T
    return T


def _make(T, kind, S, pad_mode, dev):
    if kind == "gauss":
        return T.SteeringGaussianWarp2dTorch(support_sz=S, device=dev, pad_mode=pad_mode, max_sigma=10)
    if kind == "linear":
        return T.AmplifiedLinearWarp2dTorch(device=dev, pad_mode=pad_mode)
    if kind == "nearest":
        return T.NearestWarp2dTorch(device=dev, pad_mode=pad_mode)
    return T.BicubicWarp2dTorch(device=dev, pad_mode=pad_mode)


def _g24_leaves(torch, g4, c, g, dev):
    p, layout = str(g[c + "/src"]), str(g[c + "/layout"])
    f = g4["%s/feat" % p].astype(np.float32)
    h = (g4["%s/hq" % p].astype(np.float32) / 255.0).astype(np.float32)
    x, hy = {"b2c1": (f[:2, None], h[:, :2, None]), "b1c1": (f[:1, None], h[:, :1, None]), "b1c3": (f[None], h[:, None])}[layout]
    nh = {"gauss": 3, "linear": 1}.get(str(g[c + "/kind"]), 0)
    xl = torch.tensor(x, device=dev, requires_grad=True)
    hl = [torch.tensor(hy[k], device=dev, requires_grad=True) for k in range(nh)]
    return xl, hl


def _g24_out(g, g13, c):
    """the reference's forward output of case c: stored in g24, or (same classes, same inputs) in g13"""
    if c + "/out" in g.files:
        return g[c + "/out"]
    base = g13[str(g[c + "/out_g13"])]                                     # [2,1,oH,oW]
    if str(g[c + "/layout"]) == "b2c1":
        return base
    return np.concatenate([base[:, 0], g[c + "/out_c2"][None]])[None]     # b1c3: planes 0, 1 from g13, plane 2 stored


# ---------------------------------------------------------------------------------------------- 1. golden parity
def test_golden_forward_and_gradients(torch, golden):
    T = _classes()
    g, g4, g13 = golden("g24_warp_grads.npz"), golden("g4_warp.npz"), golden("g13_torch_warp.npz")
    dev = torch.device("cuda")
    for c in g["cases"]:
        kind, S, pad = str(g[c + "/kind"]), int(g[c + "/S"]), str(g[c + "/pad_mode"])
        xl, hl = _g24_leaves(torch, g4, c, g, dev)
        B, Cn = xl.shape[:2]
        ref = _g24_out(g, g13, c)
        oH, oW = ref.shape[2:]
        w = _make(T, kind, S, pad, dev)
        w.set_shape([B, Cn, 52, 52], torch.tensor(g[c + "/matrix"], dtype=torch.float64, device=dev), [B, Cn, oH, oW])
        out = w.warp(xl, *hl)
        assert out.dtype == torch.float64 and out.requires_grad
        np.testing.assert_allclose(out.detach().cpu().numpy(), ref, rtol=0, atol=1e-9, equal_nan=True, err_msg=c)
        (out * torch.tensor(g[c + "/Gi"] / 2.0, device=dev)).sum().backward()
        assert xl.grad.dtype == torch.float32 and tuple(xl.grad.shape) == tuple(xl.shape)
        _close(xl.grad.cpu().numpy(), g[c + "/gx"])
        for k, h in enumerate(hl):
            assert h.grad.dtype == torch.float32 and tuple(h.grad.shape) == tuple(h.shape)
            _close(h.grad.cpu().numpy(), g[c + "/gh"][k])


# ---------------------------------------------------------------------------------------------- 2. adjoint identity
def _inner_minv(out_hw, in_hw, scale=0.45, off=20.0, persp=1e-6):
    """an inverse homography that keeps the whole output inside the source frame (no vanishing weights)"""
    minv = np.array([[scale, 0.01, off], [0.008, scale, off], [persp, persp, 1.0]])
    for i in (0, out_hw[0] - 1):
        for j in (0, out_hw[1] - 1):
            X, Y, Wh = minv @ np.array([j, i, 1.0])
            assert 4 <= Y / Wh <= in_hw[0] - 4 and 4 <= X / Wh <= in_hw[1] - 4
    return minv


@pytest.mark.parametrize("name", ["bilinear", "lanczos2", "lanczos3"])
@pytest.mark.parametrize("size", ["small", "4k"])
def test_adjoint_identity_fixed_kinds(torch, name, size):
    T = _classes()
    cls = {"bilinear": T.BilinearWarp2dTorch, "lanczos2": T.Lanczos2Warp2dTorch, "lanczos3": T.Lanczos3Warp2dTorch}[name]
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(24)
    if size == "small":
        in_hw, out_hw, B, Cn = (52, 52), (60, 70), 1, 3
        minv = _inner_minv(out_hw, in_hw, scale=0.6, off=5.0, persp=1e-4)
    else:
        in_hw, out_hw, B, Cn = (1080, 1920), (2160, 3840), 1, 1
        minv = _inner_minv(out_hw, in_hw)
    M = torch.tensor(np.linalg.inv(minv), dtype=torch.float64, device=dev)
    x = torch.rand((B, Cn) + in_hw, generator=gen, device=dev).requires_grad_(True)
    G = torch.randn((B, Cn) + out_hw, generator=gen, device=dev, dtype=torch.float64)
    w = cls(device=dev)
    w.set_shape([B, Cn, in_hw[0], in_hw[1]], M, [B, Cn, out_hw[0], out_hw[1]])
    out = w.warp(x)
    assert not torch.isnan(out).any()
    lhs = float((G * out).sum())
    out.backward(G)
    rhs = float((x.grad.double() * x.detach().double()).sum())
    assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), float((G.abs() * out.abs()).sum()) * 1e-3)


# ---------------------------------------------------------------------------------------------- 3. windows vs restatement
def _pad_rows(idx, n, mode, torch):
    """image pad rule of F.pad for unpadded index idx (any integer): (index, inside-or-remapped mask)"""
    if mode == "constant":
        return idx.clamp(0, n - 1), (idx >= 0) & (idx < n)
    if mode == "replicate":
        return idx.clamp(0, n - 1), torch.ones_like(idx, dtype=torch.bool)
    if mode == "reflect":
        p = 2 * (n - 1)
        m = torch.remainder(idx, p)
        return torch.where(m < n, m, p - m), torch.ones_like(idx, dtype=torch.bool)
    return torch.remainder(idx, n), torch.ones_like(idx, dtype=torch.bool)


def _restated_warp(torch, kind, S, pad_mode, minv, pads, x, hs, rows, oW, max_sigma):
    """float64 torch autograd restatement of the Gaussian / linear warp for output rows `rows`, from the formulas:
    projection with the inverse matrix, clip to [0, in], left boundary ceil(g - S/2 - eps), pad shift, field of view
    clamped to [0, in-1] in padded coordinates, float64 distances, hyper maps replicate-padded, image by `pad_mode`.
    x: float32 [N,H,W] leaf, hs: float32 [N,H,W] leaves.  Returns float64 [N, len(rows), oW]."""
    N, H, W = x.shape
    dev = x.device
    m = [float(v) for v in np.asarray(minv).reshape(9)]
    i = torch.tensor(rows, dtype=torch.float64, device=dev)[:, None]
    j = torch.arange(oW, dtype=torch.float64, device=dev)[None, :]
    Xp = m[0] * j + m[1] * i + m[2]
    Yp = m[3] * j + m[4] * i + m[5]
    Wh = m[6] * j + m[7] * i + m[8]
    r = (Yp / Wh).clamp(0, H)
    c = (Xp / Wh).clamp(0, W)
    eps = float(np.finfo(np.float32).eps)
    prl, pcl = pads[0], pads[2]
    lr = torch.ceil(r - S / 2 - eps).long() + prl
    lc = torch.ceil(c - S / 2 - eps).long() + pcl
    gr, gc = r + prl, c + pcl
    ws, vs = [], []
    for a in range(S):
        for b in range(S):
            pr = (lr + b).clamp(0, H - 1)
            pc = (lc + a).clamp(0, W - 1)
            dx, dy = gr - pr.double(), gc - pc.double()
            sr, sc = pr - prl, pc - pcl
            rcl, ccl = sr.clamp(0, H - 1), sc.clamp(0, W - 1)
            ri, rm = _pad_rows(sr, H, pad_mode, torch)
            ci, cm = _pad_rows(sc, W, pad_mode, torch)
            v = torch.where(rm & cm, x[:, ri, ci], torch.zeros((), dtype=x.dtype, device=dev))
            if kind == "gauss":
                rho = (hs[0] * 2 - 1)[:, rcl, ccl].double()
                sx = (hs[1] * max_sigma)[:, rcl, ccl].double()
                sy = (hs[2] * max_sigma)[:, rcl, ccl].double()
                e = (sx * dx) ** 2 - 2 * rho * (sx * dx * sy * dy) + (sy * dy) ** 2
                w = torch.exp(-0.5 * e)
            else:
                al = (max_sigma * (hs[0] * 2 - 1))[:, rcl, ccl].double()

                def lin(t):
                    return (al * t + 1) * ((-1 <= t) & (t < 0)) + (1 - al * t) * ((0 <= t) & (t <= 1))
                w = torch.clamp(lin(dx), 0, None) * torch.clamp(lin(dy), 0, None)
            ws.append(w)
            vs.append(v)
    Wsum = sum(ws)
    return sum(v * (w / Wsum) for v, w in zip(vs, ws))


def _window_case(torch, name):
    if name == "mild":               # 1080p -> 4K, windows of a few hundred elements: the LDS path
        in_hw, out_hw, S = (1080, 1920), (2160, 3840), 2
        minv = _inner_minv(out_hw, in_hw)
        rows = [0, 7, 777, 1500, 2159]
    elif name == "minify":           # 8x minification at S = 4: windows of ~130 x 130 > LDS, the global-atomic path
        in_hw, out_hw, S = (1080, 1920), (135, 240), 4
        minv = np.array([[8.0, 0.02, 1.0], [0.03, 8.0, 1.5], [0.0, 0.0, 1.0]])
        rows = [0, 16, 67, 134]
    else:                            # the projection's denominator changes sign between output rows 50 and 51
        in_hw, out_hw, S = (64, 64), (100, 120), 2
        minv = np.array([[1.0, 0.1, 2.0], [0.05, 1.0, 1.0], [0.0, 0.01, -0.505]])
        rows = [0, 30, 49, 50, 51, 52, 70, 99]
    return in_hw, out_hw, S, minv, rows


@pytest.mark.parametrize("name", ["mild", "minify", "horizon"])
def test_windows_against_restatement(torch, name):
    T = _classes()
    from lerf_pytorch_amd import ops
    dev = torch.device("cuda")
    in_hw, out_hw, S, minv, rows = _window_case(torch, name)
    gen = torch.Generator(device=dev).manual_seed(7)
    x = (torch.rand((1, 1) + in_hw, generator=gen, device=dev) * 255).requires_grad_(True)
    # sigma <= 3 keeps every patch's weights away from float64 underflow (no NaN pixel anywhere in the output)
    hs = [torch.rand((1, 1) + in_hw, generator=gen, device=dev).requires_grad_(True)]
    hs += [(torch.rand((1, 1) + in_hw, generator=gen, device=dev) * 0.3).requires_grad_(True) for _ in range(2)]
    M = torch.tensor(np.linalg.inv(minv), dtype=torch.float64, device=dev)
    w = T.SteeringGaussianWarp2dTorch(support_sz=S, device=dev, max_sigma=10)
    w.set_shape([1, 1, in_hw[0], in_hw[1]], M, [1, 1, out_hw[0], out_hw[1]])
    out = w.warp(x, *hs)
    assert not torch.isnan(out).any()
    G = torch.zeros_like(out)
    G[0, 0, rows] = torch.randn((len(rows), out_hw[1]), generator=gen, device=dev, dtype=torch.float64)
    out.backward(G)
    # the restatement on the same leaves (fresh copies), the same geometry (minv and pads of the class)
    geo = ops.WarpGeometry(in_hw, M, out_hw, S)
    xr = x.detach().reshape(1, *in_hw).clone().requires_grad_(True)
    hr = [h.detach().reshape(1, *in_hw).clone().requires_grad_(True) for h in hs]
    pads = (geo.struct.pad_r_lo, geo.struct.pad_r_hi, geo.struct.pad_c_lo, geo.struct.pad_c_hi)
    ref = _restated_warp(torch, "gauss", S, "constant", geo.minv, pads, xr, hr, rows, out_hw[1], 10)
    np.testing.assert_allclose(out.detach()[0, :, rows].cpu().numpy(), ref.detach().cpu().numpy(), rtol=0, atol=1e-9)
    (ref * G[0, :, rows]).sum().backward()
    _close(x.grad[0].cpu().numpy(), xr.grad.cpu().numpy())
    for h, r in zip(hs, hr):
        _close(h.grad[0].cpu().numpy(), r.grad.cpu().numpy())


# ---------------------------------------------------------------------------------------------- 4. dispatcher ops
def test_dispatcher_ops(torch, golden):
    T = _classes()
    from lerf_pytorch_amd import torch_ops  # noqa: F401  (registers the fake kernels and the autograd formulas)
    g4 = golden("g4_warp.npz")
    dev = torch.device("cuda")
    M = torch.tensor(g4["isc/matrix"], dtype=torch.float64, device=dev)
    feat = torch.from_numpy(g4["isc/feat"][:2].astype(np.float32)).unsqueeze(1).to(dev)
    hy = torch.from_numpy(g4["isc/hq"][:, :2].astype(np.float32) / np.float32(255)).unsqueeze(2).to(dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    G = torch.randn((2, 1, 60, 70), generator=gen, device=dev, dtype=torch.float64)
    for kind in ("gauss", "linear"):
        nh = 3 if kind == "gauss" else 1
        leaves_a = [feat.clone().requires_grad_(True)] + [hy[k].clone().requires_grad_(True) for k in range(nh)]
        leaves_b = [t.detach().clone().requires_grad_(True) for t in leaves_a]
        if kind == "gauss":
            o = torch.ops.lerf.warp_gauss(*leaves_a, M, 60, 70, 2, 10.0)
            w = T.SteeringGaussianWarp2dTorch(support_sz=2, device=dev, max_sigma=10)
        else:
            o = torch.ops.lerf.warp_linear(*leaves_a, M, 60, 70, 1.0)
            w = T.AmplifiedLinearWarp2dTorch(device=dev)
        w.set_shape([2, 1, 52, 52], M, [2, 1, 60, 70])
        ref = w.warp(*leaves_b)
        assert o.dtype == torch.float64 and tuple(o.shape) == (2, 1, 60, 70)
        np.testing.assert_allclose(o.detach().cpu().numpy(), ref.detach().cpu().numpy(), rtol=0, atol=1e-9, equal_nan=True)
        o.backward(G)
        ref.backward(G)
        for a, b in zip(leaves_a, leaves_b):
            _close(a.grad.cpu().numpy(), b.grad.cpu().numpy())
        gx, g0, g1, g2 = torch.ops.lerf.warp_backward(0 if kind == "gauss" else 1, G, feat, hy[0], hy[1], hy[2], M, 60, 70, 2, 10.0 if kind == "gauss" else 1.0)
        _close(gx.cpu().numpy(), leaves_b[0].grad.cpu().numpy())
        _close(g0.cpu().numpy(), leaves_b[1].grad.cpu().numpy())
        if kind == "linear":
            assert not g1.any() and not g2.any()
    # fake kernels: shapes without running anything
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f = torch.empty((2, 1, 52, 52), device="cuda")
        o = torch.ops.lerf.warp_gauss(f, f, f, f, torch.empty((3, 3), dtype=torch.float64, device="cuda"), 60, 70, 2, 10.0)
        assert tuple(o.shape) == (2, 1, 60, 70) and o.dtype == torch.float64
    with pytest.raises((RuntimeError, NotImplementedError)):
        c = feat.cpu()
        torch.ops.lerf.warp_linear(c, c, M.cpu(), 60, 70, 1.0)


# ---------------------------------------------------------------------------------------------- 5. contract
def _bwd_setup(torch, golden):
    from lerf_pytorch_amd import ops
    g4 = golden("g4_warp.npz")
    dev = torch.device("cuda")
    feat = torch.from_numpy(g4["osc/feat"].astype(np.float32)).to(dev)                        # [3,52,52]
    hy = [torch.from_numpy(g4["osc/hq"][k].astype(np.float32) / np.float32(255)).to(dev) for k in range(3)]
    geo = ops.WarpGeometry((52, 52), g4["osc/matrix"], (60, 70), 2)
    G = torch.randn((3, 60, 70), generator=torch.Generator(device=dev).manual_seed(5), device=dev, dtype=torch.float64)
    return ops, feat, hy, geo, G


def test_null_maps_and_accumulation(torch, golden):
    ops, feat, hy, geo, G = _bwd_setup(torch, golden)
    full = [torch.zeros_like(feat) for _ in range(4)]
    ops.warp_bwd_planar(feat, hy, geo, "gauss", 10.0, G, full)
    assert all(bool(t.abs().sum() > 0) for t in full)
    part = [None, torch.zeros_like(feat), None, torch.zeros_like(feat)]
    ops.warp_bwd_planar(feat, hy, geo, "gauss", 10.0, G, part)
    _close(part[1].cpu().numpy(), full[1].cpu().numpy())
    _close(part[3].cpu().numpy(), full[3].cpu().numpy())
    only_x = [torch.zeros_like(feat)]
    ops.warp_bwd_planar(feat, [], geo, "cubic", 1.0, G, only_x)
    assert bool(only_x[0].abs().sum() > 0)
    base = [torch.full_like(feat, 3.0) for _ in range(4)]
    ops.warp_bwd_planar(feat, hy, geo, "gauss", 10.0, G, base)
    for b, f in zip(base, full):
        _close((b - 3.0).cpu().numpy(), f.cpu().numpy())


def test_errors(torch, golden):
    from lerf_pytorch_amd import _lib, ops
    _, feat, hy, geo, G = _bwd_setup(torch, golden)
    gx = torch.zeros_like(feat)
    lib = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)

    def call(g, f=feat, kind="gauss", S=None):
        if S is not None:
            g.struct.S = S
        return lib.lerf_warp_bwd(p(f), p(hy[0]), p(hy[1]), p(hy[2]), 3, 52, 52, g.ref(), _lib.KINDS[kind], 10.0, p(G), p(gx),
                                 None, None, None, _lib.current_stream())
    assert call(geo) == 0
    torch.cuda.synchronize()
    for field, val in (("out_y0", 1), ("out_x0", 2), ("src_y0", 1)):
        g2 = ops.WarpGeometry((52, 52), geo.matrix, (60, 70), 2)
        setattr(g2.struct, field, val)
        assert call(g2) == -2, field                             # LERF_EUNSUPPORTED: whole outputs only
    assert call(ops.WarpGeometry((52, 52), geo.matrix, (60, 70), 2), f=None) == -1      # LERF_EINVAL
    assert call(ops.WarpGeometry((52, 52), geo.matrix, (60, 70), 2), S=99) == -2
    assert lib.lerf_warp_bwd(p(feat), None, None, None, 3, 52, 52, geo.ref(), _lib.KINDS["gauss"], 10.0, p(G), p(gx),
                             None, None, None, _lib.current_stream()) == -1
    assert not torch.isnan(gx).any()


def test_no_grad_path_unchanged(torch, golden):
    T = _classes()
    from lerf_pytorch_amd import ops
    g4 = golden("g4_warp.npz")
    dev = torch.device("cuda")
    M = torch.tensor(g4["isc/matrix"], dtype=torch.float64, device=dev)
    feat = torch.from_numpy(g4["isc/feat"].astype(np.float32)).unsqueeze(0).to(dev)             # [1,3,52,52]
    hy = torch.from_numpy(g4["isc/hq"].astype(np.float32) / np.float32(255)).unsqueeze(1).to(dev)
    w = T.SteeringGaussianWarp2dTorch(support_sz=4, device=dev, max_sigma=10)
    w.set_shape([1, 3, 52, 52], M, [1, 3, 60, 70])
    plain = w.warp(feat, hy[0], hy[1], hy[2])
    assert not plain.requires_grad and plain.grad_fn is None
    direct = ops.warp_planar(feat.reshape(3, 52, 52), [h.reshape(3, 52, 52) for h in hy], w.geo, "gauss", 10, out="f64")
    assert torch.equal(plain.reshape(3, 60, 70), direct)
    with torch.no_grad():
        nog = w.warp(feat.requires_grad_(True), hy[0], hy[1], hy[2])
    assert nog.grad_fn is None and torch.equal(nog, plain)
    withg = w.warp(feat, hy[0], hy[1], hy[2])
    assert withg.grad_fn is not None and torch.equal(withg.detach(), plain)
