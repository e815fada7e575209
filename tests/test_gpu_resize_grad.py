"""Autograd through the SR resizes for every kind and image pad mode: lerf_resize_bwd_f32 (csrc/lerf_resize_bwd.hip) behind
the *Resize2dTorch twins (`_ResizeFn`).

  1. every g25 case (the reference's own torch resize classes on the CPU: Bicubic and the bilinear / lanczos kinds on its
     base class, Gaussian and linear with the F.pad modes): forward to 5e-4, gradients to 1e-3 * max(max|ref|, 1), the
     tolerances of test_gpu_train.py's test_resizer_gradients_golden;
  2. the adjoint identity <grad_x, y> == <G, resize_f64(y)> (the output is linear in the image for fixed hyper maps) for
     every kind and pad mode through the C ABI, symmetric included, and on a frame narrower than the support's reach;
  3. hyper-map and image gradients under the non-constant pads against central differences of the float64 forward;
  4. window spills -- wrap pads at both frame edges, down-sampling windows beyond the LDS -- against a float64 torch
     autograd restatement of the resize written from its formulas (`_restated_resize`);
  5. the C contract (NULL hyper maps for the fixed kinds, argument errors, accumulation) and the no-grad path.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PADS = ("constant", "edge", "reflect", "symmetric", "wrap")
TORCH_PADS = ("constant", "replicate", "reflect", "circular")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def _classes():
    from lerf_pytorch_amd.resize_right import resize_right2d_torch as T
    return T


def _twin(T, kind, S, pad_mode):
    if kind == "gauss":
        return T.SteeringGaussianResize2dTorch(support_sz=S, device="cuda", pad_mode=pad_mode, max_sigma=10)
    if kind == "linear":
        return T.AmplifiedLinearResize2dTorch(device="cuda", pad_mode=pad_mode)
    cls = {"cubic": T.BicubicResize2dTorch, "bilinear": T.BilinearResize2dTorch, "lanczos2": T.Lanczos2Resize2dTorch,
           "lanczos3": T.Lanczos3Resize2dTorch}[kind]
    r = cls(device="cuda", pad_mode=pad_mode)
    assert r.init_support_sz == S
    return r


def _close(ours, ref, rtol, what=""):
    ours, ref = np.asarray(ours, np.float64), np.asarray(ref, np.float64)
    assert ours.shape == ref.shape
    scale = max(float(np.max(np.abs(ref))), 1.0)
    err = float(np.max(np.abs(ours - ref)))
    assert err <= rtol * scale, "%s: max |ours - ref| = %g > %g" % (what, err, rtol * scale)


# ---------------------------------------------------------------------------------------------- 1. golden parity
def test_golden_forward_and_gradients(torch, golden):
    T = _classes()
    g = golden("g25_resize_grads.npz")
    for c in g["cases"]:
        kind, S, pad = str(g[c + "/kind"]), int(g[c + "/S"]), str(g[c + "/pad_mode"])
        x = g[c + "/x"]
        B, Cn, H, W = x.shape
        r = _twin(T, kind, S, pad)
        r.set_shape([B, Cn, H, W], scale_factors=[float(s) for s in g[c + "/scale"]])
        xl = torch.tensor(x.astype(np.float32), device="cuda", requires_grad=True)
        nh = {"gauss": 3, "linear": 1}.get(kind, 0)
        hl = [torch.tensor(g[c + "/hy"][k], device="cuda", requires_grad=True) for k in range(nh)]
        out = r.resize(xl, *hl)
        assert out.grad_fn is not None, c
        assert np.max(np.abs(out.detach().cpu().numpy() - g[c + "/out"])) <= 5e-4, c
        (out * torch.tensor(g[c + "/Gi"].astype(np.float32) / 2, device="cuda")).sum().backward()
        assert xl.grad.dtype == torch.float32 and tuple(xl.grad.shape) == tuple(xl.shape)
        _close(xl.grad.cpu().numpy(), g[c + "/gx"], 1e-3, c + " gx")
        for k in range(nh):
            _close(hl[k].grad.cpu().numpy(), g[c + "/gh"][k], 1e-3, c + " gh%d" % k)


def test_gradients_in_leaf_dtype(torch):
    T = _classes()
    r = _twin(T, "cubic", 4, "reflect")
    r.set_shape([1, 2, 9, 9], scale_factors=2.0)
    x = torch.rand((1, 2, 9, 9), device="cuda", dtype=torch.float64, requires_grad=True)
    out = r.resize(x)
    assert out.dtype == torch.float32
    out.sum().backward()
    assert x.grad.dtype == torch.float64 and bool(x.grad.abs().sum() > 0)


# ---------------------------------------------------------------------------------------------- 2. adjoint identity
KIND_S = [("nearest", 1), ("cubic", 1), ("cubic", 4), ("bilinear", 2), ("lanczos2", 4), ("lanczos3", 6), ("gauss", 1),
          ("gauss", 2), ("gauss", 4), ("gauss", 6), ("linear", 2)]


def _operands(torch, kind, shape, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    nh = {"gauss": 3, "linear": 1}.get(kind, 0)
    x = torch.rand(shape, generator=gen, device="cuda") * 255
    hs = [0.1 + 0.8 * torch.rand(shape, generator=gen, device="cuda") for _ in range(nh)]
    y = torch.randn(shape, generator=gen, device="cuda")
    return gen, x, hs, y


def _adjoint(torch, kind, S, pad, shape, scale, seed):
    from lerf_pytorch_amd import _lib, ops
    N, H, W = shape
    geo = ops.SrGeometry((H, W), [scale, scale], None, S, arithmetic="torch32", pad_mode=_lib.PAD_MODES[pad])
    gen, x, hs, y = _operands(torch, kind, shape, seed)
    ms = 10.0 if kind == "gauss" else 1.0
    G = torch.randn((N,) + geo.out_hw, generator=gen, device="cuda")
    gx = torch.zeros_like(x)
    ops.resize_bwd_planar(x, hs, geo, kind, ms, G, [gx])
    ry = ops.resize_planar(y, hs, geo, kind, ms, out="f64")
    lhs = float((gx.double() * y.double()).sum())
    rhs = float((G.double() * ry).sum())
    scale_ = float((G.double().abs() * ops.resize_planar(y.abs(), hs, geo, kind, ms, out="f64").abs()).sum())
    assert abs(lhs - rhs) <= 1e-5 * scale_, (kind, S, pad, shape, lhs, rhs)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("kind,S", KIND_S)
def test_adjoint_identity(torch, kind, S, pad):
    _adjoint(torch, kind, S, pad, (2, 13, 11), 2.5, 31 + S)
    _adjoint(torch, kind, S, pad, (1, 40, 150), 2.0, 37 + S)         # several blocks per axis


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("kind,S", [("cubic", 4), ("lanczos3", 6), ("gauss", 6), ("linear", 2)])
def test_adjoint_identity_narrow_frame(torch, kind, S, pad):
    """a 3 x 2 frame: reflect / symmetric / wrap fold the support's reach more than once (F.pad refuses such frames)"""
    _adjoint(torch, kind, S, pad, (2, 3, 2), 3.0, 41)
    _adjoint(torch, kind, S, pad, (1, 1, 5), 2.0, 43)


# ---------------------------------------------------------------------------------------------- 3. finite differences
@pytest.mark.parametrize("kind,S,pad", [("gauss", 2, "reflect"), ("gauss", 4, "wrap"), ("gauss", 2, "edge"),
                                        ("linear", 2, "wrap"), ("linear", 2, "reflect")])
def test_finite_differences_non_constant_pads(torch, kind, S, pad):
    from lerf_pytorch_amd import _lib, ops
    from lerf_pytorch_amd.resize_right.resize_right2d_torch import _ResizeFn
    rng = np.random.default_rng(S + len(pad))
    N, H, W = 2, 9, 7
    geo = ops.SrGeometry((H, W), [2.0, 2.0], None, S, arithmetic="torch32", pad_mode=_lib.PAD_MODES[pad])
    x = rng.integers(0, 256, (N, H, W)).astype(np.float32)
    nh = 3 if kind == "gauss" else 1
    hy = (0.2 + 0.6 * rng.random((nh, N, H, W))).astype(np.float32)
    G = rng.standard_normal((N,) + geo.out_hw).astype(np.float32)
    ms = 10.0 if kind == "gauss" else 1.0

    def f64(xv, hv):
        o = ops.resize_planar(torch.tensor(xv, device="cuda"), [torch.tensor(h, device="cuda") for h in hv], geo, kind, ms, out="f64")
        return float((o * torch.tensor(G, device="cuda").double()).sum())

    xt = torch.tensor(x, device="cuda", requires_grad=True)
    ht = [torch.tensor(hy[k], device="cuda", requires_grad=True) for k in range(nh)]
    (_ResizeFn.apply(geo, kind, ms, xt, *ht) * torch.tensor(G, device="cuda")).sum().backward()
    eps = 1e-3
    # frame-edge pixels first: the ones a non-constant pad reaches
    points = [(0, 0, 0), (1, H - 1, W - 1), (0, 0, W - 1), (1, H - 1, 0), (0, 1, 0), (1, 0, 1)]
    points += [tuple(int(v) for v in (rng.integers(0, N), rng.integers(0, H), rng.integers(0, W))) for _ in range(6)]
    for n, y, xx in points:
        for k in range(nh):
            hp, hm = hy.copy(), hy.copy()
            hp[k, n, y, xx] += eps
            hm[k, n, y, xx] -= eps
            fd = (f64(x, hp) - f64(x, hm)) / (2 * eps)
            an = float(ht[k].grad[n, y, xx])
            assert abs(fd - an) <= 2e-2 * max(1.0, abs(fd)), (kind, pad, k, (n, y, xx), fd, an)
        xp, xm = x.copy(), x.copy()
        xp[n, y, xx] += 1.0
        xm[n, y, xx] -= 1.0
        fd = (f64(xp, hy) - f64(xm, hy)) / 2.0
        assert abs(fd - float(xt.grad[n, y, xx])) <= 1e-3 * max(1.0, abs(fd)), (kind, pad, (n, y, xx))


# ---------------------------------------------------------------------------------------------- 4. windows vs restatement
def _pad_np(idx, n, mode):
    """numpy.pad's rule for unpadded indices idx: (source index, has-a-pixel mask)"""
    if mode == "constant":
        return np.clip(idx, 0, n - 1), (idx >= 0) & (idx < n)
    ok = np.ones(idx.shape, bool)
    if mode == "edge":
        return np.clip(idx, 0, n - 1), ok
    if mode == "reflect":
        p = 2 * (n - 1)
        if p == 0:
            return np.zeros_like(idx), ok
        m = np.mod(idx, p)
        return np.where(m < n, m, p - m), ok
    if mode == "symmetric":
        m = np.mod(idx, 2 * n)
        return np.where(m < n, m, 2 * n - 1 - m), ok
    return np.mod(idx, n), ok


def _kernel_1d(torch, kind, d):
    a = d.abs()
    if kind == "cubic":
        return (1.5 * a ** 3 - 2.5 * a ** 2 + 1) * (a <= 1) + (-0.5 * a ** 3 + 2.5 * a ** 2 - 4 * a + 2) * ((1 < a) & (a <= 2))
    if kind in ("lanczos2", "lanczos3"):
        L = 2 if kind == "lanczos2" else 3
        eps = float(np.finfo(np.float32).eps)
        return ((torch.sin(np.pi * d) * torch.sin(np.pi * d / L) + eps) / (np.pi ** 2 * d * d / L + eps)) * (a < L)
    if kind == "bilinear":
        return (d + 1) * ((-1 <= d) & (d < 0)) + (1 - d) * ((0 <= d) & (d <= 1))
    return (((-1 <= d) & (d < 0)) | ((0 <= d) & (d <= 1))).double()


def _restated_resize(torch, kind, S, pad, geo, x, hs, ms):
    """float64 torch autograd restatement of the SR resize from its formulas: float32 distance tables of `geo`, taps at
    left + k (unpadded), hyper maps read at the clamped tap (replicate), the image under `pad` (numpy names).
    x, hs: float32 [N,H,W] leaves.  Returns float64 [N, oH, oW]."""
    N, H, W = x.shape
    h = geo.host
    dev = x.device
    ws, vs = [], []
    for a in range(S):
        for b in range(S):
            rows, cols = h["left_r"].astype(np.int64) + b, h["left_c"].astype(np.int64) + a
            ri, rm = _pad_np(rows, H, pad)
            ci, cm = _pad_np(cols, W, pad)
            rcl, ccl = np.clip(rows, 0, H - 1), np.clip(cols, 0, W - 1)
            dx = torch.tensor(h["dis_r32"][:, b].astype(np.float64), device=dev)[:, None]
            dy = torch.tensor(h["dis_c32"][:, a].astype(np.float64), device=dev)[None, :]
            mask = torch.tensor(rm[:, None] & cm[None, :], device=dev)
            v = torch.where(mask, x[:, ri][:, :, ci].double(), torch.zeros((), dtype=torch.float64, device=dev))
            at = lambda t: t[:, rcl][:, :, ccl].double()
            if kind == "gauss":
                rho, sx, sy = at(hs[0] * 2 - 1), at(hs[1] * ms), at(hs[2] * ms)
                w = torch.exp(-0.5 * ((sx * dx) ** 2 - 2 * rho * (sx * dx * sy * dy) + (sy * dy) ** 2))
            elif kind == "linear":
                al = at(ms * (hs[0] * 2 - 1))

                def lin(t):
                    return (al * t + 1) * ((-1 <= t) & (t < 0)) + (1 - al * t) * ((0 <= t) & (t <= 1))
                w = torch.clamp(lin(dx), 0, None) * torch.clamp(lin(dy), 0, None)
            else:
                w = (_kernel_1d(torch, kind, dx) * _kernel_1d(torch, kind, dy)).expand(N, -1, -1)
            ws.append(w)
            vs.append(v)
    if S == 1 and kind not in ("gauss", "linear"):
        return vs[0] * ws[0]
    Wsum = sum(ws)
    return sum(v * (w / Wsum) for v, w in zip(vs, ws))


@pytest.mark.parametrize("case", ["wrap_edges_cubic", "wrap_edges_lanczos3", "wrap_edges_gauss", "reflect_edges_linear",
                                  "down2_gauss", "down2_cubic", "down4_cubic", "down4_gauss_wrap"])
def test_windows_against_restatement(torch, case):
    """wrap sends the edge blocks' taps to the far side of the frame (outside the LDS window: global atomics); a 0.5x
    down-sampling overflows the four-map window of the Gaussian kernel (global path) but fits the fixed kinds' larger one;
    0.25x overflows both"""
    from lerf_pytorch_amd import _lib, ops
    kind_S = {"cubic": 4, "lanczos3": 6, "gauss": 4, "linear": 2}
    if case.startswith(("wrap", "reflect")):
        pad, _, kind = case.split("_")
        shape, scale = (2, 40, 150), 2.0
    else:
        parts = case.split("_")
        kind, pad = parts[1], (parts[2] if len(parts) > 2 else "reflect")
        shape, scale = (1, 300, 300), {"down2": 0.5, "down4": 0.25}[parts[0]]
    S = kind_S[kind]
    N, H, W = shape
    geo = ops.SrGeometry((H, W), [scale, scale], None, S, arithmetic="torch32", pad_mode=_lib.PAD_MODES[pad])
    assert geo.pad_vec[1] == geo.pad_vec[2]
    gen, x, hs, _ = _operands(torch, kind, shape, 53)
    ms = 10.0 if kind == "gauss" else 1.0
    if kind == "gauss":
        hs[1], hs[2] = hs[1] * 0.3, hs[2] * 0.3          # sigma <= 3: no patch's weights underflow
    G = torch.randn((N,) + geo.out_hw, generator=gen, device="cuda")
    grads = [torch.zeros_like(x) for _ in range(1 + len(hs))]
    ops.resize_bwd_planar(x, hs, geo, kind, ms, G, grads)
    xr = x.clone().requires_grad_(True)
    hr = [h.clone().requires_grad_(True) for h in hs]
    ref = _restated_resize(torch, kind, S, pad, geo, xr, hr, ms)
    f32 = ops.resize_planar(x, hs, geo, kind, ms, out="f32")
    _close(f32.cpu().numpy(), ref.detach().cpu().numpy(), 1e-5, case + " forward")
    (ref * G.double()).sum().backward()
    _close(grads[0].cpu().numpy(), xr.grad.cpu().numpy(), 1e-5, case + " gx")
    for k, t in enumerate(hr):
        _close(grads[1 + k].cpu().numpy(), t.grad.cpu().numpy(), 2e-4, case + " gh%d" % k)


# ---------------------------------------------------------------------------------------------- 5. contract
def _call(torch, lib, geo, kind, x, hs, G, grads, ms=1.0):
    from lerf_pytorch_amd import _lib
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)
    hs = list(hs) + [None] * (3 - len(hs))
    grads = list(grads) + [None] * (4 - len(grads))
    return lib.lerf_resize_bwd_f32(p(x), p(hs[0]), p(hs[1]), p(hs[2]), x.shape[0], x.shape[1], x.shape[2], geo.ref(),
                                   _lib.KINDS[kind], ms, p(G), p(grads[0]), p(grads[1]), p(grads[2]), p(grads[3]),
                                   _lib.current_stream())


def test_c_contract(torch):
    from lerf_pytorch_amd import _lib, ops
    lib = _lib.lib()
    N, H, W = 2, 12, 10
    geo = ops.SrGeometry((H, W), [2.0, 2.0], None, 4, arithmetic="torch32", pad_mode=_lib.PAD_MODES["reflect"])
    gen, x, hs, _ = _operands(torch, "gauss", (N, H, W), 61)
    G = torch.randn((N,) + geo.out_hw, generator=gen, device="cuda")
    # fixed kinds: NULL hyper maps and hyper gradients
    for kind in ("nearest", "cubic", "bilinear", "lanczos2", "lanczos3"):
        gx = torch.zeros_like(x)
        assert _call(torch, lib, geo, kind, x, [], G, [gx]) == 0, kind
        torch.cuda.synchronize()
        assert bool(gx.abs().sum() > 0), kind
        # accumulation: a second call adds the same gradient
        one = gx.clone()
        assert _call(torch, lib, geo, kind, x, [], G, [gx]) == 0
        torch.cuda.synchronize()
        _close(gx.cpu().numpy(), 2 * one.cpu().numpy(), 1e-6, kind + " accumulate")
        assert _call(torch, lib, geo, kind, x, [], G, [None]) == 0            # nothing requested
    # GAUSS still needs all three maps, LINEAR its one
    gx = torch.zeros_like(x)
    assert _call(torch, lib, geo, "gauss", x, hs[:1], G, [gx]) == -1
    assert _call(torch, lib, geo, "gauss", x, [hs[0], hs[1]], G, [gx]) == -1
    assert _call(torch, lib, geo, "linear", x, [], G, [gx]) == -1
    assert not bool(gx.any())
    # gauss / linear accumulate too (max_sigma 1 for linear: larger slopes can zero a whole patch, a NaN pixel)
    for kind, nh, ms in (("gauss", 3, 10.0), ("linear", 1, 1.0)):
        g1 = [torch.zeros_like(x) for _ in range(1 + nh)]
        assert _call(torch, lib, geo, kind, x, hs[:nh], G, g1, ms) == 0
        g2 = [t.clone() for t in g1]
        assert _call(torch, lib, geo, kind, x, hs[:nh], G, g2, ms) == 0
        torch.cuda.synchronize()
        for a, b in zip(g1, g2):
            _close(b.cpu().numpy(), 2 * a.cpu().numpy(), 1e-5, kind + " accumulate")
    # pad_mode outside LERF_PAD_CONSTANT..LERF_PAD_WRAP, unknown kind
    for bad in (-1, 5):
        geo.struct.pad_mode = bad
        assert _call(torch, lib, geo, "cubic", x, [], G, [gx]) == -1, bad
        assert _call(torch, lib, geo, "gauss", x, hs, G, [gx], 10.0) == -1, bad
    geo.struct.pad_mode = _lib.PAD_MODES["reflect"]
    assert lib.lerf_resize_bwd_f32(C.c_void_p(x.data_ptr()), None, None, None, N, H, W, geo.ref(), 7, 1.0, C.c_void_p(G.data_ptr()),
                                   C.c_void_p(gx.data_ptr()), None, None, None, _lib.current_stream()) == -2
    torch.cuda.synchronize()
    assert not bool(gx.any())


@pytest.mark.parametrize("pad", TORCH_PADS)
def test_no_grad_path_unchanged(torch, pad):
    T = _classes()
    from lerf_pytorch_amd import ops
    B, Cn, H, W = 1, 3, 11, 13
    gen = torch.Generator(device="cuda").manual_seed(71)
    x = torch.rand((B, Cn, H, W), generator=gen, device="cuda") * 255
    hy = [0.1 + 0.8 * torch.rand((B, Cn, H, W), generator=gen, device="cuda") for _ in range(3)]
    for kind, S in (("cubic", 4), ("bilinear", 2), ("lanczos2", 4), ("lanczos3", 6), ("gauss", 4), ("linear", 2)):
        r = _twin(T, kind, S, pad)
        r.set_shape([B, Cn, H, W], scale_factors=2.0)
        nh = {"gauss": 3, "linear": 1}.get(kind, 0)
        plain = r.resize(x, *hy[:nh])
        assert not plain.requires_grad and plain.grad_fn is None
        ms = {"gauss": 10, "linear": 1}.get(kind, 1.0)
        direct = ops.resize_planar(x.reshape(Cn, H, W), [h.reshape(Cn, H, W) for h in hy[:nh]], r.geo, kind, ms, out="f32")
        assert torch.equal(plain.reshape(direct.shape), direct), (kind, pad)
        xg = x.clone().requires_grad_(True)
        with torch.no_grad():
            nog = r.resize(xg, *hy[:nh])
        assert nog.grad_fn is None and torch.equal(nog, plain)
        withg = r.resize(xg, *hy[:nh])
        assert withg.grad_fn is not None and torch.equal(withg.detach(), plain), (kind, pad)
