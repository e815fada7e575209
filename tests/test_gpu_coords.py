"""Coordinate maps on the device (csrc/lerf_coords.hip behind ops.coords_* and coords.py):

  1. forward parity: every device entry point bit-equal to its host twin on the same arguments -- the three models, both mesh
     interps, float32 / float64 on both sides, strided tiles with an origin inside sentinel-filled buffers, compose's special
     entries;
  2. the mesh adjoint: against float64 autograd of the torch restatement (tests/coords_ref.py), the inner-product identity, the
     accumulate contract, run-to-run determinism, reaches beyond one pass of a workgroup;
  3. autograd end to end: from_mesh_torch -> GaussRemap2dTorch.enable_backward() -> loss, against the chained restatements;
  4. the engine: remap through a device-built map = warp's bytes; remap through compose(identity, B) = remap through B;
  5. refusals through ops and coords.
"""
import numpy as np
import pytest

import coords_ref as R
import remap_grad_ref
from test_coords_cpu import DIST8, K0, MESHES, _ctrl, _maps, _radial_params, _rot, special_maps
from test_gpu_remap_grad import _close, _make, _classes, _operands

pytestmark = pytest.mark.gpu

HWS = [(37, 53), (70, 130), (1, 9)]       # 70 x 130: more than one block in each direction (blocks are 4 x 64), ragged edges
ADJ_TOL = 1e-9                            # DESIGN 4.8's rule for a float64 map gradient: ADJ_TOL * max(max|ref|, 1)
# The adjoint's single pass: 4 rows of a vertex row's reach per workgroup in pass 1, 64 columns of a vertex's reach per wave in
# pass 2 (csrc/lerf_coords.hip).  A 2 x 2 mesh under 70 x 130 reaches 70 rows and 130 columns per vertex: 18 and 3 passes.
ADJ_PASS_ROWS, ADJ_PASS_COLS = 4, 64


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tdt(torch, dt):
    return torch.float32 if np.dtype(dt) == np.float32 else torch.float64


def _models(hw):
    from lerf_pytorch_amd import coords
    M = np.array([[2.05, 0.12, 15.0], [-0.08, 1.95, 40.0], [1.5e-5, -1.0e-5, 1.0]])
    return [("homography", np.linalg.inv(M).reshape(9)), ("radial", _radial_params((40, 64), hw, 0.08, -0.02, (19.3, 30.9))),
            ("brown", coords.brown_params(K0, DIST8, _rot(0.02, -0.03, 0.01), K0 * np.array([[0.9], [0.9], [1.0]])))]


# ---------------------------------------------------------------------------------------------- 1. forward parity
@pytest.mark.parametrize("hw", HWS)
def test_build_is_bit_equal_to_its_host_twin(torch, hw):
    from lerf_pytorch_amd import _lib, ops
    for model, p in _models(hw):
        for dt in (np.float64, np.float32):
            host = _lib.coords_build_host(model, p, hw, dt)
            got = ops.coords_build(model, p, hw, dtype=_tdt(torch, dt))
            assert got.is_cuda and R.same_bits(got.cpu().numpy(), host), (model, dt)
    if hw[0] > 20:                                                               # a strided tile with an origin, sentinels around it
        for model, p in _models(hw):
            whole = _lib.coords_build_host(model, p, hw)
            for dt in (np.float64, np.float32):
                buf = torch.full((hw[0], hw[1] + 3, 2), -7.0, dtype=_tdt(torch, dt), device="cuda")
                ops.coords_build(model, p, (hw[0] - 9, hw[1] - 11), out=buf[5:hw[0] - 4, 7:hw[1] - 4], origin=(5, 7))
                b = buf.cpu().numpy()
                assert R.same_bits(np.ascontiguousarray(b[5:hw[0] - 4, 7:hw[1] - 4]), whole[5:hw[0] - 4, 7:hw[1] - 4].astype(dt))
                b[5:hw[0] - 4, 7:hw[1] - 4] = -7.0
                assert (b == -7.0).all()


def test_coords_builders_on_a_device_equal_their_host_forms(torch):
    from lerf_pytorch_amd import coords
    hw = (37, 53)
    M = np.array([[2.05, 0.12, 15.0], [-0.08, 1.95, 40.0], [1.5e-5, -1.0e-5, 1.0]])
    for dt in (None, np.float32):
        pairs = [(coords.from_homography(M, hw, device="cuda", dtype=dt), coords.from_homography(M, hw, dtype=dt)),
                 (coords.radial((40, 64), hw, 0.08, -0.02, centre=(19.3, 30.9), device="cuda", dtype=dt),
                  coords.radial((40, 64), hw, 0.08, -0.02, centre=(19.3, 30.9), dtype=dt)),
                 (coords.undistort_rectify(K0, DIST8, _rot(0.02, -0.03, 0.01), None, hw, device="cuda", dtype=dt),
                  coords.undistort_rectify(K0, DIST8, _rot(0.02, -0.03, 0.01), None, hw, dtype=dt)),
                 (coords.from_mesh(_ctrl((3, 5), hw), hw, "bicubic", device="cuda", dtype=dt), coords.from_mesh(_ctrl((3, 5), hw), hw, "bicubic", dtype=dt))]
        for got, host in pairs:
            assert got.is_cuda and R.same_bits(got.cpu().numpy(), host)


@pytest.mark.parametrize("interp", ["bilinear", "bicubic"])
@pytest.mark.parametrize("hw", HWS)
def test_mesh_is_bit_equal_to_its_host_twin(torch, interp, hw):
    from lerf_pytorch_amd import _lib, ops
    for ghw in MESHES + [hw if hw[0] > 1 else (2, 9)]:
        for cdt in (np.float64, np.float32):
            c = _ctrl(ghw, hw, dtype=cdt)
            for odt in (np.float64, np.float32):
                host = _lib.coords_mesh_host(c, hw, interp, odt)
                got = ops.coords_mesh(_dev(torch, c), hw, interp, dtype=_tdt(torch, odt))
                assert R.same_bits(got.cpu().numpy(), host), (ghw, cdt, odt)
    if hw[0] > 20:
        c = _ctrl((3, 5), hw)
        whole = _lib.coords_mesh_host(c, hw, interp)
        buf = torch.full((hw[0], hw[1] + 2, 2), -7.0, dtype=torch.float64, device="cuda")
        ops.coords_mesh(_dev(torch, c), (hw[0] - 9, hw[1] - 11), interp, out=buf[5:hw[0] - 4, 7:hw[1] - 4], origin=(5, 7), full_hw=hw)
        b = buf.cpu().numpy()
        assert R.same_bits(np.ascontiguousarray(b[5:hw[0] - 4, 7:hw[1] - 4]), whole[5:hw[0] - 4, 7:hw[1] - 4])
        b[5:hw[0] - 4, 7:hw[1] - 4] = -7.0
        assert (b == -7.0).all()


@pytest.mark.parametrize("b_hw", HWS)
def test_compose_is_bit_equal_to_its_host_twin(torch, b_hw):
    from lerf_pytorch_amd import _lib, ops
    a, b = _maps(a_hw=(20, 30), b_hw=b_hw)
    for adt in (np.float64, np.float32):
        for bdt in (np.float64, np.float32):
            aa, bb = a.astype(adt), b.astype(bdt)
            for odt in (np.float64, np.float32):
                host = _lib.coords_compose_host(aa, bb, odt)
                got = ops.coords_compose(_dev(torch, aa), _dev(torch, bb), dtype=_tdt(torch, odt))
                assert R.same_bits(got.cpu().numpy(), host), (adt, bdt, odt)
    # every operand a strided view, sentinels around the output
    wa = torch.full((20, 33, 2), float("nan"), dtype=torch.float64, device="cuda")
    wb = torch.full((b_hw[0], b_hw[1] + 2, 2), float("nan"), dtype=torch.float64, device="cuda")
    wo = torch.full((b_hw[0], b_hw[1] + 4, 2), -7.0, dtype=torch.float64, device="cuda")
    wa[:, :30], wb[:, 1:b_hw[1] + 1] = _dev(torch, a), _dev(torch, b)
    ops.coords_compose(wa[:, :30], wb[:, 1:b_hw[1] + 1], out=wo[:, 2:b_hw[1] + 2])
    o = wo.cpu().numpy()
    assert R.same_bits(np.ascontiguousarray(o[:, 2:b_hw[1] + 2]), _lib.coords_compose_host(a, b))
    o[:, 2:b_hw[1] + 2] = -7.0
    assert (o == -7.0).all()


def test_compose_special_entries(torch):
    from lerf_pytorch_amd import _lib, coords
    a, b, want = special_maps()
    got = coords.compose(_dev(torch, a), _dev(torch, b)).cpu().numpy()
    assert R.same_bits(got, _lib.coords_compose_host(a, b)) and R.same_bits(got, want)
    one_row = np.arange(10, dtype=np.float64).reshape(1, 5, 2)
    b1 = np.array([[[0.0, 1.5], [7.0, 4.0], [-3.0, 0.0], [np.nan, 0.0]]])
    assert R.same_bits(coords.compose(_dev(torch, one_row), _dev(torch, b1)).cpu().numpy(), _lib.coords_compose_host(one_row, b1))
    one = np.array([[[3.0, 4.0]]])
    assert R.same_bits(coords.compose(_dev(torch, one), _dev(torch, b1)).cpu().numpy(), _lib.coords_compose_host(one, b1))


# ---------------------------------------------------------------------------------------------- 2. the mesh adjoint
ADJ_CASES = [((3, 5), (37, 53)), ((7, 4), (70, 130)), ((2, 2), (70, 130)), ((37, 53), (37, 53)), ((2, 2), (1, 9)), ((3, 5), (1, 9))]


def _adjoint_ref(torch, ghw, hw, interp, G):
    c = torch.zeros(ghw + (2,), dtype=torch.float64, device="cuda", requires_grad=True)
    return torch.autograd.grad((R.mesh_torch(c, hw, interp) * G).sum(), c)[0]


@pytest.mark.parametrize("interp", ["bilinear", "bicubic"])
@pytest.mark.parametrize("ghw,hw", ADJ_CASES)
def test_mesh_adjoint(torch, interp, ghw, hw):
    """against autograd of the restatement, the inner-product identity, accumulation and determinism -- the 2 x 2 mesh under
    70 x 130 reaches past one pass of a workgroup in both passes (ADJ_PASS_ROWS, ADJ_PASS_COLS)"""
    from lerf_pytorch_amd import ops
    if ghw == (2, 2) and hw == (70, 130):
        assert hw[0] > ADJ_PASS_ROWS and hw[1] > ADJ_PASS_COLS
    gen = torch.Generator(device="cuda").manual_seed(11)
    G = torch.randn(hw + (2,), generator=gen, device="cuda", dtype=torch.float64)
    c = torch.randn(ghw + (2,), generator=gen, device="cuda", dtype=torch.float64)
    ref = _adjoint_ref(torch, ghw, hw, interp, G)
    got = ops.coords_mesh_bwd(G, ghw, interp)
    scale = max(float(ref.abs().max()), 1.0)
    err = float((got - ref).abs().max())
    print("mesh adjoint %s %s under %s: max error %.3g, scale %.3g, bound %.3g" % (interp, ghw, hw, err, scale, ADJ_TOL * scale))
    assert err <= ADJ_TOL * scale
    # <M c, G> = <c, M^T G>
    lhs, rhs = float((ops.coords_mesh(c, hw, interp) * G).sum()), float((c * got).sum())
    print("inner products: %.17g, %.17g" % (lhs, rhs))
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0)
    # two runs are bit-equal; a second call into the same buffer doubles it (x + x is exact)
    again = ops.coords_mesh_bwd(G, ghw, interp)
    assert torch.equal(got, again)
    ops.coords_mesh_bwd(G, ghw, interp, grad_ctrl=again)
    assert torch.equal(again, 2 * got)


# ---------------------------------------------------------------------------------------------- 3. autograd end to end
IN_HW, OUT_HW, FIT_SEED = (40, 48), (9, 11), {"bilinear": 5, "bicubic": 1}


def _fit_ctrl(interp):
    """a jittered 3 x 4 mesh over the frame whose upsampled map keeps every sample > 1e-3 away from a tap discontinuity (the seed
    was picked for that; the condition is checked here with the restatement alone, like the CPU anchor of the map gradient)"""
    rng = np.random.default_rng(FIT_SEED[interp])
    a, b = np.meshgrid(np.linspace(2.2, IN_HW[0] - 3.3, 3), np.linspace(1.7, IN_HW[1] - 2.9, 4), indexing="ij")
    c = np.stack([a, b], axis=-1) + rng.normal(0, 0.8, (3, 4, 2))
    cm = R.mesh(c, OUT_HW, interp)
    pads = remap_grad_ref.pads_of(cm, IN_HW, 2)
    assert float(remap_grad_ref.margins("gauss", 2, cm, pads, IN_HW).min()) > 1e-3
    return c, pads


@pytest.mark.parametrize("interp", ["bilinear", "bicubic"])
@pytest.mark.parametrize("dt", ["float64", "float32"])
def test_autograd_from_the_control_mesh_to_the_loss(torch, interp, dt):
    from lerf_pytorch_amd import coords
    T = _classes()
    c, pads = _fit_ctrl(interp)
    x, hs = _operands(torch, "gauss", planes=2)
    ctrl = _dev(torch, c).to(getattr(torch, dt)).requires_grad_(True)
    cm = coords.from_mesh_torch(ctrl, OUT_HW, interp)
    assert cm.requires_grad and cm.dtype == ctrl.dtype and tuple(cm.shape) == OUT_HW + (2,)
    w = _make(T, "gauss", 2, "constant").enable_backward()
    w.set_shape([1, 2] + list(IN_HW), cm)
    loss = (w.warp(x[None], *[h[None] for h in hs]) ** 2).sum()
    loss.backward()
    assert ctrl.grad.dtype == ctrl.dtype and tuple(ctrl.grad.shape) == (3, 4, 2)
    cr = ctrl.detach().clone().requires_grad_(True)
    ref = (remap_grad_ref.restated_remap("gauss", 2, "constant", R.mesh_torch(cr, OUT_HW, interp).to(cr.dtype), pads, x, hs, 10.0) ** 2).sum()
    gref, = torch.autograd.grad(ref, cr)
    print("loss %.9g (restatement %.9g), max |grad| %.3g" % (float(loss.detach()), float(ref.detach()), float(gref.abs().max())))
    _close(ctrl.grad.cpu().numpy(), gref.cpu().numpy())
    assert bool((ctrl.grad != 0).any())


# ---------------------------------------------------------------------------------------------- 4. the engine
def _frame(hw=(40, 56)):
    return np.random.default_rng(0).integers(0, 256, hw + (3,), dtype=np.uint8)


def test_engine_remap_through_a_device_built_map_is_the_warp(torch):
    import lerf_pytorch_amd as L
    from lerf_pytorch_amd import coords
    eng = L.LerfEngine.shipped("lerf-g")
    img = _frame()
    M = np.array([[2.05, 0.12, 1.5], [-0.08, 1.95, 4.0], [1.5e-4, -1.0e-4, 1.0]])
    hw = (80, 112)
    want = eng.warp(img, M, hw, return_mask=False)[0]
    got = eng.remap(img, coords.from_homography(M, hw, device="cuda"), return_mask=False)[0]
    assert np.array_equal(np.asarray(got), np.asarray(want))


def test_engine_remap_through_the_identity_composed_with_a_flow(torch):
    import lerf_pytorch_amd as L
    from lerf_pytorch_amd import coords
    H, W = 40, 56
    hw = (70, 90)
    ii, jj = np.meshgrid(np.arange(hw[0]), np.arange(hw[1]), indexing="ij")
    B = np.stack([1.0 + ii * (H - 3.0) / hw[0] + 0.8 * np.sin(jj / 9.0), 1.5 + jj * (W - 4.0) / hw[1] + 0.7 * np.cos(ii / 7.0)], axis=-1)
    assert B[..., 0].min() >= 0 and B[..., 0].max() <= H - 1 and B[..., 1].min() >= 0 and B[..., 1].max() <= W - 1
    ident = coords.from_flow(np.zeros((H, W, 2)))
    # the restatement alone, on the CPU first: the identity composes to B within a few roundings of the coordinates (not bit for
    # bit), far below what moves a byte except at a rounding tie
    dev_h = float(np.max(np.abs(R.compose(ident, B) - B)))
    print("restatement: max |compose(identity, B) - B| = %.3g" % dev_h)
    assert dev_h <= 64 * np.finfo(np.float64).eps * max(H, W)
    eng = L.LerfEngine.shipped("lerf-g")
    img = _frame((H, W))
    Bd = _dev(torch, B)
    Cd = coords.compose(_dev(torch, ident), Bd)
    assert float((Cd - Bd).abs().max()) <= 64 * np.finfo(np.float64).eps * max(H, W)
    one = np.asarray(eng.remap(img, Bd, return_mask=False)[0]).astype(np.int32)
    two = np.asarray(eng.remap(img, Cd, return_mask=False)[0]).astype(np.int32)
    diff = np.abs(one - two)
    print("bytes differing: %d of %d, max %d" % (int((diff != 0).sum()), diff.size, int(diff.max())))
    assert int(diff.max()) <= 1 and int((diff != 0).sum()) <= 0.001 * diff.size


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_refusals(torch):
    from lerf_pytorch_amd import coords, ops
    out = torch.full((6, 8, 2), -7.0, dtype=torch.float64, device="cuda")
    p = np.linalg.inv(np.array([[1.0, 0.1, 2.0], [0.0, 1.1, 1.0], [0.0, 0.0, 1.0]])).reshape(9)
    bad = p.copy()
    bad[3] = np.nan
    with pytest.raises(ValueError, match="lerf_coords_build"):
        ops.coords_build("homography", bad, (6, 8), out=out)
    with pytest.raises(ValueError, match="lerf_coords_build"):
        ops.coords_build("radial", p, (6, 8), out=out)                         # 9 parameters: not the model's count
    with pytest.raises(ValueError, match="lerf_coords_build"):
        ops.coords_build("homography", p, (6, 8), out=out, origin=(-1, 0))
    with pytest.raises(ValueError, match="model"):
        ops.coords_build("fisheye", p, (6, 8), out=out)
    with pytest.raises(ValueError, match="lerf_coords_mesh"):
        ops.coords_mesh(torch.zeros((1, 4, 2), dtype=torch.float64, device="cuda"), (6, 8), out=out)
    with pytest.raises(ValueError, match="lerf_coords_mesh"):
        ops.coords_mesh(torch.zeros((3, 4, 2), dtype=torch.float64, device="cuda"), (6, 8), out=out, origin=(1, 0))
    with pytest.raises(ValueError, match="interp"):
        ops.coords_mesh(torch.zeros((3, 4, 2), dtype=torch.float64, device="cuda"), (6, 8), "lanczos", out=out)
    with pytest.raises(ValueError, match="lerf_coords_mesh_bwd"):
        ops.coords_mesh_bwd(torch.zeros((6, 8, 2), dtype=torch.float32, device="cuda"), (3, 4))
    with pytest.raises(ValueError, match="lerf_coords_mesh_bwd"):
        ops.coords_mesh_bwd(torch.zeros((6, 8, 2), dtype=torch.float64, device="cuda"), (1, 4))
    with pytest.raises(ValueError, match="lerf_coords_compose"):
        ops.coords_compose(out, out, out=torch.empty((5, 8, 2), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="column stride"):
        ops.coords_compose(out[:, ::2], out)
    assert bool((out == -7.0).all())
    host, dev = np.zeros((4, 5, 2)), torch.zeros((4, 5, 2), dtype=torch.float64, device="cuda")
    for a, b in ((host, dev), (dev, host), (torch.from_numpy(host), dev)):
        with pytest.raises(ValueError, match="mixed"):
            coords.compose(a, b)
    leaf = dev.clone().requires_grad_(True)
    with pytest.raises(ValueError, match="autograd"):
        coords.compose(leaf, dev)
    with pytest.raises(ValueError, match="autograd"):
        coords.compose(dev, leaf)
    with torch.no_grad():
        assert tuple(coords.compose(leaf, dev).shape) == (4, 5, 2)
    with pytest.raises(ValueError, match="reference"):
        coords.from_homography(np.eye(3), (4, 4), arithmetic="reference", device="cuda")
    with pytest.raises(ValueError):
        coords.from_mesh_torch(torch.zeros((3, 4, 2)), (6, 8))                   # a host tensor
