"""The model builders with device parameters and their adjoint on the device (entry_kernel<BuildDevOp> and
coords_build_bwd_{partial,sum}_kernel of csrc/lerf_coords.hip behind ops.coords_build_params / coords_build_bwd and
coords.from_homography_torch / radial_torch / undistort_rectify_torch).  The bounds are the ones tests/test_coords_build_grad_cpu.py
settles on the host twin:

  4. forward: bit-equal to ops.coords_build of the same doubles -- every model, float64 and float32 maps, one set and a batch, strided
     tile views inside NaN-filled buffers, an origin;
  5. backward: bit-equal to the host twin and from run to run, a batch equal to its single calls, within ADJ_TOL of autograd of the
     restatement; the accumulate contract; the masked non-finite entries; the refusals;
  6. the differentiable twins: the plain kernel under no_grad, gradient dtypes, the batch forms, the refusals;
  7. autograd end to end through the remap from a matrix and from camera parameters, and a short fit.

Shapes of the backward.  A block of pass 1 owns 64 columns x a band of 64 rows and leaves ONE partial vector; pass 2 gives lane l the
partials l, l + 64, ...  1 x 1: one lane; 4 x 64: one full row per wave; 5 x 65: one over in both directions (a second column tile, a
second row in wave 0); 67 x 257: a second band and a ragged fifth column tile; 130 x 520: 3 bands x 9 tiles = 27 partials, still one
round of pass 2; 453 x 520: 8 bands x 9 tiles = 72 partials, so lanes 0 .. 7 of pass 2 take a second round -- the smallest kind of
map on which the order of pass 2 beyond its first round shows.
"""
import numpy as np
import pytest

import coords_build_grad_ref as BR
import coords_ref as R
import remap_grad_ref
from test_coords_build_grad_cpu import FULL_HW, MIN_DIVISOR, MODELS, adj_close, crossing_case, upstream
from test_coords_grad_cpu import ADJ_TOL
from test_gpu_remap_grad import _close, _make, _classes, _operands

pytestmark = pytest.mark.gpu

BWD_HWS = [(1, 1), (4, 64), (5, 65), (67, 257), (130, 520), (453, 520)]
ORIGIN = (3, 7)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _scalar(torch, v, dt=None):
    return torch.tensor(float(v), dtype=torch.float64 if dt is None else dt, device="cuda")


def _sets(model, full_hw, n):
    """n parameter sets of `model`: the suite's own and gentle rescalings of it"""
    return np.stack([BR.cases(full_hw)[model] * (1.0 + 0.01 * s) for s in range(n)])


_REF = {}


def _bwd_case(model, hw):
    """(params, upstream, host twin's gradient, autograd's gradient) of one model and shape, computed once and left unchanged"""
    from lerf_pytorch_amd import _lib
    if (model, hw) not in _REF:
        full = (max(FULL_HW[0], hw[0] + ORIGIN[0]), max(FULL_HW[1], hw[1] + ORIGIN[1]))
        p, g = BR.cases(full)[model], upstream(hw)
        assert BR.denominators(model, p, hw, ORIGIN) >= MIN_DIVISOR
        _REF[(model, hw)] = (p, g, _lib.coords_build_bwd_host(model, p, g, origin=ORIGIN), BR.params_grad_ref(model, p, g, hw, ORIGIN))
    return _REF[(model, hw)]


# ---------------------------------------------------------------------------------------------- 4. forward
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dt", ["float64", "float32"])
@pytest.mark.parametrize("model", MODELS)
def test_forward_from_device_parameters_is_the_plain_kernel(torch, model, dt, B):
    from lerf_pytorch_amd import ops
    tdt = getattr(torch, dt)
    hw = (37, 131)
    ps = _sets(model, FULL_HW, B)
    want = torch.stack([ops.coords_build(model, ps[b], hw, dtype=tdt, origin=ORIGIN) for b in range(B)])
    got = ops.coords_build_params(model, _dev(torch, ps), hw, dtype=tdt, origin=ORIGIN)
    assert got.dtype == tdt and tuple(got.shape) == (B,) + hw + (2,) and torch.equal(got, want)
    one = ops.coords_build_params(model, _dev(torch, ps[B - 1]), hw, dtype=tdt, origin=ORIGIN)          # [n] -> [oH, oW, 2]
    assert tuple(one.shape) == hw + (2,) and torch.equal(one, want[B - 1])
    # strided tile views inside NaN-filled buffers: every map in place, nothing outside the views written
    buf = torch.full((B, hw[0] + 3, hw[1] + 4, 2), float("nan"), dtype=tdt, device="cuda")
    view = buf[:, 1:1 + hw[0], 2:2 + hw[1]]
    assert ops.coords_build_params(model, _dev(torch, ps), hw, out=view, origin=ORIGIN).data_ptr() == view.data_ptr()
    assert torch.equal(view, want)
    assert int(torch.isnan(buf).sum()) == buf.numel() - view.numel()
    buf1 = torch.full((hw[0] + 3, hw[1] + 4, 2), float("nan"), dtype=tdt, device="cuda")
    ops.coords_build_params(model, _dev(torch, ps[0]), hw, out=buf1[2:2 + hw[0], 1:1 + hw[1]], origin=ORIGIN)
    assert torch.equal(buf1[2:2 + hw[0], 1:1 + hw[1]], want[0]) and int(torch.isnan(buf1).sum()) == buf1.numel() - want[0].numel()


def test_forward_with_non_finite_parameters_is_not_refused(torch):
    from lerf_pytorch_amd import ops
    p = BR.cases(FULL_HW)["homography"].copy()
    p[8] = np.nan
    with pytest.raises(ValueError):
        ops.coords_build("homography", p, (4, 5))                            # the host sees them
    assert bool(torch.isnan(ops.coords_build_params("homography", _dev(torch, p), (4, 5))).all())


# ---------------------------------------------------------------------------------------------- 5. backward
@pytest.mark.parametrize("hw", BWD_HWS)
@pytest.mark.parametrize("model", MODELS)
def test_backward_is_bit_equal_to_the_host_twin_and_from_run_to_run(torch, model, hw):
    from lerf_pytorch_amd import ops
    p, g, host, ref = _bwd_case(model, hw)
    pd, gd = _dev(torch, p), _dev(torch, g)
    got = ops.coords_build_bwd(model, pd, gd, origin=ORIGIN)
    assert got.dtype == torch.float64 and tuple(got.shape) == p.shape
    again = ops.coords_build_bwd(model, pd, gd, origin=ORIGIN)
    print("%s %s: max |device - host| = %.3g" % (model, hw, float(np.max(np.abs(_np(got) - host)))))
    assert R.same_bits(_np(got), host)
    assert torch.equal(again, got)
    adj_close(_np(got), ref, "%s %s vs autograd" % (model, hw))


@pytest.mark.parametrize("model", MODELS)
def test_a_batch_of_sets_equals_the_single_calls_and_accumulates(torch, model):
    from lerf_pytorch_amd import _lib, ops
    hw, Bn = (67, 257), 3
    ps = _sets(model, (hw[0] + ORIGIN[0], hw[1] + ORIGIN[1]), Bn)
    gs = np.stack([upstream(hw, 20 + s) for s in range(Bn)])
    pd, gd = _dev(torch, ps), _dev(torch, gs)
    got = ops.coords_build_bwd(model, pd, gd, origin=ORIGIN)
    singles = torch.stack([ops.coords_build_bwd(model, pd[b], gd[b], origin=ORIGIN) for b in range(Bn)])
    assert tuple(got.shape) == ps.shape and torch.equal(got, singles)
    assert R.same_bits(_np(got), _lib.coords_build_bwd_host(model, ps, gs, origin=ORIGIN))
    # the accumulate contract: a pre-filled buffer gains the sum by ONE add per value, and is the tensor returned
    pre = np.random.default_rng(12).standard_normal(ps.shape)
    buf = _dev(torch, pre)
    assert ops.coords_build_bwd(model, pd, gd, grad_params=buf, origin=ORIGIN).data_ptr() == buf.data_ptr()
    assert R.same_bits(_np(buf), pre + _np(got)) and bool((got != 0).all())


def test_masked_entries_that_are_not_finite(torch):
    from lerf_pytorch_amd import _lib, ops
    p, hw, mask, g = crossing_case()
    F = ops.coords_build_params("homography", _dev(torch, p), hw)
    assert np.array_equal(~np.isfinite(_np(F)).all(-1), mask)
    got = _np(ops.coords_build_bwd("homography", _dev(torch, p), _dev(torch, g)))
    assert np.all(np.isfinite(got)) and R.same_bits(got, _lib.coords_build_bwd_host("homography", p, g))
    adj_close(got, BR.params_grad_ref("homography", p, g, hw, mask=mask), "masked crossing")
    only = np.where(mask[..., None], g, 0.0)
    assert not bool(ops.coords_build_bwd("homography", _dev(torch, p), _dev(torch, only)).any())
    g2 = upstream(hw, 9)
    g2[1, 3, 1] = np.nan                                                     # a NaN upstream at a finite point propagates
    got2 = _np(ops.coords_build_bwd("homography", _dev(torch, p), _dev(torch, g2)))
    assert np.all(np.isnan(got2[[0, 1, 2, 6, 7, 8]])) and np.all(np.isfinite(got2[3:6]))


def test_ops_refusals_write_nothing(torch):
    from lerf_pytorch_amd import ops
    z = lambda *s, dt=torch.float64: torch.full(s, -7.0, dtype=dt, device="cuda")
    p, g, gp, out = z(9), z(4, 5, 2), z(9), z(4, 5, 2)
    pb, gb = z(2, 9), z(2, 4, 5, 2)
    bad = [lambda: ops.coords_build_bwd("fisheye", p, g), lambda: ops.coords_build_bwd("homography", z(8), g),
           lambda: ops.coords_build_bwd("radial", p, g), lambda: ops.coords_build_bwd("homography", z(9, dt=torch.float32), g),
           lambda: ops.coords_build_bwd("homography", p.cpu(), g), lambda: ops.coords_build_bwd("homography", p, g.cpu()),
           lambda: ops.coords_build_bwd("homography", p, z(4, 5, 2, dt=torch.float32)), lambda: ops.coords_build_bwd("homography", p, z(4, 5, 3)),
           lambda: ops.coords_build_bwd("homography", p, gb), lambda: ops.coords_build_bwd("homography", pb, g),
           lambda: ops.coords_build_bwd("homography", pb, z(3, 4, 5, 2)), lambda: ops.coords_build_bwd("homography", p, z(4, 10, 2)[:, ::2]),
           lambda: ops.coords_build_bwd("homography", p, g, grad_params=z(8)), lambda: ops.coords_build_bwd("homography", p, g, grad_params=pb),
           lambda: ops.coords_build_bwd("homography", p, g, grad_params=z(9, dt=torch.float32)),
           lambda: ops.coords_build_bwd("homography", p, g, grad_params=p),                        # the gradient over its own parameters
           lambda: ops.coords_build_bwd("homography", p, g, origin=(-1, 0)), lambda: ops.coords_build_bwd("homography", np.zeros(9), g),
           lambda: ops.coords_build_params("fisheye", p, (4, 5)), lambda: ops.coords_build_params("homography", z(8), (4, 5)),
           lambda: ops.coords_build_params("homography", p.cpu(), (4, 5)), lambda: ops.coords_build_params("homography", p, (0, 5)),
           lambda: ops.coords_build_params("homography", p, (4, 5), dtype=torch.float16),
           lambda: ops.coords_build_params("homography", p, (4, 5), out=z(4, 6, 2)), lambda: ops.coords_build_params("homography", pb, (4, 5), out=out),
           lambda: ops.coords_build_params("homography", p, (4, 5), out=gb), lambda: ops.coords_build_params("homography", p, (4, 5), out=out.cpu()),
           lambda: ops.coords_build_params("homography", p, (4, 5), out=z(4, 10, 2)[:, ::2]),
           lambda: ops.coords_build_params("homography", p, (4, 5), out=out, origin=(0, -1)),
           lambda: ops.coords_build_params("homography", pb, (4, 5), out=z(1, 4, 5, 2).expand(2, 4, 5, 2))]  # two maps on the same memory
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
    assert all(bool((t == -7.0).all()) for t in (p, g, gp, out, pb, gb))


# ---------------------------------------------------------------------------------------------- 6. the differentiable twins
def _twin_operands(torch, dt=None):
    dt = torch.float64 if dt is None else dt
    t = lambda a: _dev(torch, np.asarray(a, np.float64)).to(dt)
    return t(BR.M_ISC), (t(BR.BROWN_K), t(BR.BROWN_DIST), t(BR.BROWN_R), t(BR.BROWN_NEW_K))


def test_twins_under_no_grad_are_the_plain_kernel(torch):
    from lerf_pytorch_amd import coords, ops
    hw = (37, 131)
    M, cam = _twin_operands(torch)
    lM = M.clone().requires_grad_(True)
    with torch.no_grad():
        minv = _np(torch.linalg.inv(lM.double())).reshape(9)             # the same parameter doubles
        assert torch.equal(coords.from_homography_torch(lM, hw), ops.coords_build("homography", minv, hw))
        assert torch.equal(coords.from_homography_torch(lM, hw, dtype=np.float32), ops.coords_build("homography", minv, hw, dtype=torch.float32))
        p = _np(coords.brown_params_torch(*cam))
        assert torch.equal(coords.undistort_rectify_torch(*cam, hw), ops.coords_build("brown", p, hw))
        k1, k2, c = _scalar(torch, -0.18), _scalar(torch, 0.03), _dev(torch, np.array([19.3, 30.9]))
        assert torch.equal(coords.radial_torch((40, 64), hw, k1.requires_grad_(True), k2, c), coords.radial((40, 64), hw, -0.18, 0.03, (19.3, 30.9), device="cuda"))
        assert torch.equal(coords.radial_torch((40, 64), hw, k1), coords.radial((40, 64), hw, -0.18, device="cuda"))
    # no leaf: plain, no graph; a leaf: the same bits, in the graph
    assert not coords.from_homography_torch(M, hw).requires_grad
    out = coords.from_homography_torch(lM, hw)
    assert out.requires_grad and torch.equal(out.detach(), coords.from_homography_torch(M, hw))
    # brown_params_torch restates brown_params
    want = coords.brown_params(BR.BROWN_K, BR.BROWN_DIST[:5], BR.BROWN_R, None)
    got = _np(coords.brown_params_torch(cam[0], cam[1][:5], cam[2], None))
    assert got.shape == (21,) and float(np.max(np.abs(got - want))) <= 1e-12 * float(np.max(np.abs(want)))


@pytest.mark.parametrize("dt", ["float64", "float32"])
def test_twin_gradients_and_their_dtypes(torch, dt):
    """a float32 operand's gradient is the float64 gradient rounded once: half a unit of 2^-23 of its magnitude on top of ADJ_TOL"""
    from lerf_pytorch_amd import coords
    tdt = getattr(torch, dt)
    tol = ADJ_TOL if dt == "float64" else ADJ_TOL + 2.0 ** -24
    hw = (37, 131)
    g = upstream(hw)
    gd = _dev(torch, g).to(tdt)
    gref = torch.from_numpy(_np(gd.double()))

    def close(got, ref, what):
        scale = max(float(ref.abs().max()), 1.0)
        err = float((got.detach().cpu().double() - ref).abs().max())
        print("%s %s: max error %.3g, scale %.3g, bound %.3g" % (what, dt, err, scale, tol * scale))
        assert got.dtype == tdt and tuple(got.shape) == tuple(ref.shape) and err <= tol * scale, what

    M, cam = _twin_operands(torch, tdt)
    lM = M.clone().requires_grad_(True)
    out = coords.from_homography_torch(lM, hw)
    assert out.dtype == tdt
    out.backward(gd)
    rM = M.cpu().clone().requires_grad_(True)
    (BR.model_map("homography", torch.linalg.inv(rM.double()).reshape(9), hw) * gref).sum().backward()
    close(lM.grad, rM.grad.double(), "matrix")
    # the camera operands, each a leaf
    leaves = [t.clone().requires_grad_(True) for t in cam]
    out = coords.undistort_rectify_torch(*leaves, hw)
    assert out.dtype == tdt
    out.backward(gd)
    refs = [t.cpu().clone().requires_grad_(True) for t in cam]
    (BR.model_map("brown", BR.brown_params_ref(*refs), hw) * gref).sum().backward()
    for leaf, ref, name in zip(leaves, refs, ("K", "dist", "R", "new_K")):
        close(leaf.grad, ref.grad.double(), name)
    assert not bool(leaves[0].grad[0, 1]) and not bool(leaves[0].grad[2].any())          # the entries of K the model does not read
    # radial: k1, k2 and the centre; the geometry scalars' entries are dropped
    k1, k2 = _scalar(torch, -0.18, tdt).requires_grad_(True), _scalar(torch, 0.03, tdt).requires_grad_(True)
    c = _dev(torch, np.array([19.3, 30.9])).to(tdt).requires_grad_(True)
    out = coords.radial_torch((40, 64), hw, k1, k2, c)
    assert out.dtype == tdt
    out.backward(gd)
    pr = torch.from_numpy(BR.radial_params((40, 64), hw, float(k1.detach().double()), float(k2.detach().double()),
                                           _np(c.double()))).requires_grad_(True)
    (BR.model_map("radial", pr, hw) * gref).sum().backward()
    close(k1.grad, pr.grad[6], "k1"), close(k2.grad, pr.grad[7], "k2"), close(c.grad, pr.grad[:2], "centre")


def test_batch_forms_equal_the_per_sample_calls(torch):
    from lerf_pytorch_amd import coords
    hw, Bn = (37, 131), 3
    Ms = np.stack([BR.M_ISC + s * np.array([[0.01, 0.0, 0.5], [0.0, -0.01, 0.25], [1e-6, 0.0, 0.0]]) for s in range(Bn)])
    gs = _dev(torch, np.stack([upstream(hw, 30 + s) for s in range(Bn)]))
    lM = _dev(torch, Ms).requires_grad_(True)
    out = coords.from_homography_torch(lM, hw)
    assert tuple(out.shape) == (Bn,) + hw + (2,)
    out.backward(gs)
    for b in range(Bn):
        m1 = _dev(torch, Ms[b]).requires_grad_(True)
        o1 = coords.from_homography_torch(m1, hw)
        # torch.linalg.inv of a batch may round unlike that of one matrix: the maps agree to the forward's bound, not bit for bit
        assert float((o1.detach() - out[b].detach()).abs().max()) <= 1e-9
        o1.backward(gs[b])
        adj_close(_np(lM.grad[b]), _np(m1.grad), "batch matrix %d" % b)
    # one shared K with a batch of distortions: [B, oH, oW, 2], K's gradient is the sum over the samples
    _, (K, dist, Rm, new_K) = _twin_operands(torch)
    ds = torch.stack([dist * (1.0 + 0.1 * s) for s in range(Bn)]).requires_grad_(True)
    lK = K.clone().requires_grad_(True)
    out = coords.undistort_rectify_torch(lK, ds, Rm, new_K, hw)
    assert tuple(out.shape) == (Bn,) + hw + (2,)
    out.backward(gs)
    sumK = torch.zeros_like(K)
    for b in range(Bn):
        k1, d1 = K.clone().requires_grad_(True), ds[b].detach().clone().requires_grad_(True)
        o1 = coords.undistort_rectify_torch(k1, d1, Rm, new_K, hw)
        assert torch.equal(o1.detach(), out[b].detach())
        o1.backward(gs[b])
        assert torch.equal(d1.grad, ds.grad[b])
        sumK += k1.grad
    adj_close(_np(lK.grad), _np(sumK), "shared K")
    k1s = _dev(torch, np.array([-0.18, 0.05, 0.0]))
    out = coords.radial_torch((40, 64), hw, k1s, 0.03)
    assert tuple(out.shape) == (Bn,) + hw + (2,)
    for b in range(Bn):
        assert torch.equal(out[b], coords.radial((40, 64), hw, float(k1s[b]), 0.03, device="cuda"))


def test_twin_refusals(torch):
    from lerf_pytorch_amd import coords
    M, (K, dist, Rm, new_K) = _twin_operands(torch)
    k1 = _scalar(torch, -0.18)
    bad = [lambda: coords.from_homography_torch(_np(M), (4, 5)), lambda: coords.from_homography_torch(M.cpu(), (4, 5)),
           lambda: coords.from_homography_torch(M.half(), (4, 5)), lambda: coords.from_homography_torch(M.long(), (4, 5)),
           lambda: coords.from_homography_torch(M[:2], (4, 5)), lambda: coords.from_homography_torch(M[None, None], (4, 5)),
           lambda: coords.from_homography_torch(M, (0, 5)), lambda: coords.from_homography_torch(M, (4, 5), dtype=np.float16),
           lambda: coords.radial_torch((40, 64), (4, 5), -0.18), lambda: coords.radial_torch((40, 64), (4, 5), k1.cpu()),
           lambda: coords.radial_torch((40, 64), (4, 5), k1, k1.cpu()), lambda: coords.radial_torch((40, 64), (4, 5), k1, 0.0, [19.3, 30.9]),
           lambda: coords.radial_torch((40, 64), (4, 5), k1, 0.0, _dev(torch, np.zeros(3))),
           lambda: coords.radial_torch((40, 64), (4, 5), _dev(torch, np.zeros(2)), _dev(torch, np.zeros(3))),
           lambda: coords.radial_torch((40, 64), (0, 5), k1),
           lambda: coords.undistort_rectify_torch(_np(K), dist, Rm, new_K, (4, 5)), lambda: coords.undistort_rectify_torch(K, dist.cpu(), Rm, new_K, (4, 5)),
           lambda: coords.undistort_rectify_torch(K, dist[:2], Rm, new_K, (4, 5)), lambda: coords.undistort_rectify_torch(K, dist, Rm[:2], new_K, (4, 5)),
           lambda: coords.undistort_rectify_torch(K[:, :2], dist, Rm, new_K, (4, 5)),
           lambda: coords.undistort_rectify_torch(torch.stack([K, K]), torch.stack([dist] * 3), Rm, new_K, (4, 5)),
           lambda: coords.undistort_rectify_torch(K + _dev(torch, np.array([[0, 0.1, 0], [0, 0, 0], [0, 0, 0.0]])), dist, Rm, new_K, (4, 5)),
           lambda: coords.brown_params_torch(K * 2.0)]                                               # K[2, 2] != 1
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
    # the plain builders are unchanged: host numbers in, a detached map out
    assert not coords.from_homography(M.clone().requires_grad_(True), (4, 5), device="cuda").requires_grad


# ---------------------------------------------------------------------------------------------- 7. autograd end to end
IN_HW, OUT_HW = (40, 48), (9, 11)
HOM_SEEDS, BROWN_SEED = (0, 2), 5


def hom_case(seed, dt="float64"):
    """(matrix source -> output rounded to dt, pads, ok): ok says that the map of the matrix stays > 1e-3 off every discontinuity of the
    remap -- decided on the CPU by the restatements alone"""
    import torch as t
    rng = np.random.default_rng(seed)
    minv = np.array([[3.7, 0.21, 2.13], [-0.17, 3.3, 1.77], [1e-3, -2e-3, 1.0]]) + \
        rng.normal(0, 1, (3, 3)) * np.array([[0.05, 0.05, 0.3], [0.05, 0.05, 0.3], [1e-4, 1e-4, 0]])
    M = np.linalg.inv(minv).astype(dt).astype(np.float64)
    cm = BR.model_map("homography", t.from_numpy(np.linalg.inv(M).reshape(9)), OUT_HW).numpy()
    pads = remap_grad_ref.pads_of(cm, IN_HW, 2)
    return M, pads, float(remap_grad_ref.margins("gauss", 2, cm, pads, IN_HW).min()) > 1e-3


def brown_case(seed=BROWN_SEED):
    """((K, dist, R, new_K), pads, ok) of a camera pair between the 40 x 48 source and the 9 x 11 output"""
    import torch as t
    rng = np.random.default_rng(seed)
    K = np.array([[30.0, 0, 24.3], [0, 31.0, 19.6], [0, 0, 1]]) + rng.normal(0, 0.2, (3, 3)) * np.array([[1, 0, 1], [0, 1, 1], [0, 0, 0]])
    new_K = np.array([[7.1, 0, 5.2], [0, 6.9, 4.1], [0, 0, 1.0]])
    p = BR.brown_params_np(K, BR.BROWN_DIST, BR.BROWN_R, new_K)
    cm = BR.model_map("brown", t.from_numpy(p), OUT_HW).numpy()
    pads = remap_grad_ref.pads_of(cm, IN_HW, 2)
    ok = BR.denominators("brown", p, OUT_HW) >= MIN_DIVISOR and float(remap_grad_ref.margins("gauss", 2, cm, pads, IN_HW).min()) > 1e-3
    return (K, BR.BROWN_DIST, BR.BROWN_R, new_K), pads, ok


@pytest.mark.parametrize("dt", ["float64", "float32"])
def test_autograd_from_a_matrix_through_the_map_to_the_loss(torch, dt):
    from lerf_pytorch_amd import coords
    T = _classes()
    M0, pads, ok = hom_case(HOM_SEEDS[0], dt)
    assert ok
    x, hs = _operands(torch, "gauss", planes=2)
    tdt = getattr(torch, dt)
    M = _dev(torch, M0).to(tdt).requires_grad_(True)
    cm = coords.from_homography_torch(M, OUT_HW)
    assert cm.requires_grad and cm.dtype == tdt and tuple(cm.shape) == OUT_HW + (2,)
    w = _make(T, "gauss", 2, "constant").enable_backward()
    w.set_shape([1, 2] + list(IN_HW), cm)
    loss = (w.warp(x[None], *[h[None] for h in hs]) ** 2).sum()
    loss.backward()
    assert M.grad.dtype == tdt
    Mr = M.detach().clone().requires_grad_(True)
    cr = BR.model_map("homography", torch.linalg.inv(Mr.double()).reshape(9), OUT_HW).to(tdt)
    ref = (remap_grad_ref.restated_remap("gauss", 2, "constant", cr, pads, x, hs, 10.0) ** 2).sum()
    gr, = torch.autograd.grad(ref, Mr)
    print("loss %.9g (restatement %.9g), max |grad| %.3g" % (float(loss.detach()), float(ref.detach()), float(gr.abs().max())))
    _close(_np(M.grad), _np(gr))
    assert bool((M.grad != 0).all())


def test_autograd_from_camera_parameters_through_the_map_to_the_loss(torch):
    from lerf_pytorch_amd import coords
    T = _classes()
    cam0, pads, ok = brown_case()
    assert ok
    x, hs = _operands(torch, "gauss", planes=2)
    cam = [_dev(torch, np.asarray(a, np.float64)).requires_grad_(True) for a in cam0]
    cm = coords.undistort_rectify_torch(*cam, OUT_HW)
    assert cm.requires_grad and cm.dtype == torch.float64 and tuple(cm.shape) == OUT_HW + (2,)
    w = _make(T, "gauss", 2, "constant").enable_backward()
    w.set_shape([1, 2] + list(IN_HW), cm)
    loss = (w.warp(x[None], *[h[None] for h in hs]) ** 2).sum()
    loss.backward()
    refs = [t.detach().clone().requires_grad_(True) for t in cam]
    cr = BR.model_map("brown", BR.brown_params_ref(*refs), OUT_HW)
    ref = (remap_grad_ref.restated_remap("gauss", 2, "constant", cr, pads, x, hs, 10.0) ** 2).sum()
    grs = torch.autograd.grad(ref, refs)
    print("loss %.9g (restatement %.9g)" % (float(loss.detach()), float(ref.detach())))
    for leaf, gr, name in zip(cam, grs, ("K", "dist", "R", "new_K")):
        print("%s: max |grad| %.3g" % (name, float(gr.abs().max())))
        _close(_np(leaf.grad), _np(gr))
        assert bool((leaf.grad != 0).any())


def test_autograd_from_a_batch_of_matrices_one_map_per_sample(torch):
    from lerf_pytorch_amd import coords
    T = _classes()
    cases = [hom_case(s) for s in HOM_SEEDS]
    assert all(c[2] for c in cases) and len(cases) == 2
    x, hs = _operands(torch, "gauss", planes=4)
    xb, hb = x.reshape((2, 2) + IN_HW), [h.reshape((2, 2) + IN_HW) for h in hs]
    M = _dev(torch, np.stack([c[0] for c in cases])).requires_grad_(True)
    cm = coords.from_homography_torch(M, OUT_HW)
    assert cm.requires_grad and tuple(cm.shape) == (2,) + OUT_HW + (2,)
    w = _make(T, "gauss", 2, "constant").enable_backward()
    w.set_shape([2, 2] + list(IN_HW), cm)
    loss = (w.warp(xb, *hb) ** 2).sum()
    loss.backward()
    Mr = M.detach().clone().requires_grad_(True)
    ref = 0.0
    for b in range(2):
        cr = BR.model_map("homography", torch.linalg.inv(Mr[b]).reshape(9), OUT_HW)
        ref = ref + (remap_grad_ref.restated_remap("gauss", 2, "constant", cr, cases[b][1], xb[b], [h[b] for h in hb], 10.0) ** 2).sum()
    gr, = torch.autograd.grad(ref, Mr)
    print("loss %.9g (restatement %.9g), max |grad| %.3g" % (float(loss.detach()), float(ref.detach()), float(gr.abs().max())))
    for b in range(2):
        _close(_np(M.grad[b]), _np(gr[b]))
    assert bool((M.grad != 0).all())


FIT_LR, FIT_STEPS, FIT_OUT = 1e-9, 10, (62, 66)
# M_ISC followed by a shift of the output window, so that every output pixel reads inside the 48 x 48 source (a bicubic value outside
# the field of view is NaN, and a NaN upstream at a finite point reaches every parameter)
FIT_M = np.array([[1.0, 0.0, -32.0], [0.0, 1.0, -56.0], [0.0, 0.0, 1.0]]) @ BR.M_ISC


def test_a_homography_fitted_by_gradient_steps_lowers_the_photometric_loss(torch):
    """plain gradient descent on the nine entries of a matrix perturbed from FIT_M towards the warp of FIT_M itself.  The perspective
    row's gradient is four orders of magnitude above the translation's, so the plain step is tiny; on the CPU restatement it takes
    the loss from 50.9 to 45.8 in ten steps.  Only the decrease is asserted."""
    from lerf_pytorch_amd import coords
    T = _classes()
    n = 48
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    img = (100 + 50 * np.sin(2 * np.pi * ii / 24) + 40 * np.cos(2 * np.pi * jj / 16) + 30 * np.sin(2 * np.pi * (ii + jj) / 32)).astype(np.float32)
    x = torch.from_numpy(img)[None, None].cuda()

    def forward(M):
        w = T.BicubicRemap2dTorch().enable_backward()
        w.set_shape([1, 1, n, n], coords.from_homography_torch(M, FIT_OUT))
        return w.warp(x)

    with torch.no_grad():
        target = forward(_dev(torch, FIT_M))
    assert not bool(torch.isnan(target).any())
    M = (_dev(torch, FIT_M) + _dev(torch, np.array([[0.01, 0.0, 0.8], [0.0, -0.01, -0.6], [0.0, 0.0, 0.0]]))).requires_grad_(True)
    losses = []
    for step in range(FIT_STEPS + 1):
        loss = ((forward(M) - target) ** 2).mean()
        losses.append(float(loss.detach()))
        if step == FIT_STEPS:
            break
        g, = torch.autograd.grad(loss, M)
        with torch.no_grad():
            M -= FIT_LR * g
    print("losses: " + " ".join("%.5g" % v for v in losses))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
