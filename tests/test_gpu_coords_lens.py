"""The fisheye and equirectangular map models on the device (entry_kernel<BuildOp>, entry_kernel<BuildDevOp>, coords_build_bwd_partial_kernel
of csrc/lerf_coords.hip instantiated for the model codes 16 and 17, and coords_math_kernel) behind ops.coords_build / coords_build_params
/ coords_build_bwd / coords_math and coords.fisheye_undistort_rectify[_torch] / equirect_view[_torch].  The bounds are the ones
tests/test_coords_lens_cpu.py settles on the host twins:

  5. the helpers: ops.coords_math equals the host twin BIT FOR BIT on the whole sweep -- the claim the two models rest on;
  6. forward: bit-equal to the host twin -- float64 and float32, a strided tile with an origin inside a NaN-filled buffer, host and
     device parameters, one set and a batch;
  7. backward: bit-equal to the host twin and from run to run on the build-gradient suite's shapes (one lane up to a second round of pass
     2), a batch equal to its single calls, within ADJ_TOL of autograd of the restatement; the selects;
  8. the differentiable twins: the plain kernel under no_grad, gradient dtypes, the batch forms, the refusals;
  9. end to end through LerfEngine.remap, and a short fit of k1, k2.
"""
import numpy as np
import pytest

import coords_lens_ref as LR
import coords_ref as R
from test_coords_build_grad_cpu import adj_close, upstream
from test_coords_grad_cpu import ADJ_TOL
from test_coords_lens_cpu import BEHIND, FISH_EXACT, MODELS, ORIGIN, POLE_EXACT, assert_smooth, lens_case, math_sweep
from test_gpu_remap_grad import _classes

pytestmark = pytest.mark.gpu

BWD_HWS = [(1, 1), (4, 64), (5, 65), (67, 257), (130, 520), (453, 520)]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _sets(model, hw, n):
    return np.stack([lens_case(model, hw)[0] * (1.0 + 0.01 * s) for s in range(n)])


_REF = {}


def _bwd_case(model, hw):
    """(params, upstream, host twin's gradient, autograd's gradient) of one model and shape, computed once and left unchanged"""
    from lerf_pytorch_amd import _lib
    if (model, hw) not in _REF:
        p, _ = lens_case(model, hw)
        assert_smooth(model, p, hw, ORIGIN)
        g = upstream(hw)
        _REF[(model, hw)] = (p, g, _lib.coords_build_bwd_host(model, p, g, origin=ORIGIN), LR.params_grad_ref(model, p, g, hw, ORIGIN))
    return _REF[(model, hw)]


# ---------------------------------------------------------------------------------------------- 5. the helpers
def test_helpers_on_the_device_equal_the_host_twin_bit_for_bit(torch):
    from lerf_pytorch_amd import _lib, ops
    s, a, y, x = math_sweep()
    special = np.array([0.0, -0.0, 4.0, 5e-324, 1e-310, 2.2250738585072014e-308, 1.7976931348623157e308, np.inf, -1.0, -np.inf, np.nan, 1e-300])
    for op, args in (("sqrt", (np.concatenate([s, special]),)), ("atan", (np.concatenate([a, special, -special]),)), ("atan2", (y, x)),
                     ("atan2", (np.repeat(special, special.size), np.tile(special, special.size)))):
        got = _np(ops.coords_math(op, *[_dev(torch, v) for v in args]))
        want = _lib.coords_math_host(op, *args)
        diff = int((R.bits(got) != R.bits(want)).sum())
        print("%s: %d arguments, %d differ in their bits" % (op, got.size, diff))
        assert got.shape == want.shape and diff == 0
    t = _dev(torch, s[:10])
    bad = [lambda: ops.coords_math("sin", t), lambda: ops.coords_math("atan2", t), lambda: ops.coords_math("atan2", t, t[:5]),
           lambda: ops.coords_math("sqrt", t.float()), lambda: ops.coords_math("sqrt", t.cpu()), lambda: ops.coords_math("atan2", t, t.cpu()),
           lambda: ops.coords_math("sqrt", s[:10])]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    assert tuple(ops.coords_math("sqrt", t[:0]).shape) == (0,)              # nothing to do, nothing launched


# ---------------------------------------------------------------------------------------------- 6. forward
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dt", ["float64", "float32"])
@pytest.mark.parametrize("model", MODELS)
def test_forward_is_bit_equal_to_the_host_twin(torch, model, dt, B):
    from lerf_pytorch_amd import _lib, ops
    tdt, ndt = getattr(torch, dt), np.dtype(dt)
    hw = (37, 131)
    ps = _sets(model, hw, B)
    if model == "fisheye":
        ps[B - 1] = np.concatenate([BEHIND[:9], ps[B - 1][9:]])              # one set with rays behind the camera: NaN entries
    want = np.stack([_lib.coords_build_host(model, ps[b], hw, dtype=ndt, origin=ORIGIN) for b in range(B)])
    assert np.isnan(want).any() == (model == "fisheye")
    for b in range(B):                                                       # host parameters: lerf_coords_build, a strided tile in place
        buf = torch.full((hw[0] + 3, hw[1] + 4, 2), float("nan"), dtype=tdt, device="cuda")
        view = buf[2:2 + hw[0], 1:1 + hw[1]]
        assert ops.coords_build(model, ps[b], hw, out=view, origin=ORIGIN).data_ptr() == view.data_ptr()
        assert R.same_bits(_np(view), want[b])
        assert int(torch.isnan(buf).sum()) == buf.numel() - view.numel() + int(np.isnan(want[b]).sum())
        assert R.same_bits(_np(ops.coords_build(model, ps[b], hw, dtype=tdt, origin=ORIGIN)), want[b])
    got = ops.coords_build_params(model, _dev(torch, ps), hw, dtype=tdt, origin=ORIGIN)      # device parameters: lerf_coords_build_dev
    assert got.dtype == tdt and tuple(got.shape) == (B,) + hw + (2,) and R.same_bits(_np(got), want)
    one = ops.coords_build_params(model, _dev(torch, ps[B - 1]), hw, dtype=tdt, origin=ORIGIN)
    assert tuple(one.shape) == hw + (2,) and R.same_bits(_np(one), want[B - 1])
    buf = torch.full((B, hw[0] + 3, hw[1] + 4, 2), float("nan"), dtype=tdt, device="cuda")
    view = buf[:, 1:1 + hw[0], 2:2 + hw[1]]
    ops.coords_build_params(model, _dev(torch, ps), hw, out=view, origin=ORIGIN)
    assert R.same_bits(_np(view), want) and int(torch.isnan(buf).sum()) == buf.numel() - view.numel() + int(np.isnan(want).sum())


@pytest.mark.parametrize("model", MODELS)
def test_the_builders_with_a_device_are_the_host_builders(torch, model):
    from lerf_pytorch_amd import coords
    hw = (37, 53)
    for dt in (None, np.float32):
        if model == "fisheye":
            args = (LR.FISH_K, LR.FISH_DIST, LR.FISH_R, LR.FISH_NEW_K, hw)
            host, dev = coords.fisheye_undistort_rectify(*args, dtype=dt), coords.fisheye_undistort_rectify(*args, device="cuda", dtype=dt)
        else:
            args = (LR.PANO_HW, LR.VIEW_K, LR.VIEW_R, hw)
            host, dev = coords.equirect_view(*args, dtype=dt), coords.equirect_view(*args, device="cuda", dtype=dt)
        assert dev.is_cuda and R.same_bits(_np(dev), host) and host.dtype == (np.float64 if dt is None else np.float32)


# ---------------------------------------------------------------------------------------------- 7. backward
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
    ps = _sets(model, hw, Bn)
    gs = np.stack([upstream(hw, 20 + s) for s in range(Bn)])
    pd, gd = _dev(torch, ps), _dev(torch, gs)
    got = ops.coords_build_bwd(model, pd, gd, origin=ORIGIN)
    singles = torch.stack([ops.coords_build_bwd(model, pd[b], gd[b], origin=ORIGIN) for b in range(Bn)])
    assert tuple(got.shape) == ps.shape and torch.equal(got, singles)
    assert R.same_bits(_np(got), _lib.coords_build_bwd_host(model, ps, gs, origin=ORIGIN))
    pre = np.random.default_rng(12).standard_normal(ps.shape)
    buf = _dev(torch, pre)
    assert ops.coords_build_bwd(model, pd, gd, grad_params=buf, origin=ORIGIN).data_ptr() == buf.data_ptr()
    assert R.same_bits(_np(buf), pre + _np(got)) and bool((got != 0).all())


def test_the_selects_on_the_device(torch):
    """the principal ray, a pole, rays behind the camera with NaN upstream there: the host twin's bits (what they mean: the CPU suite)"""
    from lerf_pytorch_amd import _lib, ops
    for model, p, hw in (("fisheye", FISH_EXACT, (37, 53)), ("equirect", POLE_EXACT, (37, 53)), ("fisheye", BEHIND, (6, 17))):
        g = upstream(hw, 9)
        if p is BEHIND:
            g[2, 8, 0], g[3, 12, 1], g[0, 16, 0] = np.nan, np.inf, np.nan
        got = _np(ops.coords_build_bwd(model, _dev(torch, p), _dev(torch, g)))
        assert np.all(np.isfinite(got)) and R.same_bits(got, _lib.coords_build_bwd_host(model, p, g))
    mask = np.zeros((6, 17), bool)
    mask[:, 8:] = True
    only = np.where(mask[..., None], g, 0.0)
    assert not bool(ops.coords_build_bwd("fisheye", _dev(torch, BEHIND), _dev(torch, only)).any())


def test_ops_refusals_write_nothing(torch):
    from lerf_pytorch_amd import ops
    z = lambda *s, dt=torch.float64: torch.full(s, -7.0, dtype=dt, device="cuda")
    g, out = z(4, 5, 2), z(4, 5, 2)
    bad = [lambda: ops.coords_build_bwd("fisheye", z(9), g), lambda: ops.coords_build_bwd("fisheye", z(13), g), lambda: ops.coords_build_bwd("fisheye", z(21), g),
           lambda: ops.coords_build_bwd("equirect", z(17), g), lambda: ops.coords_build_params("fisheye", z(13), (4, 5)),
           lambda: ops.coords_build_params("equirect", z(17), (4, 5)), lambda: ops.coords_build_params("fisheye", z(17, dt=torch.float32), (4, 5)),
           lambda: ops.coords_build("fisheye", np.zeros(13), (4, 5), out=out), lambda: ops.coords_build("equirect", np.zeros(17), (4, 5), out=out),
           lambda: ops.coords_build("fisheye", np.full(17, np.nan), (4, 5), out=out)]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    assert bool((g == -7.0).all()) and bool((out == -7.0).all())


# ---------------------------------------------------------------------------------------------- 8. the differentiable twins
def _cams(torch, dt=None):
    dt = torch.float64 if dt is None else dt
    t = lambda a: _dev(torch, np.asarray(a, np.float64)).to(dt)
    return (t(LR.FISH_K), t(LR.FISH_DIST), t(LR.FISH_R), t(LR.FISH_NEW_K)), (t(LR.VIEW_K), t(LR.VIEW_R))


def test_twins_under_no_grad_are_the_plain_kernel(torch):
    from lerf_pytorch_amd import coords, ops
    hw = (37, 131)
    fish, view = _cams(torch)
    leaves = [t.clone().requires_grad_(True) for t in fish]
    with torch.no_grad():
        p = _np(coords.fisheye_params_torch(*leaves))
        assert p.shape == (17,) and torch.equal(coords.fisheye_undistort_rectify_torch(*leaves, hw), ops.coords_build("fisheye", p, hw))
        assert torch.equal(coords.fisheye_undistort_rectify_torch(*leaves, hw, dtype=np.float32), ops.coords_build("fisheye", p, hw, dtype=torch.float32))
        pe = np.concatenate([_np(torch.linalg.inv(view[0] @ view[1])).reshape(9), LR.pano_scalars(LR.PANO_HW)])
        assert torch.equal(coords.equirect_view_torch(LR.PANO_HW, view[0].clone().requires_grad_(True), view[1], hw), ops.coords_build("equirect", pe, hw))
    assert not coords.fisheye_undistort_rectify_torch(*fish, hw).requires_grad and not coords.equirect_view_torch(LR.PANO_HW, *view, hw).requires_grad
    out = coords.fisheye_undistort_rectify_torch(*leaves, hw)
    assert out.requires_grad and torch.equal(out.detach(), coords.fisheye_undistort_rectify_torch(*fish, hw))
    # the torch assemblies restate the host ones
    want = coords.fisheye_params(LR.FISH_K, LR.FISH_DIST, LR.FISH_R, None)
    got = _np(coords.fisheye_params_torch(fish[0], fish[1], fish[2], None))
    assert float(np.max(np.abs(got - want))) <= 1e-12 * float(np.max(np.abs(want)))
    assert not bool(coords.fisheye_params_torch(fish[0])[13:].any())
    want = coords.equirect_view(LR.PANO_HW, LR.VIEW_K, None, hw)
    assert float((coords.equirect_view_torch(LR.PANO_HW, view[0], None, hw).cpu() - torch.from_numpy(want)).abs().max()) <= 1e-9


@pytest.mark.parametrize("dt", ["float64", "float32"])
def test_twin_gradients_and_their_dtypes(torch, dt):
    """a float32 operand's gradient is the float64 gradient rounded once: half a unit of 2^-23 of its magnitude on top of ADJ_TOL"""
    from lerf_pytorch_amd import coords
    tdt = getattr(torch, dt)
    tol = ADJ_TOL if dt == "float64" else ADJ_TOL + 2.0 ** -24
    hw = (37, 131)
    gd = _dev(torch, upstream(hw)).to(tdt)
    gref = torch.from_numpy(_np(gd.double()))

    def close(got, ref, what):
        scale = max(float(ref.abs().max()), 1.0)
        err = float((got.detach().cpu().double() - ref).abs().max())
        print("%s %s: max error %.3g, scale %.3g, bound %.3g" % (what, dt, err, scale, tol * scale))
        assert got.dtype == tdt and tuple(got.shape) == tuple(ref.shape) and err <= tol * scale, what

    fish, view = _cams(torch, tdt)
    leaves = [t.clone().requires_grad_(True) for t in fish]
    out = coords.fisheye_undistort_rectify_torch(*leaves, hw)
    assert out.dtype == tdt
    out.backward(gd)
    refs = [t.cpu().clone().requires_grad_(True) for t in fish]
    pr = LR.camera_params_ref(*refs)
    assert_smooth("fisheye", pr.detach().numpy(), hw, (0, 0))
    (LR.model_map("fisheye", pr, hw) * gref).sum().backward()
    for leaf, ref, name in zip(leaves, refs, ("K", "dist", "R", "new_K")):
        close(leaf.grad, ref.grad.double(), "fisheye " + name)
        assert bool((leaf.grad != 0).any())
    assert not bool(leaves[0].grad[0, 1]) and not bool(leaves[0].grad[2].any())          # the entries of K the model does not read
    leaves = [t.clone().requires_grad_(True) for t in view]
    out = coords.equirect_view_torch(LR.PANO_HW, *leaves, hw)
    assert out.dtype == tdt
    out.backward(gd)
    refs = [t.cpu().clone().requires_grad_(True) for t in view]
    pr = LR.equirect_params_ref(LR.PANO_HW, *refs)
    assert_smooth("equirect", pr.detach().numpy(), hw, (0, 0))
    (LR.model_map("equirect", pr, hw) * gref).sum().backward()
    for leaf, ref, name in zip(leaves, refs, ("K_view", "R")):
        close(leaf.grad, ref.grad.double(), "equirect " + name)
        assert bool((leaf.grad != 0).any())


def test_batch_forms_equal_the_per_sample_calls(torch):
    from lerf_pytorch_amd import coords
    hw, Bn = (37, 131), 3
    gs = _dev(torch, np.stack([upstream(hw, 30 + s) for s in range(Bn)]))
    (K, dist, Rm, new_K), (Kv, Rv) = _cams(torch)
    # one shared K with a batch of distortions: [B, oH, oW, 2] in one launch, K's gradient is the sum over the samples
    ds = torch.stack([dist * (1.0 + 0.1 * s) for s in range(Bn)]).requires_grad_(True)
    lK = K.clone().requires_grad_(True)
    out = coords.fisheye_undistort_rectify_torch(lK, ds, Rm, new_K, hw)
    assert tuple(out.shape) == (Bn,) + hw + (2,)
    out.backward(gs)
    sumK = torch.zeros_like(K)
    for b in range(Bn):
        k1, d1 = K.clone().requires_grad_(True), ds[b].detach().clone().requires_grad_(True)
        o1 = coords.fisheye_undistort_rectify_torch(k1, d1, Rm, new_K, hw)
        assert torch.equal(o1.detach(), out[b].detach())
        o1.backward(gs[b])
        assert torch.equal(d1.grad, ds.grad[b])
        sumK += k1.grad
    adj_close(_np(lK.grad), _np(sumK), "shared K")
    # a batch of view matrices over one rotation
    Ks = torch.stack([Kv * _dev(torch, np.array([[1.0 + 0.05 * s], [1.0 + 0.05 * s], [1.0]])) for s in range(Bn)]).requires_grad_(True)
    out = coords.equirect_view_torch(LR.PANO_HW, Ks, Rv, hw)
    assert tuple(out.shape) == (Bn,) + hw + (2,)
    out.backward(gs)
    for b in range(Bn):
        k1 = Ks[b].detach().clone().requires_grad_(True)
        o1 = coords.equirect_view_torch(LR.PANO_HW, k1, Rv, hw)
        # torch.linalg.inv of a batch may round unlike that of one matrix: the maps agree to the forward's bound, not bit for bit
        assert float((o1.detach() - out[b].detach()).abs().max()) <= 1e-9
        o1.backward(gs[b])
        adj_close(_np(Ks.grad[b]), _np(k1.grad), "batch K_view %d" % b)


def test_twin_refusals(torch):
    from lerf_pytorch_amd import coords
    (K, dist, Rm, new_K), (Kv, Rv) = _cams(torch)
    skew = _dev(torch, np.array([[0, 0.1, 0], [0, 0, 0], [0, 0, 0.0]]))
    bad = [lambda: coords.fisheye_undistort_rectify_torch(_np(K), dist, Rm, new_K, (4, 5)), lambda: coords.fisheye_undistort_rectify_torch(K, dist.cpu(), Rm, new_K, (4, 5)),
           lambda: coords.fisheye_undistort_rectify_torch(K, dist[:3], Rm, new_K, (4, 5)), lambda: coords.fisheye_undistort_rectify_torch(K, torch.cat([dist, dist]), Rm, new_K, (4, 5)),
           lambda: coords.fisheye_undistort_rectify_torch(K, dist, Rm[:2], new_K, (4, 5)), lambda: coords.fisheye_undistort_rectify_torch(K[:, :2], dist, Rm, new_K, (4, 5)),
           lambda: coords.fisheye_undistort_rectify_torch(torch.stack([K, K]), torch.stack([dist] * 3), Rm, new_K, (4, 5)),
           lambda: coords.fisheye_undistort_rectify_torch(K + skew, dist, Rm, new_K, (4, 5)), lambda: coords.fisheye_params_torch(K * 2.0),
           lambda: coords.fisheye_undistort_rectify_torch(K, dist, Rm, new_K, (0, 5)), lambda: coords.fisheye_undistort_rectify_torch(K.half(), dist, Rm, new_K, (4, 5)),
           lambda: coords.fisheye_undistort_rectify_torch(K, dist, Rm, new_K, (4, 5), dtype=np.float16),
           lambda: coords.equirect_view_torch(LR.PANO_HW, _np(Kv), Rv, (4, 5)), lambda: coords.equirect_view_torch(LR.PANO_HW, Kv, Rv.cpu(), (4, 5)),
           lambda: coords.equirect_view_torch(LR.PANO_HW, Kv + skew, Rv, (4, 5)), lambda: coords.equirect_view_torch((0, 8), Kv, Rv, (4, 5)),
           lambda: coords.equirect_view_torch(LR.PANO_HW, Kv, Rv[:2], (4, 5)), lambda: coords.equirect_view_torch(LR.PANO_HW, Kv, Rv, (4, 0)),
           lambda: coords.equirect_view_torch(LR.PANO_HW, torch.stack([Kv, Kv]), torch.stack([Rv] * 3), (4, 5))]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    # the plain builders take host numbers and return a detached map
    assert not coords.fisheye_undistort_rectify(K.clone().requires_grad_(True), dist, Rm, new_K, (4, 5), device="cuda").requires_grad


# ---------------------------------------------------------------------------------------------- 9. end to end
FIT_K = np.array([[40.0, 0, 23.5], [0, 40.0, 23.5], [0, 0, 1]])
FIT_NEW_K = np.array([[36.0, 0, 17.5], [0, 36.0, 17.5], [0, 0, 1]])
FIT_OUT, FIT_LR, FIT_STEPS = (36, 36), 1e-4, 10
FIT_TRUE, FIT_START, FIT_K34 = (0.05, -0.012), (-0.05, 0.02), (0.004, -0.0009)


def _frame48():
    ii, jj = np.meshgrid(np.arange(48), np.arange(48), indexing="ij")
    return 100 + 50 * np.sin(2 * np.pi * ii / 24) + 40 * np.cos(2 * np.pi * jj / 16) + 30 * np.sin(2 * np.pi * (ii + jj) / 32)


def test_distort_with_the_inverse_and_undistort_through_the_engine(torch):
    """G = invert(fisheye map) distorts a pinhole frame into the fisheye's, the fisheye map F undistorts it.  border = 0 leaves the
    engine's mask with one reason to be false: an entry of the map that is NaN -- a fisheye pixel the pinhole view does not reach"""
    import lerf_pytorch_amd as L
    from lerf_pytorch_amd import coords
    eng = L.LerfEngine.shipped("lerf-g")
    img = np.repeat(_frame48().astype(np.uint8)[..., None], 3, axis=2)
    new_K = np.array([[45.0, 0, 23.5], [0, 45.0, 23.5], [0, 0, 1]])        # a 48 x 48 pinhole view that ends inside the fisheye frame
    F = coords.fisheye_undistort_rectify(FIT_K, FIT_TRUE + FIT_K34, None, new_K, (48, 48), device="cuda")
    assert not bool(torch.isnan(F).any())
    G = coords.invert(F, (48, 48))
    nan = torch.isnan(G).any(-1)
    assert 0 < int(nan.sum()) < nan.numel() // 2 and R.same_bits(_np(G), coords.invert(_np(F), (48, 48)))
    fish, mask = eng.remap(img, G, border=0)
    assert tuple(np.asarray(fish).shape) == (48, 48, 3)
    assert np.array_equal(np.asarray(mask), ~_np(nan)[..., None].repeat(3, axis=2))       # false exactly on the NaN entries
    back, mask2 = eng.remap(np.asarray(fish), F, border=0)
    assert bool(np.asarray(mask2).all()) and tuple(np.asarray(back).shape) == (48, 48, 3)
    inner = np.abs(np.asarray(back).astype(int) - img.astype(int))[12:36, 12:36]
    print("undistort(distort(frame)) - frame on the central 24 x 24: mean %.3g, max %d grey levels" % (float(inner.mean()), int(inner.max())))


def test_k1_k2_fitted_by_gradient_steps_lower_the_photometric_loss(torch):
    """plain gradient descent on (k1, k2) of a fisheye camera from FIT_START towards the frame undistorted with FIT_TRUE, through
    fisheye_undistort_rectify_torch, the build backward and the remap backward.  The same loop runs with the map built by the torch
    restatement (autograd instead of the build backward, the same remap): the two maps agree to 1e-12 of a coordinate and the bicubic
    remap is continuous in its map, so the two loss ratios agree far inside 1e-6 of each other.  The step is a third of the largest
    stable one of this loss (a bicubic stand-in on the CPU diverges at 1e-3 and takes the loss from 10.3 to 0.04 in ten steps at 1e-4)."""
    from lerf_pytorch_amd import coords
    T = _classes()
    x = torch.from_numpy(_frame48().astype(np.float32))[None, None].cuda()
    t = lambda a: _dev(torch, np.asarray(a, np.float64))
    K, new_K, k34, eye = t(FIT_K), t(FIT_NEW_K), t(FIT_K34), t(np.eye(3))

    def by_kernel(k12):
        return coords.fisheye_undistort_rectify_torch(K, torch.cat([k12, k34]), None, new_K, FIT_OUT)

    def by_restatement(k12):
        return LR.model_map("fisheye", LR.camera_params_ref(K, torch.cat([k12, k34]), eye, new_K), FIT_OUT)

    def forward(build, k12):
        w = T.BicubicRemap2dTorch().enable_backward()
        w.set_shape([1, 1, 48, 48], build(k12))
        return w.warp(x)

    with torch.no_grad():
        target = forward(by_kernel, t(FIT_TRUE))
    assert not bool(torch.isnan(target).any())
    ratios = []
    for build in (by_kernel, by_restatement):
        k = t(FIT_START).requires_grad_(True)
        losses = []
        for step in range(FIT_STEPS + 1):
            loss = ((forward(build, k) - target) ** 2).mean()
            losses.append(float(loss.detach()))
            if step == FIT_STEPS:
                break
            g, = torch.autograd.grad(loss, k)
            with torch.no_grad():
                k -= FIT_LR * g
        print("%s: losses %s -> k1, k2 = %s" % (build.__name__, " ".join("%.5g" % v for v in losses), _np(k)))
        assert np.isfinite(losses).all() and losses[-1] < losses[0]
        ratios.append(losses[-1] / losses[0])
    print("loss ratios: kernel %.9g, restatement %.9g" % tuple(ratios))
    assert abs(ratios[0] - ratios[1]) <= 1e-6 * max(ratios)
