"""Reproject by depth on the device (entry_kernel<ReprojectOp> and coords_reproject_bwd_kernel of csrc/lerf_coords.hip behind
ops.coords_reproject / coords_reproject_bwd and coords.reproject / reproject_torch), against the host twins whose bounds
tests/test_coords_reproject_cpu.py settles:

  1. the device map and zo are the host twin's bit for bit: kinds, dtype mixes, special depths, a strided out at an origin, three sets;
  2. the gradients are the host twin's bit for bit, equal from run to run, a batch equal to its single calls;
  3. reproject_torch through a remap class to depth, K_src, K_dst, R and t, and the two skipped halves;
  4. the backward warp of the identity pose is the remap by the identity homography, byte for byte;
  5. the forward splat of an occluded scene through invert_raster's depth test;
  6. the Python-level refusals.

Shapes of the backward: 70 x 130 spans two 64-row bands and three 64-column blocks (one of each kind of partial), 5 x 67 one ragged
second block, 1 x 1 one lane.
"""
import numpy as np
import pytest

import coords_ref as R
import coords_reproject_ref as PR
from test_coords_grad_cpu import ADJ_TOL
from test_coords_reproject_cpu import (K_EXACT, K_OTHER, KINDS, adjoint_case, cameras, check_occluded, forward_cases, occluded_scene, rotation,
                                       special_depth)
from test_gpu_remap_grad import _classes

pytestmark = pytest.mark.gpu

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


# ---------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("kind,ddt,odt,hw", forward_cases())
def test_device_map_and_depth_are_the_host_twins(torch, kind, ddt, odt, hw):
    from lerf_pytorch_amd import _lib, ops
    P = cameras()
    depth = np.stack([special_depth(hw, ddt, seed=s) for s in range(3)])
    ref, ref_zo = _lib.coords_reproject_host(kind, P, depth, odt, origin=ORIGIN, depth_out=True)
    buf = torch.full((3, hw[0], hw[1] + 3, 2), -7.0, dtype=getattr(torch, np.dtype(odt).name), device="cuda")
    out = buf[:, :, :hw[1]]
    assert out.stride(1) == 2 * (hw[1] + 3)
    got, zo = ops.coords_reproject(kind, _dev(torch, P), _dev(torch, depth), out=out, origin=ORIGIN, depth_out=True)
    assert got is out and zo.dtype == torch.float32
    assert R.same_bits(_np(got.contiguous()), ref) and R.same_bits(_np(zo), ref_zo)
    assert bool((buf[:, :, hw[1]:] == -7.0).all())
    # one set, a new tensor, no depth_out; one depth plane shared by the sets
    one = ops.coords_reproject(kind, _dev(torch, P[1]), _dev(torch, depth[1]), dtype=out.dtype, origin=ORIGIN)
    assert R.same_bits(_np(one), ref[1])
    shared = ops.coords_reproject(kind, _dev(torch, P), _dev(torch, depth[0]), dtype=out.dtype, origin=ORIGIN)
    assert R.same_bits(_np(shared), _lib.coords_reproject_host(kind, P, depth[0], odt, origin=ORIGIN))


# ---------------------------------------------------------------------------------------------- 2. backward
@pytest.mark.parametrize("hw", [(70, 130), (5, 67), (1, 1)])
@pytest.mark.parametrize("n_sets", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_gradients_are_the_host_twins_bit_for_bit(torch, kind, n_sets, hw):
    from lerf_pytorch_amd import _lib, ops
    P = cameras()[:n_sets]
    cases = [adjoint_case(kind, hw, True, np.float32 if s == 1 else np.float64, seed=20 + s) for s in range(n_sets)]
    for ddt in ((np.float64,) if n_sets == 1 else (np.float64, np.float32)):
        d = np.stack([c[1].astype(ddt) for c in cases])
        g, gz = (np.stack([c[k] for c in cases]) for k in (2, 3))
        hd, hp = _lib.coords_reproject_bwd_host(kind, P, d, g, gz, origin=ORIGIN)
        tP, td, tg, tgz = (_dev(torch, a) for a in (P, d, g, gz))
        gd, gp = ops.coords_reproject_bwd(kind, tP, td, tg, tgz, origin=ORIGIN)
        assert R.same_bits(_np(gd), hd) and R.same_bits(_np(gp), hp)
        gd2, gp2 = ops.coords_reproject_bwd(kind, tP, td, tg, tgz, origin=ORIGIN)
        assert torch.equal(gd.view(torch.int64), gd2.view(torch.int64)) and torch.equal(gp.view(torch.int64), gp2.view(torch.int64))
        for s in range(n_sets):                                     # a batch is its single-set calls
            sd, sp = ops.coords_reproject_bwd(kind, tP[s], td[s], tg[s], tgz[s], origin=ORIGIN)
            assert R.same_bits(_np(sd), hd[s]) and R.same_bits(_np(sp), hp[s])
        # without an upstream for zo, each half alone, into pre-filled buffers
        hd0, hp0 = _lib.coords_reproject_bwd_host(kind, P, d, g, None, origin=ORIGIN)
        pre_d, pre_p = torch.full_like(gd, 0.5), torch.full_like(gp, -0.25)
        od, none = ops.coords_reproject_bwd(kind, tP, td, tg, None, grad_depth=pre_d, need=(True, False), origin=ORIGIN)
        none2, op = ops.coords_reproject_bwd(kind, tP, td, tg, None, grad_params=pre_p, need=(False, True), origin=ORIGIN)
        assert none is None and none2 is None and od is pre_d and op is pre_p
        assert R.same_bits(_np(od), 0.5 + hd0) and R.same_bits(_np(op), -0.25 + hp0)


# ---------------------------------------------------------------------------------------------- 3. reproject_torch
K_WIDE = np.array([[28.0, 0.0, 15.5], [0.0, 28.0, 12.0], [0.0, 0.0, 1.0]])          # a shorter focal length: the 24 x 32 view lands inside the frame


def _pose(torch, requires_grad):
    """K_src, K_dst, R, t: every pixel of the 24 x 32 view of K_OTHER lands at least 2 px inside the 24 x 32 frame of K_WIDE (the remap's
    taps stay in the image, its map gradient is finite)"""
    Rm, t = rotation(0.01, -0.015, 0.02), np.array([0.05, -0.04, 0.1])
    return [_dev(torch, a).requires_grad_(requires_grad) for a in (K_OTHER, K_WIDE, Rm, t)]


def _depth(torch, hw, inverse, requires_grad):
    ii, jj = np.meshgrid(np.arange(hw[0]), np.arange(hw[1]), indexing="ij")
    z = 4.0 + np.sin(ii / 5.0) + 0.5 * np.cos(jj / 7.0)
    return _dev(torch, 1.0 / z if inverse else z).requires_grad_(requires_grad)


@pytest.mark.parametrize("inverse", [False, True])
def test_reproject_torch_reaches_depth_cameras_and_pose_through_a_remap(torch, inverse, monkeypatch):
    from lerf_pytorch_amd import coords, ops
    T = _classes()
    hw = (24, 32)
    kind = "inverse" if inverse else "z"
    ii, jj = np.meshgrid(np.arange(hw[0]), np.arange(hw[1]), indexing="ij")
    img = (100 + 50 * np.sin(2 * np.pi * ii / 12) + 40 * np.cos(2 * np.pi * jj / 16)).astype(np.float32)
    x = torch.from_numpy(img)[None, None].cuda()
    needs = []
    real = ops.coords_reproject_bwd
    monkeypatch.setattr(ops, "coords_reproject_bwd", lambda *a, **kw: needs.append(tuple(kw["need"])) or real(*a, **kw))

    def run(depth_grad, pose_grad):
        """(leaves, their gradients, the map, the remap's gradient on the map)"""
        depth, cams = _depth(torch, hw, inverse, depth_grad), _pose(torch, pose_grad)
        cm = coords.reproject_torch(depth, *cams, inverse_depth=inverse)
        assert cm.requires_grad and cm.dtype == torch.float64 and tuple(cm.shape) == hw + (2,)
        cm.retain_grad()
        w = T.BicubicRemap2dTorch().enable_backward()
        w.set_shape([1, 1] + list(hw), cm)
        (w.warp(x) ** 2).sum().backward()
        return [depth] + cams, cm, cm.grad.detach()

    def reference(leaves, g):
        """float64 autograd through the stock-torch restatement of the map, the remap's map gradient held fixed"""
        refs = [t.detach().clone().requires_grad_(t.requires_grad) for t in leaves]
        m, _ = PR.forward_torch(kind, PR.params_torch(*refs[1:]), refs[0])
        want = [t for t in refs if t.requires_grad]
        return dict(zip([id(t) for t in want], torch.autograd.grad((m * g).sum(), want))), refs

    for depth_grad, pose_grad in ((True, True), (True, False), (False, True)):
        leaves, cm, g = run(depth_grad, pose_grad)
        assert needs.pop() == (depth_grad, pose_grad) and not needs
        lo, hi = cm.detach().amin(dim=(0, 1)), cm.detach().amax(dim=(0, 1))
        assert float(lo.min()) >= 2.0 and float(hi[0]) <= hw[0] - 3.0 and float(hi[1]) <= hw[1] - 3.0
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
        grads, refs = reference(leaves, g)
        for leaf, ref, name in zip(leaves, refs, ("depth", "K_src", "K_dst", "R", "t")):
            if not leaf.requires_grad:
                assert leaf.grad is None
                continue
            gr = _np(grads[id(ref)])
            scale = max(float(np.max(np.abs(gr))), 1.0)
            err = float(np.max(np.abs(_np(leaf.grad) - gr)))
            print("%s %s: max |grad| %.3g, error %.3g, bound %.3g" % (kind, name, float(np.max(np.abs(gr))), err, ADJ_TOL * scale))
            assert leaf.grad.dtype == leaf.dtype and np.isfinite(err) and err <= ADJ_TOL * scale, name
            assert bool((leaf.grad != 0).any())


def test_reproject_torch_without_grad_is_the_plain_kernel_and_returns_depth(torch):
    from lerf_pytorch_amd import coords
    hw = (24, 32)
    depth, cams = _depth(torch, hw, False, False), _pose(torch, False)
    m, z = coords.reproject_torch(depth, *cams, return_depth=True)
    p = coords.reproject_params_torch(*cams)
    assert tuple(p.shape) == (12,) and p.dtype == torch.float64
    assert np.allclose(_np(p), coords.reproject_params(*[_np(c) for c in cams]), rtol=0, atol=1e-12)
    from lerf_pytorch_amd import _lib
    hm, hz = _lib.coords_reproject_host("z", _np(p), _np(depth), depth_out=True)
    assert not m.requires_grad and R.same_bits(_np(m), hm) and R.same_bits(_np(z), hz)
    # zo carries a gradient too: d sum(zo) / d t_z = the number of entries
    depth, cams = _depth(torch, hw, False, True), _pose(torch, True)
    m, z = coords.reproject_torch(depth, *cams, return_depth=True)
    z.double().sum().backward()
    assert abs(float(cams[3].grad[2]) - hw[0] * hw[1]) < 1e-9 and bool((depth.grad != 0).all())
    # a batch of depth planes under one camera pair: one map per sample, the cameras' gradient summed by autograd
    db = torch.stack([_depth(torch, hw, False, False), _depth(torch, hw, False, False) + 0.5]).requires_grad_(True)
    cams = _pose(torch, True)
    mb = coords.reproject_torch(db, *cams)
    assert tuple(mb.shape) == (2,) + hw + (2,)
    mb.sum().backward()
    assert tuple(db.grad.shape) == (2,) + hw and cams[0].grad is not None and bool((cams[3].grad != 0).any())


# ---------------------------------------------------------------------------------------------- 4. the backward warp
def test_backward_warp_of_the_identity_pose_is_the_identity_homographys_remap(torch):
    from lerf_pytorch_amd import coords
    T = _classes()
    hw = (24, 32)
    img = torch.from_numpy(np.random.default_rng(3).uniform(0, 255, (1, 3) + hw).astype(np.float32)).cuda()
    depth = _dev(torch, np.full(hw, 8.0, np.float32))
    m = coords.reproject(depth, K_EXACT, K_EXACT)
    h = coords.from_homography(np.eye(3), hw, device="cuda")
    assert m.is_cuda and m.dtype == torch.float64 and R.same_bits(_np(m), _np(h))
    outs = []
    for cm in (m, h):
        w = T.BicubicRemap2dTorch()
        w.set_shape([1, 3] + list(hw), cm)
        outs.append(w.warp(img))
    assert outs[0].shape == outs[1].shape and torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert R.same_bits(_np(m), coords.reproject(_np(depth), K_EXACT, K_EXACT))


# ---------------------------------------------------------------------------------------------- 5. the forward splat
def test_forward_splat_with_occlusion(torch):
    from lerf_pytorch_amd import _lib, coords, ops
    d, K, t = occluded_scene()
    m, z = coords.reproject(_dev(torch, d), K, K, None, t, return_depth=True)
    assert m.is_cuda and z.is_cuda and z.dtype == torch.float32
    hm, hz = coords.reproject(d, K, K, None, t, return_depth=True)
    assert R.same_bits(_np(m), hm) and R.same_bits(_np(z), hz)
    G = coords.invert_raster(m, (24, 32), depth=z, max_span=4, orient=1)
    G2, keys = ops.coords_invert_raster(m, (24, 32), depth=z, max_span=4, orient=1, return_keys=True)
    hG, hkeys = _lib.coords_invert_raster_host(hm, (24, 32), depth=hz, max_span=4, orient=1, return_keys=True)
    assert R.same_bits(_np(G), hG) and R.same_bits(_np(G2), hG) and np.array_equal(_np(keys).view(np.uint64), hkeys)
    check_occluded(_np(G), _np(keys), _np(coords.invert_raster(m, (24, 32), max_span=4, orient=1)))


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_python_level_refusals_launch_nothing(torch, monkeypatch):
    from lerf_pytorch_amd import _lib, coords, ops
    L = _lib.lib()
    launched = []
    for name in ("lerf_coords_reproject", "lerf_coords_reproject_bwd"):
        monkeypatch.setattr(L, name, lambda *a, _n=name: launched.append(_n) or 0)
    hw = (6, 9)
    dh, dd = np.full(hw, 2.0), _dev(torch, np.full(hw, 2.0))
    Kh, Kd = torch.from_numpy(K_EXACT), _dev(torch, K_EXACT)
    bad_K = np.array([[40.0, 0, 15.5], [0, 36.0, 11.5], [0, 0, 2.0]])
    for call in (lambda: coords.reproject(dh, Kd, K_EXACT),                              # a device camera beside a host depth
                 lambda: coords.reproject(dd, Kh, K_EXACT),                              # a host tensor beside a device depth
                 lambda: coords.reproject(dd, K_EXACT, K_EXACT, None, Kh[0]),
                 lambda: coords.reproject(dd, K_EXACT, bad_K),
                 lambda: coords.reproject_torch(dd, Kd, _dev(torch, bad_K)),
                 lambda: coords.reproject(dd[0], K_EXACT, K_EXACT),                      # a depth of the wrong rank
                 lambda: coords.reproject(dd[None, None], K_EXACT, K_EXACT),
                 lambda: coords.reproject_torch(dd[0], Kd, Kd),
                 lambda: coords.reproject_torch(torch.from_numpy(dh), Kd, Kd),           # a host tensor
                 lambda: coords.reproject_torch(dd, Kh, Kd),
                 lambda: coords.reproject_torch(dh, Kd, Kd),
                 lambda: coords.reproject_torch(dd.to(torch.float16), Kd, Kd),
                 lambda: coords.reproject(dd.clone().requires_grad_(True), K_EXACT, K_EXACT),
                 lambda: coords.reproject_torch(torch.stack([dd, dd]), torch.stack([Kd, Kd, Kd]), Kd),
                 lambda: ops.coords_reproject("z", _dev(torch, cameras()[0]), dh),
                 lambda: ops.coords_reproject("z", cameras()[0], dd),
                 lambda: ops.coords_reproject("depth", _dev(torch, cameras()[0]), dd),
                 lambda: ops.coords_reproject("z", _dev(torch, cameras()[0][:9]), dd),
                 lambda: ops.coords_reproject_bwd("z", _dev(torch, cameras()[0]), dd, None),
                 lambda: ops.coords_reproject_bwd("z", _dev(torch, cameras()[0]), dd, torch.ones(hw + (2,), dtype=torch.float64)),
                 lambda: ops.coords_reproject_bwd("z", _dev(torch, cameras()[0]), dd, torch.ones(hw + (2,), dtype=torch.float64, device="cuda"),
                                                  need=(False, False))):
        with pytest.raises((ValueError, _lib.LerfError)):
            call()
    assert not launched
    monkeypatch.undo()
    # the C entry point refuses what the wrappers cannot see: out's bytes on depth's
    buf = torch.zeros(hw + (2,), dtype=torch.float64, device="cuda")
    with pytest.raises((ValueError, _lib.LerfError)):
        ops.coords_reproject("z", _dev(torch, cameras()[0]), buf.view(-1)[:hw[0] * hw[1]].view(hw), out=buf)
    assert bool((buf == 0).all())
