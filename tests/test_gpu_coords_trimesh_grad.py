"""GPU: the adjoint of the triangle-mesh rasteriser (lerf_coords_trimesh_bwd) and coords.from_triangles_torch.

  1. the meshes of tests/test_coords_trimesh_grad_cpu.py on the device against the host twin BY INTEGER PATTERN, two runs equal, the cap;
  2. the 70 x 130 -> 90 x 160 folded grid mesh of the forward's GPU test: 17 802 faces (more than one scan block), valences of 6;
  3. from_triangles_torch: the forward's bits, loss.backward() to pos, attr and w within the restatement's bound, a batch of 3 with a
     shared attr, LerfError above max_adders, the refusals;
  4. one end-to-end chain: a remap twin after enable_backward() over from_triangles_torch.
"""
import numpy as np
import pytest

import coords_ref as R
import coords_trimesh_grad_ref as GR
from test_coords_raster_cpu import _ij
from test_coords_trimesh_grad_cpu import CASES, face_plane, perspective_mesh, upstream
from test_coords_trimesh_cpu import fan_mesh, random_mesh
from test_gpu_coords_trimesh import _big_map
from test_gpu_remap_grad import _classes, _make

pytestmark = pytest.mark.gpu
NO_KEY = np.uint64(2 ** 64 - 1)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def _dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _both(torch, pos, attr, faces, hw, kw, need, **extra):
    """the forward and the backward on the host and on the device, the device twice -> (host grads, device grads, device again, keys)"""
    from lerf_pytorch_amd import _lib, ops
    out, keys = _lib.coords_trimesh_host(pos, attr, faces, hw, return_keys=True, **kw)
    g = upstream(keys)
    host = _lib.coords_trimesh_bwd_host(pos, attr, faces, hw, keys, g, need=need, **kw, **extra)
    dkw = {k: (v if isinstance(v, (int, tuple)) else _dev(torch, v)) for k, v in kw.items()}
    dout, dkeys = ops.coords_trimesh(_dev(torch, pos), _dev(torch, attr), _dev(torch, faces), hw, return_keys=True, **dkw)
    assert np.array_equal(_np(dkeys).view(np.uint64), keys)
    runs = [ops.coords_trimesh_bwd(_dev(torch, pos), _dev(torch, attr), _dev(torch, faces), hw, dkeys, _dev(torch, g), need=need, **dkw, **extra)
            for _ in range(2)]
    return host, runs[0], runs[1], keys


def _equal(a, b):
    return all((x is None and y is None) or R.same_bits(_np(x) if hasattr(x, "cpu") else x, _np(y) if hasattr(y, "cpu") else y)
               for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- 1. the meshes of the CPU file
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_the_host_twin_bit_for_bit(torch, name):
    pos, attr, faces, hw, kw = CASES[name]
    host, a, b, keys = _both(torch, pos, attr, faces, hw, kw, (True, True, "w" in kw))
    assert _equal(a, host), name
    assert _equal(b, a), name
    assert all(t is None or np.isfinite(_np(t)).all() for t in a)


def test_the_cap_poisons_the_centre_of_the_fan_alone(torch):
    from lerf_pytorch_amd import _lib, ops
    pos, attr, faces = fan_mesh()
    dev = lambda x: _dev(torch, x)
    out, keys = ops.coords_trimesh(dev(pos), dev(attr), dev(faces), (29, 37), return_keys=True)
    g = dev(upstream(_np(keys)))
    ga, gp, _ = ops.coords_trimesh_bwd(dev(pos), dev(attr), dev(faces), (29, 37), keys, g, max_adders=7)
    ha, hp, _ = _lib.coords_trimesh_bwd_host(pos, attr, faces, (29, 37), _np(keys).view(np.uint64), _np(g), max_adders=6)
    pre_a, pre_p = torch.zeros((8, 2), dtype=torch.float64, device="cuda"), torch.zeros((8, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.LerfError, match="max_adders"):
        ops.coords_trimesh_bwd(dev(pos), dev(attr), dev(faces), (29, 37), keys, g, grad_attr=pre_a, grad_pos=pre_p, max_adders=6)
    assert R.same_bits(_np(pre_a), ha) and R.same_bits(_np(pre_p), hp)          # the centre NaN, every other vertex exact
    assert np.isnan(ha[0]).all() and R.same_bits(ha[1:], _np(ga)[1:]) and R.same_bits(hp[1:], _np(gp)[1:])


# ---------------------------------------------------------------------------------------------- 2. many faces
def test_a_mesh_of_several_scan_blocks(torch):
    from lerf_pytorch_amd import _lib, coords
    f_hw, hw = (70, 130), (90, 160)
    F, depth = _big_map(f_hw)
    faces = coords.grid_faces(*f_hw)
    assert len(faces) == 17802 and len(F.reshape(-1, 2)) > _lib.scan_block()
    attr = np.stack(_ij(f_hw), axis=-1).reshape(-1, 2)
    w = (1.0 + 0.5 * np.sin(np.arange(len(attr)) / 11.0))
    kw = {"depth": depth.reshape(-1), "w": w, "max_span": 16}
    pos = np.ascontiguousarray(F.reshape(-1, 2))
    host, a, b, keys = _both(torch, pos, attr, faces, hw, kw, (True, True, True), max_adders=6)
    assert _equal(a, host) and _equal(b, a)
    assert all(np.isfinite(t).all() for t in host) and all(np.abs(t).max() > 0 for t in host)
    most = _lib.coords_trimesh_bwd_host(pos, attr, faces, hw, keys, upstream(keys), need=(True, False, False), return_most=True, **kw)[3]
    assert most == 6
    holes = (keys == NO_KEY).mean()
    assert 0.0 < holes < 0.9


# ---------------------------------------------------------------------------------------------- 3. from_triangles_torch
def _leaf(torch, a, dt=None):
    t = _dev(torch, a)
    return (t if dt is None else t.to(dt)).requires_grad_(True)


def _check(name, got, ref):
    err, bound = GR.within(got, ref)
    print("%s: max error %.3g, bound %.3g" % (name, err, bound))
    assert err <= bound, (name, err, bound)


def test_from_triangles_torch_forward_bits_and_backward(torch):
    from lerf_pytorch_amd import coords
    pos, attr, faces, w = perspective_mesh()
    hw = (70, 90)
    P, A, Wv = _leaf(torch, pos), _leaf(torch, attr), _leaf(torch, w)
    m, face = coords.from_triangles_torch(P, A, _dev(torch, faces), hw, w=Wv, return_faces=True)
    want, wface = coords.from_triangles(pos, attr, faces, hw, w=w, return_faces=True)
    assert m.requires_grad and not face.requires_grad and R.same_bits(_np(m), want) and np.array_equal(_np(face), wface)
    g = upstream(np.where(wface < 0, NO_KEY, wface.astype(np.uint64)))
    gd = torch.nan_to_num(_dev(torch, g))
    (torch.nan_to_num(m) * gd).sum().backward()
    ra, rp, rw = GR.gradients(wface, pos, attr, faces, g, w=w)
    _check("attr", _np(A.grad), ra)
    _check("pos", _np(P.grad), rp)
    _check("w", _np(Wv.grad), rw)
    # float32 operands: the forward's bits, gradients in the operands' dtype
    P32, A32 = _leaf(torch, pos, torch.float32), _leaf(torch, attr, torch.float32)
    m32 = coords.from_triangles_torch(P32, A32, _dev(torch, faces.astype(np.int64)), hw)
    assert m32.dtype == torch.float32 and R.same_bits(_np(m32), coords.from_triangles(pos.astype(np.float32), attr.astype(np.float32), faces, hw))
    torch.nan_to_num(m32).sum().backward()
    assert P32.grad.dtype == torch.float32 and A32.grad.dtype == torch.float32 and bool(P32.grad.abs().sum() > 0)
    # with depth: the depth result is not differentiable, a depth that requires grad is refused
    pos, attr, faces, depth = random_mesh()
    P, A = _leaf(torch, pos), _leaf(torch, attr)
    m, z, face = coords.from_triangles_torch(P, A, _dev(torch, faces), (29, 37), depth=_dev(torch, depth), return_depth=True, return_faces=True)
    want = coords.from_triangles(pos, attr, faces, (29, 37), depth=depth, return_depth=True, return_faces=True)
    assert not z.requires_grad and all(R.same_bits(_np(x), y) for x, y in zip((m, z), want[:2])) and np.array_equal(_np(face), want[2])
    g = upstream(np.where(want[2] < 0, NO_KEY, want[2].astype(np.uint64)))
    (torch.nan_to_num(m) * torch.nan_to_num(_dev(torch, g))).sum().backward()
    ra, rp, _ = GR.gradients(want[2], pos, attr, faces, g)
    _check("attr (depth)", _np(A.grad), ra)
    _check("pos (depth)", _np(P.grad), rp)
    with pytest.raises(ValueError, match="depth"):
        coords.from_triangles_torch(P, A, _dev(torch, faces), (29, 37), depth=_dev(torch, depth).requires_grad_(True))
    with pytest.raises(ValueError, match="device tensor"):
        coords.from_triangles_torch(pos, A, _dev(torch, faces), (29, 37))
    with pytest.raises(ValueError, match="return_depth"):
        coords.from_triangles_torch(P, A, _dev(torch, faces), (29, 37), return_depth=True)
    with pytest.raises(ValueError, match="autograd"):
        coords.from_triangles(P, A, _dev(torch, faces), (29, 37))          # from_triangles itself stays as it is


def test_a_batch_of_three_with_a_shared_attr(torch):
    from lerf_pytorch_amd import coords
    pos, attr, faces, depth = random_mesh()
    rng = np.random.default_rng(5)
    Pn = np.stack([pos, pos + rng.uniform(-2.0, 2.0, pos.shape), pos[::-1]])
    fd = _dev(torch, faces)
    P, A = _leaf(torch, Pn), _leaf(torch, attr)
    m, face = coords.from_triangles_torch(P, A, fd, (29, 37), return_faces=True)
    assert tuple(m.shape) == (3, 29, 37, 2)
    G = np.stack([upstream(np.where(_np(face[s]) < 0, NO_KEY, _np(face[s]).astype(np.uint64)), seed=s) for s in range(3)])
    Gd = torch.nan_to_num(_dev(torch, G))
    (torch.nan_to_num(m) * Gd).sum().backward()
    assert tuple(A.grad.shape) == (12, 2) and tuple(P.grad.shape) == (3, 12, 2)
    total = None
    for s in range(3):
        Ps, As = _leaf(torch, Pn[s]), _leaf(torch, attr)
        ms = coords.from_triangles_torch(Ps, As, fd, (29, 37))
        assert R.same_bits(_np(ms), _np(m[s]))
        (torch.nan_to_num(ms) * Gd[s]).sum().backward()
        assert R.same_bits(_np(Ps.grad), _np(P.grad[s]))
        total = As.grad if total is None else total + As.grad
    assert R.same_bits(_np(total), _np(A.grad))                           # the sum of the three per-sample gradients, sample 0 first


def test_lerf_error_above_max_adders(torch):
    from lerf_pytorch_amd import _lib, coords
    pos, attr, faces = fan_mesh()
    P, A = _leaf(torch, pos), _leaf(torch, attr)
    m = coords.from_triangles_torch(P, A, _dev(torch, faces), (29, 37), max_adders=6)
    with pytest.raises(_lib.LerfError, match="max_adders"):
        m.sum().backward()
    P, A = _leaf(torch, pos), _leaf(torch, attr)
    coords.from_triangles_torch(P, A, _dev(torch, faces), (29, 37), max_adders=7).sum().backward()
    assert bool(torch.isfinite(P.grad).all()) and bool(torch.isfinite(A.grad).all())


# ---------------------------------------------------------------------------------------------- 4. end to end
def test_a_loss_reaches_the_vertices_through_a_remap_twin(torch):
    from lerf_pytorch_amd import coords
    T = _classes()
    hw = (24, 32)
    # a jittered 4 x 5 vertex grid that covers the whole frame and shows the source moved and slightly sheared
    ii, jj = np.meshgrid(np.linspace(-1.0, 24.0, 4), np.linspace(-1.0, 32.0, 5), indexing="ij")
    pos = np.stack([ii, jj], axis=-1).reshape(-1, 2)
    pos[[6, 7, 8, 11, 12, 13]] += np.random.default_rng(2).uniform(-1.5, 1.5, (6, 2))
    attr = pos @ np.array([[0.9, 0.05], [-0.04, 0.92]]) + np.array([1.5, 2.25])
    faces = coords.grid_faces(4, 5)
    P, A = _leaf(torch, pos), _leaf(torch, attr)
    cm = coords.from_triangles_torch(P, A, _dev(torch, faces), hw)
    assert cm.requires_grad and not bool(torch.isnan(cm).any())
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.rand((1, 2) + hw, generator=gen, device="cuda") * 255
    w = _make(T, "bilinear", 2, "constant").enable_backward()
    w.set_shape([1, 2] + list(hw), cm)
    loss = (w.warp(x) ** 2).sum()
    loss.backward()
    assert bool(torch.isfinite(P.grad).all()) and bool(torch.isfinite(A.grad).all())
    assert bool((P.grad[[6, 7, 8, 11, 12, 13]] != 0).any()) and bool((A.grad != 0).any())
