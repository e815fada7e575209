"""The triangle-mesh rasteriser on the device (entry_kernel<KeyFillOp>, entry_kernel<TriCountOp>, scan_exclusive_u32,
trimesh_raster_kernel, entry_kernel<TriResolveOp> of csrc/lerf_coords.hip behind ops.coords_trimesh and coords.from_triangles).  The
host twin is the reference throughout, BY INTEGER PATTERN in out, keys and depth_out (tests/test_coords_trimesh_cpu.py ties it to the
independent restatement):

  1. every mesh of the CPU file's item 2;
  2. invert_raster's own triangulation: every case of raster_cases(), and the 70 x 130 -> 90 x 160 folded map -- 17 802 faces, more than
     one block of the scan, several items a wave, ragged last blocks in the count and resolve passes -- in every dtype mix;
  3. a minifying noisy mesh where hundreds of faces contend for one pixel: the same bits in two runs, and the host's;
  4. a single item in total, and a single face with hundreds of items;
  5. coords.from_triangles on device tensors and on a batch of 3 equals the numpy path;
  6. LerfEngine.remap along a pure translation mesh smaller than the frame;
  7. the Python refusals, without a launch.

No frame is larger than 90 x 160 (one case: 256 x 640, one face).
"""
import numpy as np
import pytest

import coords_ref as R
from test_coords_raster_cpu import _identity, _ij, raster_cases
from test_coords_trimesh_cpu import CASES, check_case, grid_call, random_mesh, run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def _dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _same(got, want):
    """device results against the host twin's: maps and depth by bits, int64 keys against uint64"""
    if not isinstance(got, tuple):
        got, want = (got,), (want,)
    assert len(got) == len(want)
    for g, h in zip(got, want):
        g = _np(g)
        if not (np.array_equal(g.view(np.uint64), h) if h.dtype == np.uint64 else R.same_bits(g, h)):
            return False
    return True


def _big_map(hw):
    """tests/test_gpu_coords_raster.py's map: a stretch by 1.2 with a sinusoidal fold along the columns and a ripple along the rows,
    and a depth to go with it"""
    ii, jj = _ij(hw)
    F = np.stack([1.2 * ii + 1.5 * np.sin(jj / 9.0), 1.2 * jj + 4.5 * np.sin(jj / 2.5) + 0.5 * np.cos(ii / 3.0)], axis=-1)
    depth = (3.0 + np.sin(ii / 4.0 + jj / 7.0) + 0.25 * np.cos(jj * 1.7)).astype(np.float32)
    return F, depth


# ---------------------------------------------------------------------------------------------- 1. the meshes of the CPU file
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_mesh_is_bit_equal_to_the_restatement(torch, name):
    from lerf_pytorch_amd import ops
    check_case(name, *run_case(ops.coords_trimesh, name, wrap=lambda a: _dev(torch, a)), to_numpy=_np)


# ---------------------------------------------------------------------------------------------- 2. against invert_raster
@pytest.mark.parametrize("case", raster_cases(), ids=lambda c: c[0])
def test_grid_faces_give_invert_raster(torch, case):
    from lerf_pytorch_amd import _lib, ops
    name, F, hw, depth, span, orient = case
    want = _lib.coords_invert_raster_host(np.ascontiguousarray(F), hw, depth=depth, max_span=span, orient=orient, return_keys=True)
    assert _same(grid_call(F, hw, depth, span, orient, one=ops.coords_trimesh, wrap=lambda a: _dev(torch, a)), want)


def test_a_mesh_of_several_scan_blocks(torch):
    from lerf_pytorch_amd import _lib, coords, ops
    f_hw, hw = (70, 130), (90, 160)
    F, depth = _big_map(f_hw)
    faces = coords.grid_faces(*f_hw)
    assert len(faces) == 17802 and len(faces) + 1 > _lib.scan_block()
    assert len(faces) % 256 and (len(faces) + 1) % 4 and hw[0] % 4 and hw[1] % 64          # ragged last blocks
    attr = np.stack(_ij(f_hw), axis=-1).reshape(-1, 2)
    fd, dd, zd = _dev(torch, faces), _dev(torch, depth.reshape(-1)), depth.reshape(-1)
    for d, ddev in ((None, None), (zd, dd)):
        want = _lib.coords_invert_raster_host(F, hw, depth=None if d is None else depth, max_span=16, return_keys=True)
        got = ops.coords_trimesh(_dev(torch, F.reshape(-1, 2)), _dev(torch, attr), fd, hw, depth=ddev, max_span=16, return_keys=True)
        assert _same(got, want)
    for pdt in (np.float64, np.float32):
        for adt in (np.float64, np.float32):
            for odt in (np.float64, np.float32):
                P, A = np.ascontiguousarray(F.reshape(-1, 2).astype(pdt)), attr.astype(adt)
                tdt = torch.float32 if odt == np.float32 else torch.float64
                for span, orient in ((0, 0), (4, 1)):
                    want = _lib.coords_trimesh_host(P, A, faces, hw, depth=zd, dtype=odt, max_span=span, orient=orient, return_keys=True,
                                                    return_depth=True)
                    got = ops.coords_trimesh(_dev(torch, P), _dev(torch, A), fd, hw, depth=dd, dtype=tdt, max_span=span, orient=orient,
                                             return_keys=True, return_depth=True)
                    assert _same(got, want), (pdt, adt, odt, span, orient)
    holes = np.isnan(want[0][..., 0]).mean()
    assert 0.0 < holes < 0.9


# ---------------------------------------------------------------------------------------------- 3. contention
def test_hundreds_of_faces_on_one_pixel_give_the_same_bits_every_run(torch):
    from lerf_pytorch_amd import _lib, coords, ops
    f_hw = (70, 130)
    F = np.ascontiguousarray(0.05 * _identity(f_hw) + np.random.default_rng(7).uniform(-0.6, 0.6, f_hw + (2,))).reshape(-1, 2)
    attr = np.stack(_ij(f_hw), axis=-1).reshape(-1, 2)
    faces = coords.grid_faces(*f_hw)
    depth = np.random.default_rng(5).uniform(1.0, 2.0, len(F)).astype(np.float32)
    Pd, Ad, fd, dd = (_dev(torch, a) for a in (F, attr, faces, depth))
    for d, ddev in ((None, None), (depth, dd)):
        want = _lib.coords_trimesh_host(F, attr, faces, (5, 8), depth=d, return_keys=True)
        a = ops.coords_trimesh(Pd, Ad, fd, (5, 8), depth=ddev, return_keys=True)
        b = ops.coords_trimesh(Pd, Ad, fd, (5, 8), depth=ddev, return_keys=True)
        assert _same(a, want) and _same(b, want)
    # the faces whose pixel box holds pixel (2, 3): every one of them sends a wave there
    lo, hi = np.ceil(F[faces].min(axis=1)), np.floor(F[faces].max(axis=1))
    boxes = int(((lo <= (2.0, 3.0)) & (hi >= (2.0, 3.0))).all(axis=1).sum())
    print("faces whose box holds pixel (2, 3): %d" % boxes)
    assert boxes > 200 and not np.isnan(want[0][1:4, 1:6]).any()


# ---------------------------------------------------------------------------------------------- 4. the ends of the item list
def test_a_single_item_and_a_single_face_of_hundreds_of_items(torch):
    from lerf_pytorch_amd import _lib, ops
    attr = np.array([[1.0, 2.0], [3.0, 5.0], [8.0, 13.0]])
    one = np.array([[0, 1, 2]], np.int32)
    # one face inside one 4 x 16 tile: one item
    small = np.array([[4.5, 17.0], [4.5, 30.0], [7.5, 17.0]])
    # one face over 256 x 640: 64 x 40 = 2560 items, one a wave
    large = np.array([[-5.0, -5.0], [-5.0, 1400.0], [600.0, -5.0]])
    for pos, hw, items in ((small, (12, 48), 1), (large, (256, 640), 2560)):
        want = _lib.coords_trimesh_host(pos, attr, one, hw, return_keys=True)
        got = ops.coords_trimesh(_dev(torch, pos), _dev(torch, attr), _dev(torch, one), hw, return_keys=True)
        assert _same(got, want)
        covered = want[1] != np.uint64(2 ** 64 - 1)
        tiles = covered.reshape(hw[0] // 4, 4, hw[1] // 16, 16).any(axis=(1, 3)).sum()
        assert tiles == items, tiles
    # one face among skipped ones, drawn into a 1 x 1 frame: one item, most waves have nothing to do
    faces = np.array([[0, 0, 1]] * 300 + [[0, 1, 2]] + [[2, 2, 1]] * 300, np.int32)
    want = _lib.coords_trimesh_host(small, attr, faces, (1, 1), origin=(5, 18), return_keys=True)
    got = ops.coords_trimesh(_dev(torch, small), _dev(torch, attr), _dev(torch, faces), (1, 1), origin=(5, 18), return_keys=True)
    assert _same(got, want) and int(want[1][0, 0]) & 0xffffffff == 300


# ---------------------------------------------------------------------------------------------- 5. coords.from_triangles on device tensors
def test_from_triangles_on_device_tensors(torch):
    from lerf_pytorch_amd import coords
    pos, attr, faces, depth = random_mesh()
    w = np.linspace(0.75, 1.5, len(pos))
    dev = lambda a: _dev(torch, a)
    got = coords.from_triangles(dev(pos), dev(attr), dev(faces), (29, 37), depth=dev(depth), w=dev(w), return_depth=True, return_faces=True)
    want = coords.from_triangles(pos, attr, faces, (29, 37), depth=depth, w=w, return_depth=True, return_faces=True)
    assert all(g.is_cuda for g in got) and got[0].dtype == torch.float64 and got[2].dtype == torch.int64
    assert R.same_bits(_np(got[0]), want[0]) and R.same_bits(_np(got[1]), want[1]) and np.array_equal(_np(got[2]), want[2])
    got = coords.from_triangles(dev(pos.astype(np.float32)), dev(attr), dev(faces.astype(np.int64)), (30, 44), orient=1, max_span=40, dtype=np.float32)
    want = coords.from_triangles(pos.astype(np.float32), attr, faces.astype(np.int64), (30, 44), orient=1, max_span=40, dtype=np.float32)
    assert got.dtype == torch.float32 and R.same_bits(_np(got), want)
    rng = np.random.default_rng(5)
    P = np.stack([pos, pos + rng.uniform(-2.0, 2.0, pos.shape), pos[::-1]])
    D = np.stack([depth, depth[::-1], depth])
    afaces = np.roll(faces, 1, axis=1)
    for kw in (dict(), dict(depth=D), dict(depth=D, attr_faces=afaces, w=np.stack([w, w[::-1], w]).astype(np.float32))):
        got = coords.from_triangles(dev(P), dev(attr), dev(faces), (30, 44), return_faces=True, **{k: dev(v) for k, v in kw.items()})
        want = coords.from_triangles(P, attr, faces, (30, 44), return_faces=True, **kw)
        assert tuple(got[0].shape) == (3, 30, 44, 2) and R.same_bits(_np(got[0]), want[0]) and np.array_equal(_np(got[1]), want[1])


# ---------------------------------------------------------------------------------------------- 6. end to end
def test_engine_remap_along_a_translation_mesh(torch):
    import lerf_pytorch_amd as L
    from lerf_pytorch_amd import coords
    hw = (32, 40)
    img = np.random.default_rng(0).integers(0, 256, hw + (3,), dtype=np.uint8)
    shift = np.array([2.5, -3.25])
    # an irregular mesh over rows 6 .. 25, columns 8 .. 33 of the output, which shows the source moved by `shift`
    pos = np.array([[6.0, 8.0], [6.0, 33.0], [25.0, 8.0], [25.0, 33.0], [14.3, 17.9], [9.1, 27.2], [20.6, 24.4]])
    faces = np.array([[0, 1, 5], [0, 5, 4], [0, 4, 2], [4, 5, 6], [1, 3, 5], [5, 3, 6], [4, 6, 2], [6, 3, 2]], np.int32)
    M = coords.from_triangles(_dev(torch, pos), _dev(torch, pos - shift), _dev(torch, faces), hw)
    nan = torch.isnan(M).any(dim=-1).cpu().numpy()
    inside = np.zeros(hw, bool)
    inside[6:26, 8:34] = True
    assert np.array_equal(nan, ~inside)                                  # watertight inside, nothing outside
    eng = L.LerfEngine.shipped("lerf-g")
    out, mask = eng.remap(img, M, border=0)
    assert out.shape == hw + (3,) and np.array_equal(~mask, np.broadcast_to(nan[..., None], mask.shape))
    assert not out[nan].any()
    ident = _identity(hw)
    moved, _ = eng.remap(img, _dev(torch, ident - shift), border=0)
    # dyadic positions and a dyadic shift: the interpolated attribute is the translation's map to the last bit or two
    assert np.abs(M.cpu().numpy()[inside] - (ident - shift)[inside]).max() < 1e-12
    assert np.array_equal(out[inside], moved[inside]) and out[inside].any()


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_ops_refusals_leave_out_and_keys_untouched(torch):
    from lerf_pytorch_amd import _lib, coords, ops
    pos, attr, faces, depth = (_dev(torch, a) for a in random_mesh())
    out = torch.full((6, 8, 2), -7.0, dtype=torch.float64, device="cuda")
    keys = torch.full((6, 8), 5, dtype=torch.int64, device="cuda")
    for kw in (dict(max_span=-1), dict(max_span=65537), dict(orient=2), dict(origin=(0, -1))):
        with pytest.raises(ValueError, match="lerf_coords_trimesh"):
            ops.coords_trimesh(pos, attr, faces, (6, 8), out=out, keys=keys, **kw)
    with pytest.raises(ValueError, match="lerf_coords_trimesh"):
        ops.coords_trimesh(out.reshape(-1, 2), attr, faces, (6, 8), out=out, keys=keys)      # out IS pos
    with pytest.raises(ValueError, match="keys"):
        ops.coords_trimesh(pos, attr, faces, (6, 8), out=out, keys=keys[:, :4])
    with pytest.raises(ValueError, match="depth"):
        ops.coords_trimesh(pos, attr, faces, (6, 8), out=out, keys=keys, depth=depth.double())
    with pytest.raises(ValueError, match="depth"):
        ops.coords_trimesh(pos, attr, faces, (6, 8), out=out, keys=keys, return_depth=True)
    with pytest.raises(ValueError, match="faces"):
        ops.coords_trimesh(pos, attr, faces.long(), (6, 8), out=out, keys=keys)
    with pytest.raises(ValueError, match="faces"):
        ops.coords_trimesh(pos, attr, faces.cpu(), (6, 8), out=out, keys=keys)
    with pytest.raises(_lib.LerfError, match="max_span"):
        ops.coords_trimesh(pos, attr, torch.zeros((33141, 3), dtype=torch.int32, device="cuda"), (2160, 3840))
    for a, d in ((pos, depth.cpu()), (pos.cpu(), depth)):
        with pytest.raises(ValueError, match="mixed"):
            coords.from_triangles(a, attr, faces, (6, 8), depth=d)
    with pytest.raises(ValueError, match="autograd"):
        coords.from_triangles(pos.clone().requires_grad_(True), attr, faces, (6, 8))
    assert bool((out == -7.0).all()) and bool((keys == 5).all())
