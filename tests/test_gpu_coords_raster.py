"""The rasterising inverse on the device (entry_kernel<KeyFillOp>, cell_kernel<RasterOp>, entry_kernel<ResolveOp> of
csrc/lerf_coords.hip behind ops.coords_invert_raster and coords.invert_raster):

  1. G and keys equal the host twin's BY INTEGER PATTERN on every map of the CPU file's items 2, 3 and 5, and on 23 x 31 and 70 x 130
     inputs (more than one 64-column and 4-row block in both passes, ragged last blocks): 5 x 67 and 1 x 1 tiles at origin (3, 7) in a
     strided out, every dtype mix, with and without depth, every orient, max_span 1, 4, 16, 64;
  2. the minifying noisy map, where many triangles contend for one pixel: the same bits in two runs and the host's bits;
  3. coords.invert_raster / invert_flow_raster on device tensors and a batch of 3 equal the numpy path;
  4. coords.invert from the rasterised start on the folded map: no NaN, the host path's bits;
  5. LerfEngine.remap along invert_flow_raster(flow, depth) of the two-layer flow: the mask is false exactly on the NaN entries and
     the landing zone holds what a remap by the block's pure translation holds.

No map is larger than 70 x 130 in or 96 x 160 out; the host twin is the reference throughout (tests/test_coords_raster_cpu.py ties
it to the independent restatement).
"""
import numpy as np
import pytest

import coords_ref as R
from test_coords_raster_cpu import BLOCK, CASES, _identity, _ij, fold_map, minify_map, raster_cases, two_layer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def _dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tdt(torch, dt):
    return torch.float32 if np.dtype(dt) == np.float32 else torch.float64


def _bits(t):
    """the integer pattern of a device result: float maps as uint32 / uint64, int64 keys as uint64"""
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else R.bits(a)


def _same(torch, got, want):
    (G, K), (Gh, Kh) = got, want
    assert G.is_cuda and K.is_cuda and K.dtype == torch.int64 and Kh.dtype == np.uint64
    return G.cpu().numpy().dtype == Gh.dtype and np.array_equal(_bits(G), R.bits(Gh)) and np.array_equal(_bits(K), Kh)


def _big_map(hw):
    """a stretch by 1.2 with a sinusoidal fold along the columns and a ripple along the rows, and a depth to go with it"""
    ii, jj = _ij(hw)
    F = np.stack([1.2 * ii + 1.5 * np.sin(jj / 9.0), 1.2 * jj + 4.5 * np.sin(jj / 2.5) + 0.5 * np.cos(ii / 3.0)], axis=-1)
    depth = (3.0 + np.sin(ii / 4.0 + jj / 7.0) + 0.25 * np.cos(jj * 1.7)).astype(np.float32)
    return F, depth


# ---------------------------------------------------------------------------------------------- 1. bit equality
@pytest.mark.parametrize("name", [c[0] for c in raster_cases()])
def test_raster_is_bit_equal_to_its_host_twin(torch, name):
    from lerf_pytorch_amd import _lib, ops
    F, hw, depth, span, orient = CASES[name]
    F = np.ascontiguousarray(F)
    host = _lib.coords_invert_raster_host(F, hw, depth=depth, max_span=span, orient=orient, return_keys=True)
    got = ops.coords_invert_raster(_dev(torch, F), hw, depth=_dev(torch, depth), max_span=span, orient=orient, return_keys=True)
    assert _same(torch, got, host)


@pytest.mark.parametrize("f_hw,hw", [((23, 31), (30, 40)), ((70, 130), (90, 160))])
def test_every_dtype_depth_orient_and_span(torch, f_hw, hw):
    from lerf_pytorch_amd import _lib, ops
    F, depth = _big_map(f_hw)
    dd = _dev(torch, depth)
    for fdt in (np.float64, np.float32):
        Ff = F.astype(fdt)
        Fd = _dev(torch, Ff)
        for odt in (np.float64, np.float32):
            for d in (None, depth):
                for orient in (-1, 0, 1):
                    for span in (1, 4, 16, 64):
                        host = _lib.coords_invert_raster_host(Ff, hw, depth=d, dtype=odt, max_span=span, orient=orient, return_keys=True)
                        got = ops.coords_invert_raster(Fd, hw, depth=None if d is None else dd, dtype=_tdt(torch, odt), max_span=span,
                                                       orient=orient, return_keys=True)
                        assert _same(torch, got, host), (fdt, odt, d is None, orient, span)
    holes = np.isnan(_lib.coords_invert_raster_host(F, hw, depth=depth)[..., 0]).mean()
    assert 0.0 < holes < 0.5                                          # the map covers most of the frame and not all of it
    assert ops.coords_invert_raster(_dev(torch, F.astype(np.float32)), hw).dtype == torch.float32      # the default dtype is f's


@pytest.mark.parametrize("f_hw,hw", [((23, 31), (30, 40)), ((70, 130), (90, 160))])
def test_strided_tiles_in_place(torch, f_hw, hw):
    from lerf_pytorch_amd import _lib, ops
    F, depth = _big_map(f_hw)
    whole, whole_k = _lib.coords_invert_raster_host(F, hw, depth=depth, max_span=16, return_keys=True)
    wf = torch.full((f_hw[0], f_hw[1] + 3, 2), float("nan"), dtype=torch.float64, device="cuda")
    wf[:, 2:f_hw[1] + 2] = _dev(torch, F)
    for dt in (np.float64, np.float32):
        for th, tw in ((5, 67), (1, 1)):
            if 7 + tw > hw[1]:
                tw = hw[1] - 7
            buf = torch.full((hw[0], hw[1] + 3, 2), -7.0, dtype=_tdt(torch, dt), device="cuda")
            keys = torch.full((th, tw), 5, dtype=torch.int64, device="cuda")
            view = buf[3:3 + th, 7:7 + tw]
            got, k = ops.coords_invert_raster(wf[:, 2:f_hw[1] + 2], (th, tw), depth=_dev(torch, depth), out=view, origin=(3, 7), keys=keys,
                                              return_keys=True)
            assert got is view and k is keys
            b = buf.cpu().numpy()
            assert R.same_bits(np.ascontiguousarray(b[3:3 + th, 7:7 + tw]), whole[3:3 + th, 7:7 + tw].astype(dt))
            assert np.array_equal(_bits(keys), whole_k[3:3 + th, 7:7 + tw])
            b[3:3 + th, 7:7 + tw] = -7.0
            assert (b == -7.0).all()


# ---------------------------------------------------------------------------------------------- 2. contention
def test_many_triangles_on_one_pixel_give_the_same_bits_every_run(torch):
    from lerf_pytorch_amd import _lib, ops
    F = np.ascontiguousarray(minify_map((70, 130)))
    depth = np.random.default_rng(5).uniform(1.0, 2.0, (70, 130)).astype(np.float32)
    Fd, dd = _dev(torch, F), _dev(torch, depth)
    for d, ddev in ((None, None), (depth, dd)):
        host = _lib.coords_invert_raster_host(F, (18, 33), depth=d, return_keys=True)
        a = ops.coords_invert_raster(Fd, (18, 33), depth=ddev, return_keys=True)
        b = ops.coords_invert_raster(Fd, (18, 33), depth=ddev, return_keys=True)
        assert _same(torch, a, host) and _same(torch, b, host)
        assert not np.isnan(host[0][1:-1, 1:-1]).any()                # some sixteen cells land on every pixel


# ---------------------------------------------------------------------------------------------- 3. coords.* on device tensors
def test_coords_invert_raster_on_device_tensors(torch):
    from lerf_pytorch_amd import coords
    flow, depth = two_layer()
    F = _identity((32, 40)) + flow
    got = coords.invert_raster(_dev(torch, F), (32, 40), depth=_dev(torch, depth), max_span=4)
    assert got.is_cuda and got.dtype == torch.float64 and R.same_bits(got.cpu().numpy(), coords.invert_raster(F, (32, 40), depth, 4))
    got = coords.invert_raster(_dev(torch, F), (30, 44), orient=1, dtype=np.float32)
    assert got.dtype == torch.float32 and R.same_bits(got.cpu().numpy(), coords.invert_raster(F, (30, 44), orient=1, dtype=np.float32))
    batch = np.stack([fold_map(), F, _identity((32, 40)) + np.array([1.0, 2.0])])
    depths = np.stack([depth, depth[::-1].copy(), depth])
    for d in (None, depths):
        got = coords.invert_raster(_dev(torch, batch), (30, 44), depth=_dev(torch, d), max_span=4)
        assert tuple(got.shape) == (3, 30, 44, 2)
        assert R.same_bits(got.cpu().numpy(), coords.invert_raster(batch, (30, 44), depth=d, max_span=4))
    for f in (flow, flow.astype(np.float32)):
        b = coords.invert_flow_raster(_dev(torch, f), _dev(torch, depth), max_span=4)
        assert b.is_cuda and R.same_bits(b.cpu().numpy(), coords.invert_flow_raster(f, depth, max_span=4))
    # refusals of the device forms
    dev = _dev(torch, F)
    for a, d in ((dev, depth), (F, _dev(torch, depth)), (torch.from_numpy(F), _dev(torch, depth))):
        with pytest.raises(ValueError, match="mixed"):
            coords.invert_raster(a, (32, 40), depth=d)
    with pytest.raises(ValueError, match="autograd"):
        coords.invert_raster(dev.clone().requires_grad_(True), (32, 40))
    with pytest.raises(ValueError, match="autograd"):
        coords.invert_flow_raster(_dev(torch, flow).requires_grad_(True))


def test_ops_refusals_leave_out_and_keys_untouched(torch):
    from lerf_pytorch_amd import ops
    f = torch.zeros((4, 5, 2), dtype=torch.float64, device="cuda")
    out = torch.full((6, 8, 2), -7.0, dtype=torch.float64, device="cuda")
    keys = torch.full((6, 8), 5, dtype=torch.int64, device="cuda")
    for kw in (dict(max_span=0), dict(max_span=65), dict(orient=2), dict(origin=(0, -1))):
        with pytest.raises(ValueError, match="lerf_coords_invert_raster"):
            ops.coords_invert_raster(f, (6, 8), out=out, keys=keys, **kw)
    with pytest.raises(ValueError, match="lerf_coords_invert_raster"):
        ops.coords_invert_raster(f[:1], (6, 8), out=out, keys=keys)
    with pytest.raises(ValueError, match="lerf_coords_invert_raster"):
        ops.coords_invert_raster(out, (6, 8), out=out, keys=keys)     # out IS f
    with pytest.raises(ValueError, match="keys"):
        ops.coords_invert_raster(f, (6, 8), out=out, keys=keys[:, :4])
    with pytest.raises(ValueError, match="depth"):
        ops.coords_invert_raster(f, (6, 8), out=out, keys=keys, depth=torch.ones((4, 5), dtype=torch.float64, device="cuda"))
    assert bool((out == -7.0).all()) and bool((keys == 5).all())


# ---------------------------------------------------------------------------------------------- 4. the start Newton's method lacks
def test_newton_from_the_rasterised_start_on_the_device(torch):
    from lerf_pytorch_amd import coords
    F, hw = fold_map(), (32, 40)
    Fd = _dev(torch, F)
    G = coords.invert(Fd, hw, init=coords.invert_raster(Fd, hw))
    assert G.is_cuda and not bool(torch.isnan(G).any())
    assert R.same_bits(G.cpu().numpy(), coords.invert(F, hw, init=coords.invert_raster(F, hw)))
    assert int(torch.isnan(coords.invert(Fd, hw)[..., 0]).sum()) == 288


# ---------------------------------------------------------------------------------------------- 5. end to end
def test_engine_remap_carries_a_frame_forward_along_its_flow(torch):
    import lerf_pytorch_amd as L
    from lerf_pytorch_amd import coords
    hw = (32, 40)
    img = np.random.default_rng(0).integers(0, 256, hw + (3,), dtype=np.uint8)
    flow, depth = two_layer(hw)
    ident = _dev(torch, _identity(hw))
    M = coords.invert_flow_raster(_dev(torch, flow), _dev(torch, depth), max_span=4) + ident
    nan = torch.isnan(M).any(dim=-1).cpu().numpy()
    assert int(nan.sum()) == 177
    eng = L.LerfEngine.shipped("lerf-g")
    # border=0: the white frame has no black rim, so the mask is false only where the remap reads no source at all
    out, mask = eng.remap(img, M, border=0)
    assert out.shape == hw + (3,) and np.array_equal(~mask, np.broadcast_to(nan[..., None], mask.shape))
    assert not out[nan].any()
    moved, _ = eng.remap(img, ident - _dev(torch, BLOCK), border=0)   # the whole frame by the block's translation
    zone = np.zeros(hw, bool)
    zone[12:21, 13:24] = True
    assert R.same_bits(M.cpu().numpy()[zone], (_identity(hw) - BLOCK)[zone])
    assert np.array_equal(out[zone], moved[zone]) and out[zone].any()
