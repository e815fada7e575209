"""CPU-only: one coordinate map per sample -- the C ABI surface of lerf_remap_batched / lerf_remap_packed_batched /
lerf_remap_bwd_batched and their host-side refusals, ops.RemapGeometry on a [B, oH, oW, 2] map against the single-map
geometries and the numpy restatement, and the batched map builders of coords.py (from_flow, from_flow_torch,
from_grid_sample).

The three maps of the batch are chosen so that their derived low pads DIFFER inside the batch (asserted below): a batched
call that takes its pads, or anything else, from map 0 cannot pass."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO

import lerf_pytorch_amd as L
from lerf_pytorch_amd import _lib, coords, ops

import remap_ref

IN_HW, OUT_HW = (40, 48), (33, 37)
NEW = ["lerf_remap_batched", "lerf_remap_packed_batched", "lerf_remap_bwd_batched"]
EINVAL = -1
PADS = {2: [(1, 0), (1, 0), (0, 0)], 4: [(2, 0), (2, 1), (0, 0)]}      # S -> low pads of (sinus, folded, scatter)


def scatter(in_hw=IN_HW, out_hw=OUT_HW, seed=9):
    """the seeded scatter of tests/test_gpu_remap_grad.py (uniform over [-3, H + 3] x [-3, W + 3])"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-3, in_hw[0] + 3, out_hw), rng.uniform(-3, in_hw[1] + 3, out_hw)], axis=-1)


def maps3(scatter_first=False):
    m = [remap_ref.sinus_flow(IN_HW, OUT_HW), remap_ref.folded(IN_HW, OUT_HW), scatter()]
    return np.ascontiguousarray(np.stack(m[2:] + m[:2] if scatter_first else m))


def test_batched_symbols_declared_exported_and_resolve():
    src = open(os.path.join(REPO, "include", "lerf_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(lerf_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(L.LIB_PATH)
    for n in NEW:
        assert n in declared, "%s is not declared in include/lerf_hip.h" % n
        assert n in _lib.EXPORTS
        assert hasattr(lib, n), "liblerf_hip.so does not export %s" % n
        assert getattr(_lib.lib(), n).argtypes
    assert lib.lerf_abi_version() == 7
    assert ctypes.sizeof(_lib.RemapGeo) == 56


@pytest.mark.parametrize("scatter_first", [False, True])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("S", [1, 2, 4])
def test_batched_geometry_is_the_single_map_geometries(S, dtype, scatter_first):
    cm = maps3(scatter_first).astype(dtype)
    geo = ops.RemapGeometry(IN_HW, cm, S)
    assert geo.batched and geo.n_maps == 3 and geo.out_hw == OUT_HW
    got, pads = geo.host_geometry(), geo.pads()
    assert pads.shape == (3, 2) and np.array_equal(got[4], pads)
    for b in range(3):
        one = ops.RemapGeometry(IN_HW, cm[b], S)
        assert not one.batched and one.n_maps == 1
        ref = remap_ref.map_geometry(cm[b], IN_HW, OUT_HW, S)
        hg = one.host_geometry()
        for k, name in enumerate(("gx", "gy", "lx", "ly")):
            assert got[k][b].dtype == hg[k].dtype and np.array_equal(got[k][b], hg[k])      # bit-equal float64 / int32
            assert np.array_equal(got[k][b], ref[name])
        assert tuple(pads[b]) == one.pads() == hg[4] == (ref["pad"][0], ref["pad"][2])
    if S in PADS:                                              # the pads differ inside the batch: map 0's are not the others'
        want = PADS[S][2:] + PADS[S][:2] if scatter_first else PADS[S]
        assert [tuple(p) for p in pads] == want
    with pytest.raises(ValueError, match="rows"):
        geo.rows(0, 4)
    # explicit pads apply to every map
    ex = ops.RemapGeometry(IN_HW, cm, S, pads=(1, 0))
    assert np.array_equal(ex.pads(), [[1, 0]] * 3) and np.array_equal(ex.host_geometry()[4], [[1, 0]] * 3)
    assert np.array_equal(ex.host_geometry()[0][2], ops.RemapGeometry(IN_HW, cm[2], S, pads=(1, 0)).host_geometry()[0])


def test_a_3d_map_is_unchanged():
    cm = remap_ref.sinus_flow(IN_HW, OUT_HW)
    geo = ops.RemapGeometry(IN_HW, cm, 2)
    assert not geo.batched and geo.n_maps == 1 and geo.pads() == (1, 0)
    assert isinstance(geo.pads(), tuple) and geo.host_geometry()[0].shape == OUT_HW
    assert geo.rows(3, 9).out_hw == (6, OUT_HW[1])
    one = ops.RemapGeometry(IN_HW, cm[None], 2)                # [1, oH, oW, 2] is a batch of one
    assert one.batched and one.n_maps == 1 and one.pads().shape == (1, 2)
    for bad in (np.zeros((2, 3)), np.zeros((2, 2, 3, 4, 2)), np.zeros((0, 3, 4, 2)), np.zeros((2, 3, 4, 3))):
        with pytest.raises(ValueError):
            ops.RemapGeometry(IN_HW, bad, 2)


# ---------------------------------------------------------------------------------------------- host-side refusals, no GPU
def _geo(cm, S=2):
    g = _lib.RemapGeo()
    g.S, g.out_h, g.out_w = S, cm.shape[1], cm.shape[2]
    g.coords, g.coords_dtype, g.row_stride = cm.ctypes.data, _lib.LERF_F64, 2 * cm.shape[2]
    g.pad_r_lo = g.pad_c_lo = _lib.REMAP_PADS_FROM_MAP
    return g


def test_batched_entry_points_refuse_on_the_host():
    """every refusal comes before anything is launched: the pointers below are HOST memory and there is no GPU here, so a call
    that got past its checks would not return LERF_EINVAL"""
    lib = _lib.lib()
    cm = maps3()
    oH, oW = OUT_HW
    stride = cm.strides[0] // 8
    assert stride == oH * 2 * oW
    buf = np.zeros(6 * IN_HW[0] * IN_HW[1], np.float32)
    big = np.zeros(6 * oH * oW * 2, np.float64)
    P = _lib.Plane
    p = lambda a: ctypes.c_void_p(a.ctypes.data)

    def planar(n_maps=3, map_stride=stride, ppm=2, planes=6, **fields):
        g = _geo(cm)
        for k, v in fields.items():
            setattr(g, k, v)
        pf = P(buf.ctypes.data, _lib.LERF_F32, IN_HW[1], 1, IN_HW[0] * IN_HW[1])
        ph = (P * 3)(pf, pf, pf)
        po = P(big.ctypes.data, _lib.LERF_F64, oW, 1, oH * oW)
        return lib.lerf_remap_batched(ctypes.byref(pf), ph, IN_HW[0], IN_HW[1], planes, ctypes.byref(g), n_maps, map_stride, ppm,
                                      _lib.KINDS["gauss"], 10.0, ctypes.byref(po), None)

    def packed(n_maps=3, map_stride=stride, n=3, **fields):
        g = _geo(cm)
        for k, v in fields.items():
            setattr(g, k, v)
        po = P(big.ctypes.data, _lib.LERF_F32, oW * 3, 3, 1)
        return lib.lerf_remap_packed_batched(p(buf), IN_HW[0] * IN_HW[1] * 3, n, IN_HW[0], IN_HW[1], 3, ctypes.byref(g), n_maps,
                                             map_stride, _lib.KINDS["gauss"], 10.0, ctypes.byref(po), oH * oW * 3, None)

    def bwd(n_maps=3, map_stride=stride, ppm=2, N=6, **fields):
        g = _geo(cm)
        for k, v in fields.items():
            setattr(g, k, v)
        return lib.lerf_remap_bwd_batched(p(buf), p(buf), p(buf), p(buf), N, IN_HW[0], IN_HW[1], ctypes.byref(g), n_maps, map_stride, ppm,
                                          _lib.KINDS["gauss"], 10.0, p(big), p(buf), None, None, None, p(big), None)

    extent = (oH - 1) * 2 * oW + 2 * oW
    for call in (planar, packed, bwd):
        assert call(n_maps=0) == EINVAL and call(n_maps=-1) == EINVAL
        assert call(map_stride=stride + 1) == EINVAL                     # odd: breaks the entry alignment of map 1
        assert call(map_stride=extent - 2) == EINVAL                     # maps overlap
        assert call(map_stride=0) == EINVAL and call(map_stride=-stride) == EINVAL
        assert call(coords=None) == EINVAL and call(row_stride=2 * oW + 1) == EINVAL     # what the plain entry points refuse
    # one map with matching counts: an odd stride is still refused
    assert planar(n_maps=1, ppm=6, map_stride=stride + 1) == EINVAL and bwd(n_maps=1, ppm=6, map_stride=stride + 1) == EINVAL
    assert packed(n_maps=1, n=1, map_stride=stride + 1) == EINVAL
    # a strided batch needs a stride of the strided extent
    assert planar(row_stride=2 * oW + 4, map_stride=extent) == EINVAL
    # plane / frame counts that n_maps does not divide, or that do not equal n_maps * planes per map
    assert planar(planes=7) == EINVAL and planar(planes=6, ppm=3) == EINVAL and planar(planes=4, ppm=2) == EINVAL
    assert planar(ppm=0) == EINVAL
    assert bwd(N=7) == EINVAL and bwd(N=6, ppm=3) == EINVAL and bwd(ppm=0) == EINVAL
    assert packed(n=2) == EINVAL and packed(n=6) == EINVAL and packed(n_maps=2) == EINVAL
    assert not buf.any() and not big.any()


def test_shape_mismatches_raise_value_error():
    """what can be refused without a GPU (the ops-level plane and frame counts need device operands: test_gpu_remap_batch.py)"""
    pytest.importorskip("torch")
    from lerf_pytorch_amd.resize_right import resize_right2d_torch as T
    w = T.NearestRemap2dTorch()
    with pytest.raises(ValueError, match="one map per sample"):
        w.set_shape([2, 2] + list(IN_HW), maps3())             # 3 maps for a batch of 2
    w.set_shape([3, 2] + list(IN_HW), maps3())
    assert w.out_shape == [3, 2] + list(OUT_HW) and w.geo.n_maps == 3
    w.set_shape([5, 2] + list(IN_HW), maps3()[0])              # a 3-D map serves any batch, as before
    assert w.out_shape == [5, 2] + list(OUT_HW) and not w.geo.batched
    geo = ops.RemapGeometry(IN_HW, maps3(), 2)
    with pytest.raises(ValueError, match="no batch stride"):
        ops.RemapGeometry(IN_HW, maps3()[0], 2).map_stride("cuda:0")
    assert geo.n_maps == 3


# ---------------------------------------------------------------------------------------------- map builders
def test_from_flow_of_a_batched_zero_flow_is_b_identity_grids():
    torch = pytest.importorskip("torch")
    ii, jj = np.meshgrid(np.arange(5), np.arange(7), indexing="ij")
    ident = np.stack([ii, jj], axis=-1).astype(np.float64)
    got = coords.from_flow(np.zeros((3, 5, 7, 2)))
    assert got.shape == (3, 5, 7, 2) and got.dtype == np.float64 and all(np.array_equal(g, ident) for g in got)
    assert np.array_equal(coords.from_flow(np.zeros((5, 7, 2))), ident)
    for dt in (torch.float32, torch.float64):
        t = coords.from_flow_torch(torch.zeros((3, 5, 7, 2), dtype=dt))
        assert t.dtype == dt and tuple(t.shape) == (3, 5, 7, 2) and all(np.array_equal(g.numpy(), ident) for g in t)
    f = torch.full((2, 5, 7, 2), 0.25, dtype=torch.float64, requires_grad=True)
    (coords.from_flow_torch(f) * 2).sum().backward()
    assert tuple(f.grad.shape) == (2, 5, 7, 2) and bool((f.grad == 2).all())
    assert np.array_equal(coords.from_flow_torch(f).detach().numpy(), coords.from_flow(f))
    for bad in (np.zeros((5, 7)), np.zeros((1, 2, 5, 7, 2)), np.zeros((5, 7, 3))):
        with pytest.raises(ValueError):
            coords.from_flow(bad)
        with pytest.raises(ValueError):
            coords.from_flow_torch(torch.from_numpy(bad))


@pytest.mark.parametrize("align", [True, False])
def test_from_grid_sample(align):
    torch = pytest.importorskip("torch")
    H, W = 11, 7
    # (x, y) = corners and one interior value: x = 0.5 -> col, y = -0.2 -> row
    grid = torch.tensor([[[[-1.0, -1.0], [1.0, 1.0]], [[0.5, -0.2], [-1.0, 1.0]]]], dtype=torch.float64).repeat(2, 1, 1, 1)
    grid.requires_grad_(True)
    cm = coords.from_grid_sample(grid, (H, W), align_corners=align)
    assert tuple(cm.shape) == (2, 2, 2, 2) and cm.dtype == torch.float64 and cm.requires_grad
    lo_r, hi_r, lo_c, hi_c = (0.0, H - 1.0, 0.0, W - 1.0) if align else (-0.5, H - 0.5, -0.5, W - 0.5)
    got = cm.detach().numpy()
    assert np.array_equal(got[0], got[1])
    assert tuple(got[0, 0, 0]) == (lo_r, lo_c) and tuple(got[0, 0, 1]) == (hi_r, hi_c)            # exact in float64
    assert tuple(got[0, 1, 1]) == (hi_r, lo_c)                                                    # (x, y) -> (row, col)
    want = ((-0.2 + 1) / 2 * (H - 1), (0.5 + 1) / 2 * (W - 1)) if align else (((-0.2 + 1) * H - 1) / 2, ((0.5 + 1) * W - 1) / 2)
    np.testing.assert_allclose(got[0, 1, 0], want, rtol=0, atol=4 * np.finfo(np.float64).eps * max(H, W))
    # gradient flow on the CPU: d row / d y and d col / d x are the constant scale factors, nothing crosses
    (cm[..., 0].sum() * 3 + cm[..., 1].sum() * 5).backward()
    sy, sx = ((H - 1) / 2, (W - 1) / 2) if align else (H / 2, W / 2)
    np.testing.assert_allclose(grid.grad[..., 1].numpy(), 3 * sy, rtol=1e-15)
    np.testing.assert_allclose(grid.grad[..., 0].numpy(), 5 * sx, rtol=1e-15)
    # the pixel grid of F.grid_sample's own convention comes back as the identity map
    ii = torch.arange(H, dtype=torch.float64)
    y = ii / (H - 1) * 2 - 1 if align else (2 * ii + 1) / H - 1
    g = torch.stack([torch.zeros(H, dtype=torch.float64), y], dim=-1)[None, :, None]
    np.testing.assert_allclose(coords.from_grid_sample(g, (H, W), align)[0, :, 0, 0].numpy(), np.arange(H), rtol=0, atol=1e-13)
    # 3-D grid, float32, refusals
    assert tuple(coords.from_grid_sample(grid[0].detach().float(), (H, W), align).shape) == (2, 2, 2)
    for bad in (grid.detach().numpy(), torch.zeros((2, 2)), torch.zeros((2, 2, 3)), torch.zeros((2, 2, 2), dtype=torch.int32)):
        with pytest.raises(ValueError):
            coords.from_grid_sample(bad, (H, W), align)
    with pytest.raises(ValueError):
        coords.from_grid_sample(grid, (0, W), align)
