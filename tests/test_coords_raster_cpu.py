"""CPU-only: the rasterising inverse's host twin (lerf_coords_invert_raster_host: raster_cell / raster_resolve of
csrc/lerf_coords_models.h in a row-major loop with a plain min) and coords.invert_raster / invert_flow_raster on numpy arrays.

  1. the two entry points are declared, listed and exported; the ABI version stays 7;
  2. exact cases: the identity, an integer shift, a dyadic stretch without a hole, a dyadic rotation that covers exactly its closed
     image (the closed image counted in exact rational arithmetic: 416 pixels -- the figure 413 of the issue that asked for this
     test is not the closed image's count under any reading of its matrix; the SET is what is asserted);
  3. the host twin equals the independent restatement (tests/coords_raster_ref.py) BIT FOR BIT in G and in keys: smooth maps, a fold,
     a two-layer flow with an occlusion (with and without depth, every max_span and orient), a minifying map with noise;
  4. the contract: the winning triangle's interpolant at G[q] returns q; the nearest layer wins and the disoccluded area stays
     empty; what invert cannot do on a folded map and what it can do from the rasterised start;
  5. special entries: NaN, +-inf and 1e300 in F and NaN in depth remove their triangles and nothing else; degenerate maps; 2 x 2 and
     1 x 1;
  6. tiles in place, every dtype mix, a batch, the flow round trip;
  7. every refused argument.
"""
import functools
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import coords_invert_ref as IR
import coords_raster_ref as RR
import coords_ref as R
from conftest import REPO

from lerf_pytorch_amd import _lib, coords

EINVAL = -1
NO_KEY = np.uint64(2 ** 64 - 1)
ROT = np.array([[0.75, -1.25], [1.25, 0.75]])
BLOCK, BG = np.array([3.5, 6.25]), np.array([-0.5, 0.75])


def _identity(hw):
    return coords.from_flow(np.zeros(tuple(hw) + (2,)))


def _ij(hw):
    return np.meshgrid(np.arange(hw[0], dtype=np.float64), np.arange(hw[1], dtype=np.float64), indexing="ij")


def smooth_map(a, hw=(24, 31)):
    ii, jj = _ij(hw)
    return np.stack([1.7 * ii + a * np.sin(jj / 5.0) * np.cos(ii / 7.0), 1.7 * jj + a * np.cos(jj / 6.0) * np.sin(ii / 4.0)], axis=-1)


def fold_map(hw=(32, 40)):
    """identity + (0, 4 sin(j / 2.5)): 28 % of the cells are reversed"""
    ii, jj = _ij(hw)
    return np.stack([ii, jj + 4.0 * np.sin(jj / 2.5)], axis=-1)


def two_layer(hw=(32, 40)):
    """(flow, depth): the background moves by BG at depth 5, a 10 x 12 block at rows 8..17, cols 6..17 by BLOCK at depth 1"""
    flow = np.zeros(tuple(hw) + (2,)) + BG
    depth = np.full(hw, 5.0, np.float32)
    flow[8:18, 6:18] = BLOCK
    depth[8:18, 6:18] = 1.0
    return flow, depth


def minify_map(hw=(64, 80)):
    rng = np.random.default_rng(7)
    return 0.25 * _identity(hw) + rng.uniform(-0.6, 0.6, tuple(hw) + (2,))


def rotation_map():
    return _identity((13, 17)) @ ROT.T + np.array([20.0, 0.0])


def special_cases():
    """name -> (F, out_hw, depth): entries that are not finite, degenerate maps, the smallest shapes"""
    base = smooth_map(0.8)
    hw = (40, 52)
    nan_block, infs, huge = base.copy(), base.copy(), base.copy()
    nan_block[5:9, 11:14] = np.nan
    nan_block[15, 20, 1] = np.nan
    infs[3, 4, 0], infs[10, 12, 1], infs[20, 30] = np.inf, -np.inf, (np.inf, -np.inf)
    huge[7, 7, 0], huge[12, 25, 1], huge[0, 0] = 1e300, -1e300, (1e300, 1e300)
    depth = (2.0 + np.cos(np.arange(24 * 31, dtype=np.float64)).reshape(24, 31)).astype(np.float32)
    nan_depth = depth.copy()
    nan_depth[6:8, 3:9] = np.nan
    nan_depth[18, 18] = np.nan
    return {"nan_block": (nan_block, hw, None), "infs": (infs, hw, None), "huge": (huge, hw, None), "nan_depth": (base, hw, nan_depth),
            "inf_depth": (base, hw, np.where(nan_depth != nan_depth, np.float32(np.inf), depth)),
            "constant": (np.full((6, 7, 2), 3.0), (8, 8), None), "collinear": (np.stack([_ij((6, 7))[1]] * 2, axis=-1), (8, 8), None),
            "two_by_two": (np.array([[[0.5, 0.25], [1.0, 6.5]], [[5.75, 0.0], [6.0, 7.0]]]), (8, 9), None),
            "one_pixel": (smooth_map(0.8), (1, 1), None)}


def raster_cases():
    """(name, F, out_hw, depth, max_span, orient) of items 2, 3 and 5: what the host twin, the restatement and the kernel agree on"""
    flow, depth = two_layer()
    two = _identity(flow.shape[:2]) + flow
    cases = [("identity", _identity((23, 31)), (23, 31), None, 16, 0),
             ("shift", _identity((24, 31)) + np.array([2.0, -3.0]), (24, 31), None, 16, 0),
             ("stretch", 1.5 * _identity((13, 17)), (19, 25), None, 16, 0),
             ("rotation", rotation_map(), (30, 28), None, 16, 0),
             ("smooth0.8", smooth_map(0.8), (40, 52), None, 16, 0), ("smooth2.0", smooth_map(2.0), (40, 52), None, 16, 0),
             ("fold", fold_map(), (32, 40), None, 16, 0),
             ("minify", minify_map(), (16, 20), None, 16, 0),
             ("minify_depth", minify_map(), (16, 20), np.random.default_rng(3).uniform(1.0, 2.0, (64, 80)).astype(np.float32), 16, 0)]
    for d in (None, depth):
        for span in (1, 4, 16, 64):
            for orient in (-1, 0, 1):
                cases.append(("two_layer%s_span%d_orient%d" % ("" if d is None else "_depth", span, orient), two, (32, 40), d, span, orient))
    for name, (F, hw, d) in special_cases().items():
        cases.append((name, F, hw, d, 16, 0))
    return cases


CASES = {c[0]: c[1:] for c in raster_cases()}


@functools.lru_cache(maxsize=None)
def restated(name):
    """(G, keys) of a case by the restatement: computed once, shared, left unchanged"""
    F, hw, depth, span, orient = CASES[name]
    G, K = RR.raster(F, hw, depth, span, orient)
    G.setflags(write=False), K.setflags(write=False)
    return G, K


def _host(name, **kw):
    F, hw, depth, span, orient = CASES[name]
    return _lib.coords_invert_raster_host(np.ascontiguousarray(F), hw, depth=depth, max_span=span, orient=orient, return_keys=True, **kw)


def _holes(G):
    nan = np.isnan(G)
    assert np.array_equal(nan[..., 0], nan[..., 1])
    return nan[..., 0]


def _ptr(a):
    return a.ctypes.data


# ---------------------------------------------------------------------------------------------- 1. exports
def test_exports_and_abi_version():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "lerf_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lerf_[a-z0-9_]+)\s*\(", src))
    for n in ("lerf_coords_invert_raster", "lerf_coords_invert_raster_host"):
        assert n in declared and n in _lib.EXPORTS and hasattr(_lib.lib(), n), n
    assert _lib.lib().lerf_abi_version() == 7


# ---------------------------------------------------------------------------------------------- 2. exact cases
def test_exact_cases():
    ident = _identity((23, 31))
    for got in (_host("identity")[0], coords.invert_raster(ident, (23, 31)), restated("identity")[0]):
        assert R.same_bits(got, ident)
    # F[i, j] = (i + 2, j - 3) on 24 x 31: q comes from q - (2, -3) where that is a vertex of F, from nowhere else: 128 holes
    G, K = _host("shift")
    u = _identity((24, 31)) - np.array([2.0, -3.0])
    inside = (u[..., 0] >= 0) & (u[..., 0] <= 23) & (u[..., 1] >= 0) & (u[..., 1] <= 30)
    assert R.same_bits(G, np.where(inside[..., None], u, np.nan)) and int(_holes(G).sum()) == 128
    assert np.array_equal(K == NO_KEY, ~inside)
    # 1.5 x identity, 13 x 17 -> 19 x 25: every pixel of the closed image is covered, vertices and shared edges included
    G, _ = _host("stretch")
    assert not _holes(G).any() and np.allclose(G, _identity((19, 25)) / 1.5, rtol=0, atol=1e-14)


def test_a_dyadic_rotation_covers_exactly_its_closed_image():
    """every number is dyadic, so the edge functions are exact and the covered set must be the closed image itself"""
    G, _ = _host("rotation")
    a, b, c, d = (Fraction(float(v)) for v in ROT.reshape(4))
    det = a * d - b * c
    closed = np.zeros((30, 28), bool)
    for r in range(30):
        for q in range(28):
            x, y = Fraction(r) - 20, Fraction(q)
            i, j = (d * x - b * y) / det, (-c * x + a * y) / det
            closed[r, q] = 0 <= i <= 12 and 0 <= j <= 16
    print("closed image: %d pixels, covered: %d" % (closed.sum(), (~_holes(G)).sum()))
    assert np.array_equal(~_holes(G), closed) and int(closed.sum()) == 416
    q = np.stack(_ij((30, 28)), axis=-1) - np.array([20.0, 0.0])
    want = q @ np.linalg.inv(ROT).T
    assert np.max(np.abs(G - want)[closed]) <= 1e-13


# ---------------------------------------------------------------------------------------------- 3. the restatement, bit for bit
@pytest.mark.parametrize("name", [c[0] for c in raster_cases()])
def test_host_twin_equals_the_restatement_bit_for_bit(name):
    G, K = _host(name)
    Gr, Kr = restated(name)
    assert K.dtype == np.uint64 and np.array_equal(K, Kr)
    assert R.same_bits(G, Gr)
    assert np.array_equal(_holes(G), K == NO_KEY)


@pytest.mark.parametrize("name", ["smooth0.8", "smooth2.0"])
def test_a_smooth_map_leaves_no_hole_inside(name):
    assert not _holes(_host(name)[0])[3:-4, 3:-4].any()


# ---------------------------------------------------------------------------------------------- 4. the contract
@pytest.mark.parametrize("name", ["smooth0.8", "smooth2.0", "fold", "minify", "minify_depth", "two_layer_depth_span4_orient0", "rotation"])
def test_the_winning_triangle_maps_the_entry_back_onto_its_pixel(name):
    """T_t(G[q]) = q within 1e-12 max(|q|, 1), t the triangle the key names (the restatement's worst is a few 1e-15)"""
    F = CASES[name][0]
    G, K = _host(name)
    worst = 0.0
    for r, c in zip(*np.nonzero(K != NO_KEY)):
        back = RR.tri_sample(F, int(K[r, c]) & 0xFFFFFFFF, G[r, c])
        for got, q in zip(back, (r, c)):
            worst = max(worst, abs(got - q) / max(abs(q), 1.0))
    print("%s: worst relative residual %.3g" % (name, worst))
    assert worst <= 1e-12


def test_the_nearest_layer_wins_and_the_disoccluded_area_stays_empty():
    flow, depth = two_layer()
    b = coords.invert_flow_raster(flow, depth, max_span=4)
    G = b + _identity((32, 40))
    q = _identity((32, 40))
    from_block, from_bg, holes = np.all(G == q - BLOCK, axis=-1), np.all(G == q - BG, axis=-1), _holes(G)
    zone = np.zeros((32, 40), bool)
    zone[12:21, 13:24] = True                                         # the integer pixels inside the block's landing zone
    assert np.array_equal(from_block, zone) and int(zone.sum()) == 99
    assert int(from_bg.sum()) == 1004 and int(holes.sum()) == 177
    assert (from_block | from_bg | holes).all()
    assert R.same_bits(G, _host("two_layer_depth_span4_orient0")[0])


def test_newton_finishes_from_the_rasterised_start_on_a_folded_map():
    F, hw = fold_map(), (32, 40)
    assert int(np.isnan(IR.invert(F, hw)[..., 0]).sum()) == 288          # what Newton's method alone leaves
    G0 = coords.invert_raster(F, hw)
    assert not np.isnan(G0).any()
    G = coords.invert(F, hw, init=G0)
    assert not np.isnan(G).any()
    back = _lib.coords_compose_host(np.ascontiguousarray(F), G)
    assert np.max(np.abs(back - _identity(hw))) <= 1e-9


# ---------------------------------------------------------------------------------------------- 5. special entries
@pytest.mark.parametrize("name", ["nan_block", "infs", "huge", "nan_depth"])
def test_an_entry_that_is_not_finite_removes_its_triangles_only(name):
    F, hw, depth, span, orient = CASES[name]
    clean_depth = None if depth is None else np.where(depth != depth, np.float32(2.0), depth)
    Gc, Kc = _lib.coords_invert_raster_host(smooth_map(0.8), hw, depth=clean_depth, return_keys=True)
    G, K = _host(name)
    with np.errstate(invalid="ignore"):                                # 1e300 is finite: its triangles go by the tear rule
        bad = ~(np.abs(F) < 1e100).all(axis=-1) if depth is None else np.isnan(depth)
    fW = F.shape[1]
    removed = np.zeros(2 * (F.shape[0] - 1) * (fW - 1), bool)
    for t in range(removed.size):
        removed[t] = any(bad[v] for v in RR.tri_vertices(t, fW))
    assert removed.any() and not removed.all()
    kept = (Kc != NO_KEY) & ~removed[(Kc & np.uint64(0xFFFFFFFF)).astype(np.int64) * (Kc != NO_KEY)]
    assert np.array_equal(K[kept], Kc[kept]) and R.same_bits(G[kept], Gc[kept])          # an intact winner stays the winner
    won = (K & np.uint64(0xFFFFFFFF)).astype(np.int64)[K != NO_KEY]
    assert not removed[won].any()                                                           # no removed triangle wins anywhere
    assert (K[(Kc == NO_KEY)] == NO_KEY).all() and (K != NO_KEY).sum() < (Kc != NO_KEY).sum()
    assert np.isfinite(G[K != NO_KEY]).all()


def test_degenerate_maps_and_the_smallest_shapes():
    for name in ("constant", "collinear"):
        G, K = _host(name)
        assert np.isnan(G).all() and (K == NO_KEY).all()
    G, K = _host("two_by_two")
    assert set(np.unique(K[K != NO_KEY]) & np.uint64(0xFFFFFFFF)) == {0, 1} and (K == NO_KEY).any()
    G, K = _host("one_pixel")
    assert G.shape == (1, 1, 2) and R.same_bits(G, np.zeros((1, 1, 2))) and int(K[0, 0]) == 0x80000000 << 32


# ---------------------------------------------------------------------------------------------- 6. tiles, dtypes, batches, flows
@pytest.mark.parametrize("name", ["smooth2.0", "two_layer_depth_span4_orient0"])
def test_a_tile_written_in_place_equals_the_slice_of_the_whole(name):
    F, hw, depth, span, orient = CASES[name]
    G, K = _host(name)
    for (i0, j0), (th, tw) in (((5, 9), (11, 23)), ((5, 9), (1, 1)), ((0, 0), hw)):
        whole = np.full(tuple(hw) + (2,), -7.0)
        view = whole[i0:i0 + th, j0:j0 + tw]
        got, keys = _lib.coords_invert_raster_host(np.ascontiguousarray(F), (th, tw), depth=depth, out=view, origin=(i0, j0), max_span=span,
                                                   orient=orient, return_keys=True)
        assert got is view and R.same_bits(view, G[i0:i0 + th, j0:j0 + tw]) and np.array_equal(keys, K[i0:i0 + th, j0:j0 + tw])
        pad = np.ones(hw, bool)
        pad[i0:i0 + th, j0:j0 + tw] = False
        assert (whole[pad] == -7.0).all()


@pytest.mark.parametrize("f_dt", [np.float32, np.float64])
@pytest.mark.parametrize("o_dt", [np.float32, np.float64])
def test_every_dtype_mix(f_dt, o_dt):
    flow, depth = two_layer()
    for F, hw, d, span in ((smooth_map(2.0).astype(f_dt), (40, 52), None, 16), ((_identity((32, 40)) + flow).astype(f_dt), (32, 40), depth, 4)):
        wide = np.zeros((F.shape[0], F.shape[1] + 3, 2), f_dt)           # F as a view with a row stride of its own
        wide[:, :F.shape[1]] = F
        G, K = _lib.coords_invert_raster_host(wide[:, :F.shape[1]], hw, depth=d, dtype=o_dt, max_span=span, return_keys=True)
        Gr, Kr = RR.raster(F, hw, d, span)
        assert G.dtype == o_dt and np.array_equal(K, Kr) and R.same_bits(G, Gr.astype(o_dt))


def test_a_batch_equals_single_calls():
    flow, depth = two_layer()
    maps = np.stack([fold_map(), _identity((32, 40)) + flow, _identity((32, 40)) + np.array([1.0, 2.0])])
    depths = np.stack([depth, depth[::-1].copy(), depth])
    for d in (None, depths):
        G = coords.invert_raster(maps, (30, 44), depth=d, max_span=4, orient=0, dtype=np.float32)
        assert G.shape == (3, 30, 44, 2) and G.dtype == np.float32
        for n in range(3):
            one = coords.invert_raster(maps[n], (30, 44), depth=None if d is None else d[n], max_span=4, dtype=np.float32)
            assert R.same_bits(G[n], one)
    assert R.same_bits(coords.invert_raster(maps[0], (30, 44), depth=depth.astype(np.float64)), coords.invert_raster(maps[0], (30, 44), depth=depth))


def test_invert_flow_raster_round_trip():
    ident = _identity((24, 31))
    b = coords.invert_flow_raster(np.zeros((24, 31, 2)) + np.array([2.0, -3.0]))
    assert int(_holes(b).sum()) == 128 and (b[~_holes(b)] == np.array([-2.0, 3.0])).all()
    ii, jj = _ij((24, 31))
    flow = np.stack([1.5 * np.sin(jj / 6.0), 1.25 * np.cos(ii / 5.0)], axis=-1)
    b = coords.invert_flow_raster(flow, max_span=8, orient=1)
    assert R.same_bits(b, coords.invert_raster(ident + flow, (24, 31), max_span=8, orient=1) - ident)
    ok = ~_holes(b)
    assert ok[3:-3, 3:-3].all()
    # forward along the flow from where the backward flow points: back at the pixel (the two interpolants differ by O(h^2 f''))
    back = _lib.coords_compose_host(np.ascontiguousarray(ident + flow), np.ascontiguousarray(ident + b))
    assert np.max(np.abs(back - ident)[ok]) <= 0.05
    f32 = coords.invert_flow_raster(flow.astype(np.float32))
    assert f32.dtype == np.float32 and f32.shape == (24, 31, 2)


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_every_refused_argument_returns_einval_and_writes_nothing():
    lib = _lib.lib()
    F64, F32 = _lib.LERF_F64, _lib.LERF_F32
    f = np.ascontiguousarray(_identity((4, 5)))
    dep = np.ones((4, 5), np.float32)
    out = np.full((6, 8, 2), -7.0)
    keys = np.full((6, 8), 5, np.uint64)
    big = np.full((12, 8, 2), -7.0)                                   # two operands inside one buffer

    def ras(Fm=f, fdt=F64, sf=10, fH=4, fW=5, D=dep, o=out, dt=F64, so=16, oH=6, oW=8, i0=0, j0=0, span=16, orient=0, K=keys, foff=0, doff=0,
            off=0, koff=0, host=True):
        args = (None if Fm is None else _ptr(Fm) + foff, fdt, sf, fH, fW, None if D is None else _ptr(D) + doff, None if o is None else _ptr(o) + off,
                dt, so, oH, oW, i0, j0, span, orient, None if K is None else _ptr(K) + koff)
        return lib.lerf_coords_invert_raster_host(*args) if host else lib.lerf_coords_invert_raster(*args, None)
    assert ras() == 0 and ras(D=None) == 0
    out[:] = -7.0
    keys[:] = 5
    for host in (True, False):                                        # the device entry point refuses before it touches the GPU
        calls = [ras(Fm=None, host=host), ras(o=None, host=host), ras(K=None, host=host), ras(fdt=0, host=host), ras(dt=9, host=host),
                 ras(sf=9, host=host), ras(sf=8, host=host), ras(so=15, host=host), ras(so=14, host=host), ras(fH=1, host=host),
                 ras(fW=1, host=host), ras(fH=0, host=host), ras(oH=0, host=host), ras(oW=0, host=host), ras(oH=-1, host=host),
                 ras(foff=8, host=host), ras(off=8, host=host), ras(koff=4, host=host), ras(doff=2, host=host),
                 ras(span=0, host=host), ras(span=65, host=host), ras(span=-1, host=host), ras(orient=2, host=host), ras(orient=-2, host=host),
                 ras(i0=-1, host=host), ras(j0=-1, host=host), ras(i0=2 ** 31 - 3, host=host),
                 ras(fH=2 ** 16 + 1, fW=2 ** 15 + 1, sf=2 ** 16 + 2, host=host),                  # 2^32 triangles
                 ras(o=f, oH=4, oW=5, so=10, host=host),                                          # out IS f
                 ras(K=f, oH=4, oW=5, host=host),                                                 # keys inside f
                 ras(K=out, host=host),                                                           # keys inside out
                 ras(o=dep, dt=F32, oH=2, oW=5, so=10, host=host),                                # out IS depth
                 ras(K=dep, oH=2, oW=5, host=host),                                               # keys inside depth
                 ras(Fm=big, o=big, off=16 * 8 * 3, sf=16, host=host)]                            # out begins inside f's rows
        assert calls == [EINVAL] * len(calls), (host, calls)
    assert (out == -7.0).all() and (big == -7.0).all() and (keys == 5).all() and (dep == 1.0).all() and R.same_bits(f, _identity((4, 5)))
    # side by side in one buffer without sharing a byte: accepted
    assert ras(Fm=big, o=big, off=16 * 8 * 6, sf=16) == 0
    assert (big[:6] == -7.0).all() and not (big[6:] == -7.0).any()
    # through the Python layer: a ValueError that names the entry point
    with pytest.raises(ValueError, match="lerf_coords_invert_raster_host"):
        _lib.coords_invert_raster_host(f, (6, 8), max_span=0)
    with pytest.raises(ValueError, match="lerf_coords_invert_raster_host"):
        _lib.coords_invert_raster_host(f, (6, 8), orient=3)
    with pytest.raises(ValueError, match="depth"):
        _lib.coords_invert_raster_host(f, (6, 8), depth=np.ones((4, 5)))
    with pytest.raises(ValueError, match="keys"):
        _lib.coords_invert_raster_host(f, (6, 8), keys=np.zeros((6, 8), np.int64))
    with pytest.raises(ValueError):
        _lib.coords_invert_raster_host(f[:, :1], (6, 8))


def test_invert_raster_refuses_mixed_operands_and_autograd():
    import torch
    f = _identity((4, 5))

    class Dev:                                                        # stands for a device tensor: invert_raster looks at is_cuda
        is_cuda, ndim, shape, requires_grad = True, 2, (4, 5), False
    with pytest.raises(ValueError, match="mixed"):
        coords.invert_raster(f, (4, 5), depth=Dev())
    leaf = torch.from_numpy(f).requires_grad_(True)
    with pytest.raises(ValueError, match="autograd"):
        coords.invert_raster(leaf, (4, 5))
    with pytest.raises(ValueError, match="autograd"):
        coords.invert_raster(f, (4, 5), depth=torch.ones((4, 5), requires_grad=True))
    with pytest.raises(ValueError, match="autograd"):
        coords.invert_flow_raster(leaf)
    with torch.no_grad():
        assert R.same_bits(coords.invert_raster(leaf, (4, 5)), f)
    for bad in (lambda: coords.invert_raster(f, (0, 5)), lambda: coords.invert_raster(f[0], (4, 5)),
                lambda: coords.invert_raster(f, (4, 5), depth=np.ones((4, 4))), lambda: coords.invert_raster(np.stack([f, f]), (4, 5), depth=np.ones((4, 5))),
                lambda: coords.invert_flow_raster(np.zeros((4, 5)))):
        with pytest.raises(ValueError):
            bad()
