"""CPU-only: the coordinate-map builders' host twins (lerf_coords_build_host, lerf_coords_mesh_host, lerf_coords_compose_host)
-- the kernels' own arithmetic (csrc/lerf_coords_models.h) in a plain loop -- against coords.py's numpy builders and the
restatements of tests/coords_ref.py, bit for bit where the contract says so; the restatements anchored on independent ground
first; every refused argument."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import coords_ref as R
from conftest import REPO

from lerf_pytorch_amd import _lib, coords

HWS = [(37, 53), (1, 9)]
NEW = ["lerf_coords_build", "lerf_coords_build_host", "lerf_coords_mesh", "lerf_coords_mesh_host", "lerf_coords_mesh_bwd",
       "lerf_coords_mesh_bwd_workspace_bytes", "lerf_coords_compose", "lerf_coords_compose_host"]
K0 = np.array([[61.5, 0.0, 25.25], [0.0, 58.75, 17.5], [0.0, 0.0, 1.0]])
DIST8 = [0.11, -0.04, 0.002, -0.003, 0.013, 0.02, -0.007, 0.001]
EINVAL = -1


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    return np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ \
        np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])


def _anchor(got, ref, tol=1e-12):
    bound = tol * max(1.0, float(np.max(np.abs(ref))))
    err = float(np.max(np.abs(got - ref)))
    print("max error %.3g, bound %.3g" % (err, bound))
    assert err <= bound


def test_exports_and_abi():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "lerf_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lerf_[a-z0-9_]+)\s*\(", src))
    lib = _lib.lib()
    for n in NEW:
        assert n in declared and n in _lib.EXPORTS and hasattr(lib, n), n
    assert lib.lerf_abi_version() == 7


# ---------------------------------------------------------------------------------------------- models
def _matrices(golden):
    g = golden("g4_warp.npz")
    rng = np.random.default_rng(3)
    rnd = np.eye(3) + rng.normal(0, 0.05, (3, 3)) * np.array([[1, 1, 20], [1, 1, 20], [1e-4, 1e-4, 0]])
    return [g["isc/matrix"], g["osc/matrix"], rnd]


@pytest.mark.parametrize("hw", HWS)
def test_homography_is_bit_equal_to_from_homography(golden, hw):
    for M in _matrices(golden):
        ref = coords.from_homography(M, hw, arithmetic="device")
        got = _lib.coords_build_host("homography", np.linalg.inv(M).reshape(9), hw)
        assert R.same_bits(got, ref)
        assert R.same_bits(coords.from_homography(M, hw, dtype=np.float32), ref.astype(np.float32))
        assert R.same_bits(_lib.coords_build_host("homography", np.linalg.inv(M).reshape(9), hw, np.float32), ref.astype(np.float32))


def _radial_params(in_hw, out_hw, k1, k2, centre):
    (H, W), (oH, oW) = in_hw, out_hw
    return [centre[0], centre[1], np.hypot(oH, oW) / 2.0, np.hypot(H, W) / 2.0, (oH - 1) / 2.0, (oW - 1) / 2.0, k1, k2]


@pytest.mark.parametrize("hw", HWS)
@pytest.mark.parametrize("k", [(0.0, 0.0), (0.08, -0.02)])
def test_radial_is_bit_equal_to_coords_radial(hw, k):
    centre = (19.3, 30.9)
    ref = coords.radial((40, 64), hw, k[0], k[1], centre=centre)
    assert R.same_bits(_lib.coords_build_host("radial", _radial_params((40, 64), hw, k[0], k[1], centre), hw), ref)


def test_a_tile_with_an_origin_equals_the_slice_of_the_whole(golden):
    hw = (37, 53)
    M = _matrices(golden)[0]
    cases = [("homography", np.linalg.inv(M).reshape(9)), ("radial", _radial_params((40, 64), hw, 0.08, -0.02, (19.3, 30.9))),
             ("brown", coords.brown_params(K0, DIST8, _rot(0.02, -0.03, 0.01), K0 * np.array([[0.9], [0.9], [1.0]])))]
    for model, p in cases:
        whole = _lib.coords_build_host(model, p, hw)
        for dt in (np.float64, np.float32):
            buf = np.full((hw[0], hw[1] + 3, 2), -7.0, dtype=dt)                 # a strided tile inside a wider, sentinel-filled map
            tile = buf[5:16, 7:30]
            _lib.coords_build_host(model, p, (11, 23), out=tile, origin=(5, 7))
            assert R.same_bits(np.ascontiguousarray(tile), whole[5:16, 7:30].astype(dt))
            probe = buf.copy()
            probe[5:16, 7:30] = -7.0
            assert (probe == -7.0).all()                                          # nothing outside the tile was written


def _brown_cases():
    return [(K0, DIST8, _rot(0.02, -0.03, 0.01), K0 * np.array([[0.9], [0.9], [1.0]])), (K0, DIST8[:5], None, None),
            (K0, DIST8[:4], _rot(0.0, 0.0, 0.1), None), (K0, None, None, K0)]


@pytest.mark.parametrize("hw", HWS)
def test_brown_is_bit_equal_to_the_restatement(hw):
    for K, dist, rot, new_K in _brown_cases():
        p = coords.brown_params(K, dist, rot, new_K)
        ref = R.brown(p[:9].reshape(3, 3), p[9], p[10], p[11], p[12], p[13:], hw)
        got = coords.undistort_rectify(K, dist, rot, new_K, hw)
        assert got.dtype == np.float64 and R.same_bits(got, ref)
        assert R.same_bits(coords.undistort_rectify(K, dist, rot, new_K, hw, dtype=np.float32), ref.astype(np.float32))


def test_brown_anchors():
    hw, in_hw = (37, 53), (40, 64)
    new_K = np.array([[44.0, 0.0, 27.5], [0.0, 47.0, 16.0], [0.0, 0.0, 1.0]])
    # the map whose projection (the INVERSE of from_homography's matrix argument) is K . inv(new_K); np.dot, as the reference writes it
    hom = coords.from_homography(new_K @ np.linalg.inv(K0), hw, arithmetic="reference")
    zero = [0.0] * 8
    # a camera that reproduces coords.radial's normalisation: new_K = (no, no, centre of the output), K = (ni, ni, centre)
    no, ni, centre, k = np.hypot(*hw) / 2.0, np.hypot(*in_hw) / 2.0, (19.3, 30.9), (0.08, -0.02)
    rK = np.array([[ni, 0.0, centre[1]], [0.0, ni, centre[0]], [0.0, 0.0, 1.0]])
    rN = np.array([[no, 0.0, (hw[1] - 1) / 2.0], [0.0, no, (hw[0] - 1) / 2.0], [0.0, 0.0, 1.0]])
    rad = coords.radial(in_hw, hw, k[0], k[1], centre=centre)
    rdist = [k[0], k[1], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    # the restatement alone, then the library
    _anchor(R.brown(np.linalg.inv(new_K), K0[0, 0], K0[1, 1], K0[0, 2], K0[1, 2], zero, hw), hom)
    _anchor(R.brown(np.linalg.inv(rN), ni, ni, centre[1], centre[0], rdist, hw), rad)
    _anchor(coords.undistort_rectify(K0, zero, np.eye(3), new_K, hw), hom)
    _anchor(coords.undistort_rectify(rK, rdist[:4], None, rN, hw), rad)


def test_builder_argument_checks():
    with pytest.raises(ValueError, match="skew"):
        coords.undistort_rectify(K0 + np.array([[0, 0.1, 0], [0, 0, 0], [0, 0, 0]]), None, None, None, (4, 4))
    with pytest.raises(ValueError, match="4, 5 or 8"):
        coords.undistort_rectify(K0, [0.1, 0.2], None, None, (4, 4))
    with pytest.raises(ValueError, match="reference"):
        coords.from_homography(np.eye(3), (4, 4), arithmetic="reference", device="cuda")
    with pytest.raises(ValueError):
        coords.radial((4, 4), (0, 4), 0.1, device=None, dtype=np.float16)
    with pytest.raises(ValueError, match="interp"):
        coords.from_mesh(np.zeros((2, 2, 2)), (4, 4), interp="nearest")
    with pytest.raises(ValueError, match="mixed"):
        class Dev:                                                                # stands for a device tensor: compose looks at is_cuda
            is_cuda = True
        coords.compose(np.zeros((2, 2, 2)), Dev())


# ---------------------------------------------------------------------------------------------- mesh
MESHES = [(2, 2), (3, 5), (7, 4)]


def _ctrl(ghw, out_hw, seed=0, dtype=np.float64):
    """a jittered regular mesh over a 40 x 64 source"""
    rng = np.random.default_rng(seed)
    a, b = np.meshgrid(np.linspace(0, 39, ghw[0]), np.linspace(0, 63, ghw[1]), indexing="ij")
    return (np.stack([a, b], axis=-1) + rng.normal(0, 1.5, ghw + (2,))).astype(dtype)


@pytest.mark.parametrize("interp", ["bilinear", "bicubic"])
def test_mesh_restatement_against_torch_interpolate(interp):
    import torch
    import torch.nn.functional as F
    for ghw in MESHES + [(37, 53)]:
        for hw in HWS:
            c = _ctrl(ghw, hw)
            ref = F.interpolate(torch.from_numpy(c).permute(2, 0, 1)[None], size=hw, mode=interp, align_corners=True)[0].permute(1, 2, 0).numpy()
            _anchor(R.mesh(c, hw, interp), ref)


@pytest.mark.parametrize("interp", ["bilinear", "bicubic"])
@pytest.mark.parametrize("hw", HWS)
def test_mesh_is_bit_equal_to_the_restatement(interp, hw):
    for ghw in MESHES + [hw if hw[0] > 1 else (2, 9)]:
        for cdt in (np.float64, np.float32):
            c = _ctrl(ghw, hw, dtype=cdt)
            ref = R.mesh(c, hw, interp)
            for odt in (np.float64, np.float32):
                assert R.same_bits(_lib.coords_mesh_host(c, hw, interp, odt), ref.astype(odt)), (ghw, cdt, odt)
            assert R.same_bits(coords.from_mesh(c, hw, interp), ref.astype(cdt))
    if hw[0] > 6:                                                                 # a strided tile of the whole map, in place
        c = _ctrl((3, 5), hw)
        whole = R.mesh(c, hw, interp)
        assert R.same_bits(R.mesh(c, (4, 21), interp, origin=(2, 9), full_hw=hw), whole[2:6, 9:30])
        buf = np.full((hw[0], hw[1] + 2, 2), -7.0)
        _lib.coords_mesh_host(c, (4, 21), interp, out=buf[2:6, 9:30], origin=(2, 9), full_hw=hw)
        assert R.same_bits(np.ascontiguousarray(buf[2:6, 9:30]), whole[2:6, 9:30])
        buf[2:6, 9:30] = -7.0
        assert (buf == -7.0).all()


@pytest.mark.parametrize("interp", ["bilinear", "bicubic"])
def test_identity_upsample_and_vertex_positions(interp):
    c = _ctrl((37, 53), (37, 53))
    assert R.same_bits(_lib.coords_mesh_host(c, (37, 53), interp), c)          # gh, gw = oH, oW: every pixel is a vertex
    c = _ctrl((3, 5), (37, 53))
    m = _lib.coords_mesh_host(c, (37, 53), interp)                              # vertex a at row a * 36 / 2, vertex b at column b * 52 / 4
    assert R.same_bits(np.ascontiguousarray(m[::18, ::13]), c)


# ---------------------------------------------------------------------------------------------- compose
def _maps(seed=5, a_hw=(20, 30), b_hw=(11, 13)):
    rng = np.random.default_rng(seed)
    a = coords.radial((40, 64), a_hw, 0.05, 0.01) + rng.normal(0, 0.2, a_hw + (2,))
    b = np.stack([rng.uniform(-2, a_hw[0] + 1, b_hw), rng.uniform(-2, a_hw[1] + 1, b_hw)], axis=-1)
    return a, b


def test_compose_is_bit_equal_to_the_restatement():
    a, b = _maps()
    for adt in (np.float64, np.float32):
        for bdt in (np.float64, np.float32):
            aa, bb = a.astype(adt), b.astype(bdt)
            ref = R.compose(aa, bb)
            for odt in (np.float64, np.float32):
                assert R.same_bits(_lib.coords_compose_host(aa, bb, odt), ref.astype(odt))
    assert R.same_bits(coords.compose(a, b), R.compose(a, b))
    wide_a, wide_b, wide_o = np.full((20, 33, 2), np.nan), np.full((11, 15, 2), np.nan), np.full((11, 17, 2), -7.0)
    wide_a[:, :30], wide_b[:, 1:14] = a, b                                      # every operand a strided view
    _lib.coords_compose_host(wide_a[:, :30], wide_b[:, 1:14], out=wide_o[:, 2:15])
    assert R.same_bits(np.ascontiguousarray(wide_o[:, 2:15]), R.compose(a, b))
    wide_o[:, 2:15] = -7.0
    assert (wide_o == -7.0).all()


def test_compose_of_an_affine_outer_map_is_the_affine_of_the_inner():
    a_hw = (20, 30)
    ii, jj = np.meshgrid(np.arange(a_hw[0], dtype=np.float64), np.arange(a_hw[1], dtype=np.float64), indexing="ij")
    aff = np.stack([1.5 * ii - 0.25 * jj + 3.0, 0.4 * ii + 2.0 * jj - 7.0], axis=-1)
    rng = np.random.default_rng(6)
    b = np.stack([rng.uniform(0, a_hw[0] - 1, (11, 13)), rng.uniform(0, a_hw[1] - 1, (11, 13))], axis=-1)
    ref = np.stack([1.5 * b[..., 0] - 0.25 * b[..., 1] + 3.0, 0.4 * b[..., 0] + 2.0 * b[..., 1] - 7.0], axis=-1)
    for got in (R.compose(aff, b), _lib.coords_compose_host(aff, b)):
        _anchor(got, ref, 1e-9)


def special_maps():
    """(A, B, expected C) of compose's special entries; shared with the GPU parity test"""
    a = np.arange(4 * 5 * 2, dtype=np.float64).reshape(4, 5, 2) * 0.5 + 1.0
    a[2, 3] = np.nan
    inf = np.inf
    b = np.array([[[np.nan, 1.0], [1.0, np.nan], [-inf, -inf], [inf, inf]],
                  [[3.0, 4.0], [2.0, 2.0], [2.0, 3.0], [1.5, 3.0]],
                  [[2.0, 3.5], [1.0, 3.0], [-5.0, 2.25], [9.0, -1.0]]])
    nan2 = [np.nan, np.nan]
    want = np.array([[nan2, nan2, a[0, 0], a[3, 4]],
                     [a[3, 4], a[2, 2], nan2, nan2],
                     [nan2, a[1, 3], 0.75 * a[0, 2] + 0.25 * a[0, 3], a[3, 0]]])
    return a, b, want


def test_compose_special_entries():
    a, b, want = special_maps()
    for got in (R.compose(a, b), _lib.coords_compose_host(a, b)):
        # NaN in B -> (NaN, NaN); +-inf -> the border; B on the last row and column; on (2, 2) the NaN at (2, 3) sits behind
        # zero-weight taps and is not seen; at (2, 3), (1.5, 3) and (2, 3.5) it is behind a counted tap and is seen
        assert R.same_bits(got, want)
    one_row = np.arange(10, dtype=np.float64).reshape(1, 5, 2)                   # aH == 1: the row coordinate is irrelevant
    b1 = np.array([[[0.0, 1.5], [7.0, 4.0], [-3.0, 0.0]]])
    want1 = np.array([[0.5 * one_row[0, 1] + 0.5 * one_row[0, 2], one_row[0, 4], one_row[0, 0]]])
    for got in (R.compose(one_row, b1), _lib.coords_compose_host(one_row, b1)):
        assert R.same_bits(got, want1)
    one = np.array([[[3.0, 4.0]]])                                               # aH == aW == 1
    assert R.same_bits(_lib.coords_compose_host(one, b1), np.broadcast_to(one[0, 0], (1, 3, 2)).copy())


# ---------------------------------------------------------------------------------------------- refusals
def _ptr(a):
    return a.ctypes.data


def test_every_refused_argument_returns_einval_and_writes_nothing():
    lib = _lib.lib()
    out = np.full((6, 8, 2), -7.0)
    out32 = np.full((6, 8, 2), -7.0, dtype=np.float32)
    p = np.linalg.inv(np.array([[1.0, 0.1, 2.0], [0.0, 1.1, 1.0], [0.0, 0.0, 1.0]])).reshape(9).copy()
    F64, F32 = _lib.LERF_F64, _lib.LERF_F32

    def build(model=0, params=p, n=9, o=out, dt=F64, stride=16, oH=6, oW=8, i0=0, j0=0, off=0):
        return lib.lerf_coords_build_host(model, None if params is None else _ptr(params), n, None if o is None else _ptr(o) + off, dt,
                                          stride, oH, oW, i0, j0)
    assert build() == 0
    out[:] = -7.0
    bad = p.copy()
    bad[4] = np.inf
    nanp = p.copy()
    nanp[0] = np.nan
    calls = [build(params=None), build(o=None), build(model=3), build(model=-1), build(n=8), build(model=1, n=9), build(model=2, n=9),
             build(dt=_lib.LERF_U8), build(dt=7), build(stride=15), build(stride=14), build(oH=0), build(oW=0), build(oH=-1),
             build(off=8), build(o=out32, dt=F32, off=4, stride=16), build(params=bad), build(params=nanp), build(i0=-1), build(j0=-1)]
    assert calls == [EINVAL] * len(calls), calls

    ctrl = np.zeros((3, 4, 2))

    def mesh(c=ctrl, cdt=F64, gh=3, gw=4, interp=0, fh=6, fw=8, o=out, dt=F64, stride=16, oH=6, oW=8, i0=0, j0=0, off=0, coff=0):
        return lib.lerf_coords_mesh_host(None if c is None else _ptr(c) + coff, cdt, gh, gw, interp, fh, fw, None if o is None else _ptr(o) + off,
                                         dt, stride, oH, oW, i0, j0)
    assert mesh() == 0
    out[:] = -7.0
    calls = [mesh(c=None), mesh(o=None), mesh(gh=1), mesh(gw=1), mesh(gh=0), mesh(interp=2), mesh(interp=-1), mesh(cdt=_lib.LERF_U8),
             mesh(dt=_lib.LERF_I16), mesh(stride=15), mesh(stride=12), mesh(oH=0), mesh(oW=0), mesh(off=8), mesh(coff=8), mesh(i0=-1),
             mesh(fh=5), mesh(fw=7), mesh(i0=1), mesh(j0=1)]
    assert calls == [EINVAL] * len(calls), calls

    a, b = np.zeros((4, 5, 2)), np.ones((6, 8, 2))

    def comp(A=a, adt=F64, sa=10, aH=4, aW=5, B=b, bdt=F64, sb=16, o=out, dt=F64, so=16, oH=6, oW=8, off=0, aoff=0, boff=0):
        return lib.lerf_coords_compose_host(None if A is None else _ptr(A) + aoff, adt, sa, aH, aW, None if B is None else _ptr(B) + boff, bdt,
                                            sb, None if o is None else _ptr(o) + off, dt, so, oH, oW)
    assert comp() == 0
    out[:] = -7.0
    calls = [comp(A=None), comp(B=None), comp(o=None), comp(adt=0), comp(bdt=3), comp(dt=9), comp(sa=9), comp(sa=8), comp(sb=15), comp(sb=14),
             comp(so=15), comp(so=14), comp(aH=0), comp(aW=0), comp(oH=0), comp(oW=0), comp(off=8), comp(aoff=8), comp(boff=8)]
    assert calls == [EINVAL] * len(calls), calls
    assert (out == -7.0).all() and (out32 == -7.0).all()

    # the device entry points refuse the same arguments before they touch the GPU (no launch: this machine has none)
    assert lib.lerf_coords_build(0, _ptr(p), 9, None, F64, 16, 6, 8, 0, 0, None) == EINVAL
    assert lib.lerf_coords_build(0, _ptr(bad), 9, _ptr(out), F64, 16, 6, 8, 0, 0, None) == EINVAL
    assert lib.lerf_coords_mesh(_ptr(ctrl), F64, 1, 4, 0, 6, 8, _ptr(out), F64, 16, 6, 8, 0, 0, None) == EINVAL
    assert lib.lerf_coords_compose(_ptr(a), F64, 9, 4, 5, _ptr(b), F64, 16, _ptr(out), F64, 16, 6, 8, None) == EINVAL
    ws = np.zeros(3 * 8 * 2)
    g = np.zeros((6, 8, 2))
    gc = np.full((3, 4, 2), -7.0)
    assert lib.lerf_coords_mesh_bwd_workspace_bytes(3, 4, 6, 8) == 3 * 8 * 16
    assert lib.lerf_coords_mesh_bwd_workspace_bytes(1, 4, 6, 8) == 0
    for args in [(None, 6, 8, 0, 3, 4, _ptr(gc), _ptr(ws), ws.nbytes), (_ptr(g), 6, 8, 0, 3, 4, None, _ptr(ws), ws.nbytes),
                 (_ptr(g), 6, 8, 0, 3, 4, _ptr(gc), None, ws.nbytes), (_ptr(g), 6, 8, 0, 3, 4, _ptr(gc), _ptr(ws), ws.nbytes - 1),
                 (_ptr(g), 6, 8, 2, 3, 4, _ptr(gc), _ptr(ws), ws.nbytes), (_ptr(g), 6, 8, 0, 1, 4, _ptr(gc), _ptr(ws), ws.nbytes),
                 (_ptr(g), 0, 8, 0, 3, 4, _ptr(gc), _ptr(ws), ws.nbytes), (_ptr(g) + 8, 6, 8, 0, 3, 4, _ptr(gc), _ptr(ws), ws.nbytes),
                 (_ptr(g), 6, 8, 0, 3, 4, _ptr(gc) + 8, _ptr(ws), ws.nbytes)]:
        assert lib.lerf_coords_mesh_bwd(*args, None) == EINVAL, args
    assert (gc == -7.0).all()
