"""CPU-only: the remap's C ABI surface, its host geometry (lerf_remap_host_geometry: what the remap kernels derive from a
coordinate map, from the same header they compile) against the oracle, and the map builders of coords.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO

import lerf_pytorch_amd as L
from lerf_pytorch_amd import _lib, coords, ops

import remap_ref

IN_HW, OUT_HW = (37, 53), (45, 61)
NEW = ["lerf_remap", "lerf_remap_packed", "lerf_remap_host_geometry"]


def test_remap_symbols_declared_exported_and_resolve():
    src = open(os.path.join(REPO, "include", "lerf_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(lerf_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(L.LIB_PATH)
    for n in NEW:
        assert n in declared, "%s is not declared in include/lerf_hip.h" % n
        assert n in _lib.EXPORTS
        assert hasattr(lib, n), "liblerf_hip.so does not export %s" % n
        assert getattr(_lib.lib(), n).argtypes
    assert "lerf_remap_geo_t" in src and "LERF_REMAP_PADS_FROM_MAP" in src
    assert lib.lerf_abi_version() == 7
    assert ctypes.sizeof(_lib.RemapGeo) == 56            # int x3, pad, ptr, int, pad, int64, int x3, pad


def _same(got, geo):
    gr, gc, lr, lc, pads = got
    assert np.array_equal(gr, geo["gx"]) and np.array_equal(gc, geo["gy"])          # bit-equal float64
    assert np.array_equal(lr, geo["lx"]) and np.array_equal(lc, geo["ly"])
    assert pads == (geo["pad"][0], geo["pad"][2])


@pytest.mark.parametrize("S", [1, 2, 4])
def test_remap_pixel_equals_oracle_on_a_homography_map(golden, oracle, S):
    M = golden("g4_warp.npz")["isc/matrix"]
    cm = coords.from_homography(M, OUT_HW, arithmetic="reference")                  # the oracle's own np.dot (:327)
    geo = oracle.warp_geometry(M, IN_HW, OUT_HW, S)
    _same(_lib.remap_host_geometry(cm, IN_HW, S), geo)
    # the default map rounds the three-term sums like the device's project_point instead of like BLAS: the same taps and pads,
    # the points within a few ulp of the oracle's (1 ulp of a coordinate below 64 is 7e-15)
    gr, gc, lr, lc, pads = _lib.remap_host_geometry(coords.from_homography(M, OUT_HW), IN_HW, S)
    assert np.array_equal(lr, geo["lx"]) and np.array_equal(lc, geo["ly"]) and pads == (geo["pad"][0], geo["pad"][2])
    assert np.max(np.abs(gr - geo["gx"])) <= 4 * 7.2e-15 and np.max(np.abs(gc - geo["gy"])) <= 4 * 7.2e-15
    _same(ops.RemapGeometry(IN_HW, cm, S).host_geometry(), geo)                     # the geometry object's host mirror
    # a strided map (rows of a wider buffer) and explicit pads are the same geometry
    wide = np.full((OUT_HW[0], OUT_HW[1] + 3, 2), np.nan)
    wide[:, :OUT_HW[1]] = cm
    g = _lib.RemapGeo()
    g.S, g.out_h, g.out_w = S, OUT_HW[0], OUT_HW[1]
    g.coords, g.coords_dtype, g.row_stride = wide.ctypes.data, _lib.LERF_F64, wide.strides[0] // 8
    g.pad_r_lo, g.pad_c_lo = geo["pad"][0], geo["pad"][2]
    gr = np.zeros(OUT_HW)
    lc = np.zeros(OUT_HW, np.int32)
    pads = np.zeros(2, np.int32)
    assert _lib.lib().lerf_remap_host_geometry(ctypes.byref(g), IN_HW[0], IN_HW[1], gr.ctypes.data, None, None, lc.ctypes.data,
                                               pads.ctypes.data) == 0
    assert np.array_equal(gr, geo["gx"]) and np.array_equal(lc, geo["ly"]) and tuple(pads) == (geo["pad"][0], geo["pad"][2])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("S", [1, 2, 4])
def test_remap_pixel_equals_the_map_fed_restatement(S, dtype):
    cm = remap_ref.sinus_flow(IN_HW, OUT_HW).astype(dtype)
    geo = remap_ref.map_geometry(cm, IN_HW, OUT_HW, S)
    _same(_lib.remap_host_geometry(cm, IN_HW, S), geo)
    if S > 1:
        assert geo["pad"][0] > 0 and geo["pad"][2] == 0          # the map leaves the frame above its first row
    whole = ops.RemapGeometry(IN_HW, cm, S)
    assert whole.pads() == (geo["pad"][0], geo["pad"][2])
    # rows of the map with the whole map's pads: those rows of the whole geometry
    part = whole.rows(7, 19).host_geometry()
    for a, b in zip(part[:4], whole.host_geometry()[:4]):
        assert np.array_equal(a, b[7:19])


def test_map_restatement_is_warp_geometry(golden, oracle):
    """the restatement fed warp_geometry's own unclipped grid returns warp_geometry's result (so what the GPU tests compare
    against IS the oracle's geometry from the clip on)"""
    M = golden("g4_warp.npz")["isc/matrix"]
    for S in (1, 2, 4):
        a = oracle.warp_geometry(M, IN_HW, OUT_HW, S)
        b = remap_ref.map_geometry(coords.from_homography(M, OUT_HW, arithmetic="reference"), IN_HW, OUT_HW, S)
        assert a["pad"] == b["pad"] and all(np.array_equal(a[k], b[k]) for k in ("gx", "gy", "lx", "ly"))


def test_non_finite_entries_cannot_leave_the_frame():
    cm = remap_ref.sinus_flow(IN_HW, OUT_HW)
    cm[3, 4] = (np.nan, 5.0)
    cm[5, 6] = (np.inf, -np.inf)
    cm[7, 8] = (-1e300, 1e300)
    cm[0, 0] = (np.nan, np.nan)                                # the pads' entry: NaN clips to 0
    for S in (1, 2, 4, 8):
        gr, gc, lr, lc, pads = _lib.remap_host_geometry(cm, IN_HW, S)
        assert pads == (S // 2, S // 2)
        assert np.all((gr >= pads[0]) & (gr <= IN_HW[0] + pads[0])) and np.all((gc >= pads[1]) & (gc <= IN_HW[1] + pads[1]))
        assert np.all((lr >= 0) & (lr <= IN_HW[0] + pads[0])) and np.all((lc >= 0) & (lc <= IN_HW[1] + pads[1]))
        assert (gr[5, 6], gc[5, 6]) == (IN_HW[0] + pads[0], pads[1]) and (gr[7, 8], gc[7, 8]) == (pads[0], IN_HW[1] + pads[1])


def test_host_geometry_rejects_bad_descriptors():
    cm = remap_ref.sinus_flow(IN_HW, OUT_HW)
    g = _lib.RemapGeo()
    g.S, g.out_h, g.out_w = 2, OUT_HW[0], OUT_HW[1]
    g.coords, g.coords_dtype, g.row_stride = cm.ctypes.data, _lib.LERF_F64, 2 * OUT_HW[1] - 2      # rows overlap
    g.pad_r_lo = g.pad_c_lo = _lib.REMAP_PADS_FROM_MAP
    call = lambda: _lib.lib().lerf_remap_host_geometry(ctypes.byref(g), IN_HW[0], IN_HW[1], None, None, None, None, None)
    assert call() == -1
    g.row_stride, g.coords_dtype = 2 * OUT_HW[1], _lib.LERF_U8
    assert call() == -1
    g.coords_dtype, g.S = _lib.LERF_F64, 0
    assert call() == -1
    g.S = 2
    assert call() == 0
    with pytest.raises(ValueError):
        _lib.remap_host_geometry(cm[..., :1], IN_HW, 2)
    with pytest.raises(ValueError):
        ops.RemapGeometry(IN_HW, cm, 2, pads=(-2, 0))


def test_coords_builders():
    M = np.array([[1.1, 0.02, 3.0], [-0.03, 0.9, 1.5], [1e-4, -2e-4, 1.0]])
    h = coords.from_homography(M, OUT_HW)
    assert h.shape == OUT_HW + (2,) and h.dtype == np.float64 and h.flags.c_contiguous
    # unclipped: the projection of the output corner, (row, col) order
    p = np.linalg.inv(M) @ np.array([OUT_HW[1] - 1.0, OUT_HW[0] - 1.0, 1.0])
    np.testing.assert_allclose(h[-1, -1], [p[1] / p[2], p[0] / p[2]], rtol=1e-13)
    r = coords.from_homography(M, OUT_HW, arithmetic="reference")
    assert r.shape == h.shape and r.dtype == np.float64 and np.max(np.abs(r - h)) < 1e-12
    with pytest.raises(ValueError):
        coords.from_homography(M, OUT_HW, arithmetic="fast")
    ident = coords.from_homography(np.eye(3), (4, 5))
    ii, jj = np.meshgrid(np.arange(4), np.arange(5), indexing="ij")
    assert np.array_equal(ident[..., 0], ii) and np.array_equal(ident[..., 1], jj)
    f = coords.from_flow(np.zeros((6, 7, 2), np.float32))
    ii, jj = np.meshgrid(np.arange(6), np.arange(7), indexing="ij")
    assert f.shape == (6, 7, 2) and f.dtype == np.float64
    assert np.array_equal(f[..., 0], ii) and np.array_equal(f[..., 1], jj)
    d = np.zeros((6, 7, 2))
    d[2, 3] = (0.5, -1.25)
    assert tuple(coords.from_flow(d)[2, 3]) == (2.5, 1.75)
    r = coords.radial(IN_HW, OUT_HW, 0.0, 0.0)
    assert r.shape == OUT_HW + (2,) and r.dtype == np.float64
    np.testing.assert_allclose(r[(OUT_HW[0] - 1) // 2, (OUT_HW[1] - 1) // 2], [(IN_HW[0] - 1) / 2, (IN_HW[1] - 1) / 2])   # centre -> centre
    b = coords.radial(IN_HW, OUT_HW, 0.3, 0.1, centre=(10.0, 20.0))
    np.testing.assert_allclose(b[(OUT_HW[0] - 1) // 2, (OUT_HW[1] - 1) // 2], [10.0, 20.0])
    # barrel: positive k pushes the corners further out than the plain resize does
    assert b[0, 0, 0] - 10.0 < r[0, 0, 0] - (IN_HW[0] - 1) / 2 < 0
    with pytest.raises(ValueError):
        coords.from_homography(np.eye(2), (3, 3))
    with pytest.raises(ValueError):
        coords.from_flow(np.zeros((3, 3)))
