"""CPU-only: the C-ABI library loads, exports every symbol include/lerf_hip.h
declares, and its host-side helpers agree with the oracle / golden vectors.
No device entry point runs here: the stage-3 ones are called with arguments they refuse, and only those."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO

import lerf_pytorch_amd as L
from lerf_pytorch_amd import _lib


def _declared_functions():
    src = open(os.path.join(REPO, "include", "lerf_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(lerf_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    names = _declared_functions()
    assert len(names) >= 14
    lib = ctypes.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), "liblerf_hip.so does not export %s" % n
    assert sorted(_lib.EXPORTS) == names
    assert lib.lerf_abi_version() == 7


def test_error_strings():
    lib = _lib.lib()
    assert lib.lerf_strerror(0) == b"ok"
    assert b"invalid" in lib.lerf_strerror(-1)


@pytest.mark.parametrize("mode", list("sctdy"))
def test_mode_offsets_match_oracle(oracle, mode):
    for r in range(4):
        dy, dx = _lib.mode_offsets(mode, r)
        assert list(zip(dy.tolist(), dx.tolist())) == [tuple(o) for o in oracle.rotated_offsets(mode, r)]


def test_unknown_mode_is_value_error():
    with pytest.raises(ValueError, match="Mode q not implemented."):
        _lib.mode_offsets("q", 0)


@pytest.mark.parametrize("n_in,scale,S", [(32, 2, 2), (40, 2, 4), (30, 1.5, 2), (17, 3, 2), (23, 3, 4), (16, 4, 2),
                                          (5, 2.4, 2), (6, 1.3, 2), (9, 1.0, 2), (1080, 2, 2), (1920, 2.0, 2),
                                          (1080, 1.5, 2), (333, 3.0, 4), (7, 7.77, 8)])
def test_sr_tables_bit_equal_oracle(oracle, n_in, scale, S):
    n_out = oracle.out_size(n_in, scale)
    assert _lib.out_size(n_in, scale) == n_out
    left, d64, d32, pads = _lib.sr_axis_tables(n_in, n_out, scale, S)
    ol, od, plo, phi = oracle.sr_axis_tables(n_in, n_out, scale, S)
    assert np.array_equal(left, ol)
    assert np.array_equal(d64, od)              # bit-equal float64
    assert pads == (plo, phi)
    # float32 table keeps the linear kernel's mask classes of the float64 distances
    cls = lambda x: np.where((x >= -1) & (x < 0), 1, np.where((x >= 0) & (x <= 1), 2, 0))
    assert np.array_equal(cls(d64), cls(d32.astype(np.float64)))
    assert np.max(np.abs(d32 - d64)) < 2.5e-7


@pytest.mark.parametrize("ci", range(8))
def test_sr_tables_match_reference_golden(golden, ci):
    g = golden("g23_sr.npz")
    H, W, sh, sw, S = g["gauss/%d/cfg" % ci]
    H, W, S = int(H), int(W), int(S)
    lx, dx, _, px = _lib.sr_axis_tables(H, _lib.out_size(H, sh), sh, S)
    ly, dy, _, py = _lib.sr_axis_tables(W, _lib.out_size(W, sw), sw, S)
    assert list(px) + list(py) == list(g["gauss/%d/pad" % ci])
    assert np.array_equal(dx, g["gauss/%d/disx" % ci])
    assert np.array_equal(dy, g["gauss/%d/disy" % ci])
    assert np.array_equal(lx[:, None] + px[0] + np.arange(S), g["gauss/%d/fovx" % ci])
    assert np.array_equal(ly[:, None] + py[0] + np.arange(S), g["gauss/%d/fovy" % ci])


@pytest.mark.parametrize("p", ["isc", "osc"])
def test_warp_pads_match_reference_golden(golden, p):
    g = golden("g4_warp.npz")
    minv = np.linalg.inv(g["%s/matrix" % p])
    for S in (2, 4):
        assert list(_lib.warp_pads(minv, (52, 52), (60, 70), S)) == list(g["%s/60x70/S%d/pad" % (p, S)])
    assert list(_lib.warp_pads(minv, (52, 52), (344, 228), 2)) == list(g["%s/344x228/S2/pad" % p])


def test_invert3x3():
    m = np.array([[2.05, 0.12, 15.0], [-0.08, 1.95, 40.0], [1.5e-5, -1.0e-5, 1.0]])
    out = np.zeros(9)
    assert _lib.lib().lerf_invert3x3(np.ascontiguousarray(m).ctypes.data, out.ctypes.data) == 0
    np.testing.assert_allclose(out.reshape(3, 3), np.linalg.inv(m), rtol=1e-12)
    sing = np.zeros(9)
    assert _lib.lib().lerf_invert3x3(sing.ctypes.data, out.ctypes.data) == -1


def test_device_path_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(L.LerfError, match="no CPU fallback"):
        L.LutSet.shipped("lerf-g")
    with pytest.raises(L.LerfError):
        L.sr(np.zeros((8, 8, 3), np.uint8), 2)


def test_lut_loader_shapes():
    for name, oC in (("lerf-g", 3), ("lerf-l", 1)):
        from lerf_pytorch_amd.luts import ASSET_DIR
        d = L.load_lut_arrays(os.path.join(ASSET_DIR, name), linear=(oC == 1))
        assert sorted(d) == sorted(["s1_%sr0" % m for m in "sct"] + ["s2_%sr%d" % (m, r) for m in "sct" for r in (0, 1)])
        assert d["s1_sr0"].shape == (83521, 1) and d["s2_tr1"].shape == (83521, oC)
        assert all(v.dtype == np.int8 for v in d.values())


# ---- property tests (hypothesis): host geometry == oracle for arbitrary sizes / scales / supports
from hypothesis import given, settings, strategies as st


@settings(max_examples=150, deadline=None)
@given(n_in=st.integers(1, 3000), scale=st.one_of(st.sampled_from([1.0, 1.5, 2.0, 2.4, 3.0, 4.0]),
                                                   st.floats(1.0, 8.0, allow_nan=False, allow_infinity=False)),
       S=st.integers(1, 8))
def test_sr_tables_property(n_in, scale, S):
    from oracle import lerf_oracle as O
    n_out = O.out_size(n_in, scale)
    assert _lib.out_size(n_in, scale) == n_out
    left, d64, d32, pads = _lib.sr_axis_tables(n_in, n_out, scale, S)
    ol, od, plo, phi = O.sr_axis_tables(n_in, n_out, scale, S)
    assert np.array_equal(left, ol) and np.array_equal(d64, od) and pads == (plo, phi)
    assert np.all(np.diff(left) >= 0)                       # monotone: what the tile / strip ownership search relies on
    cls = lambda x: np.where((x >= -1) & (x < 0), 1, np.where((x >= 0) & (x <= 1), 2, 0))
    assert np.array_equal(cls(d64), cls(d32.astype(np.float64)))


@settings(max_examples=60, deadline=None)
@given(H=st.integers(16, 400), world=st.integers(1, 8), S=st.sampled_from([2, 4]),
       scale=st.sampled_from([1.0, 1.5, 2.0, 2.4, 3.0, 4.0]))
def test_strip_plan_property(H, world, S, scale):
    from oracle import lerf_oracle as O
    from lerf_pytorch_amd import dist as ldist
    if H < world * ldist.halo_rows(S):
        return
    left, _, _, _ = O.sr_axis_tables(H, O.out_size(H, scale), scale, S)
    prev = 0
    for r in range(world):
        p = ldist.StripPlan(H, world, r, S, left)
        assert p.check_support(left)
        assert p.out_rows()[0] == prev
        prev = p.out_rows()[1]
    assert prev == len(left)


@pytest.mark.parametrize("n_in,scale,S", [(6, 3, 2), (17, 3, 4), (33, 1.7, 2), (1080, 2, 2), (10, 2.5, 4), (48, 4, 2), (7, 1.0, 2)])
def test_torch32_axis_tables_equal_oracle(oracle, n_in, scale, S):
    """lerf_sr_axis_tables_f32 == the float32 restatement of Resize2dTorch.get_distance (pinned to the reference's
    tensors when the goldens were generated: tests/golden/gen_golden.py g6 / g9 / g11 outputs depend on them)."""
    from lerf_pytorch_amd import _lib
    n_out = oracle.out_size(n_in, scale)
    left, dis64, dis32, pads = _lib.sr_axis_tables_f32(n_in, n_out, scale, S)
    rl, rd, plo, phi = oracle.sr_axis_tables_torch32(n_in, n_out, scale, S)
    assert np.array_equal(left, rl) and np.array_equal(dis64, rd) and pads == (plo, phi)


# ---- refusal codes of the stage-3 entry points: what the C ABI turns down before it launches anything, and which check wins
EINVAL, EUNSUPPORTED = -1, -2
_RH, _RW, _RC, _ROH, _ROW = 6, 5, 3, 4, 7                  # a 6 x 5 RGB frame to a 4 x 7 output, S = 2
_RBUF = np.zeros(4096, np.float64)                          # every pointer below is HOST memory (16-byte aligned): a call that got
_RBUF_PTR = _RBUF.ctypes.data                               # past its checks would launch on it, so every case must be refused
assert _RBUF_PTR % 16 == 0
_NULL = None


def _refusal_geo(cls, fields):
    g = cls()
    g.S, g.out_h, g.out_w = 2, _ROH, _ROW
    if cls is _lib.SrGeo:
        g.left_r = g.dis_r = g.left_c = g.dis_c = g.dis_r64 = g.dis_c64 = _RBUF_PTR
    elif cls is _lib.WarpGeo:
        g.minv[0] = g.minv[4] = g.minv[8] = 1.0
    else:
        g.coords, g.coords_dtype, g.row_stride = _RBUF_PTR, _lib.LERF_F64, 2 * _ROW
        g.pad_r_lo = g.pad_c_lo = _lib.REMAP_PADS_FROM_MAP
    for k, v in fields.items():
        setattr(g, k, v)
    return g


def _refused(entry, **kw):
    """call `entry` with valid arguments except for the overrides `kw` (g_<field>: a field of the geometry struct)"""
    lib, P, ref = _lib.lib(), _lib.Plane, ctypes.byref
    a = dict(H=_RH, W=_RW, C=_RC, n=2, N=4, kind=0, in_dtype=_lib.LERF_U8, h_dtype=_lib.LERF_U8, out_dtype=_lib.LERF_U8, feat=_RBUF_PTR,
             out=_RBUF_PTR, hyper="ok", geo=True, n_maps=2, map_stride=2 * _ROW * _ROH, ppm=None, h0=_RBUF_PTR, h1=_RBUF_PTR, h2=_RBUF_PTR,
             grad_out=_RBUF_PTR, grad_coords=_RBUF_PTR, luts=True, boxes=_RBUF_PTR, ws=_RBUF_PTR, ws_short=0)
    gf = {k[2:]: kw.pop(k) for k in list(kw) if k.startswith("g_")}
    assert set(kw) <= set(a), kw
    a.update(kw)
    if entry == "lerf_remap_batched" and "C" not in kw:
        a["C"] = 6                                          # n_maps = 2 maps, three planes each
    H, W, Cn = a["H"], a["W"], a["C"]
    cls = _lib.SrGeo if "resize" in entry else (_lib.WarpGeo if "warp" in entry else _lib.RemapGeo)
    g = ref(_refusal_geo(cls, gf)) if a["geo"] else _NULL
    fn = getattr(lib, entry)
    if entry in ("lerf_resize", "lerf_warp", "lerf_remap", "lerf_remap_batched"):
        pf = P(a["feat"], a["in_dtype"], W * Cn, Cn, 1)
        hs = [P(_RBUF_PTR, a["h_dtype"], W * Cn * 3, Cn * 3, 3) for _ in range(3)]
        if a["hyper"] == "stride":
            hs[1].sx += 1
        elif a["hyper"] == "dtype":
            hs[2].dtype = _lib.LERF_F64
        elif a["hyper"] == "null2":
            hs[2].ptr = None
        ph = _NULL if a["hyper"] is None else (P * 3)(*hs)
        po = P(a["out"], a["out_dtype"], _ROW * Cn, Cn, 1)
        if entry == "lerf_remap_batched":
            ppm = Cn // 2 if a["ppm"] is None else a["ppm"]
            return fn(ref(pf), ph, H, W, Cn, g, a["n_maps"], a["map_stride"], ppm, a["kind"], 10.0, ref(po), None)
        return fn(ref(pf), ph, H, W, Cn, g, a["kind"], 10.0, ref(po), None)
    if "packed" in entry:
        po = P(a["out"], a["out_dtype"], _ROW * Cn, Cn, 1)
        head = (a["feat"], H * W * Cn, a["n"], H, W, Cn, g)
        tail = (a["kind"], 10.0, ref(po), _ROH * _ROW * Cn, None)
        return fn(*head, a["n_maps"], a["map_stride"], *tail) if entry.endswith("batched") else fn(*head, *tail)
    if entry == "lerf_warp_fused_u8":
        need = int(lib.lerf_sr_fused_workspace_bytes(_RH, _RW, _RC, 2))     # of the valid call: enough for every case's sizes
        assert need > a["ws_short"] >= 0
        luts = ref(_lib.Luts()) if a["luts"] else _NULL
        return fn(a["feat"], H * W * Cn, a["n"], H, W, Cn, luts, g, a["boxes"], a["kind"], 10.0, a["out"], _ROH * _ROW * Cn, a["ws"],
                  need - a["ws_short"], None)
    N = a["N"]
    head = (a["feat"], a["h0"], a["h1"], a["h2"], N, H, W, g)
    tail = (a["kind"], 10.0, a["grad_out"], _RBUF_PTR, _RBUF_PTR, _RBUF_PTR, _RBUF_PTR)
    if entry == "lerf_remap_bwd_batched":
        ppm = N // 2 if a["ppm"] is None else a["ppm"]
        return fn(*head, a["n_maps"], a["map_stride"], ppm, *tail, a["grad_coords"], None)
    if entry == "lerf_remap_bwd":
        return fn(*head, *tail, a["grad_coords"], None)
    return fn(*head, *tail, None)


_EDGE, _F32, _F64, _I16 = 1, 1, 2, 3                       # LERF_PAD_EDGE; LERF_F32, LERF_F64, LERF_I16
_PLANES = dict(feat=_NULL), dict(geo=False), dict(out=_NULL), dict(H=0), dict(W=0), dict(C=0)
_HYPER = dict(hyper=None), dict(hyper="stride"), dict(hyper="dtype"), dict(hyper="null2"), dict(hyper=None, kind=1)
_REMAP_GEO = (dict(g_coords=_NULL), dict(g_out_h=0), dict(g_out_w=0), dict(g_coords_dtype=0), dict(g_coords=_RBUF_PTR + 8),
              dict(g_row_stride=2 * _ROW + 1), dict(g_row_stride=2 * _ROW - 2), dict(g_pad_mode=5), dict(g_pad_mode=-1), dict(g_pad_r_lo=9),
              dict(g_pad_c_lo=-2))
_BATCH = (dict(n_maps=0), dict(n_maps=-1), dict(map_stride=2 * _ROW * _ROH + 1), dict(map_stride=-2), dict(map_stride=2 * _ROW * _ROH - 2))
_BWD = (dict(feat=_NULL), dict(geo=False), dict(grad_out=_NULL), dict(N=0), dict(H=0), dict(W=0))
_BWD_H = (dict(h0=_NULL), dict(h0=_NULL, kind=1), dict(h1=_NULL), dict(h2=_NULL))
_DTYPES = (dict(h_dtype=_F32), dict(in_dtype=_F32), dict(out_dtype=_I16), dict(in_dtype=_F64, h_dtype=_F64, out_dtype=_F64),
           dict(in_dtype=_F32, h_dtype=_F32), dict(in_dtype=_F64, kind=3, out_dtype=_F64))

REFUSALS = {
    "lerf_resize": {
        EINVAL: _PLANES + _HYPER + (dict(g_left_r=_NULL), dict(g_left_c=_NULL), dict(g_out_h=0), dict(g_out_w=0), dict(g_pad_mode=5),
                                    dict(g_pad_mode=-1),
                                    # the distance table of the arithmetic is missing: float32 for uint8 outputs, float64 for the rest
                                    dict(g_dis_r=_NULL), dict(g_dis_c=_NULL, kind=1), dict(g_dis_r64=_NULL, out_dtype=_F32),
                                    dict(g_dis_c64=_NULL, in_dtype=_F32, h_dtype=_F32, out_dtype=_F64), dict(g_dis_r=_NULL, kind=3),
                                    dict(g_dis_r64=_NULL, kind=6, out_dtype=_F64),
                                    # two at once
                                    dict(kind=7, feat=_NULL), dict(g_pad_mode=5, g_S=9), dict(hyper="stride", g_S=0),
                                    dict(g_left_r=_NULL, out_dtype=_I16)),
        EUNSUPPORTED: (dict(kind=7), dict(kind=-1), dict(g_S=0), dict(g_S=9), dict(g_S=9, kind=4)) + _DTYPES
                      + (dict(kind=7, hyper=None), dict(kind=9, g_pad_mode=5), dict(kind=-1, g_left_r=_NULL), dict(g_S=9, g_dis_r=_NULL)),
    },
    "lerf_warp": {
        EINVAL: _PLANES + _HYPER + (dict(g_out_h=0), dict(g_out_w=0), dict(g_out_y0=-1), dict(g_out_x0=-1), dict(g_src_y0=-1),
                                    dict(g_src_y0=_RH), dict(g_pad_mode=5), dict(g_pad_mode=-1),
                                    dict(kind=7, feat=_NULL), dict(g_pad_mode=5, out_dtype=0), dict(g_src_y0=-1, g_pad_mode=_EDGE),
                                    dict(g_out_y0=-1, g_S=9), dict(hyper="null2", g_S=9)),
        EUNSUPPORTED: (dict(kind=7), dict(kind=-1), dict(g_pad_mode=_EDGE), dict(g_pad_mode=4, kind=3), dict(g_S=0), dict(g_S=9),
                       dict(g_S=9, kind=5)) + _DTYPES[:5] + (dict(in_dtype=_F64, kind=3, out_dtype=_F64),)
                      + (dict(kind=7, g_out_h=0), dict(kind=7, hyper=None), dict(kind=-1, g_src_y0=-1), dict(g_pad_mode=_EDGE, g_S=9)),
    },
    "lerf_warp_packed": {
        EINVAL: (dict(feat=_NULL), dict(geo=False), dict(out=_NULL), dict(n=0), dict(H=0), dict(W=0), dict(C=0), dict(g_out_h=0),
                 dict(g_out_w=0), dict(g_out_y0=-1), dict(g_out_x0=-1), dict(g_src_y0=-1), dict(g_src_y0=_RH),
                 dict(g_pad_mode=_EDGE, g_out_h=0), dict(g_src_y0=_RH, g_S=9), dict(g_out_x0=-1, kind=3)),
        EUNSUPPORTED: (dict(g_pad_mode=_EDGE), dict(g_pad_mode=5), dict(g_pad_mode=-1), dict(g_S=0), dict(g_S=9), dict(n=65536),
                       dict(g_out_h=65536), dict(kind=2), dict(kind=6), dict(kind=7), dict(kind=-1), dict(out_dtype=_F64),
                       dict(out_dtype=_I16, kind=1), dict(out_dtype=_F64, C=1), dict(kind=3, C=1), dict(kind=3, g_S=4),
                       dict(g_pad_mode=_EDGE, g_src_y0=-1), dict(g_pad_mode=5, g_out_y0=-1), dict(g_S=9, kind=7)),
    },
    "lerf_warp_fused_u8": {
        EINVAL: (dict(feat=_NULL), dict(luts=False), dict(geo=False), dict(boxes=_NULL), dict(out=_NULL), dict(ws=_NULL), dict(n=0),
                 dict(H=0), dict(W=0), dict(C=0), dict(ws_short=1),
                 dict(g_out_y0=1, ws_short=1), dict(g_src_y0=1, feat=_NULL), dict(g_out_x0=1, boxes=_NULL)),
        EUNSUPPORTED: (dict(g_out_y0=1), dict(g_out_x0=1), dict(g_src_y0=1), dict(g_out_y0=-1)),
    },
    "lerf_remap": {
        EINVAL: _PLANES + _HYPER + _REMAP_GEO + (dict(g_coords=_NULL, g_pad_mode=_EDGE), dict(g_pad_mode=5, out_dtype=0),
                                                 dict(hyper="stride", kind=0, g_S=9), dict(g_row_stride=2 * _ROW + 1, g_S=9),
                                                 dict(kind=7, out=_NULL)),
        EUNSUPPORTED: (dict(kind=7), dict(kind=-1), dict(g_pad_mode=_EDGE), dict(g_pad_mode=2, kind=4), dict(g_S=0), dict(g_S=9),
                       dict(g_out_h=65536), dict(g_S=9, kind=2)) + _DTYPES[:5] + (dict(in_dtype=_F64, kind=3, out_dtype=_F64),)
                      + (dict(kind=7, g_coords=_NULL), dict(kind=7, hyper=None), dict(g_pad_mode=_EDGE, g_S=9), dict(kind=-1, g_pad_mode=5)),
    },
    "lerf_remap_batched": {
        EINVAL: _PLANES + _HYPER + _REMAP_GEO + _BATCH + (dict(C=7), dict(C=6, ppm=2), dict(C=4, ppm=3), dict(ppm=0),
                                                              dict(n_maps=0, g_pad_mode=_EDGE), dict(map_stride=-2, g_S=9),
                                                              dict(hyper=None, n_maps=0)),
        EUNSUPPORTED: (dict(kind=7), dict(g_pad_mode=_EDGE), dict(g_S=9), dict(h_dtype=_F32), dict(out_dtype=_I16),
                       dict(kind=7, n_maps=0), dict(kind=-1, ppm=0), dict(g_pad_mode=_EDGE, g_S=0)),
    },
    "lerf_remap_packed": {
        EINVAL: (dict(feat=_NULL), dict(geo=False), dict(out=_NULL), dict(n=0), dict(H=0), dict(W=0), dict(C=0)) + _REMAP_GEO
                + (dict(g_coords=_NULL, g_pad_mode=_EDGE), dict(g_out_h=0, kind=3), dict(g_row_stride=2, g_S=9)),
        EUNSUPPORTED: (dict(g_pad_mode=_EDGE), dict(g_pad_mode=4), dict(g_S=0), dict(g_S=9), dict(n=65536), dict(g_out_h=65536),
                       dict(kind=2), dict(kind=6), dict(kind=7), dict(kind=-1), dict(out_dtype=_F64), dict(out_dtype=_I16, kind=1),
                       dict(out_dtype=_F64, C=1), dict(kind=3, C=1), dict(kind=3, g_S=4),
                       dict(g_pad_mode=_EDGE, g_S=9), dict(g_pad_mode=_EDGE, kind=7), dict(g_S=9, out_dtype=_F64)),
    },
    "lerf_remap_packed_batched": {
        EINVAL: (dict(feat=_NULL), dict(geo=False), dict(out=_NULL), dict(n=0), dict(H=0), dict(W=0), dict(C=0)) + _REMAP_GEO + _BATCH
                + (dict(n=3), dict(n=4), dict(n_maps=3), dict(n_maps=0, g_pad_mode=_EDGE), dict(n=3, g_pad_mode=_EDGE), dict(n_maps=0, kind=7),
                   dict(map_stride=-2, g_S=9)),
        EUNSUPPORTED: (dict(g_pad_mode=_EDGE), dict(g_S=9), dict(kind=3), dict(kind=7), dict(out_dtype=_F64), dict(out_dtype=_F64, C=1),
                       dict(g_pad_mode=_EDGE, g_S=9), dict(g_pad_mode=_EDGE, kind=7)),
    },
    "lerf_resize_bwd_f32": {
        EINVAL: _BWD + _BWD_H + (dict(g_pad_mode=5), dict(g_pad_mode=-1), dict(g_left_r=_NULL), dict(g_left_c=_NULL), dict(g_dis_r=_NULL),
                                 dict(g_dis_c=_NULL), dict(g_out_h=0), dict(g_out_w=0),
                                 dict(g_pad_mode=5, kind=7), dict(h0=_NULL, g_S=9), dict(g_dis_r=_NULL, g_S=9), dict(kind=7, feat=_NULL),
                                 dict(h1=_NULL, g_out_h=0)),
        EUNSUPPORTED: (dict(kind=7), dict(kind=-1), dict(g_S=0), dict(g_S=9), dict(g_S=9, kind=1), dict(g_S=9, kind=3),
                       dict(kind=7, h0=_NULL), dict(kind=-1, g_left_r=_NULL), dict(kind=7, g_S=9)),
    },
    "lerf_warp_bwd": {
        EINVAL: _BWD + _BWD_H + (dict(g_out_h=0), dict(g_out_w=0), dict(g_pad_mode=5), dict(g_pad_mode=-1), dict(N=65536),
                                 dict(g_out_h=65535 * 16 + 1),
                                 dict(g_pad_mode=5, kind=7), dict(h1=_NULL, g_S=9), dict(h0=_NULL, g_out_y0=1), dict(g_out_w=0, kind=-1)),
        EUNSUPPORTED: (dict(kind=7), dict(kind=-1), dict(g_S=0), dict(g_S=9), dict(g_S=9, kind=4), dict(g_out_y0=1), dict(g_out_x0=1),
                       dict(g_src_y0=1), dict(g_out_y0=-1),
                       dict(kind=7, h0=_NULL), dict(g_out_y0=1, N=65536), dict(g_S=9, N=65536), dict(kind=7, g_S=9)),
    },
    "lerf_remap_bwd": {
        EINVAL: _BWD + _BWD_H + _REMAP_GEO + (dict(N=65536), dict(g_out_h=65535 * 16 + 1), dict(grad_coords=_RBUF_PTR + 8),
                                              dict(g_coords=_NULL, kind=7), dict(g_pad_mode=5, kind=-1), dict(h0=_NULL, g_S=9),
                                              dict(N=65536, grad_coords=_RBUF_PTR + 8)),
        EUNSUPPORTED: (dict(kind=7), dict(kind=-1), dict(g_S=0), dict(g_S=9), dict(g_S=9, kind=2),
                       dict(kind=7, h0=_NULL), dict(g_S=9, N=65536), dict(g_S=9, grad_coords=_RBUF_PTR + 8), dict(kind=7, N=65536)),
    },
    "lerf_remap_bwd_batched": {
        EINVAL: _BWD + _BWD_H + _REMAP_GEO + _BATCH + (dict(N=5), dict(N=6, ppm=2), dict(ppm=0), dict(grad_coords=_RBUF_PTR + 8),
                                                      dict(n_maps=0, kind=7), dict(ppm=0, kind=-1), dict(h2=_NULL, g_S=9)),
        EUNSUPPORTED: (dict(kind=7), dict(g_S=9), dict(kind=7, h0=_NULL), dict(g_S=0, grad_coords=_RBUF_PTR + 8)),
    },
}


@pytest.mark.parametrize("entry", sorted(REFUSALS))
def test_stage3_entry_points_refuse_with_the_same_code(entry):
    """every argument set below is turned down on the host, before a launch, with exactly this code; the sets with two violations pin
    which check an entry point makes first (lerf_warp_packed answers a bad pad mode before a bad source row, lerf_remap_bwd a bad
    map before a bad kind, ...)"""
    for code, cases in REFUSALS[entry].items():
        assert len(cases) >= 4
        for case in cases:
            assert _refused(entry, **case) == code, (entry, case)
    assert not _RBUF.any()
