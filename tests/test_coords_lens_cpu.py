"""CPU-only: the fisheye and equirectangular map models and the helpers they stand on (sqrt_pm, atan_pm, atan2_pm of
csrc/lerf_coords_models.h), through the host twins lerf_coords_math_host, lerf_coords_build_host and lerf_coords_build_bwd_host.
Every bound the GPU suite uses is settled here, against references that do not import the library (tests/coords_lens_ref.py):

  1. the exports; the exact cases of the helpers; their error against numpy on a fixed-seed sweep;
  2. the maps against the numpy restatement, both dtypes, tiles with an origin; anchors that need no restatement;
  3. the backward against autograd of the torch restatement; the selects at the principal ray, at a pole and behind the camera;
     a batch; the accumulate contract;
  4. every refusal.

HELPER_ULP.  The helpers are not libm's: on the sweep below (2^20 arguments each, plus the boundaries of atan_pm's intervals and their
neighbours) they differ from numpy's sqrt / arctan / arctan2 by at most 1, 1 and 2 units of the last place (measured with glibc's libm,
itself within 1 ulp; against the exact value sqrt_pm stays within 0.75 ulp, atan_pm within 0.84, atan2_pm within 1.5 -- its quotient
y / x is rounded before the arc tangent sees it).  The bound is that plus 1 ulp for another libm: 2, 2, 3.

MAP_TOL = 1e-12 * max(1, |coordinate|): a helper a few ulp off goes through about ten operations and a focal length or a panorama scale
below 1e3, about 1e-15 relative; the bound is the mesh builder's, three orders above that.
"""
import os
import re

import numpy as np
import pytest
import torch

import coords_lens_ref as LR
import coords_ref as R
from conftest import REPO
from test_coords_build_grad_cpu import adj_close, upstream

from lerf_pytorch_amd import _lib

MODELS = ["fisheye", "equirect"]
CODE = {"fisheye": 16, "equirect": 17}
HELPER_ULP = {"sqrt": 2.0, "atan": 2.0, "atan2": 3.0}
MAP_TOL = 1e-12
HWS = [(1, 1), (37, 53), (64, 64)]
BWD_HWS = [(5, 65), (67, 257)]
ORIGIN = (3, 7)
# what the backward divides by, over every map a gradient is compared on: Wh and h at least 0.5; r at least 1e-3 -- near the principal
# ray d s / d r is the difference of two terms of size ds / r that cancel to O(r), an error of about eps * fx / r per entry: 1e-11 at
# r = 1e-3, two orders under ADJ_TOL
MIN_WH, MIN_H, MIN_R = 0.5, 0.5, 1e-3
EINVAL = -1
PI, HALF_PI = float(np.pi), float(np.pi / 2)


def math_sweep(n=1 << 20, seed=7):
    """(s, a, y, x): arguments of sqrt over 2^+-300, of atan over +-2^+-30 plus the boundaries of its reduction and their neighbours,
    and of atan2 (y, x) over all four quadrants, magnitudes 2^+-30; shared with the GPU suite"""
    rng = np.random.default_rng(seed)
    mant = lambda: 1.0 + rng.random(n)
    sgn = lambda: np.where(rng.random(n) < 0.5, -1.0, 1.0)
    s = np.ldexp(mant(), rng.integers(-300, 301, n))
    a = sgn() * np.ldexp(mant(), rng.integers(-30, 31, n))
    edges = np.array([0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** -29])
    edges = np.concatenate([np.nextafter(edges, 0), edges, np.nextafter(edges, np.inf)])
    a = np.concatenate([a, edges, -edges])
    y = sgn() * np.ldexp(mant(), rng.integers(-30, 31, n))
    x = sgn() * np.ldexp(mant(), rng.integers(-30, 31, n))
    return s, a, y, x


def ulps(got, ref):
    return float(np.max(np.abs(got - ref) / np.spacing(np.abs(ref))))


def lens_case(model, hw, origin=ORIGIN):
    """(params, min of the divisors) of the suite's camera for a map of hw at origin; the field of view is that of a 48 x 144 map"""
    p = LR.cases((max(48, hw[0] + origin[0]), max(144, hw[1] + origin[1])))[model]
    return p, LR.divisors(model, p, hw, origin)


def assert_smooth(model, p, hw, origin):
    """the inputs of a gradient comparison stay away from r = 0, h = 0 and Wh <= 0"""
    t = torch.from_numpy(p)
    ds = [float(d.min()) for d in LR._one(model, t, hw, origin)[1]]
    print("%s %s at %s: divisors %s" % (model, hw, origin, ", ".join("%.3g" % d for d in ds)))
    if model == "fisheye":
        assert ds[0] >= MIN_WH and ds[1] >= MIN_R
    else:
        assert ds[0] >= MIN_H


def map_close(got, ref, what):
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    err = np.abs(got[ok] - ref[ok]) / np.maximum(1.0, np.abs(ref[ok]))
    print("%s: max error %.3g of max(1, |coordinate|), bound %.3g" % (what, float(err.max()), MAP_TOL))
    assert float(err.max()) <= MAP_TOL, what


# exact parameter sets: every entry a dyadic rational, so the rays through the pixels named below are exact
FISH_EXACT = np.array([1 / 64, 0, -26 / 64, 0, 1 / 32, -18 / 32, 0, 0, 1, 64, 32, 26, 18, 0.05, -0.012, 0.004, -0.0009])   # K = new_K, R = I
VIEW_EXACT = np.concatenate([[1 / 64, 0, -26 / 64, 0, 1 / 64, -18 / 64, 0, 0, 1], LR.pano_scalars((96, 192))])            # R = I
# the view turned a quarter turn about x: pixel (18, 26), the principal one, looks along -y, straight at a pole of the panorama
POLE_EXACT = np.concatenate([[1 / 64, 0, -26 / 64, 0, 0, -1, 0, 1 / 64, -18 / 64], LR.pano_scalars((96, 192))])
# a fisheye camera tilted so that Wh = 1 - j / 8 crosses zero on column 8 and is negative beyond it
BEHIND = np.array([1 / 64, 0, -4 / 64, 0, 1 / 32, -3 / 32, -1 / 8, 0, 1, 64, 32, 4, 3, 0.05, -0.012, 0.004, -0.0009])


# ---------------------------------------------------------------------------------------------- 1. exports and helpers
def test_exports_and_abi_version():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "lerf_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lerf_[a-z0-9_]+)\s*\(", src))
    for n in ("lerf_coords_math", "lerf_coords_math_host"):
        assert n in declared and n in _lib.EXPORTS and hasattr(_lib.lib(), n), n
    assert _lib.lib().lerf_abi_version() == 7
    assert _lib.COORDS_MODELS["fisheye"] == 16 and _lib.COORDS_MODELS["equirect"] == 17
    assert _lib.COORDS_MODEL_PARAMS["fisheye"] == 17 and _lib.COORDS_MODEL_PARAMS["equirect"] == 13
    assert re.search(r"LERF_COORDS_FISHEYE\s*=\s*16\b", src) and re.search(r"LERF_COORDS_EQUIRECT\s*=\s*17\b", src)
    assert re.search(r"#define\s+LERF_COORDS_MAX_PARAMS\s+21\b", src)


def test_exact_cases_of_sqrt():
    tiny = np.float64(5e-324)                                              # the smallest subnormal, 2^-1074
    got = _lib.coords_math_host("sqrt", [0.0, -0.0, 4.0, tiny, 2.0 ** -1040, np.inf, -1.0, -np.inf, np.nan, 1.0, 2.25])
    want = np.array([0.0, 0.0, 2.0, 2.0 ** -537, 2.0 ** -520, np.inf, np.nan, np.nan, np.nan, 1.0, 1.5])
    assert R.same_bits(got[:6], want[:6]) and np.all(np.isnan(got[6:9])) and R.same_bits(got[9:], want[9:])
    sub = np.ldexp(1.0 + np.random.default_rng(1).random(1000), -1060)     # subnormals that are no powers of two
    assert ulps(_lib.coords_math_host("sqrt", sub), np.sqrt(sub)) <= HELPER_ULP["sqrt"]


def test_exact_cases_of_atan_and_its_odd_symmetry():
    got = _lib.coords_math_host("atan", [np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-300, -1e-300, 2.0 ** -30])
    assert R.same_bits(got[:2], np.array([HALF_PI, -HALF_PI])) and np.isnan(got[2])
    assert R.same_bits(got[3:], np.array([0.0, -0.0, 1e-300, -1e-300, 2.0 ** -30]))                   # |x| tiny -> x
    a = math_sweep()[1]
    assert R.same_bits(_lib.coords_math_host("atan", -a), -_lib.coords_math_host("atan", a))         # bit for bit


def test_exact_cases_of_atan2():
    f = lambda y, x: _lib.coords_math_host("atan2", np.array(y, np.float64), np.array(x, np.float64))
    # the four axes, the origin, and y = +-0 left of the origin: both count as +
    got = f([0.0, 3.0, 0.0, -3.0, 0.0, -0.0, 0.0, -0.0], [2.0, 0.0, -2.0, 0.0, 0.0, 0.0, -5.0, -5.0])
    assert R.same_bits(got, np.array([0.0, HALF_PI, PI, -HALF_PI, 0.0, 0.0, PI, PI]))
    assert R.same_bits(f([-1e-300, 1e-300], [-1.0, -1.0]), np.array([-PI, PI]))                       # y < 0 goes to -pi
    assert R.same_bits(f([1.0, -1.0, 1.0, -1.0], [1.0, 1.0, -1.0, -1.0]), np.array([PI / 4, -PI / 4, 3 * PI / 4, -3 * PI / 4]))
    assert np.all(np.isnan(f([np.nan, 1.0, np.nan, np.nan], [1.0, np.nan, 0.0, np.nan])))
    _, _, y, x = math_sweep()
    assert R.same_bits(f(-y, x), -f(y, x))                                                             # odd in y, bit for bit


def test_helper_error_against_numpy_on_the_sweep():
    s, a, y, x = math_sweep()
    assert s.size >= 10 ** 6 and a.size >= 10 ** 6 and y.size >= 10 ** 6
    assert all(int(((y < 0) == qy).sum() > 10 ** 5) and int(((x < 0) == qx).sum()) > 10 ** 5 for qy in (0, 1) for qx in (0, 1))
    errs = {"sqrt": ulps(_lib.coords_math_host("sqrt", s), np.sqrt(s)), "atan": ulps(_lib.coords_math_host("atan", a), np.arctan(a)),
            "atan2": ulps(_lib.coords_math_host("atan2", y, x), np.arctan2(y, x))}
    for op, e in errs.items():
        print("%s: %.3g ulp from numpy, bound %.3g" % (op, e, HELPER_ULP[op]))
    assert all(HELPER_ULP[op] <= 4.0 and errs[op] <= HELPER_ULP[op] for op in errs), errs


# ---------------------------------------------------------------------------------------------- 2. the maps
def _cameras():
    """{model: [parameter vectors]}: with and without R / new_K, through the package's own assembly"""
    from lerf_pytorch_amd import coords
    return {"fisheye": [coords.fisheye_params(LR.FISH_K, LR.FISH_DIST, LR.FISH_R, LR.FISH_NEW_K), coords.fisheye_params(LR.FISH_K, LR.FISH_DIST),
                        coords.fisheye_params(LR.FISH_K, None, LR.FISH_R)],
            "equirect": [coords.equirect_params(LR.PANO_HW, LR.VIEW_K, LR.VIEW_R), coords.equirect_params(LR.PANO_HW, LR.VIEW_K)]}


def test_params_are_the_restatements():
    cams = _cameras()
    assert np.allclose(cams["fisheye"][0], LR.fisheye_params_np(LR.FISH_K, LR.FISH_DIST, LR.FISH_R, LR.FISH_NEW_K), rtol=1e-13, atol=0)
    assert np.allclose(cams["fisheye"][1], LR.fisheye_params_np(LR.FISH_K, LR.FISH_DIST), rtol=1e-13, atol=1e-18)
    assert np.array_equal(cams["fisheye"][2][13:], np.zeros(4)) and cams["fisheye"][0].shape == (17,)
    assert np.allclose(cams["equirect"][0], LR.equirect_params_np(LR.PANO_HW, LR.VIEW_K, LR.VIEW_R), rtol=1e-13, atol=0)
    assert np.array_equal(cams["equirect"][1][9:], [192 / (2 * np.pi), 96 / np.pi, 95.5, 47.5]) and cams["equirect"][1].shape == (13,)


@pytest.mark.parametrize("hw", HWS)
@pytest.mark.parametrize("model", MODELS)
def test_maps_against_the_restatement_in_both_dtypes(model, hw):
    for k, p in enumerate(_cameras()[model]):
        for origin in ((0, 0), ORIGIN):
            ref = LR.model_map_np(model, p, hw, origin)
            got = _lib.coords_build_host(model, p, hw, origin=origin)
            assert got.dtype == np.float64 and np.all(np.isfinite(ref))
            map_close(got, ref, "%s camera %d %s at %s" % (model, k, hw, origin))
            got32 = _lib.coords_build_host(model, p, hw, dtype=np.float32, origin=origin)
            assert got32.dtype == np.float32 and R.same_bits(got32, got.astype(np.float32))          # the float64 map rounded once


def test_fisheye_principal_pixel_maps_to_itself_exactly():
    """integer cx, cy, R = I, new_K = K with powers of two for focal lengths: x = y = 0 exactly at pixel (18, 26), r == 0, the select"""
    F = _lib.coords_build_host("fisheye", FISH_EXACT, (37, 53))
    assert F[18, 26, 0] == 18.0 and F[18, 26, 1] == 26.0 and np.all(np.isfinite(F))
    map_close(F, LR.model_map_np("fisheye", FISH_EXACT, (37, 53)), "fisheye, exact parameters")


def test_fisheye_without_distortion_is_the_equidistant_projection():
    p = FISH_EXACT.copy()
    p[13:] = 0.0
    F = _lib.coords_build_host("fisheye", p, (37, 53))
    j = np.arange(53, dtype=np.float64)
    want = 64.0 * np.arctan((j - 26.0) / 64.0)                             # col - cx = fx atan((j - cx) / fx) on the central row
    err = np.abs((F[18, :, 1] - 26.0) - want) / np.maximum(1.0, np.abs(F[18, :, 1]))
    print("max error %.3g" % float(err.max()))
    assert float(err.max()) <= MAP_TOL and np.all(F[18, :, 0] == 18.0)


def test_equirect_anchors():
    E = _lib.coords_build_host("equirect", VIEW_EXACT, (37, 53))
    assert E[18, 26, 0] == 47.5 and E[18, 26, 1] == 95.5                   # the principal pixel lands on (cyp, cxp) exactly
    assert np.all(E[:, 26, 1] == 95.5)                                     # lon = 0 down the central column
    # lon is antisymmetric about the central column bit for bit; cxp + sx lon rounds the sum, so it is read off a panorama with cxp = 0
    p0 = VIEW_EXACT.copy()
    p0[11] = 0.0
    E0 = _lib.coords_build_host("equirect", p0, (37, 53))
    assert R.same_bits(E0[:, :26, 1][:, ::-1], -E0[:, 27:, 1]) and np.all(E0[:, 27:, 1] > 0)
    assert R.same_bits(E0[..., 0], E[..., 0])                                                         # rows do not depend on cxp
    P = _lib.coords_build_host("equirect", np.concatenate([POLE_EXACT[:9], p0[9:]]), (37, 53))       # lon beyond +-pi/2: the -+pi branch
    assert R.same_bits(P[:, :26, 1][:, ::-1], -P[:, 27:, 1]) and float(np.abs(P[:18, 27:, 1]).min()) > p0[9] * HALF_PI


def test_compose_with_the_inverse_is_the_identity_on_a_fisheye_map():
    """F: a 48 x 64 pinhole view of a 40 x 56 fisheye frame; invert(F) distorts; F(invert(F)(q)) = q wherever the inverse exists"""
    from lerf_pytorch_amd import coords
    K = np.array([[40.0, 0, 27.5], [0, 40.0, 19.5], [0, 0, 1]])
    new_K = np.array([[30.0, 0, 31.5], [0, 30.0, 23.5], [0, 0, 1]])
    F = coords.fisheye_undistort_rectify(K, LR.FISH_DIST, None, new_K, (48, 64))
    tol = 1e-9
    G = coords.invert(F, (40, 56), tol=tol)
    ok = ~np.isnan(G).any(-1)
    assert ok.mean() > 0.9
    C = coords.compose(F, G)
    ii, jj = np.meshgrid(np.arange(40.0), np.arange(56.0), indexing="ij")
    err = np.maximum(np.abs(C[..., 0] - ii), np.abs(C[..., 1] - jj))[ok]
    print("inverse exists at %.1f %%, max |F(G(q)) - q| = %.3g" % (100 * ok.mean(), float(err.max())))
    assert float(err.max()) <= tol


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("model", MODELS)
def test_tile_with_an_origin_inside_a_sentinel_filled_buffer(model, dt):
    p = _cameras()[model][0]
    whole = _lib.coords_build_host(model, p, (48, 144), dtype=dt)
    buf = np.full((37 + 5, 131 + 6, 2), -7.0, dt)
    tile = buf[2:2 + 37, 3:3 + 131]
    _lib.coords_build_host(model, p, (37, 131), out=tile, origin=ORIGIN)
    assert R.same_bits(np.ascontiguousarray(tile), np.ascontiguousarray(whole[3:40, 7:138]))
    assert int((buf == -7.0).sum()) == buf.size - tile.size


# ---------------------------------------------------------------------------------------------- 3. the backward
@pytest.mark.parametrize("hw", BWD_HWS)
@pytest.mark.parametrize("model", MODELS)
def test_backward_against_autograd_of_the_restatement(model, hw):
    p, _ = lens_case(model, hw)
    assert_smooth(model, p, hw, ORIGIN)
    g = upstream(hw)
    got = _lib.coords_build_bwd_host(model, p, g, origin=ORIGIN)
    assert got.shape == p.shape and got.dtype == np.float64 and np.all(got != 0)
    adj_close(got, LR.params_grad_ref(model, p, g, hw, ORIGIN), "%s %s" % (model, hw))


def _pinhole_grad(p, i, j, g):
    """the gradient of ONE entry of the pinhole col = fx X / Wh + cx, row = fy Y / Wh + cy w.r.t. the 17 fisheye parameters"""
    t = torch.from_numpy(p).requires_grad_(True)
    Wh = t[6] * j + t[7] * i + t[8]
    loss = (t[10] * ((t[3] * j + t[4] * i + t[5]) / Wh) + t[12]) * g[0] + (t[9] * ((t[0] * j + t[1] * i + t[2]) / Wh) + t[11]) * g[1]
    return torch.autograd.grad(loss, t)[0].numpy()


def test_the_selects_at_the_principal_ray_a_pole_and_behind_the_camera():
    """What divides by r (fisheye) or h (equirect) is 0 by a select where they are 0, so the entry contributes what is left and no NaN:
    at r == 0 the model is the pinhole's (s = 1, d s / d r = 0), so the entry gives the pinhole's gradient and nothing to k1 .. k4; at a
    pole lon and lat are constants, so the entry gives g to (cxp, cyp), g.r lat to sy and nothing to the matrix.  An entry behind the
    camera (Wh <= 0) is not finite: it contributes exactly 0 whatever the upstream holds, a NaN included."""
    hw = (37, 53)
    # --- fisheye, the principal pixel alone
    g = np.zeros(hw + (2,))
    g[18, 26] = (0.75, -1.25)
    got = _lib.coords_build_bwd_host("fisheye", FISH_EXACT, g)
    assert np.all(np.isfinite(got)) and not np.any(got[13:]) and got[11] == -1.25 and got[12] == 0.75 and got[9] == 0 and got[10] == 0
    adj_close(got, _pinhole_grad(FISH_EXACT, 18.0, 26.0, g[18, 26]), "fisheye at r == 0")
    assert np.all(got[[0, 1, 2, 3, 4, 5]] != 0)
    # --- fisheye, the whole map with the principal pixel in it: the rest by autograd, that entry by the pinhole
    g = upstream(hw)
    got = _lib.coords_build_bwd_host("fisheye", FISH_EXACT, g)
    rest = g.copy()
    rest[18, 26] = 0.0
    p = torch.from_numpy(FISH_EXACT).requires_grad_(True)
    v, u = LR._grid(p, hw, (0, 0))
    u = torch.where((v == 18) & (u == 26), u + 0.5, u)                     # evaluate that entry elsewhere: its weight is 0
    X, Y, Z = p[0] * u + p[1] * v + p[2], p[3] * u + p[4] * v + p[5], p[6] * u + p[7] * v + p[8]
    x, y = X / Z, Y / Z
    r = torch.sqrt(x * x + y * y)
    th = torch.atan(r)
    th2 = th * th
    s = th * (1 + th2 * (p[13] + th2 * (p[14] + th2 * (p[15] + th2 * p[16])))) / r
    ref, = torch.autograd.grad((torch.stack([p[10] * (y * s) + p[12], p[9] * (x * s) + p[11]], -1) * torch.from_numpy(rest)).sum(), p)
    adj_close(got, ref.numpy() + _pinhole_grad(FISH_EXACT, 18.0, 26.0, g[18, 26]), "fisheye through r == 0")
    # --- equirect, the pole alone and inside a map
    E = _lib.coords_build_host("equirect", POLE_EXACT, hw)
    assert E[18, 26, 0] == 47.5 - (96 / np.pi) * HALF_PI and E[18, 26, 1] == 95.5 and np.all(np.isfinite(E))   # lat = -pi/2, lon = 0
    g = np.zeros(hw + (2,))
    g[18, 26] = (0.75, -1.25)
    got = _lib.coords_build_bwd_host("equirect", POLE_EXACT, g)
    assert not np.any(got[:9]) and got[9] == 0 and got[10] == 0.75 * -HALF_PI and got[11] == -1.25 and got[12] == 0.75
    g = upstream(hw)
    got = _lib.coords_build_bwd_host("equirect", POLE_EXACT, g)
    rest = g.copy()
    rest[18, 26] = 0.0
    p = torch.from_numpy(POLE_EXACT).requires_grad_(True)
    v, u = LR._grid(p, hw, (0, 0))
    u = torch.where((v == 18) & (u == 26), u + 0.5, u)
    X, Y, Z = p[0] * u + p[1] * v + p[2], p[3] * u + p[4] * v + p[5], p[6] * u + p[7] * v + p[8]
    out = torch.stack([p[12] + p[10] * torch.atan2(Y, torch.sqrt(X * X + Z * Z)), p[11] + p[9] * torch.atan2(X, Z)], -1)
    ref, = torch.autograd.grad((out * torch.from_numpy(rest)).sum(), p)
    at_pole = np.zeros(13)
    at_pole[10], at_pole[11], at_pole[12] = g[18, 26, 0] * -HALF_PI, g[18, 26, 1], g[18, 26, 0]
    adj_close(got, ref.numpy() + at_pole, "equirect through a pole")
    # --- fisheye, behind the camera: columns 8 .. of BEHIND are NaN, they contribute exactly 0, a NaN upstream there does not leak
    hw = (6, 17)
    F = _lib.coords_build_host("fisheye", BEHIND, hw)
    mask = np.zeros(hw, bool)
    mask[:, 8:] = True
    assert np.array_equal(np.isnan(F).all(-1), mask) and np.array_equal(np.isnan(F).any(-1), mask)
    map_close(F, LR.model_map_np("fisheye", BEHIND, hw), "fisheye with rays behind the camera")
    g = upstream(hw, 9)
    g[2, 8, 0], g[3, 12, 1], g[0, 16, 0] = np.nan, np.inf, np.nan
    got = _lib.coords_build_bwd_host("fisheye", BEHIND, g)
    assert np.all(np.isfinite(got)) and np.all(got != 0)
    front = np.where(mask[..., None], 0.0, g)
    assert R.same_bits(got, _lib.coords_build_bwd_host("fisheye", BEHIND, front))
    assert not np.any(_lib.coords_build_bwd_host("fisheye", BEHIND, np.where(mask[..., None], g, 0.0)))
    g2 = upstream(hw, 9)
    g2[1, 3, 1] = np.nan                                                   # a NaN upstream at a finite point propagates
    assert np.isnan(_lib.coords_build_bwd_host("fisheye", BEHIND, g2)[11])


@pytest.mark.parametrize("model", MODELS)
def test_accumulate_contract_and_a_batch_of_sets(model):
    L = _lib.lib()
    hw, n = (5, 65), LR.N_PARAMS[model]
    ps = np.stack([lens_case(model, hw, (1, 2))[0] * (1.0 + 0.01 * s) for s in range(3)])
    gs = np.stack([upstream(hw, 20 + s) for s in range(3)])
    singles = np.stack([_lib.coords_build_bwd_host(model, ps[s], gs[s], origin=(1, 2)) for s in range(3)])
    assert R.same_bits(_lib.coords_build_bwd_host(model, ps, gs, origin=(1, 2)), singles)            # B sets = B single calls
    assert R.same_bits(_lib.coords_build_bwd_host(model, ps[1], gs[1], origin=(1, 2)), singles[1])   # and a call repeats itself
    pre = np.random.default_rng(12).standard_normal((3, n))
    buf = pre.copy()
    assert L.lerf_coords_build_bwd_host(CODE[model], ps.ctypes.data, 3, n, gs.ctypes.data, hw[0], hw[1], 1, 2, buf.ctypes.data) == 0
    assert R.same_bits(buf, pre + singles) and np.all(singles != 0)                                  # one add per value, after the sum


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_build_refusals_write_nothing():
    L = _lib.lib()
    out = np.full((4, 5, 2), -7.0)
    gp = np.full(21, -7.0)
    g = np.ones((4, 5, 2))
    p = np.concatenate([lens_case("fisheye", (4, 5))[0], np.zeros(4)])     # 21 finite doubles

    def fwd(model, n):
        return L.lerf_coords_build_host(model, p.ctypes.data, n, out.ctypes.data, _lib.LERF_F64, 10, 4, 5, 0, 0)

    def bwd(model, n):
        return L.lerf_coords_build_bwd_host(model, p.ctypes.data, 1, n, g.ctypes.data, 4, 5, 0, 0, gp.ctypes.data)

    for call in (fwd, bwd):
        for model, n in [(16, 9), (16, 13), (16, 21), (17, 17), (17, 9), (3, 9), (3, 17), (4, 17), (15, 17), (15, 13), (18, 13), (18, 17), (-1, 17)]:
            assert call(model, n) == EINVAL, (call.__name__, model, n)
    assert (out == -7.0).all() and (gp == -7.0).all()
    assert fwd(16, 17) == 0 and fwd(17, 13) == 0 and bwd(16, 17) == 0 and bwd(17, 13) == 0
    bad = p[:17].copy()
    bad[14] = np.inf
    out[:] = -7.0
    assert L.lerf_coords_build_host(16, bad.ctypes.data, 17, out.ctypes.data, _lib.LERF_F64, 10, 4, 5, 0, 0) == EINVAL and (out == -7.0).all()


def test_math_refusals_write_nothing():
    L = _lib.lib()
    x, y, out = np.ones(8), np.ones(8), np.full(8, -7.0)
    P = lambda a: None if a is None else a.ctypes.data
    for fn in (lambda op, a, b, n, o: L.lerf_coords_math_host(op, P(a), P(b), n, P(o)),):
        for args in [(3, x, y, 8, out), (-1, x, y, 8, out), (0, None, y, 8, out), (0, x, y, 8, None), (2, x, None, 8, out), (0, x, y, -1, out),
                     (1, x, y, 2 ** 31, out)]:
            assert fn(*args) == EINVAL, args
        assert (out == -7.0).all()
        assert fn(0, x, None, 8, out) == 0 and (out == 1.0).all()          # y is ignored by the unary ops
        assert fn(1, x, y, 0, out) == 0                                    # n == 0: nothing to do
    # the device entry point checks its arguments before it touches the device: refused without a GPU too
    assert L.lerf_coords_math(3, P(x), P(y), 8, P(out), None) == EINVAL and L.lerf_coords_math(0, None, None, 8, P(out), None) == EINVAL
    assert L.lerf_coords_math(2, P(x), None, 8, P(out), None) == EINVAL and L.lerf_coords_math(0, P(x), None, -1, P(out), None) == EINVAL
    with pytest.raises(ValueError, match="op"):
        _lib.coords_math_host("sin", x)
    with pytest.raises(ValueError, match="atan2"):
        _lib.coords_math_host("atan2", x)
    with pytest.raises(ValueError, match="shape"):
        _lib.coords_math_host("atan2", x, y[:4])


def test_python_argument_checks():
    from lerf_pytorch_amd import coords
    K, d = LR.FISH_K, LR.FISH_DIST
    skew = K + np.array([[0, 0.1, 0], [0, 0, 0], [0, 0, 0.0]])
    bad = [lambda: coords.fisheye_params(skew, d), lambda: coords.fisheye_params(K * 2.0, d), lambda: coords.fisheye_params(K[:2], d),
           lambda: coords.fisheye_params(K, d[:3]), lambda: coords.fisheye_params(K, np.zeros(8)), lambda: coords.fisheye_params(K, d, np.eye(2)),
           lambda: coords.fisheye_params(K, d, None, np.eye(4)), lambda: coords.fisheye_undistort_rectify(K, d, None, None, (0, 5)),
           lambda: coords.fisheye_undistort_rectify(K, d, None, None, (4, 5), dtype=np.float16),
           lambda: coords.equirect_params((0, 10), K), lambda: coords.equirect_params((96, 192), skew),
           lambda: coords.equirect_params((96, 192), K, np.eye(2)), lambda: coords.equirect_view((96, 192), K, None, (4, 0)),
           lambda: _lib.coords_build_host("fisheye", np.zeros(13), (4, 5)), lambda: _lib.coords_build_host("equirect", np.zeros(17), (4, 5)),
           lambda: _lib.coords_build_bwd_host("equirect", np.zeros(17), np.zeros((4, 5, 2)))]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
    # mixed host and device operands are refused by the torch twins before anything runs; no GPU is needed to see it
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    for call in (lambda: coords.fisheye_undistort_rectify_torch(t(K), t(d), None, None, (4, 5)),
                 lambda: coords.fisheye_undistort_rectify_torch(K, d, None, None, (4, 5)),
                 lambda: coords.equirect_view_torch((96, 192), t(K), None, (4, 5))):
        with pytest.raises(ValueError, match="device tensor"):
            call()
