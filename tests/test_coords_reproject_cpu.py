"""CPU-only: reproject by depth through its host twins (lerf_coords_reproject_host, lerf_coords_reproject_bwd_host: the kernels' own
statements of csrc/lerf_coords_models.h, the sums in the device's order).  The references do not import the library
(tests/coords_reproject_ref.py: numpy float64 statement by statement, and the same forward in torch float64 for autograd):

  1. the exports;
  2. the host twin against the restatement bit for bit: kinds, dtypes, tiles, a strided out at an origin, three sets, special depths;
  3. an exactly invertible camera: the identity map, zo == depth, depth and inverse depth on the same bits;
  4. a plane seen from two cameras: its homography within 1e-11 px;
  5. the adjoint against autograd (ADJ_TOL) and bit for bit against the restatement's ordered sums; invalid entries, NULL halves, accumulate;
  6. every refusal leaves a sentinel-filled arena untouched;
  7. reproject -> invert_raster with the depth test on an occluded scene.

The cases the GPU suite runs against these host twins are built here (cameras(), special_depth(), forward_cases(), occluded_scene()).
"""
import os
import re

import numpy as np
import pytest
import torch

import coords_ref as R
import coords_reproject_ref as PR
from conftest import REPO
from test_coords_grad_cpu import ADJ_TOL

from lerf_pytorch_amd import _lib, coords

EINVAL = -1
F32, F64 = _lib.LERF_F32, _lib.LERF_F64
KINDS = ["z", "inverse"]
K_EXACT = np.array([[32.0, 0.0, 16.0], [0.0, 32.0, 12.0], [0.0, 0.0, 1.0]])          # inverts exactly: 1/32, -1/2, -3/8
K_OTHER = np.array([[40.0, 0.0, 15.5], [0.0, 36.0, 11.5], [0.0, 0.0, 1.0]])
NAMES = ("lerf_coords_reproject", "lerf_coords_reproject_host", "lerf_coords_reproject_bwd_workspace_bytes", "lerf_coords_reproject_bwd",
         "lerf_coords_reproject_bwd_host")


def rotation(ax=0.05, ay=-0.08, az=0.11):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def cameras():
    """three distinct parameter sets [3, 12]; set 2 has R = I and t_z = -3, so W = z - 3 exactly: depths below 3 lie behind view B"""
    return np.stack([coords.reproject_params(K_EXACT, K_OTHER, rotation(), [0.2, -0.1, 0.3]),
                     coords.reproject_params(K_OTHER, K_EXACT, rotation(-0.02, 0.03, -0.04), [-0.3, 0.25, 0.1]),
                     coords.reproject_params(K_EXACT, K_OTHER, None, [0.1, 0.2, -3.0])])


SPECIAL = [0.0, -0.0, -1.5, np.nan, np.inf, -np.inf, 1e-300, 1e300, 1e-38, 1e38, 3.0, 2.5]        # 3.0: W == 0 in set 2; 2.5: W < 0 there


def special_depth(hw, dt, seed=0):
    """a depth plane of `dt`: valid depths in [0.5, 6) with the SPECIAL values on the first entries of a stride-3 walk (as many as fit)"""
    d = np.random.default_rng(seed).uniform(0.5, 6.0, hw)
    flat = d.reshape(-1)
    n = min(len(SPECIAL), flat.size // 3)                      # 1 x 1: a valid depth (its special values: the single-entry test)
    flat[0:3 * n:3] = SPECIAL[:n]
    with np.errstate(over="ignore", under="ignore"):
        return d.astype(dt)


def forward_cases():
    """(kind, depth dtype, out dtype, hw): every mix on 5 x 67, both kinds on 1 x 1"""
    return [(k, dd, do, (5, 67)) for k in KINDS for dd in (np.float32, np.float64) for do in (np.float32, np.float64)] + \
           [(k, np.float64, np.float64, (1, 1)) for k in KINDS]


def padded_out(B, hw, dt):
    """(buffer, view): [B, oH, oW, 2] of row stride 2 (oW + 3) inside a sentinel-filled buffer"""
    buf = np.full((B, hw[0], hw[1] + 3, 2), -7.0, dt)
    return buf, buf[:, :, :hw[1]]


def occluded_scene():
    """(depth [24, 32], K, t): depth 8 with a square of depth 2 on rows 8..15 x cols 12..19; t moves the square 6 px and the rest 1.5 px"""
    d = np.full((24, 32), 8.0)
    d[8:16, 12:20] = 2.0
    return d, K_EXACT, np.array([-0.375, 0.0, 0.0])


def check_occluded(G, keys, G_nodepth):
    """the counts of the occluded scene: G and keys of invert_raster with the depth, G_nodepth without"""
    keys = np.asarray(keys).view(np.uint64)
    near = np.uint64(int(np.float32(2.0).view(np.uint32)) | 0x80000000)               # the sortable bits of the square's depth
    won = (keys >> np.uint64(32)) == near
    box = np.zeros((24, 32), bool)
    box[8:16, 6:14] = True
    assert int(won.sum()) == 64 and np.array_equal(won, box)
    src = G[won]
    assert src[:, 0].min() >= 8 and src[:, 0].max() <= 15 and src[:, 1].min() >= 12 and src[:, 1].max() <= 19
    hole = np.zeros((24, 32), bool)
    hole[8:16, 14:19] = True                                                          # what the square uncovered
    hole[:, 30:] = True                                                               # what left the frame's right edge
    nan = np.isnan(G[..., 0])
    assert int(nan.sum()) == 88 and np.array_equal(nan, hole) and np.array_equal(np.isnan(G[..., 1]), hole)
    assert int((R.bits(G) != R.bits(G_nodepth)).any(-1).sum()) == 32


# ---------------------------------------------------------------------------------------------- 1. exports
def test_exports_and_abi_version():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "lerf_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lerf_[a-z0-9_]+)\s*\(", src))
    for n in NAMES:
        assert n in declared and n in _lib.EXPORTS and hasattr(_lib.lib(), n), n
    assert _lib.lib().lerf_abi_version() == 7
    assert "LERF_DEPTH_Z = 0, LERF_DEPTH_INVERSE = 1" in src and re.search(r"#define LERF_REPROJECT_PARAMS 12\b", src)
    assert _lib.COORDS_MODELS.get("reproject") is None and 3 not in _lib.COORDS_MODELS.values()      # a family of its own, not a model code
    q = _lib.lib().lerf_coords_reproject_bwd_workspace_bytes
    assert q(1, 2160, 3840) == 12 * 60 * 34 * 8 and q(3, 1, 1) == 3 * 12 * 8 and q(2, 65, 65) == 2 * 12 * 4 * 8
    for bad in ((0, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 0)):
        assert q(*bad) == 0, bad


# ---------------------------------------------------------------------------------------------- 2. the host twin is the restatement
@pytest.mark.parametrize("kind,ddt,odt,hw", forward_cases())
def test_host_twin_is_the_restatement_bit_for_bit(kind, ddt, odt, hw):
    P, origin = cameras(), (3, 7)
    depth = np.stack([special_depth(hw, ddt, seed=s) for s in range(3)])
    ref_map, ref_zo = PR.forward(kind, P, depth, origin)
    with np.errstate(over="ignore"):
        ref_map, ref_zo = ref_map.astype(odt), ref_zo.astype(np.float32)                # rounded once
    buf, out = padded_out(3, hw, odt)
    got, zo = _lib.coords_reproject_host(kind, P, depth, odt, out=out, origin=origin, depth_out=True)
    assert got is out and R.same_bits(np.ascontiguousarray(got), ref_map) and R.same_bits(zo, ref_zo)
    assert (buf[:, :, hw[1]:] == -7.0).all()                                            # the padding columns
    assert np.isfinite(ref_map).any() and (hw == (1, 1) or np.isnan(ref_map).any())
    # a set of the batch is the single call; without depth_out the map is the same
    one = _lib.coords_reproject_host(kind, P[1], depth[1], odt, origin=origin)
    assert R.same_bits(one, ref_map[1])
    # one depth plane shared by the three sets
    shared = _lib.coords_reproject_host(kind, P, depth[0], odt, origin=origin)
    assert R.same_bits(shared, PR.forward(kind, P, depth[0], origin)[0].astype(odt))


@pytest.mark.parametrize("kind", KINDS)
def test_every_special_depth_on_a_single_entry(kind):
    P = cameras()
    for v in SPECIAL:
        for ddt in (np.float32, np.float64):
            with np.errstate(over="ignore", under="ignore"):
                d = np.full((1, 1), v).astype(ddt)
            got, zo = _lib.coords_reproject_host(kind, P[2], d, depth_out=True, origin=(3, 7))
            rm, rz = PR.forward(kind, P[2], d, (3, 7))
            with np.errstate(over="ignore"):
                rz = rz.astype(np.float32)
            assert R.same_bits(got, rm) and R.same_bits(zo, rz), (v, ddt)
    # the rules by name: a point at infinity has a finite entry and zo = +inf; W == 0 and W < 0 are not valid
    m, z = _lib.coords_reproject_host("inverse", P[0], np.zeros((1, 1)), depth_out=True)
    assert np.isfinite(m).all() and z[0, 0] == np.inf
    m, z = _lib.coords_reproject_host("inverse", P[0], np.full((1, 1), -0.0), depth_out=True)
    assert np.isfinite(m).all() and z[0, 0] == np.inf
    for v in (3.0, 2.5, 0.0, -1.0, np.nan, np.inf):
        m, z = _lib.coords_reproject_host("z", P[2], np.full((1, 1), v), depth_out=True)
        assert np.isnan(m).all() and np.isnan(z).all(), v
    m, z = _lib.coords_reproject_host("z", P[2], np.full((1, 1), 3.5), depth_out=True)
    assert np.isfinite(m).all() and z[0, 0] == 0.5


@pytest.mark.parametrize("kind", KINDS)
def test_a_tile_is_those_entries_of_the_whole_map(kind):
    P, full = cameras()[0], (12, 80)
    depth = special_depth(full, np.float32, seed=5)
    whole, wz = _lib.coords_reproject_host(kind, P, depth, depth_out=True)
    tile, tz = _lib.coords_reproject_host(kind, P, np.ascontiguousarray(depth[3:8, 7:74]), origin=(3, 7), depth_out=True)
    assert R.same_bits(tile, np.ascontiguousarray(whole[3:8, 7:74])) and R.same_bits(tz, np.ascontiguousarray(wz[3:8, 7:74]))


# ---------------------------------------------------------------------------------------------- 3. the exact identity
def test_identity_pose_is_the_identity_map_exactly():
    hw = (24, 32)
    ident = coords.from_flow(np.zeros(hw + (2,)))
    for zval in (2.0, 8.0):
        z = np.full(hw, zval, np.float32)
        m, zo = coords.reproject(z, K_EXACT, K_EXACT, return_depth=True)
        assert m.dtype == np.float64 and zo.dtype == np.float32 and R.same_bits(m, ident) and R.same_bits(zo, z)
        mi, zi = coords.reproject(1.0 / z, K_EXACT, K_EXACT, inverse_depth=True, return_depth=True)
        assert R.same_bits(mi, m) and R.same_bits(zi, zo)
    # integer depths: x * z is exact, so the quotient (x * z) / z is representable and the division returns it
    z = np.random.default_rng(1).integers(1, 65, hw).astype(np.float64)
    m, zo = coords.reproject(z, K_EXACT, K_EXACT, np.eye(3), np.zeros(3), return_depth=True)
    assert R.same_bits(m, ident) and R.same_bits(zo, z.astype(np.float32))
    assert R.same_bits(m, coords.from_homography(np.eye(3), hw))


# ---------------------------------------------------------------------------------------------- 4. a plane's homography
def plane_case():
    """(depth of the plane n . X = 5 through K_EXACT at 24 x 32, K_dst, R, t, the plane's homography source -> destination)"""
    hw = (24, 32)
    n = np.array([0.1, -0.2, 1.0])
    n = n / np.linalg.norm(n)
    Rm, t = rotation(), np.array([0.2, -0.1, 0.3])
    ii, jj = np.meshgrid(np.arange(hw[0], dtype=np.float64), np.arange(hw[1], dtype=np.float64), indexing="ij")
    rays = np.stack([jj, ii, np.ones(hw)], axis=-1) @ np.linalg.inv(K_EXACT).T                  # X = z * ray, ray.z = 1
    z = 5.0 / (rays @ n)
    H = K_OTHER @ (Rm + np.outer(t, n) / 5.0) @ np.linalg.inv(K_EXACT)
    return z, K_OTHER, Rm, t, H


def test_the_depth_of_a_plane_gives_the_planes_homography():
    z, Kd, Rm, t, H = plane_case()
    hw = z.shape
    ii, jj = np.meshgrid(np.arange(hw[0], dtype=np.float64), np.arange(hw[1], dtype=np.float64), indexing="ij")
    pts = np.stack([jj, ii, np.ones(hw)], axis=-1) @ H.T
    ref = np.stack([pts[..., 1] / pts[..., 2], pts[..., 0] / pts[..., 2]], axis=-1)
    for got in (coords.reproject(z, K_EXACT, Kd, Rm, t), coords.reproject(1.0 / z, K_EXACT, Kd, Rm, t, inverse_depth=True)):
        err = float(np.max(np.abs(got - ref)))
        print("plane-induced homography: max error %.3g px" % err)
        assert err <= 1e-11
    err = float(np.max(np.abs(PR.forward("z", coords.reproject_params(K_EXACT, Kd, Rm, t), z)[0] - ref)))
    print("the restatement alone: %.3g px" % err)
    assert err <= 1e-11
    # zo is the depth in the other view: the third coordinate of R X + t
    _, zo = coords.reproject(z, K_EXACT, Kd, Rm, t, return_depth=True)
    X = (np.stack([jj, ii, np.ones(hw)], axis=-1) @ np.linalg.inv(K_EXACT).T) * z[..., None]
    ref_z = ((X @ Rm.T) + t)[..., 2]
    assert ref_z.max() < 8.0 and np.max(np.abs(zo - ref_z)) <= 2.0 ** -24 * 8 + 1e-12          # one float32 rounding of a depth below 8


# ---------------------------------------------------------------------------------------------- 5. the adjoint
def adj_close(got, ref, what):
    scale = max(float(np.max(np.abs(ref))), 1.0)
    err = float(np.max(np.abs(got - ref)))
    print("%s: max error %.3g, scale %.3g, bound %.3g" % (what, err, scale, ADJ_TOL * scale))
    assert np.isfinite(err) and err <= ADJ_TOL * scale, what


def adjoint_case(kind, hw, with_gz, ddt=np.float64, seed=3):
    """(params, depth, grad_map, grad_depth_out or None): valid depths with a few entries that are not, and NaN / inf upstreams there"""
    rng = np.random.default_rng(seed)
    P = cameras()[0]
    d = rng.uniform(0.5, 6.0, hw)
    g, gz = rng.standard_normal(hw + (2,)), rng.standard_normal(hw)
    if hw[0] * hw[1] > 8:
        flat, fg, fz = d.reshape(-1), g.reshape(-1, 2), gz.reshape(-1)
        flat[1], flat[4], flat[7] = -2.0, np.nan, np.inf
        fg[1], fg[4, 0], fg[7, 1] = np.nan, np.inf, np.nan
        fz[1], fz[4] = np.nan, -np.inf
        if kind == "inverse":
            flat[5] = 0.0                                    # a point at infinity: a valid entry whose zo = +inf takes nothing from gz
            fz[5] = np.nan
    return P, d.astype(ddt), g, (gz if with_gz else None)


def autograd_ref(kind, P, depth, g, gz, origin=(0, 0)):
    """(d loss / d depth, d loss / d params) by CPU autograd of the restatement's forward; loss = sum over the VALID entries of
    map . g (+ zo . gz where zo is finite)"""
    p = torch.from_numpy(np.asarray(P, np.float64)).requires_grad_(True)
    d = torch.from_numpy(np.asarray(depth).astype(np.float64)).requires_grad_(True)
    m, zo = PR.forward_torch(kind, p, d, origin)
    zero = torch.zeros((), dtype=torch.float64)
    ok = torch.isfinite(m[..., 0])
    loss = (torch.where(ok[..., None], m * torch.where(ok[..., None], torch.from_numpy(g), zero), zero)).sum()
    if gz is not None:
        okz = ok & torch.isfinite(zo)
        loss = loss + torch.where(okz, zo * torch.where(okz, torch.from_numpy(gz), zero), zero).sum()
    gd, gp = torch.autograd.grad(loss, (d, p))
    return gd.numpy(), gp.numpy()


@pytest.mark.parametrize("hw", [(70, 130), (1, 1)])
@pytest.mark.parametrize("with_gz", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_adjoint_against_autograd_and_the_ordered_sums(kind, with_gz, hw):
    origin = (3, 7)
    for ddt in (np.float64, np.float32):
        P, d, g, gz = adjoint_case(kind, hw, with_gz, ddt)
        gd, gp = _lib.coords_reproject_bwd_host(kind, P, d, g, gz, origin=origin)
        rd, rp = autograd_ref(kind, P, d, g, gz, origin)
        adj_close(gd, rd, "%s %s grad_depth" % (kind, hw))
        adj_close(gp, rp, "%s %s grad_params" % (kind, hw))
        od, op = PR.grads(kind, P, d, g, gz, origin)
        assert R.same_bits(gd, od) and R.same_bits(gp, op)
        if hw != (1, 1):
            bad = ~np.isfinite(PR.forward(kind, P, d, origin)[0][..., 0])
            assert bad.sum() == 3 and np.all(R.bits(gd[bad]) == 0) and np.isfinite(gd).all() and np.isfinite(gp).all()
            assert np.all(gp != 0)


@pytest.mark.parametrize("kind", KINDS)
def test_adjoint_halves_accumulate_and_batches(kind):
    L = _lib.lib()
    hw, origin = (70, 130), (1, 2)
    P = cameras()
    cases = [adjoint_case(kind, hw, True, seed=10 + s) for s in range(3)]
    d, g, gz = (np.stack([c[k] for c in cases]) for k in (1, 2, 3))
    singles = [_lib.coords_reproject_bwd_host(kind, P[s], d[s], g[s], gz[s], origin=origin) for s in range(3)]
    gd, gp = _lib.coords_reproject_bwd_host(kind, P, d, g, gz, origin=origin)
    assert R.same_bits(gd, np.stack([s[0] for s in singles])) and R.same_bits(gp, np.stack([s[1] for s in singles]))
    # each half on its own is the same bits, the other is skipped
    only_d = _lib.coords_reproject_bwd_host(kind, P, d, g, gz, need=(True, False), origin=origin)
    only_p = _lib.coords_reproject_bwd_host(kind, P, d, g, gz, need=(False, True), origin=origin)
    assert only_d[1] is None and only_p[0] is None and R.same_bits(only_d[0], gd) and R.same_bits(only_p[1], gp)
    with pytest.raises(ValueError):
        _lib.coords_reproject_bwd_host(kind, P, d, g, gz, need=(False, False))
    args = (_lib.DEPTH_KINDS[kind], P.ctypes.data, 3, d.ctypes.data, F64, hw[0] * hw[1], g.ctypes.data, gz.ctypes.data, hw[0], hw[1], 1, 2)
    assert L.lerf_coords_reproject_bwd_host(*args, None, None) == EINVAL
    # one add per value into pre-filled buffers, after the sum
    rng = np.random.default_rng(2)
    pre_d, pre_p = rng.standard_normal(gd.shape), rng.standard_normal(gp.shape)
    buf_d, buf_p = pre_d.copy(), pre_p.copy()
    assert L.lerf_coords_reproject_bwd_host(*args, buf_d.ctypes.data, buf_p.ctypes.data) == 0
    assert R.same_bits(buf_d, pre_d + gd) and R.same_bits(buf_p, pre_p + gp)
    # one depth plane shared by the sets: one gradient plane per set
    sd, sp = _lib.coords_reproject_bwd_host(kind, P, d[0], g, gz, origin=origin)
    ref = [_lib.coords_reproject_bwd_host(kind, P[s], d[0], g[s], gz[s], origin=origin) for s in range(3)]
    assert sd.shape == (3,) + hw and R.same_bits(sd, np.stack([r[0] for r in ref])) and R.same_bits(sp, np.stack([r[1] for r in ref]))


# ---------------------------------------------------------------------------------------------- 6. refusals
def _ptr(x):
    return x if isinstance(x, (int, type(None))) else x.ctypes.data


def test_forward_refusals_write_nothing():
    L = _lib.lib()
    oH, oW, B = 4, 5, 2
    arena = np.full(4096, -7.0)                                   # every operand lives here: params | depth | out | zo, 64 doubles apart at least
    base = arena.ctypes.data
    assert base % 16 == 0
    P, D, O, Z = base, base + 8 * 64, base + 8 * 256, base + 8 * 1024
    span = 2 * oH * oW

    def call(kind=0, params=P, n_sets=B, depth=D, ddt=F64, dset=oH * oW, out=O, odt=F64, oset=span, stride=2 * oW, zo=Z, zset=oH * oW,
             h=oH, w=oW, i0=0, j0=0):
        return L.lerf_coords_reproject_host(kind, params, n_sets, depth, ddt, dset, out, odt, oset, stride, zo, zset, h, w, i0, j0)

    bad = [dict(kind=2), dict(kind=-1), dict(kind=3), dict(params=None), dict(depth=None), dict(out=None), dict(n_sets=0), dict(n_sets=-1),
           dict(n_sets=65536), dict(ddt=0), dict(ddt=3), dict(ddt=7), dict(odt=0), dict(odt=3), dict(h=0), dict(w=0), dict(h=-1),
           dict(i0=-1), dict(j0=-1), dict(i0=0x7fffffff), dict(j0=0x7fffffff), dict(stride=2 * oW - 2), dict(stride=2 * oW + 1),
           dict(params=P + 4), dict(depth=D + 4), dict(depth=D + 2, ddt=F32), dict(out=O + 8), dict(out=O + 4, odt=F32), dict(zo=Z + 2),
           dict(dset=-1), dict(dset=oH * oW - 1), dict(oset=-2), dict(oset=span + 1), dict(oset=span - 2), dict(oset=0), dict(zset=oH * oW - 1),
           dict(zset=0), dict(zset=-1),
           dict(out=D), dict(out=D + 16 * 3), dict(out=P), dict(out=P + 16 * 11), dict(zo=D), dict(zo=P + 8), dict(zo=O), dict(zo=O + 8 * (2 * span - 1)),
           dict(depth=O + 8 * (2 * span - 1)), dict(params=Z + 4 * (2 * oH * oW - 1) - 4)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
    assert (arena == -7.0).all()
    # the same arena takes a good call: the table refuses nothing it should accept (a shared depth plane, no depth_out)
    arena[:24] = np.concatenate([cameras()[0], cameras()[1]])
    arena[64:64 + 2 * oH * oW] = 2.0
    assert call() == 0 and call(dset=0) == 0 and call(zo=None, zset=0) == 0 and call(n_sets=1, oset=0, zset=0, dset=0) == 0
    assert not (arena[256:256 + 2 * span] == -7.0).any() and (arena[256 + 2 * span:1024] == -7.0).all()
    # the wrappers
    d = np.full((oH, oW), 2.0)
    with pytest.raises(ValueError, match="kind"):
        _lib.coords_reproject_host("disparity", cameras()[0], d)
    with pytest.raises(ValueError, match="params"):
        _lib.coords_reproject_host("z", cameras()[0][:11], d)
    with pytest.raises(ValueError, match="params"):
        _lib.coords_reproject_host("z", cameras()[0].astype(np.float32), d)
    with pytest.raises(ValueError, match="depth"):
        _lib.coords_reproject_host("z", cameras()[0], d[0])
    with pytest.raises(ValueError, match="depth"):
        _lib.coords_reproject_host("z", cameras(), np.stack([d, d]))
    with pytest.raises(ValueError, match="depth_out"):
        _lib.coords_reproject_host("z", cameras()[0], d, depth_out=np.zeros((oH, oW)))


def test_backward_refusals_write_nothing():
    L = _lib.lib()
    oH, oW, B = 4, 5, 2
    n = oH * oW
    arena = np.full(4096, -7.0)
    base = arena.ctypes.data
    P, D, G, GZ, GD, GP, WS = (base + 8 * k for k in (0, 64, 256, 512, 768, 1024, 1280))
    ws_bytes = L.lerf_coords_reproject_bwd_workspace_bytes(B, oH, oW)
    assert ws_bytes == B * 12 * 8

    def host(kind=0, params=P, n_sets=B, depth=D, ddt=F64, dset=n, gm=G, gz=GZ, h=oH, w=oW, i0=0, j0=0, gd=GD, gp=GP):
        return L.lerf_coords_reproject_bwd_host(kind, params, n_sets, depth, ddt, dset, gm, gz, h, w, i0, j0, gd, gp)

    def device(ws=WS, nbytes=ws_bytes, gp=GP, gd=GD, n_sets=B):
        return L.lerf_coords_reproject_bwd(0, P, n_sets, D, F64, n, G, GZ, oH, oW, 0, 0, gd, gp, ws, nbytes, None)

    bad = [dict(kind=2), dict(kind=-1), dict(params=None), dict(depth=None), dict(gm=None), dict(gd=None, gp=None), dict(n_sets=0),
           dict(n_sets=65536), dict(ddt=0), dict(ddt=3), dict(h=0), dict(w=0), dict(i0=-1), dict(j0=-1), dict(i0=0x7fffffff),
           dict(params=P + 4), dict(depth=D + 4), dict(gm=G + 8), dict(gz=GZ + 4), dict(gd=GD + 4), dict(gp=GP + 4), dict(dset=-1),
           dict(dset=n - 1), dict(gd=D), dict(gd=D + 8 * (2 * n - 1)), dict(gd=P + 8), dict(gd=G), dict(gd=G + 8 * (4 * n - 1)), dict(gd=GZ),
           dict(gp=P), dict(gp=P + 8 * 23), dict(gp=D), dict(gp=G + 16), dict(gp=GZ + 8), dict(gp=GD + 8 * (2 * n - 1)), dict(gd=GP + 8 * 23)]
    for kw in bad:
        assert host(**kw) == EINVAL, kw
    # the device entry point refuses a bad workspace (and everything above) before it touches the device
    for kw in (dict(ws=None), dict(nbytes=ws_bytes - 1), dict(nbytes=0), dict(ws=WS + 8), dict(ws=G), dict(ws=GD + 8 * (2 * n - 1)), dict(ws=GP),
               dict(ws=P + 8 * 23), dict(ws=D), dict(ws=GZ), dict(gd=None, gp=None), dict(n_sets=0)):
        assert device(**kw) == EINVAL, kw
    assert (arena == -7.0).all()
    arena[:24] = np.concatenate([cameras()[0], cameras()[1]])
    arena[64:64 + 2 * n] = 2.0
    arena[256:256 + 4 * n], arena[512:512 + 2 * n], arena[768:768 + 2 * n], arena[1024:1024 + 24] = 1.0, 1.0, 0.0, 0.0
    assert host() == 0 and host(gz=None) == 0 and host(gd=None) == 0 and host(gp=None) == 0 and host(dset=0) == 0
    assert np.all(arena[768:768 + 2 * n] != 0.0) and np.all(arena[1024:1024 + 24] != 0.0) and (arena[1024 + 24:] == -7.0).all()
    d, g = np.full((oH, oW), 2.0), np.ones((oH, oW, 2))
    with pytest.raises(ValueError, match="grad_map"):
        _lib.coords_reproject_bwd_host("z", cameras()[0], d, None)
    with pytest.raises(ValueError, match="grad_map"):
        _lib.coords_reproject_bwd_host("z", cameras()[0], d, g.astype(np.float32))
    with pytest.raises(ValueError, match="grad_depth_out"):
        _lib.coords_reproject_bwd_host("z", cameras()[0], d, g, np.ones((oH, oW + 1)))
    with pytest.raises(ValueError, match="grad_params"):
        _lib.coords_reproject_bwd_host("z", cameras()[0], d, g, grad_params=np.zeros(9))


# ---------------------------------------------------------------------------------------------- 7. the chains, the Python layer
def test_forward_splat_with_occlusion_on_the_host():
    d, K, t = occluded_scene()
    m, z = coords.reproject(d, K, K, None, t, return_depth=True)
    assert z.dtype == np.float32 and m[8, 12, 1] == 6.0 and m[0, 0, 1] == -1.5
    G, keys = _lib.coords_invert_raster_host(m, (24, 32), depth=z, max_span=4, orient=1, return_keys=True)
    assert R.same_bits(G, coords.invert_raster(m, (24, 32), depth=z, max_span=4, orient=1))
    check_occluded(G, keys, coords.invert_raster(m, (24, 32), max_span=4, orient=1))


def test_reproject_params_and_the_python_refusals():
    Rm, t = rotation(), np.array([0.2, -0.1, 0.3])
    p = coords.reproject_params(K_EXACT, K_OTHER, Rm, t)
    assert p.shape == (12,) and p.dtype == np.float64
    assert np.array_equal(p[:9], (K_OTHER @ Rm @ np.linalg.inv(K_EXACT)).reshape(9)) and np.array_equal(p[9:], K_OTHER @ t)
    assert np.array_equal(coords.reproject_params(K_EXACT, K_EXACT), np.concatenate([np.eye(3).reshape(9), np.zeros(3)]))
    pb = coords.reproject_params(K_EXACT, K_OTHER, np.stack([Rm, np.eye(3)]), t)
    assert pb.shape == (2, 12) and np.array_equal(pb[0], p) and np.array_equal(pb[1], coords.reproject_params(K_EXACT, K_OTHER, None, t))
    assert np.allclose(PR.params_torch(*(torch.from_numpy(a) for a in (K_EXACT, K_OTHER, Rm, t))).numpy(), p, rtol=0, atol=1e-13)
    for bad in ([[40, 0, 15.5], [0, 36, 11.5], [0, 0, 2]], [[40, 0, 15.5], [0, 36, 11.5], [0.001, 0, 1]], [[40, 0, 15.5], [0, 36, 11.5], [0, 1, 1]]):
        with pytest.raises(ValueError, match="last row"):
            coords.reproject_params(K_EXACT, np.array(bad, np.float64))
        with pytest.raises(ValueError, match="last row"):
            coords.reproject(np.ones((3, 4)), K_EXACT, np.array(bad, np.float64))
    with pytest.raises(ValueError):
        coords.reproject_params(K_EXACT[:2], K_OTHER)
    with pytest.raises(ValueError):
        coords.reproject_params(K_EXACT, K_OTHER, np.stack([Rm, Rm]), np.stack([t, t, t]))
    with pytest.raises(ValueError, match="depth"):
        coords.reproject(np.ones(4), K_EXACT, K_OTHER)
    with pytest.raises(ValueError, match="autograd"):
        coords.reproject(torch.ones(3, 4, dtype=torch.float64, requires_grad=True), K_EXACT, K_OTHER)
    with pytest.raises(ValueError):
        coords.reproject_torch(torch.ones(3, 4, dtype=torch.float64), *(torch.from_numpy(a) for a in (K_EXACT, K_OTHER)))


def test_a_batch_is_one_call(monkeypatch):
    calls = []
    L = _lib.lib()
    real = L.lerf_coords_reproject_host
    monkeypatch.setattr(L, "lerf_coords_reproject_host", lambda *a: calls.append(a[2]) or real(*a))
    d = np.stack([special_depth((5, 67), np.float32, seed=s) for s in range(3)])
    Rs = np.stack([rotation(), np.eye(3), rotation(0.01, 0.02, 0.03)])
    got, zo = coords.reproject(d, K_EXACT, K_OTHER, Rs, [0.2, -0.1, 0.3], return_depth=True)
    assert calls == [3] and got.shape == (3, 5, 67, 2) and zo.shape == (3, 5, 67)
    for s in range(3):
        one, z1 = coords.reproject(d[s], K_EXACT, K_OTHER, Rs[s], [0.2, -0.1, 0.3], return_depth=True)
        assert R.same_bits(got[s], one) and R.same_bits(zo[s], z1)
    # one camera pair for a batch of depth planes; float32 maps
    got = coords.reproject(d, K_EXACT, K_OTHER, dtype=np.float32)
    assert got.dtype == np.float32 and R.same_bits(got[2], coords.reproject(d[2], K_EXACT, K_OTHER, dtype=np.float32))
