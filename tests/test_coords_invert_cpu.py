"""CPU-only: the map inverse's host twin (lerf_coords_invert_host: invert_point of csrc/lerf_coords_models.h in a plain loop) and
coords.invert / invert_flow on numpy arrays.

  1. exact cases: the identity, an integer translation, a map of one cell;
  2. the residual contract: compose(F, invert(F)) is within tol of the identity wherever the inverse is not NaN -- the solver's own
     stopping test recomputed by compose's identical arithmetic, so the bound is tol itself;
  3. agreement with the independent numpy restatement (tests/coords_invert_ref.py): the same NaN set and, elsewhere, within
     2 tol ||J^-1|| -- both satisfy |F(u) - q| <= tol -- on inputs the restatement itself shows to have no borderline entry; an
     affine map against the analytic inverse;
  4. special entries: NaN in F, NaN / +-inf in init, folds and constant maps, max_iter = 1;
  5. tiles in place and every dtype combination;
  6. the flow round trip;
  7. every refused argument.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import coords_invert_ref as IR
import coords_ref as R
from conftest import REPO

from lerf_pytorch_amd import _lib, coords

F_HW, HW = (37, 53), (40, 56)             # F's shape; the frame F points into = the inverse's shape.  Blocks are 4 x 64: ragged in both
TOL = 1e-9
M_ISC = np.array([[2.05, 0.12, 15.0], [-0.08, 1.95, 40.0], [1.5e-5, -1.0e-5, 1.0]])          # BASELINE config 4
EINVAL = -1


def _identity(hw):
    return coords.from_flow(np.zeros(tuple(hw) + (2,)))


def _flow(hw=F_HW):
    """a smooth sinusoidal displacement of a few pixels"""
    ii, jj = np.meshgrid(np.arange(hw[0], dtype=np.float64), np.arange(hw[1], dtype=np.float64), indexing="ij")
    return np.stack([2.5 * np.sin(jj / 9.0 + ii / 17.0) + 1.0 * np.cos(ii / 11.0), 3.0 * np.cos(ii / 7.0 - jj / 23.0) - 1.5 * np.sin(jj / 13.0)], axis=-1)


def _mesh_ctrl():
    rng = np.random.default_rng(0)
    a, b = np.meshgrid(np.linspace(0, HW[0] - 1, 5), np.linspace(0, HW[1] - 1, 6), indexing="ij")
    return np.stack([a, b], axis=-1) + rng.uniform(-2.5, 2.5, (5, 6, 2))


def invert_maps():
    """name -> F of the residual contract; shared with the GPU parity tests"""
    return {"barrel": coords.radial(HW, F_HW, -0.18, 0.02), "pincushion": coords.radial(HW, F_HW, 0.25, 0.0),
            "homography": coords.from_homography(M_ISC, (90, 120)), "mesh": coords.from_mesh(_mesh_ctrl(), F_HW, "bicubic"),
            "flow": coords.from_flow(_flow())}


def _targets(hw=HW, origin=(0, 0)):
    ii, jj = np.meshgrid(np.arange(hw[0]) + origin[0], np.arange(hw[1]) + origin[1], indexing="ij")
    return np.stack([ii, jj], axis=-1).astype(np.float64)


def _valid(G):
    nan = np.isnan(G)
    assert np.array_equal(nan[..., 0], nan[..., 1])                  # an entry is NaN in both coordinates or in neither
    return ~nan[..., 0]


def _residual(F, G, q=None):
    """max |compose(F, G) - q| over the entries of G that are not NaN, by compose's host twin"""
    ok = _valid(G)
    q = _targets(G.shape[:2]) if q is None else q
    c = _lib.coords_compose_host(np.ascontiguousarray(F), np.ascontiguousarray(G))
    return float(np.max(np.abs(c - q)[ok])) if ok.any() else 0.0


def test_exports():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "lerf_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lerf_[a-z0-9_]+)\s*\(", src))
    for n in ("lerf_coords_invert", "lerf_coords_invert_host"):
        assert n in declared and n in _lib.EXPORTS and hasattr(_lib.lib(), n), n


# ---------------------------------------------------------------------------------------------- 1. exact cases
def test_exact_cases():
    ident = _identity(F_HW)
    for got in (_lib.coords_invert_host(ident, F_HW), coords.invert(ident, F_HW), IR.invert(ident, F_HW)):
        assert R.same_bits(got, ident)
    # F[i, j] = (i + 3, j - 2): the target q is reached from q - (3, -2) where that lies inside F, and from nowhere else
    F = ident + np.array([3.0, -2.0])
    q = _targets(HW)
    u = q - np.array([3.0, -2.0])
    inside = (u[..., 0] >= 0) & (u[..., 0] <= F_HW[0] - 1) & (u[..., 1] >= 0) & (u[..., 1] <= F_HW[1] - 1)
    want = np.where(inside[..., None], u, np.nan)
    assert inside.any() and not inside.all()
    for got in (_lib.coords_invert_host(F, HW), IR.invert(F, HW)):
        assert R.same_bits(got, want)
    # one cell in either axis: F = 2 x 53 and 37 x 2 maps that stretch a frame
    for fhw in ((2, 53), (37, 2), (2, 2)):
        ii, jj = np.meshgrid(np.linspace(0.0, HW[0] - 1.0, fhw[0]), np.linspace(0.0, HW[1] - 1.0, fhw[1]), indexing="ij")
        F = np.stack([ii + 0.01 * jj, jj - 0.02 * ii], axis=-1)
        G = _lib.coords_invert_host(F, HW)
        assert _valid(G).mean() > 0.9 and _residual(F, G) <= TOL
        assert R.same_bits(G, IR.invert(F, HW))


# ---------------------------------------------------------------------------------------------- 2. the residual contract
@pytest.mark.parametrize("name", ["barrel", "pincushion", "homography", "mesh", "flow"])
def test_compose_with_the_inverse_is_the_identity_within_tol(name):
    F = invert_maps()[name]
    G = coords.invert(F, HW)
    assert G.dtype == np.float64 and G.shape == HW + (2,)
    ok = _valid(G)
    res = _residual(F, G)
    print("%s: %.1f %% of the targets reached, max residual %.3g (tol %.3g)" % (name, 100.0 * ok.mean(), res, TOL))
    assert ok.mean() > 0.5 and res <= TOL
    assert R.same_bits(G, _lib.coords_invert_host(F, HW, max_iter=16, tol=TOL))


# ---------------------------------------------------------------------------------------------- 3. the numpy restatement
@pytest.mark.parametrize("name", ["barrel", "pincushion", "homography", "mesh", "flow"])
def test_agreement_with_the_numpy_restatement(name):
    F = invert_maps()[name]
    ref, passes, resid, jinv = IR.invert(F, HW, max_iter=16, tol=TOL, info=True)
    okr = _valid(ref)
    # the input has no borderline entry, by the restatement alone: what it accepts converged in half the passes, what it fails is
    # far from converging
    worst_pass = int(passes[okr].max())
    least_fail = float(resid[~okr].min()) if (~okr).any() else np.inf
    print("%s: accepted within %d passes, failed entries end at a residual >= %.3g, max ||J^-1|| %.3g" % (name, worst_pass, least_fail, jinv))
    assert worst_pass <= 8 and least_fail > 1e-6
    G = _lib.coords_invert_host(F, HW, max_iter=16, tol=TOL)
    ok = _valid(G)
    assert np.array_equal(ok, okr)
    err = float(np.max(np.abs(G - ref)[ok]))
    print("max |G - G_ref| = %.3g, bound %.3g" % (err, 2 * TOL * jinv))
    assert err <= 2 * TOL * jinv


def test_inverse_of_an_affine_map_is_the_inverse_matrix():
    """F(u) = A u with A = rotation by 30 degrees, scale 1.7, offset: bilinear interpolation of F is exact, so the inverse is the
    map of the inverse matrix.  ||A^-1||_inf = (cos 30 + sin 30) / 1.7 = 0.80, so a residual <= tol puts u within 0.8 tol"""
    th = np.deg2rad(30.0)
    # (col, row, 1) -> (col, row, 1), like from_homography's matrices
    A = np.array([[1.7 * np.cos(th), -1.7 * np.sin(th), 30.0], [1.7 * np.sin(th), 1.7 * np.cos(th), -12.0], [0.0, 0.0, 1.0]])
    F = coords.from_homography(np.linalg.inv(A), F_HW)               # the map applies the inverse of its matrix: F(u) = A u
    want = coords.from_homography(A, HW)
    G = _lib.coords_invert_host(F, HW)
    ok = _valid(G)
    inside = (want[..., 0] >= 0) & (want[..., 0] <= F_HW[0] - 1) & (want[..., 1] >= 0) & (want[..., 1] <= F_HW[1] - 1)
    edge = 1e-6                                                       # a target within 1e-6 of F's border may fall on either side
    sure_in = (want[..., 0] >= edge) & (want[..., 0] <= F_HW[0] - 1 - edge) & (want[..., 1] >= edge) & (want[..., 1] <= F_HW[1] - 1 - edge)
    assert ok[sure_in].all() and not ok[~inside & ~sure_in].any() and 0.2 < ok.mean() < 0.9
    err = float(np.max(np.abs(G - want)[ok]))
    print("affine: %.1f %% reached, max |G - analytic| = %.3g, bound %.3g" % (100.0 * ok.mean(), err, 2 * TOL))
    assert err <= 2 * TOL


# ---------------------------------------------------------------------------------------------- 4. special entries
NAN_BLOCK = (slice(10, 14), slice(20, 25))


def special_cases():
    """(F, init or None, max_iter) of the special entries; shared with the GPU parity test.  Every operand is finite, NaN or +-inf
    by construction and is read inside its own bounds whatever it holds."""
    maps = invert_maps()
    F = maps["barrel"]
    clean = _lib.coords_invert_host(F, HW)
    Fn = F.copy()
    Fn[NAN_BLOCK] = np.nan
    init = np.where(np.isnan(clean), 5.0, clean)
    init[3, 4] = np.nan
    init[3, 5, 1] = np.nan
    init[7, 8] = [np.inf, -np.inf]
    init[7, 9] = [-np.inf, np.inf]
    init[20, 30, 0] = np.inf
    ii, jj = np.meshgrid(np.arange(F_HW[0], dtype=np.float64), np.arange(F_HW[1], dtype=np.float64), indexing="ij")
    fold = np.stack([(ii - 17.0) * (ii - 18.0) / 8.0, jj], axis=-1)    # rows 17 and 18 hold the same value: a cell with det = 0
    const = np.broadcast_to(np.array([3.5, 4.5]), F_HW + (2,)).copy()
    return {"nan_block": (Fn, None, 16), "nan_block_from_the_solution": (Fn, np.where(np.isnan(clean), 5.0, clean), 16),
            "init_nan_inf": (F, init, 16), "fold": (fold, None, 16), "constant": (const, None, 16),
            "one_pass": (maps["homography"], None, 1), "one_pass_init": (F, init, 1)}


def test_a_nan_block_in_f():
    F = invert_maps()["barrel"]
    clean = _lib.coords_invert_host(F, HW)
    okc = _valid(clean)
    i = np.minimum(np.floor(np.nan_to_num(clean[..., 0])), F_HW[0] - 2).astype(int)
    j = np.minimum(np.floor(np.nan_to_num(clean[..., 1])), F_HW[1] - 2).astype(int)
    rs, cs = NAN_BLOCK
    touches = okc & (i + 1 >= rs.start) & (i < rs.stop) & (j + 1 >= cs.start) & (j < cs.stop)     # the converged cell holds a NaN corner
    assert 10 < touches.sum() < okc.sum() // 4
    cases = special_cases()
    # started AT the solution, the one cell read is the converged cell: NaN for exactly the targets whose cell touches the block
    Fn, init, _ = cases["nan_block_from_the_solution"]
    G = _lib.coords_invert_host(Fn, HW, init=init)
    assert np.array_equal(~_valid(G), ~okc | touches)
    assert R.same_bits(np.where(np.isnan(G), 0.0, G), np.where(touches[..., None] | ~okc[..., None], 0.0, clean))
    # from the affine start the way to the solution may cross the block too: every such target is NaN, no other entry moves
    G = _lib.coords_invert_host(Fn, HW)
    ok = _valid(G)
    assert not ok[touches].any() and not ok[~okc].any()
    assert R.same_bits(G[ok], clean[ok]) and _residual(F, G) <= TOL
    assert R.same_bits(G, IR.invert(Fn, HW))


def test_nan_and_inf_in_init():
    F, init, _ = special_cases()["init_nan_inf"]
    G = _lib.coords_invert_host(F, HW, init=init)
    assert np.isnan(G[3, 4]).all() and np.isnan(G[3, 5]).all()
    clipped = init.copy()                                             # +-inf starts where the clip puts it
    clipped[7, 8], clipped[7, 9], clipped[20, 30, 0] = [F_HW[0] - 1, 0.0], [0.0, F_HW[1] - 1], F_HW[0] - 1
    assert R.same_bits(G, _lib.coords_invert_host(F, HW, init=clipped))
    assert R.same_bits(G, IR.invert(F, HW, init=init))
    assert _residual(F, G) <= TOL
    allnan = np.full(HW + (2,), np.nan)
    assert np.isnan(_lib.coords_invert_host(F, HW, init=allnan)).all()


def test_folds_and_constant_maps_give_nan():
    cases = special_cases()
    const, _, _ = cases["constant"]
    assert np.isnan(_lib.coords_invert_host(const, HW)).all()
    assert np.isnan(_lib.coords_invert_host(const, HW, init=_targets(HW))).all()
    fold, _, _ = cases["fold"]
    G = _lib.coords_invert_host(fold, HW, max_iter=64)
    ok = _valid(G)
    # rows 17 / 18 map to 0 and the parabola's least value is -1 / 32 there: target rows 1 .. 39 are reached from both branches or
    # not at all, nothing below the least value is reached, and whatever is returned satisfies the residual contract
    assert _residual(fold, G) <= TOL and not ok[:, F_HW[1]:].any()
    assert R.same_bits(G, IR.invert(fold, HW, max_iter=64))
    start_in_flat_cell = np.full(HW + (2,), 17.5)                     # every first pass reads the cell with det = 0
    start_in_flat_cell[..., 1] = _targets(HW)[..., 1]
    G = _lib.coords_invert_host(fold, HW, init=start_in_flat_cell)
    want = np.full(HW + (2,), np.nan)
    want[0, :F_HW[1]] = start_in_flat_cell[0, :F_HW[1]]               # target row 0 IS the flat cell's value: met at once
    assert R.same_bits(G, want)


def test_one_pass_returns_only_starts_that_already_satisfy_tol():
    cases = special_cases()
    F, _, _ = cases["one_pass"]
    q = _targets(HW)
    u0 = IR.start(F, q)
    uc, V, _, _ = IR.sample(F, u0)
    hit = (np.abs(V - q) <= TOL).all(axis=-1)
    G = _lib.coords_invert_host(F, HW, max_iter=1)
    assert R.same_bits(G, np.where(hit[..., None], uc, np.nan))
    F, init, _ = cases["one_pass_init"]
    full = _lib.coords_invert_host(F, HW)
    G = _lib.coords_invert_host(F, HW, init=init, max_iter=1)
    ok = _valid(G)
    assert ok.sum() > 100 and R.same_bits(G[ok], full[ok])            # the starts that ARE the solution come back as they are
    assert not ok[3, 4] and not ok[7, 8] and not ok[_valid(full) ^ True].any()
    ident = _identity(F_HW)
    assert R.same_bits(_lib.coords_invert_host(ident, F_HW, max_iter=1), ident)


# ---------------------------------------------------------------------------------------------- 5. tiles and layouts
def test_a_tile_in_place_equals_the_slice_of_the_whole():
    F = invert_maps()["mesh"]
    whole = _lib.coords_invert_host(F, HW)
    start = np.where(np.isnan(whole), 11.0, whole) + 0.25
    whole_i = _lib.coords_invert_host(F, HW, init=start)
    wide_f = np.full((F_HW[0], F_HW[1] + 3, 2), np.nan)
    wide_f[:, 2:F_HW[1] + 2] = F
    for dt in (np.float64, np.float32):
        buf = np.full((HW[0], HW[1] + 3, 2), -7.0, dtype=dt)
        tile = buf[5:16, 7:30]
        _lib.coords_invert_host(wide_f[:, 2:F_HW[1] + 2], (11, 23), out=tile, origin=(5, 7))
        assert R.same_bits(np.ascontiguousarray(tile), whole[5:16, 7:30].astype(dt))
        probe = buf.copy()
        probe[5:16, 7:30] = -7.0
        assert (probe == -7.0).all()
        _lib.coords_invert_host(F, (11, 23), init=start[5:16, 7:30], out=tile, origin=(5, 7))      # init: a strided tile view too
        assert R.same_bits(np.ascontiguousarray(tile), whole_i[5:16, 7:30].astype(dt))


def test_every_dtype_combination():
    F = invert_maps()["barrel"]
    start = coords.radial(F_HW, HW, 0.18, -0.02)                     # a rough analytic inverse as the start
    for fdt in (np.float64, np.float32):
        Ff = F.astype(fdt)
        for idt in (None, np.float64, np.float32):
            init = None if idt is None else start.astype(idt)
            g64 = _lib.coords_invert_host(Ff, HW, init=init, dtype=np.float64)
            g32 = _lib.coords_invert_host(Ff, HW, init=init, dtype=np.float32)
            assert g64.dtype == np.float64 and g32.dtype == np.float32
            assert R.same_bits(g32, g64.astype(np.float32)), (fdt, idt)          # the float64 result rounded once
            # float32 operands are promoted exactly: the same call on the promoted arrays
            assert R.same_bits(g64, _lib.coords_invert_host(Ff.astype(np.float64), HW, init=None if init is None else init.astype(np.float64)))
            assert _valid(g64).mean() > 0.5 and _residual(Ff.astype(np.float64), g64) <= TOL
    assert coords.invert(F.astype(np.float32), HW).dtype == np.float32                # the default dtype is the map's
    assert coords.invert(F.astype(np.float32), HW, dtype=np.float64).dtype == np.float64


def test_a_batch_of_maps_equals_single_calls():
    maps = invert_maps()
    batch = np.stack([maps["barrel"], maps["mesh"], maps["flow"]])
    starts = np.stack([np.where(np.isnan(g), 9.0, g) for g in (_lib.coords_invert_host(m, HW) for m in batch)]) + 0.125
    got = coords.invert(batch, HW)
    assert got.shape == (3,) + HW + (2,)
    for n in range(3):
        assert R.same_bits(got[n], _lib.coords_invert_host(batch[n], HW))
    got = coords.invert(batch, HW, init=starts, max_iter=12, tol=1e-8)
    for n in range(3):
        assert R.same_bits(got[n], _lib.coords_invert_host(batch[n], HW, init=starts[n], max_iter=12, tol=1e-8))


# ---------------------------------------------------------------------------------------------- 6. the flow round trip
def test_flow_round_trip():
    flow = _flow()
    b = coords.invert_flow(flow)
    assert b.shape == flow.shape and b.dtype == np.float64
    ok = _valid(b)
    ident = _identity(F_HW)
    back = _lib.coords_compose_host(coords.from_flow(flow), np.where(ok[..., None], ident + b, 0.0))
    err = float(np.max(np.abs(back - ident)[ok]))
    print("flow round trip: %.1f %% of the pixels are landed on, max error %.3g (tol %.3g)" % (100.0 * ok.mean(), err, TOL))
    assert 0.5 < ok.mean() < 1.0 and err <= TOL
    assert R.same_bits(b, coords.invert(coords.from_flow(flow), F_HW) - ident)
    two = coords.invert_flow(np.stack([flow, -0.5 * flow]))
    assert R.same_bits(two[0], b) and R.same_bits(two[1], coords.invert_flow(-0.5 * flow))


# ---------------------------------------------------------------------------------------------- 7. refusals
def _ptr(a):
    return a.ctypes.data


def test_every_refused_argument_returns_einval_and_writes_nothing():
    lib = _lib.lib()
    F64, F32 = _lib.LERF_F64, _lib.LERF_F32
    f = np.ascontiguousarray(_identity((4, 5)))
    ini = np.ones((6, 8, 2))
    out = np.full((6, 8, 2), -7.0)
    big = np.full((12, 8, 2), -7.0)                                   # out and an operand inside one buffer

    def inv(Fm=f, fdt=F64, sf=10, fH=4, fW=5, I=ini, idt=F64, si=16, o=out, dt=F64, so=16, oH=6, oW=8, i0=0, j0=0, it=16, tol=1e-9,
            foff=0, ioff=0, off=0, host=True):
        args = (None if Fm is None else _ptr(Fm) + foff, fdt, sf, fH, fW, None if I is None else _ptr(I) + ioff, idt, si,
                None if o is None else _ptr(o) + off, dt, so, oH, oW, i0, j0, it, C.c_double(tol))
        return lib.lerf_coords_invert_host(*args) if host else lib.lerf_coords_invert(*args, None)
    assert inv() == 0 and inv(I=None, idt=99, si=-3) == 0             # a null init: its dtype and stride are not looked at
    out[:] = -7.0
    for host in (True, False):                                        # the device entry point refuses before it touches the GPU
        calls = [inv(Fm=None, host=host), inv(o=None, host=host), inv(fdt=0, host=host), inv(idt=3, host=host), inv(dt=9, host=host),
                 inv(sf=9, host=host), inv(sf=8, host=host), inv(si=15, host=host), inv(si=14, host=host), inv(so=15, host=host),
                 inv(so=14, host=host), inv(fH=1, host=host), inv(fW=1, host=host), inv(fH=0, host=host), inv(oH=0, host=host),
                 inv(oW=0, host=host), inv(oH=-1, host=host), inv(foff=8, host=host), inv(ioff=8, host=host), inv(off=8, host=host),
                 inv(it=0, host=host), inv(it=65, host=host), inv(it=-1, host=host), inv(tol=-1e-9, host=host),
                 inv(tol=float("inf"), host=host), inv(tol=float("nan"), host=host), inv(i0=-1, host=host), inv(j0=-1, host=host),
                 inv(i0=2 ** 31 - 3, host=host),
                 inv(o=f, oH=4, oW=5, so=10, I=None, host=host),                                  # out IS f
                 inv(o=ini, host=host),                                                           # out IS init
                 inv(Fm=big, o=big, off=16 * 8 * 3, sf=16, fH=4, fW=5, I=None, host=host),        # out begins inside f's rows
                 inv(I=big, o=big, off=16 * 8 * 5, host=host)]                                    # out begins inside init's rows
        assert calls == [EINVAL] * len(calls), (host, calls)
    assert (out == -7.0).all() and (big == -7.0).all() and (ini == 1.0).all() and R.same_bits(f, _identity((4, 5)))
    # side by side in one buffer without sharing a byte: accepted
    assert inv(I=big, o=big, off=16 * 8 * 6) == 0
    assert (big[:6] == -7.0).all() and not (big[6:] == -7.0).any()
    # through the Python layer: a ValueError that names the entry point
    with pytest.raises(ValueError, match="lerf_coords_invert_host"):
        _lib.coords_invert_host(f, (6, 8), max_iter=0)
    with pytest.raises(ValueError, match="lerf_coords_invert_host"):
        _lib.coords_invert_host(f, (6, 8), tol=-1.0)
    with pytest.raises(ValueError, match="init must have out's shape"):
        _lib.coords_invert_host(f, (6, 8), init=np.ones((6, 7, 2)))
    with pytest.raises(ValueError):
        _lib.coords_invert_host(f[:, :1], (6, 8))


def test_coords_invert_refuses_mixed_operands_and_autograd():
    import torch
    f = _identity((4, 5))

    class Dev:                                                        # stands for a device tensor: invert looks at is_cuda
        is_cuda, ndim, shape, requires_grad = True, 3, (4, 5, 2), False
    with pytest.raises(ValueError, match="mixed"):
        coords.invert(f, (4, 5), init=Dev())
    with pytest.raises(ValueError, match="mixed"):
        coords.invert(Dev(), (4, 5), init=f)
    leaf = torch.from_numpy(f).requires_grad_(True)
    with pytest.raises(ValueError, match="autograd"):
        coords.invert(leaf, (4, 5))
    with pytest.raises(ValueError, match="autograd"):
        coords.invert(f, (4, 5), init=leaf)
    with pytest.raises(ValueError, match="autograd"):
        coords.invert_flow(leaf)
    with torch.no_grad():
        assert R.same_bits(coords.invert(leaf, (4, 5)), f)
    with pytest.raises(ValueError):
        coords.invert(f, (0, 5))
    with pytest.raises(ValueError):
        coords.invert(f[0], (4, 5))
    with pytest.raises(ValueError):
        coords.invert(np.stack([f, f]), (4, 5), init=f)
