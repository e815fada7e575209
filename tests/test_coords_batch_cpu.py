"""CPU-only: the batched forms of the chained coordinate-map operations through their host twins (lerf_coords_*_batched_host: the
functors of csrc/lerf_coords.hip under OnHost / ScatterOnHost with sets > 1) and coords.* on numpy batches.

  1. the exports;
  2. set s of every batched host twin equals the single-map host twin on sample s by bit pattern (B = 3: a clean sample, one with
     NaN, +-inf and 1e300 entries, one that folds), and the NaN sample leaves its neighbours' results unchanged;
  3. strides: padded set and row strides with a sentinel in every gap, tiles at a non-zero origin, float32 / float64 mixes;
  4. sharing: a shared outer map, F, init and depth; a shared grad_a is the single-map twin accumulated in set order, bit for bit;
     n_sets = 1 with strides 0 is the plain entry point, for valid calls and for any fuzzed argument tuple;
  5. every refused argument returns its code and writes nothing, on the host twins and (without a GPU) on the device entry points;
  6. coords.* on numpy batches: the per-sample results, from ONE call of the batched entry point.

The case generators are shared with the GPU suite (tests/test_gpu_coords_batch.py).
"""
import os
import re

import numpy as np
import pytest

import coords_ref as R
from conftest import REPO
from test_coords_cpu import _ctrl, _maps
from test_coords_grad_cpu import inner_map, upstream
from test_coords_raster_cpu import fold_map, smooth_map

from lerf_pytorch_amd import _lib, coords

B = 3
EINVAL, EUNSUPPORTED = -1, -2
F64, F32 = _lib.LERF_F64, _lib.LERF_F32
NEW = ["lerf_coords_mesh_batched", "lerf_coords_mesh_batched_host", "lerf_coords_mesh_bwd_batched", "lerf_coords_compose_batched",
       "lerf_coords_compose_batched_host", "lerf_coords_invert_batched", "lerf_coords_invert_batched_host",
       "lerf_coords_invert_raster_batched", "lerf_coords_invert_raster_batched_host", "lerf_coords_compose_bwd_batched",
       "lerf_coords_compose_bwd_batched_host", "lerf_coords_invert_bwd_batched", "lerf_coords_invert_bwd_batched_host"]
HWS = [(23, 31), (5, 67)]                  # the tile: odd sizes, one wider than a block of 64
INVERT_ITER = 4                            # at which the distorted sample still gains entries (checked below)


# ---------------------------------------------------------------------------------------------- cases, shared with the GPU suite
def spoil(m, seed):
    """m with NaN, +inf, -inf, 1e300 and -1e300 at scattered entries (both coordinates take turns)"""
    m = m.copy()
    rng = np.random.default_rng(seed)
    for k, v in enumerate([np.nan, np.inf, -np.inf, 1e300, -1e300] * 2):
        m[rng.integers(0, m.shape[0]), rng.integers(0, m.shape[1]), k % 2] = v
    return m


def cast(a, dt):
    with np.errstate(over="ignore"):           # 1e300 is inf in float32
        return a.astype(dt)


def mesh_case(ghw=(4, 5)):
    """ctrl [3, gh, gw, 2]: a jittered mesh, one with special entries, one whose middle columns are swapped (it folds)"""
    fold = _ctrl(ghw, None, seed=2)
    fold[:, [1, 2]] = fold[:, [2, 1]]
    return np.stack([_ctrl(ghw, None, seed=0), spoil(_ctrl(ghw, None, seed=1), 11), fold])


def compose_case(hw, a_hw=(20, 30)):
    """(A [3, aH, aW, 2], Bm [3, h, w, 2]): a lens map, one with special entries, a folded one; inner maps that spill over the border"""
    A = np.stack([_maps(a_hw=a_hw)[0], spoil(_maps(seed=6, a_hw=a_hw)[0], 12), fold_map(a_hw)])
    Bm = np.stack([inner_map(a_hw, hw, seed=3), spoil(inner_map(a_hw, hw, seed=4), 13), inner_map(a_hw, hw, seed=5)])
    return A, Bm


def invert_case(hw):
    """(F [3, fH, fW, 2], init [3, h, w, 2]) into the frame hw: an AFFINE map (the affine start solves it: one pass), a pincushion with
    special entries that needs its passes, a map whose rows fold back"""
    f_hw = (hw[0] + 6, hw[1] + 4)
    ii, jj = np.meshgrid(np.arange(f_hw[0], dtype=np.float64), np.arange(f_hw[1], dtype=np.float64), indexing="ij")
    a, b = (hw[0] + 2.0) / (f_hw[0] - 1), (hw[1] + 4.0) / (f_hw[1] - 1)          # it covers the frame with a margin on every side
    affine = np.stack([a * ii + 0.01 * jj - 1.5, b * jj + 0.02 * ii - 2.5], axis=-1)
    lens = spoil(coords.radial(hw, f_hw, 0.25, 0.0), 14)
    fold = np.stack([(ii - 7.0) * (ii - 8.0) / 4.0, jj], axis=-1)
    F = np.stack([affine, lens, fold])
    rng = np.random.default_rng(15)
    init = np.stack([rng.uniform(0, f_hw[0] - 1, (B,) + tuple(hw)), rng.uniform(0, f_hw[1] - 1, (B,) + tuple(hw))], axis=-1)
    init[1] = spoil(init[1], 16)
    return F, init


def raster_case(hw):
    """(F [3, fH, fW, 2], depth [3, fH, fW] float32) drawn into the frame hw: a smooth stretch, one with special entries, a fold"""
    f_hw = (max(hw[0] // 2 + 3, 2), max(hw[1] // 2 + 2, 2))
    F = np.stack([smooth_map(0.8, f_hw), spoil(smooth_map(2.0, f_hw), 17), 1.3 * fold_map(f_hw)])
    depth = (2.0 + np.cos(np.arange(B * f_hw[0] * f_hw[1], dtype=np.float64))).reshape((B,) + f_hw).astype(np.float32)
    depth[1, 1, 1] = np.nan
    return F, depth


def upstream_case(hw):
    g = np.stack([upstream(hw, seed=20 + s) for s in range(B)])
    g[1, 0, 0, 1] = np.nan
    return g


def padded(a, pad_rows=2, pad_cols=3, pad_sets=1, sentinel=-7.0):
    """(buf, view): `a` [B, h, w, k] copied into a view of a wider sentinel-filled buffer -- rows and columns of padding around every
    map and a whole padding map between two sets, so the row stride and the set stride are both larger than a map needs"""
    n, h, w = a.shape[:3]
    buf = np.full((n * (1 + pad_sets), h + 2 * pad_rows, w + 2 * pad_cols) + a.shape[3:], sentinel, a.dtype)
    view = buf[::1 + pad_sets, pad_rows:pad_rows + h, pad_cols:pad_cols + w]
    view[...] = a
    return buf, view


def untouched(buf, view, sentinel=-7.0):
    """the buffer holds the sentinel everywhere outside the view"""
    keep = view.copy()
    view[...] = sentinel
    ok = bool((buf == sentinel).all())
    view[...] = keep
    return ok


# ---------------------------------------------------------------------------------------------- 1. exports
def test_exports_and_abi_version():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "lerf_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lerf_[a-z0-9_]+)\s*\(", src))
    for n in NEW:
        assert n in declared and n in _lib.EXPORTS and hasattr(_lib.lib(), n), n
    assert _lib.lib().lerf_abi_version() == 7


# ---------------------------------------------------------------------------------------------- 2. set s = the single-map call
@pytest.mark.parametrize("interp", ["bilinear", "bicubic"])
@pytest.mark.parametrize("hw", HWS)
def test_mesh_sets_equal_single_calls(interp, hw):
    ctrl = mesh_case()
    got = _lib.coords_mesh_host(ctrl, hw, interp)
    assert got.shape == (B,) + hw + (2,)
    for s in range(B):
        assert R.same_bits(got[s], _lib.coords_mesh_host(ctrl[s], hw, interp)), s
    clean = ctrl.copy()
    clean[1] = ctrl[0]
    other = _lib.coords_mesh_host(clean, hw, interp)
    assert R.same_bits(other[0], got[0]) and R.same_bits(other[2], got[2]) and np.isnan(got[1]).any() and not np.isnan(got[0]).any()


@pytest.mark.parametrize("hw", HWS)
def test_compose_sets_equal_single_calls(hw):
    A, Bm = compose_case(hw)
    got = _lib.coords_compose_host(A, Bm)
    for s in range(B):
        assert R.same_bits(got[s], _lib.coords_compose_host(A[s], Bm[s])), s
    A2, B2 = A.copy(), Bm.copy()
    A2[1], B2[1] = A[0], Bm[0]
    other = _lib.coords_compose_host(A2, B2)
    assert R.same_bits(other[0], got[0]) and R.same_bits(other[2], got[2]) and np.isnan(got[1]).any() and not np.isnan(got[0]).any()


@pytest.mark.parametrize("hw", HWS)
def test_invert_sets_equal_single_calls(hw):
    F, init = invert_case(hw)
    nans = lambda G: int(np.isnan(G[..., 0]).sum())
    for start in (None, init):
        got = _lib.coords_invert_host(F, hw, init=start, max_iter=INVERT_ITER)
        for s in range(B):
            assert R.same_bits(got[s], _lib.coords_invert_host(F[s], hw, init=None if start is None else start[s], max_iter=INVERT_ITER)), s
    got = _lib.coords_invert_host(F, hw, max_iter=INVERT_ITER)
    # sample 0 converges in one pass from the affine start; sample 1 still gains entries in its last pass; sample 2 folds
    assert nans(_lib.coords_invert_host(F[0], hw, max_iter=1)) == 0 and nans(got[0]) == 0
    if hw[0] > 8:
        assert nans(_lib.coords_invert_host(F[1], hw, max_iter=INVERT_ITER - 1)) > nans(got[1])
        assert nans(got[2]) > 0
    F2 = F.copy()
    F2[1] = F[0]
    other = _lib.coords_invert_host(F2, hw, max_iter=INVERT_ITER)
    assert R.same_bits(other[0], got[0]) and R.same_bits(other[2], got[2])


@pytest.mark.parametrize("with_depth", [False, True])
@pytest.mark.parametrize("hw", HWS)
def test_raster_sets_equal_single_calls(hw, with_depth):
    F, depth = raster_case(hw)
    d = depth if with_depth else None
    G, K = _lib.coords_invert_raster_host(F, hw, depth=d, return_keys=True)
    assert K.shape == (B,) + hw and K.dtype == np.uint64
    for s in range(B):
        g, k = _lib.coords_invert_raster_host(F[s], hw, depth=None if d is None else d[s], return_keys=True)
        assert R.same_bits(G[s], g) and np.array_equal(K[s], k), s
    F2 = F.copy()
    F2[1] = F[0]
    G2, K2 = _lib.coords_invert_raster_host(F2, hw, depth=d, return_keys=True)
    for s in (0, 2):
        assert R.same_bits(G2[s], G[s]) and np.array_equal(K2[s], K[s])
    assert (K[0] != np.uint64(2 ** 64 - 1)).any()


@pytest.mark.parametrize("hw", HWS)
def test_adjoint_sets_equal_single_calls(hw):
    A, Bm = compose_case(hw)
    g = upstream_case(hw)
    ga, gb = _lib.coords_compose_bwd_host(A, Bm, g)
    for s in range(B):
        a1, b1 = _lib.coords_compose_bwd_host(A[s], Bm[s], g[s])
        assert R.same_bits(ga[s], a1) and R.same_bits(gb[s], b1), s
    for need in ((True, False), (False, True)):
        ha, hb = _lib.coords_compose_bwd_host(A, Bm, g, need=need)
        assert (ha is None or R.same_bits(ha, ga)) and (hb is None or R.same_bits(hb, gb)) and (ha is None) != (hb is None)
    A2, B2, g2 = A.copy(), Bm.copy(), g.copy()
    A2[1], B2[1], g2[1] = A[0], Bm[0], g[0]
    oa, ob = _lib.coords_compose_bwd_host(A2, B2, g2)
    for s in (0, 2):
        assert R.same_bits(oa[s], ga[s]) and R.same_bits(ob[s], gb[s])
    F, _ = invert_case(hw)
    G = _lib.coords_invert_host(F, hw)
    gf = _lib.coords_invert_bwd_host(F, G, g)
    for s in range(B):
        assert R.same_bits(gf[s], _lib.coords_invert_bwd_host(F[s], G[s], g[s])), s
    assert np.any(gf[0] != 0)
    acc = np.full(F.shape, 0.5)
    assert _lib.coords_invert_bwd_host(F, G, g, grad_f=acc) is acc                    # the accumulate contract
    assert np.allclose(acc[0], 0.5 + gf[0], rtol=0, atol=1e-12 * max(np.abs(gf[0]).max(), 1.0))


# ---------------------------------------------------------------------------------------------- 3. strides, origins, dtypes
@pytest.mark.parametrize("dts", [(np.float64, np.float32, np.float64), (np.float32, np.float64, np.float32)])
def test_padded_strides_origins_and_dtype_mixes(dts):
    hw, origin = (9, 21), (3, 7)
    full = (hw[0] + 5, hw[1] + 9)
    ta, tb, to = dts
    # mesh: a tile at `origin` of the map `full`
    ctrl = cast(mesh_case(), ta)
    whole = _lib.coords_mesh_host(ctrl, full, "bicubic", to)
    buf, out = padded(np.zeros((B,) + hw + (2,), to))
    assert _lib.coords_mesh_host(ctrl, hw, "bicubic", out=out, origin=origin, full_hw=full) is out
    assert R.same_bits(np.ascontiguousarray(out), np.ascontiguousarray(whole[:, 3:12, 7:28])) and untouched(buf, out)
    # compose: every operand a padded view
    A, Bm = compose_case(hw)
    (_, a), (_, b) = padded(cast(A, ta), sentinel=np.nan), padded(cast(Bm, tb), sentinel=np.nan)
    buf, out = padded(np.zeros((B,) + hw + (2,), to))
    _lib.coords_compose_host(a, b, out=out)
    ref = np.stack([_lib.coords_compose_host(cast(A[s], ta), cast(Bm[s], tb), to) for s in range(B)])
    assert R.same_bits(np.ascontiguousarray(out), ref) and untouched(buf, out)
    # invert: a tile at `origin` of the whole inverse, with and without init
    F, init = invert_case(full)
    (_, f), (_, i) = padded(cast(F, ta), sentinel=np.nan), padded(cast(init[:, 3:12, 7:28], tb), sentinel=np.nan)
    for start in (None, i):
        buf, out = padded(np.zeros((B,) + hw + (2,), to))
        _lib.coords_invert_host(f, hw, init=start, out=out, origin=origin)
        ref = np.stack([_lib.coords_invert_host(cast(F[s], ta), hw, init=None if start is None else np.ascontiguousarray(start[s]),
                                                dtype=to, origin=origin) for s in range(B)])
        assert R.same_bits(np.ascontiguousarray(out), ref) and untouched(buf, out)
    # raster: a tile at `origin`
    F, depth = raster_case(full)
    (_, f) = padded(cast(F, ta), sentinel=np.nan)
    buf, out = padded(np.zeros((B,) + hw + (2,), to))
    _, K = _lib.coords_invert_raster_host(f, hw, depth=depth, out=out, origin=origin, return_keys=True)
    for s in range(B):
        g, k = _lib.coords_invert_raster_host(cast(F[s], ta), hw, depth=depth[s], dtype=to, origin=origin, return_keys=True)
        assert R.same_bits(np.ascontiguousarray(out[s]), g) and np.array_equal(K[s], k)
    assert untouched(buf, out)
    # the adjoints read padded maps
    A, Bm = compose_case(hw)
    g = upstream_case(hw)
    (_, a), (_, b) = padded(cast(A, ta), sentinel=np.nan), padded(cast(Bm, tb), sentinel=np.nan)
    ga, gb = _lib.coords_compose_bwd_host(a, b, g)
    for s in range(B):
        a1, b1 = _lib.coords_compose_bwd_host(cast(A[s], ta), cast(Bm[s], tb), g[s])
        assert R.same_bits(ga[s], a1) and R.same_bits(gb[s], b1)


def _p(a):
    return None if a is None else a.ctypes.data


def _compose_bwd_raw(fn, A, Bm, g, ga, gb, n, strides, stream=()):
    return fn(_p(A), F64, 2 * A.shape[-2], A.shape[-3], A.shape[-2], _p(Bm), F64, 2 * Bm.shape[-2], _p(g), Bm.shape[-3], Bm.shape[-2], _p(ga), _p(gb),
              n, *strides, *stream)


def test_padded_set_strides_of_the_dense_gradients():
    """the gradients are dense per set; the SET stride may still be larger than a set (the Python layer never asks for that)"""
    hw, a_hw = (5, 9), (6, 7)
    A, Bm = compose_case(hw, a_hw)
    g = upstream_case(hw)
    na, nb, pad = 2 * a_hw[0] * a_hw[1], 2 * hw[0] * hw[1], 6
    gbuf, gabuf, gbbuf = np.full((B, nb + pad), -7.0), np.full((B, na + pad), -7.0), np.full((B, nb + pad), -7.0)
    gbuf[:, :nb], gabuf[:, :na], gbbuf[:, :nb] = g.reshape(B, nb), 0.0, 0.0
    L = _lib.lib()
    rc = _compose_bwd_raw(L.lerf_coords_compose_bwd_batched_host, A, Bm, gbuf, gabuf, gbbuf, B, (na, nb, nb + pad, na + pad, nb + pad))
    assert rc == 0
    ga, gb = _lib.coords_compose_bwd_host(A, Bm, g)
    assert R.same_bits(gabuf[:, :na].reshape(A.shape), ga) and R.same_bits(gbbuf[:, :nb].reshape(Bm.shape), gb)
    assert (gabuf[:, na:] == -7.0).all() and (gbbuf[:, nb:] == -7.0).all() and (gbuf[:, nb:] == -7.0).all()
    F, _ = invert_case(hw)
    G = _lib.coords_invert_host(F, hw)
    nf = 2 * F.shape[1] * F.shape[2]
    gfbuf = np.full((B, nf + pad), -7.0)
    gfbuf[:, :nf] = 0.0
    rc = L.lerf_coords_invert_bwd_batched_host(_p(F), F64, 2 * F.shape[2], F.shape[1], F.shape[2], _p(G), F64, 2 * hw[1], _p(gbuf), hw[0], hw[1],
                                               _p(gfbuf), B, nf, nb, nb + pad, nf + pad)
    assert rc == 0
    assert R.same_bits(gfbuf[:, :nf].reshape(F.shape), _lib.coords_invert_bwd_host(F, G, g)) and (gfbuf[:, nf:] == -7.0).all()


# ---------------------------------------------------------------------------------------------- 4. sharing
def test_shared_operands():
    hw = (9, 21)
    A, Bm = compose_case(hw)
    got = _lib.coords_compose_host(A[0], Bm)                                   # one outer map for every inner map
    for s in range(B):
        assert R.same_bits(got[s], _lib.coords_compose_host(A[0], Bm[s]))
    F, init = invert_case(hw)
    got = _lib.coords_invert_host(F[0], hw, init=init)                         # one F, a start per set
    for s in range(B):
        assert R.same_bits(got[s], _lib.coords_invert_host(F[0], hw, init=init[s]))
    got = _lib.coords_invert_host(F, hw, init=init[0])                         # a map per set, one start
    for s in range(B):
        assert R.same_bits(got[s], _lib.coords_invert_host(F[s], hw, init=init[0]))
    F, depth = raster_case(hw)
    G, K = _lib.coords_invert_raster_host(F, hw, depth=depth[0], return_keys=True)        # one depth plane
    for s in range(B):
        g, k = _lib.coords_invert_raster_host(F[s], hw, depth=depth[0], return_keys=True)
        assert R.same_bits(G[s], g) and np.array_equal(K[s], k)


def test_a_shared_grad_a_is_the_single_twin_accumulated_in_set_order():
    hw = (9, 21)
    A, Bm = compose_case(hw)
    g = np.stack([upstream(hw, seed=30 + s) for s in range(B)])
    ga, gb = _lib.coords_compose_bwd_host(A[0], Bm, g)
    assert ga.shape == A[0].shape and gb.shape == Bm.shape
    acc = np.zeros(A[0].shape)
    for s in range(B):
        _, b1 = _lib.coords_compose_bwd_host(A[0], Bm[s], g[s], grad_outer=acc)
        assert R.same_bits(gb[s], b1)
    assert R.same_bits(ga, acc) and np.any(acc != 0)
    parts = sum(_lib.coords_compose_bwd_host(A[0], Bm[s], g[s], need=(True, False))[0] for s in range(B))
    assert np.allclose(ga, parts, rtol=0, atol=1e-12 * max(np.abs(parts).max(), 1.0))


def test_one_set_with_strides_zero_is_the_plain_entry_point():
    hw = (9, 21)
    A, Bm = compose_case(hw)
    a, b = A[1], Bm[1]
    L = _lib.lib()
    out = np.full(b.shape, -7.0)
    args = (_p(a), F64, 2 * a.shape[1], a.shape[0], a.shape[1], _p(b), F64, 2 * hw[1], _p(out), F64, 2 * hw[1], hw[0], hw[1])
    assert L.lerf_coords_compose_batched_host(*args, 1, 0, 0, 0) == 0
    assert R.same_bits(out, _lib.coords_compose_host(a, b))
    ctrl = mesh_case()[1]
    out = np.full(hw + (2,), -7.0)
    assert L.lerf_coords_mesh_batched_host(_p(ctrl), F64, ctrl.shape[0], ctrl.shape[1], 1, hw[0], hw[1], _p(out), F64, 2 * hw[1], hw[0], hw[1], 0, 0,
                                           1, 0, 0) == 0
    assert R.same_bits(out, _lib.coords_mesh_host(ctrl, hw, "bicubic"))
    F, _ = invert_case(hw)
    out, keys = np.full(hw + (2,), -7.0), np.zeros(hw, np.uint64)
    f = F[2]
    assert L.lerf_coords_invert_batched_host(_p(f), F64, 2 * f.shape[1], f.shape[0], f.shape[1], None, 0, 0, _p(out), F64, 2 * hw[1], hw[0], hw[1],
                                             0, 0, 16, 1e-9, 1, 0, 0, 0) == 0
    assert R.same_bits(out, _lib.coords_invert_host(f, hw))
    assert L.lerf_coords_invert_raster_batched_host(_p(f), F64, 2 * f.shape[1], f.shape[0], f.shape[1], None, _p(out), F64, 2 * hw[1], hw[0],
                                                    hw[1], 0, 0, 16, 0, _p(keys), 1, 0, 0, 0, 0) == 0
    g, k = _lib.coords_invert_raster_host(f, hw, return_keys=True)
    assert R.same_bits(out, g) and np.array_equal(keys, k)
    g = upstream(hw)
    ga, gb = np.zeros(a.shape), np.zeros(b.shape)
    assert _compose_bwd_raw(L.lerf_coords_compose_bwd_batched_host, a, b, g, ga, gb, 1, (0, 0, 0, 0, 0)) == 0
    ra, rb = _lib.coords_compose_bwd_host(a, b, g)
    assert R.same_bits(ga, ra) and R.same_bits(gb, rb)


def test_any_single_map_call_is_the_batched_call_of_one_set():
    """Not the valid calls alone: 2 000 argument tuples per chained operation from the generator of tools/fuzz_coords_args.py (a valid
    call on shapes <= 6 x 6 with zero to two arguments replaced by a value the contract tells apart; one arena holds every operand).
    The single-map host twin and the batched host twin with n_sets = 1 and every set stride 0 return the same code and leave the same
    bytes, and a refused call leaves the arena as it found it."""
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import fuzz_coords_args as Z
    L = _lib.lib()
    arena = Z.Arena()
    untouched_arena = arena.fresh.tobytes()
    for op in Z.CHAINED:
        single, batched = getattr(L, "lerf_coords_%s_host" % op), getattr(L, "lerf_coords_%s_batched_host" % op)
        codes = {0: 0, EINVAL: 0}
        for args, args_of_one_set in Z.single_and_batched(op, 2000, seed=1):
            rc, _ = Z.run_case(single, arena, args)
            left = arena.buf.tobytes()
            rc_b, _ = Z.run_case(batched, arena, args_of_one_set)
            assert rc_b == rc and arena.buf.tobytes() == left, (op, args)
            assert rc == 0 or left == untouched_arena, (op, args)
            codes[rc] += 1
        assert min(codes.values()) >= 500 and sum(codes.values()) == 2000, (op, codes)          # the generator accepts and refuses


# ---------------------------------------------------------------------------------------------- 5. refusals
def _refusal_calls(device):
    """(name, call(overrides) -> rc, the buffers that must stay untouched, the overrides that must be refused with their code) for
    every batched entry point; device: the device entry points (the same checks, made before anything touches the device -- the
    pointers are host memory that a refused call never reads)"""
    L = _lib.lib()
    suffix, stream = ("", (None,)) if device else ("_host", ())
    h, w, aH, aW, gh, gw = 4, 6, 5, 7, 3, 4
    span, a_span, c_span = 2 * h * w, 2 * aH * aW, 2 * gh * gw
    z = lambda *s: np.full(s, -7.0)
    A, Bm, out, init, g, ga, gb = z(B, aH, aW, 2), z(B, h, w, 2), z(B, h, w, 2), z(B, h, w, 2), z(B, h, w, 2), z(B, aH, aW, 2), z(B, h, w, 2)
    ctrl, depth, keys = z(B, gh, gw, 2), np.full((B, aH, aW), -7.0, np.float32), np.full((B, h, w), 7, np.uint64)
    held = [A, Bm, out, init, g, ga, gb, ctrl, depth, keys]
    bad_n = [(dict(n=0), EINVAL), (dict(n=65536), EUNSUPPORTED), (dict(n=-1), EINVAL)]

    def entry(name, head, strides, bad):
        fn = getattr(L, "lerf_coords_%s_batched%s" % (name, suffix))

        def call(**kw):
            s = dict(strides, n=B)
            s.update(kw)
            n = s.pop("n")
            return fn(*head, n, *[s[k] for k in strides], *stream)
        return name, call, bad + bad_n

    odd = lambda k, v: (dict([(k, v + 1)]), EINVAL)
    short = lambda k, v: (dict([(k, v - 2)]), EINVAL)             # a set extent beyond its stride: the sets overlap
    shared = lambda k: (dict([(k, 0)]), EINVAL)
    mesh = entry("mesh", (_p(ctrl), F64, gh, gw, 1, h, w, _p(out), F64, 2 * w, h, w, 0, 0), dict(ctrl=c_span, out=span),
                 [odd("out", span), short("out", span), shared("out"), odd("ctrl", c_span), short("ctrl", c_span), shared("ctrl"),
                  (dict(out=-span), EINVAL)])
    compose = entry("compose", (_p(A), F64, 2 * aW, aH, aW, _p(Bm), F64, 2 * w, _p(out), F64, 2 * w, h, w), dict(a=a_span, b=span, out=span),
                    [odd("a", a_span), short("a", a_span), odd("b", span), short("b", span), shared("b"), odd("out", span), short("out", span),
                     shared("out")])
    invert = entry("invert", (_p(A), F64, 2 * aW, aH, aW, _p(init), F64, 2 * w, _p(out), F64, 2 * w, h, w, 0, 0, 16, 1e-9),
                   dict(f=a_span, init=span, out=span),
                   [odd("f", a_span), short("f", a_span), odd("init", span), short("init", span), odd("out", span), short("out", span), shared("out")])
    raster = entry("invert_raster", (_p(A), F64, 2 * aW, aH, aW, _p(depth), _p(out), F64, 2 * w, h, w, 0, 0, 16, 0, _p(keys)),
                   dict(f=a_span, depth=aH * aW, out=span, keys=h * w),
                   [odd("f", a_span), short("f", a_span), (dict(depth=aH * aW - 1), EINVAL), odd("out", span), short("out", span), shared("out"),
                    (dict(keys=h * w - 1), EINVAL), shared("keys")])
    cbwd = entry("compose_bwd", (_p(A), F64, 2 * aW, aH, aW, _p(Bm), F64, 2 * w, _p(g), h, w, _p(ga), _p(gb)),
                 dict(a=a_span, b=span, gout=span, ga=a_span, gb=span),
                 [odd("a", a_span), shared("b"), short("b", span), shared("gout"), odd("gout", span), short("gout", span), odd("ga", a_span),
                  short("ga", a_span), shared("ga"),        # one gradient buffer for B different outer maps
                  shared("gb"), odd("gb", span), short("gb", span)])
    ibwd = entry("invert_bwd", (_p(A), F64, 2 * aW, aH, aW, _p(Bm), F64, 2 * w, _p(g), h, w, _p(ga)), dict(f=a_span, g=span, gout=span, gf=a_span),
                 [odd("f", a_span), shared("g"), short("g", span), shared("gout"), short("gout", span), shared("gf"), odd("gf", a_span),
                  short("gf", a_span)])
    entries = [mesh, compose, invert, raster, cbwd, ibwd]
    if device:
        ws = np.zeros(B * gh * w * 2)
        fn = L.lerf_coords_mesh_bwd_batched

        def mesh_bwd(**kw):
            s = dict(n=B, g=span, gc=c_span, ws=ws.nbytes)
            s.update(kw)
            return fn(_p(g), h, w, 1, gh, gw, _p(ctrl), _p(ws), s["ws"], s["n"], s["g"], s["gc"], None)
        entries.append(("mesh_bwd", mesh_bwd, [odd("g", span), short("g", span), shared("g"), odd("gc", c_span), short("gc", c_span), shared("gc"),
                                               (dict(ws=ws.nbytes - 8), EINVAL)] + bad_n))
    return entries, held


@pytest.mark.parametrize("device", [False, True])
def test_every_refused_argument_returns_its_code_and_writes_nothing(device):
    entries, held = _refusal_calls(device)
    before = [a.copy() for a in held]
    for name, call, bad in entries:
        for kw, code in bad:
            assert call(**kw) == code, (name, kw)
    if not device:
        assert all(np.array_equal(a, b) for a, b in zip(held, before))            # nothing was written by a refused call ...
        for name, call, bad in entries:                                          # ... and the unmodified arguments are accepted
            assert call() == 0, name
    else:
        assert all(np.array_equal(a, b) for a, b in zip(held, before))


def test_operands_that_overlap_across_the_batch_are_refused():
    L = _lib.lib()
    h, w = 4, 6
    span = 2 * h * w
    buf = np.full(2 * B * span + span, -7.0)
    # the out batch starts inside the last set of f's batch (the single-map check on set 0 alone would not see it)
    f, out = buf[:B * span], buf[(B - 1) * span + 2:]
    rc = L.lerf_coords_invert_batched_host(_p(f), F64, 2 * w, h, w, None, 0, 0, _p(out), F64, 2 * w, h, w, 0, 0, 16, 1e-9, B, span, 0, span)
    assert rc == EINVAL
    g, gb = buf[:B * span], buf[(B - 1) * span + 2:]
    A = np.full((5, 7, 2), 1.0)
    rc = L.lerf_coords_compose_bwd_batched_host(_p(A), F64, 14, 5, 7, _p(f), F64, 2 * w, _p(g), h, w, None, _p(gb), B, 0, span, span, 0, span)
    assert rc == EINVAL
    # compose: out may BE the inner batch (in place), not a shifted one
    Bm = np.stack([inner_map((5, 7), (h, w), seed=s) for s in range(B)])
    ref = _lib.coords_compose_host(A, Bm)
    args = lambda o: (_p(A), F64, 14, 5, 7, _p(Bm), F64, 2 * w, o, F64, 2 * w, h, w, B, 0, span, span)
    assert L.lerf_coords_compose_batched_host(*args(_p(Bm) + 16)) == EINVAL
    assert L.lerf_coords_compose_batched_host(*args(_p(Bm))) == 0 and R.same_bits(Bm, ref)
    assert (buf == -7.0).all()


# ---------------------------------------------------------------------------------------------- 6. the Python layer
class Counter:
    """counts the calls of the loaded library's coordinate-map entry points"""

    def __init__(self, monkeypatch):
        self.calls = {}
        L = _lib.lib()
        for name in _lib.EXPORTS:
            if name.startswith("lerf_coords_"):
                monkeypatch.setattr(L, name, self._wrap(name, getattr(L, name)))

    def _wrap(self, name, fn):
        def counted(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)
        return counted

    def take(self):
        got, self.calls = self.calls, {}
        return got


def test_coords_on_numpy_batches_make_one_batched_call(monkeypatch):
    hw = (9, 21)
    A, Bm = compose_case(hw)
    F, init = invert_case(hw)
    Fr, depth = raster_case(hw)
    ctrl = mesh_case()
    flow = np.stack([0.5 * np.sin(np.arange(hw[0] * hw[1] * 2, dtype=np.float64) * (s + 1) / 7.0).reshape(hw + (2,)) for s in range(B)])
    count = Counter(monkeypatch)
    per_sample = lambda fn: np.stack([fn(s) for s in range(B)])
    cases = [
        ("lerf_coords_mesh_batched_host", lambda: coords.from_mesh(ctrl, hw, "bicubic"), lambda s: coords.from_mesh(ctrl[s], hw, "bicubic")),
        ("lerf_coords_mesh_batched_host", lambda: coords.from_mesh(cast(ctrl, np.float32), hw), lambda s: coords.from_mesh(cast(ctrl[s], np.float32), hw)),
        ("lerf_coords_compose_batched_host", lambda: coords.compose(A, Bm), lambda s: coords.compose(A[s], Bm[s])),
        ("lerf_coords_compose_batched_host", lambda: coords.compose(A[0], Bm, dtype=np.float32), lambda s: coords.compose(A[0], Bm[s], dtype=np.float32)),
        ("lerf_coords_invert_batched_host", lambda: coords.invert(F, hw), lambda s: coords.invert(F[s], hw)),
        ("lerf_coords_invert_batched_host", lambda: coords.invert(F, hw, init=init, max_iter=3), lambda s: coords.invert(F[s], hw, init=init[s], max_iter=3)),
        ("lerf_coords_invert_batched_host", lambda: coords.invert_flow(flow), lambda s: coords.invert_flow(flow[s])),
        ("lerf_coords_invert_raster_batched_host", lambda: coords.invert_raster(Fr, hw, depth=depth), lambda s: coords.invert_raster(Fr[s], hw, depth=depth[s])),
        ("lerf_coords_invert_raster_batched_host", lambda: coords.invert_raster(Fr, hw, max_span=4, orient=1), lambda s: coords.invert_raster(Fr[s], hw, max_span=4, orient=1)),
        ("lerf_coords_invert_raster_batched_host", lambda: coords.invert_flow_raster(flow), lambda s: coords.invert_flow_raster(flow[s])),
    ]
    for name, batched, single in cases:
        got = batched()
        assert count.take() == {name: 1}, name                     # ONE call of the batched entry point, none of the single-map one
        ref = per_sample(single)
        assert count.take() == {name.replace("_batched", ""): B}
        assert got.dtype == ref.dtype and R.same_bits(got, ref), name
    assert coords.from_mesh(ctrl, hw).shape == (B,) + hw + (2,) and count.take() == {"lerf_coords_mesh_batched_host": 1}
    # a strided batch view is passed through (its batch stride is the set stride): still one call, nothing outside the view is written
    buf, out = padded(np.zeros((B,) + hw + (2,)))
    _lib.coords_compose_host(A, Bm, out=out)
    assert count.take() == {"lerf_coords_compose_batched_host": 1} and untouched(buf, out)
    # a batch whose layout the C contract does not take (reversed) is made contiguous: still one call
    assert R.same_bits(_lib.coords_compose_host(A[::-1], Bm[::-1]), _lib.coords_compose_host(A, Bm)[::-1].copy())
    with pytest.raises(ValueError):
        _lib.coords_compose_host(A, Bm[:2])
    with pytest.raises(ValueError):
        _lib.coords_compose_host(A, Bm[0])
    with pytest.raises(ValueError):
        _lib.coords_compose_host(A, Bm, out=np.zeros((B,) + hw + (2,))[::-1])
    with pytest.raises(ValueError):
        _lib.coords_invert_bwd_host(F[0], Bm, upstream_case(hw))
