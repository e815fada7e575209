"""CPU-only: the adjoint of the model builders through its host twin (lerf_coords_build_bwd_host: model_point_bwd of
csrc/lerf_coords_models.h summed in the device's order).  Every bound the GPU suite uses is settled here, against references that do
not import the library (tests/coords_build_grad_ref.py):

  1. the exports; the restatements' forward anchored on the library's host forward; the divisors of the parameter sets;
  2. the backward against autograd of the restatement (ADJ_TOL) and against central differences of the host forward (FD_H, FD_TOL),
     every model, every parameter;
  3. the non-finite rule, a NaN upstream, the accumulate contract, a batch of sets, every refusal.
"""
import os
import re

import numpy as np
import pytest
import torch

import coords_build_grad_ref as BR
import coords_ref as R
from conftest import REPO
from test_coords_grad_cpu import ADJ_TOL, FD_H, FD_TOL

from lerf_pytorch_amd import _lib

MODELS = ["homography", "radial", "brown"]
HWS = [(1, 1), (3, 5), (4, 64), (5, 65), (37, 131)]
ORIGINS = [(0, 0), (3, 7)]
FULL_HW = (48, 144)            # the whole output radial's scalars describe: every tile below lies inside it
MIN_DIVISOR = 0.5              # every divisor of every entry (Wh, no, the denominator of rad) stays at least this far from zero
EINVAL = -1
CODE = _lib.COORDS_MODELS


def upstream(shape, seed=4):
    return np.random.default_rng(seed).standard_normal(tuple(shape) + (2,))


def adj_close(got, ref, what):
    scale = max(float(np.max(np.abs(ref))), 1.0)
    err = float(np.max(np.abs(got - ref)))
    print("%s: max error %.3g, scale %.3g, bound %.3g" % (what, err, scale, ADJ_TOL * scale))
    assert np.isfinite(err) and err <= ADJ_TOL * scale, what
    return err / scale


def crossing_case():
    """(params of a homography whose Wh = 0.25 j - 2 is exactly 0 on column 8, hw, the mask of its non-finite entries, upstream with
    a NaN and an inf INSIDE the mask); shared with the GPU suite"""
    p = np.array([1.0, 0.1, 0.5, -0.25, 1.0, 2.0, 0.25, 0.0, -2.0])       # Y = i on column 8: 0 / 0 at row 0
    hw = (6, 17)
    mask = np.zeros(hw, bool)
    mask[:, 8] = True
    g = upstream(hw, 9)
    g[2, 8, 0], g[3, 8, 1] = np.nan, np.inf
    return p, hw, mask, g


# ---------------------------------------------------------------------------------------------- 1. exports, anchors
def test_exports_and_abi_version():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "lerf_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lerf_[a-z0-9_]+)\s*\(", src))
    for n in ("lerf_coords_build_dev", "lerf_coords_build_bwd_workspace_bytes", "lerf_coords_build_bwd", "lerf_coords_build_bwd_host"):
        assert n in declared and n in _lib.EXPORTS and hasattr(_lib.lib(), n), n
    assert _lib.lib().lerf_abi_version() == 7


def test_workspace_query():
    q = _lib.lib().lerf_coords_build_bwd_workspace_bytes
    assert q(21, 1, 2160, 3840) == 21 * 60 * 34 * 8 and q(9, 3, 1, 1) == 9 * 3 * 8 and q(8, 2, 65, 65) == 8 * 2 * 4 * 8
    for bad in ((0, 1, 4, 4), (22, 1, 4, 4), (9, 0, 4, 4), (9, 1, 0, 4), (9, 1, 4, 0), (9, 65536, 4, 4)):
        assert q(*bad) == 0, bad


@pytest.mark.parametrize("model", MODELS)
def test_the_restatements_forward_is_the_host_forward_and_no_divisor_is_near_zero(model):
    p = BR.cases(FULL_HW)[model]
    assert p.size == BR.N_PARAMS[model] and np.all(p[-8:] != 0 if model == "brown" else True)
    for hw in HWS:
        for origin in ORIGINS:
            assert origin[0] + hw[0] <= FULL_HW[0] and origin[1] + hw[1] <= FULL_HW[1]
            ref = BR.model_map(model, torch.from_numpy(p), hw, origin).numpy()
            got = _lib.coords_build_host(model, p, hw, origin=origin)
            err = float(np.max(np.abs(ref - got)))
            d = BR.denominators(model, p, hw, origin)
            print("%s %s at %s: max |restatement - host| = %.3g, min |divisor| = %.3g" % (model, hw, origin, err, d))
            assert err <= 1e-10 * max(float(np.max(np.abs(got))), 1.0) and d >= MIN_DIVISOR


def test_brown_params_ref_is_brown_params():
    from lerf_pytorch_amd import coords
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    for dist in (BR.BROWN_DIST, BR.BROWN_DIST[:5], BR.BROWN_DIST[:4]):
        want = coords.brown_params(BR.BROWN_K, dist, BR.BROWN_R, BR.BROWN_NEW_K)
        got = BR.brown_params_ref(t(BR.BROWN_K), t(dist), t(BR.BROWN_R), t(BR.BROWN_NEW_K)).numpy()
        assert got.shape == (21,) and float(np.max(np.abs(got - want))) <= 1e-12 * float(np.max(np.abs(want)))
    K2 = BR.BROWN_K * np.array([[1.1], [0.9], [1.0]])
    got = BR.brown_params_ref(t(np.stack([BR.BROWN_K, K2])), t(BR.BROWN_DIST), t(BR.BROWN_R), t(BR.BROWN_NEW_K)).numpy()
    assert got.shape == (2, 21)                                          # a leading B on one operand: the others are shared
    for b, K in enumerate((BR.BROWN_K, K2)):
        want = coords.brown_params(K, BR.BROWN_DIST, BR.BROWN_R, BR.BROWN_NEW_K)
        assert float(np.max(np.abs(got[b] - want))) <= 1e-12 * float(np.max(np.abs(want)))


# ---------------------------------------------------------------------------------------------- 2. the backward
@pytest.mark.parametrize("origin", ORIGINS)
@pytest.mark.parametrize("hw", HWS)
@pytest.mark.parametrize("model", MODELS)
def test_backward_against_autograd_of_the_restatement(model, hw, origin):
    p = BR.cases(FULL_HW)[model]
    g = upstream(hw)
    got = _lib.coords_build_bwd_host(model, p, g, origin=origin)
    assert got.shape == p.shape and got.dtype == np.float64 and np.any(got != 0)
    adj_close(got, BR.params_grad_ref(model, p, g, hw, origin), "%s %s at %s" % (model, hw, origin))


def test_backward_of_a_map_with_more_than_64_partials():
    """453 x 520 is 8 bands x 9 column tiles = 72 partial vectors: the second pass takes two rounds in lanes 0 .. 7"""
    hw = (453, 520)
    p = BR.cases(hw)["radial"]
    assert _lib.lib().lerf_coords_build_bwd_workspace_bytes(8, 1, *hw) == 8 * 72 * 8 and BR.denominators("radial", p, hw) >= MIN_DIVISOR
    g = upstream(hw)
    adj_close(_lib.coords_build_bwd_host("radial", p, g), BR.params_grad_ref("radial", p, g, hw), "radial %s" % (hw,))


@pytest.mark.parametrize("model", MODELS)
def test_backward_against_central_differences(model):
    """every parameter of the model perturbed by +-FD_H, the HOST forward re-built, sum(g dF) / 2h against the gradient"""
    hw, origin = (37, 131), (3, 7)
    p = BR.cases(FULL_HW)[model]
    g = upstream(hw)
    got = _lib.coords_build_bwd_host(model, p, g, origin=origin)
    worst = 0.0
    for k in range(p.size):
        step = np.zeros(p.size)
        step[k] = FD_H
        assert BR.denominators(model, p + step, hw, origin) >= MIN_DIVISOR and BR.denominators(model, p - step, hw, origin) >= MIN_DIVISOR
        fd = float(((_lib.coords_build_host(model, p + step, hw, origin=origin) - _lib.coords_build_host(model, p - step, hw, origin=origin)) * g).sum()
                   / (2 * FD_H))
        bound = FD_TOL * max(abs(got[k]), 1.0)
        worst = max(worst, abs(fd - got[k]) / bound)
        assert abs(fd - got[k]) <= bound, (model, k, fd, got[k])
    print("%s: %d parameters, worst error %.3g of the bound" % (model, p.size, worst))


# ---------------------------------------------------------------------------------------------- 3. special entries and the contract
def test_entries_that_are_not_finite_contribute_nothing():
    p, hw, mask, g = crossing_case()
    F = _lib.coords_build_host("homography", p, hw)
    assert np.array_equal(~np.isfinite(F).all(-1), mask)                 # Wh crosses zero INSIDE the map: column 8, nowhere else
    assert np.isnan(F[0, 8, 0]) and np.isinf(F[1, 8, 0])                # 0 / 0 and y / 0
    got = _lib.coords_build_bwd_host("homography", p, g)
    assert np.all(np.isfinite(got)) and np.all(got != 0)
    adj_close(got, BR.params_grad_ref("homography", p, g, hw, mask=mask), "masked crossing")
    # the select, not a product with 0: the masked entries alone give exactly zero
    only = np.where(mask[..., None], g, 0.0)
    assert not np.any(_lib.coords_build_bwd_host("homography", p, only))
    # a NaN upstream at a FINITE point propagates into every sum it reaches
    g2 = upstream(hw, 9)
    g2[1, 3, 1] = np.nan
    got2 = _lib.coords_build_bwd_host("homography", p, g2)
    assert np.all(np.isnan(got2[[0, 1, 2, 6, 7, 8]])) and np.all(np.isfinite(got2[3:6]))
    # brown with a non-finite parameter: every entry is non-finite, nothing is contributed
    pb = BR.cases(FULL_HW)["brown"].copy()
    pb[13] = np.inf
    assert not np.any(_lib.coords_build_bwd_host("brown", pb, upstream((5, 9))))


@pytest.mark.parametrize("model", MODELS)
def test_accumulate_contract_and_a_batch_of_sets(model):
    L = _lib.lib()
    hw, n = (5, 65), BR.N_PARAMS[model]
    rng = np.random.default_rng(12)
    ps = np.stack([BR.cases(FULL_HW)[model] * (1.0 + 0.01 * s) for s in range(3)])
    gs = np.stack([upstream(hw, 20 + s) for s in range(3)])
    singles = np.stack([_lib.coords_build_bwd_host(model, ps[s], gs[s], origin=(1, 2)) for s in range(3)])
    assert R.same_bits(_lib.coords_build_bwd_host(model, ps, gs, origin=(1, 2)), singles)            # B sets = B single calls
    assert R.same_bits(_lib.coords_build_bwd_host(model, ps[1], gs[1], origin=(1, 2)), singles[1])   # and a call repeats itself
    pre = rng.standard_normal((3, n))
    buf = pre.copy()
    assert L.lerf_coords_build_bwd_host(CODE[model], ps.ctypes.data, 3, n, gs.ctypes.data, hw[0], hw[1], 1, 2, buf.ctypes.data) == 0
    assert R.same_bits(buf, pre + singles) and np.all(singles != 0)                                  # one add per value, after the sum


def test_refusals_write_nothing():
    L = _lib.lib()
    p = BR.cases(FULL_HW)["homography"].copy()
    p0 = p.copy()
    g = np.ones((2, 4, 5, 2))
    gp = np.full((2, 9), -7.0)
    pp = np.stack([p, p])
    big = np.full(200, -7.0)

    def call(model=0, params=pp, n_sets=2, n_params=9, gm=g, oH=4, oW=5, i0=0, j0=0, out=gp):
        ptr = lambda x: x if isinstance(x, (int, type(None))) else x.ctypes.data
        return L.lerf_coords_build_bwd_host(model, ptr(params), n_sets, n_params, ptr(gm), oH, oW, i0, j0, ptr(out))

    assert call() == 0 and np.all(gp != -7.0)
    gp[:] = -7.0
    bad = [dict(model=3), dict(model=-1), dict(params=None), dict(gm=None), dict(out=None), dict(n_params=8), dict(n_params=21),
           dict(model=1, n_params=9), dict(model=2, n_params=9), dict(n_sets=0), dict(n_sets=-1), dict(n_sets=65536), dict(oH=0), dict(oW=0),
           dict(i0=-1), dict(j0=-1), dict(i0=0x7fffffff), dict(j0=0x7fffffff), dict(gm=g.ctypes.data + 8), dict(params=pp.ctypes.data + 4),
           dict(out=gp.ctypes.data + 4), dict(out=pp), dict(out=g), dict(params=big.ctypes.data, out=big.ctypes.data + 8 * 17),
           dict(gm=big.ctypes.data, n_sets=1, out=big.ctypes.data + 16 * 19)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
    assert (gp == -7.0).all() and (big == -7.0).all() and (g == 1.0).all() and np.array_equal(pp[0], p0)
    # the wrapper turns the code and its own checks into ValueError
    with pytest.raises(ValueError, match="lerf_coords_build_bwd_host"):
        _lib.coords_build_bwd_host("homography", p[:8], g[0])
    with pytest.raises(ValueError, match="lerf_coords_build_bwd_host"):
        _lib.coords_build_bwd_host("homography", pp, g[0])
    with pytest.raises(ValueError, match="grad_map"):
        _lib.coords_build_bwd_host("homography", p, g[0].astype(np.float32))
    with pytest.raises(ValueError, match="unknown"):
        _lib.coords_build_bwd_host("fisheye", p, g[0])
