"""CPU-only: the adjoints of compose and invert through their host twins (lerf_coords_compose_bwd_host, lerf_coords_invert_bwd_host:
compose_bwd_point / invert_bwd_point of csrc/lerf_coords_models.h in a plain row-major loop).  Every bound the GPU suite uses is
settled here, against references that do not import the library (tests/coords_grad_ref.py):

  1. the exports; the restatement's forward anchored on coords_ref.compose;
  2. compose backward against autograd of compose_ref (both halves, ADJ_TOL), the linearity identity in the outer map, central
     differences of the host forward for the inner gradient;
  3. invert backward against autograd of invert_ift_ref, against central differences through the host inverse, and the
     cancellation identity D + I = 0;
  4. special entries, the accumulate contract, the null halves, every refusal.
"""
import os
import re

import numpy as np
import pytest
import torch

import coords_grad_ref as GR
import coords_ref as R
from conftest import REPO
from test_coords_invert_cpu import HW, _valid, invert_maps

from lerf_pytorch_amd import _lib

ADJ_TOL = 1e-9                 # DESIGN 4.8's rule for a float64 map gradient: ADJ_TOL * max(max|ref|, 1)
FD_H, FD_TOL = 1e-6, 1e-5      # central differences: step, and the bound FD_TOL * max(|g|, 1) of DESIGN 4.8
NAMES = ["barrel", "homography", "mesh", "flow"]         # radial, homography, bicubic mesh, sinusoidal flow
INNER_HW = (23, 31)            # the inner map's shape: not the outer's
EINVAL = -1
F64, F32 = _lib.LERF_F64, _lib.LERF_F32


def inner_map(a_hw, hw=INNER_HW, seed=3, spill=2.0):
    """positions scattered over the outer map and `spill` beyond it on every side: generic (non-integer), some clipped"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-spill, a_hw[0] - 1 + spill, hw), rng.uniform(-spill, a_hw[1] - 1 + spill, hw)], axis=-1)


def upstream(hw, seed=4):
    return np.random.default_rng(seed).standard_normal(tuple(hw) + (2,))


def compose_grads_ref(A, B, g):
    """(grad_outer, grad_inner) by autograd of the restatement, float64 numpy"""
    a = torch.from_numpy(np.asarray(A, np.float64)).requires_grad_(True)
    b = torch.from_numpy(np.asarray(B, np.float64)).requires_grad_(True)
    ga, gb = torch.autograd.grad((GR.compose_ref(a, b) * torch.from_numpy(g)).sum(), (a, b))
    return ga.numpy(), gb.numpy()


def finite_inverse(G):
    """(G with its NaN entries replaced by a valid entry's position, the valid mask): what the restatement can read"""
    ok = _valid(G)
    return np.where(ok[..., None], G, G[ok][0]), ok


def invert_grad_ref(F, G, g):
    """grad_F by autograd of the one-step restatement; g must be 0 where G is NaN"""
    Gf, ok = finite_inverse(G)
    assert not np.any(g[~ok])
    f = torch.from_numpy(np.asarray(F, np.float64)).requires_grad_(True)
    gf, = torch.autograd.grad((GR.invert_ift_ref(f, torch.from_numpy(Gf)) * torch.from_numpy(g)).sum(), f)
    return gf.numpy()


def adj_close(got, ref, what):
    scale = max(float(np.max(np.abs(ref))), 1.0)
    err = float(np.max(np.abs(got - ref)))
    print("%s: max error %.3g, scale %.3g, bound %.3g" % (what, err, scale, ADJ_TOL * scale))
    assert np.isfinite(err) and err <= ADJ_TOL * scale, what
    return err / scale


# ---------------------------------------------------------------------------------------------- 1. exports, the anchor
def test_exports_and_abi_version():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "lerf_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lerf_[a-z0-9_]+)\s*\(", src))
    for n in ("lerf_coords_compose_bwd", "lerf_coords_compose_bwd_host", "lerf_coords_invert_bwd", "lerf_coords_invert_bwd_host"):
        assert n in declared and n in _lib.EXPORTS and hasattr(_lib.lib(), n), n
    assert _lib.lib().lerf_abi_version() == 7


@pytest.mark.parametrize("name", NAMES)
def test_the_restatements_forward_is_compose(name):
    A = invert_maps()[name]
    B = inner_map(A.shape[:2])
    ref = GR.compose_ref(torch.from_numpy(A), torch.from_numpy(B)).numpy()
    err = float(np.max(np.abs(ref - R.compose(A, B))))
    print("%s: max |compose_ref - coords_ref.compose| = %.3g" % (name, err))
    assert err <= 1e-12
    assert float(np.max(np.abs(ref - _lib.coords_compose_host(A, B)))) <= 1e-12


# ---------------------------------------------------------------------------------------------- 2. compose backward
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("name", NAMES)
def test_compose_backward_against_autograd_of_the_restatement(name, dt):
    A = invert_maps()[name].astype(dt)
    B = inner_map(A.shape[:2]).astype(dt)
    g = upstream(INNER_HW)
    assert A.shape[:2] != B.shape[:2]
    ga, gb = _lib.coords_compose_bwd_host(A, B, g)
    ra, rb = compose_grads_ref(A, B, g)
    adj_close(ga, ra, "%s %s grad_outer" % (name, np.dtype(dt).name))
    adj_close(gb, rb, "%s %s grad_inner" % (name, np.dtype(dt).name))
    blocked = (B[..., 0] < 0) | (B[..., 0] > A.shape[0] - 1)
    assert blocked.any() and not np.any(gb[..., 0][blocked]) and np.all(gb[..., 0][~blocked] != 0)
    if dt == np.float32:               # mixed operand dtypes: float32 is promoted exactly, so its float64 copy gives the same bits
        for a_, b_ in ((A.astype(np.float64), B), (A, B.astype(np.float64))):
            ga2, gb2 = _lib.coords_compose_bwd_host(a_, b_, g)
            assert R.same_bits(ga2, ga) and R.same_bits(gb2, gb)


@pytest.mark.parametrize("name", NAMES)
def test_compose_is_linear_in_the_outer_map(name):
    """<grad_out, compose(dA, B)> = <grad_a, dA> for a random dA: the scatter is the exact transpose of the forward's gather"""
    A = invert_maps()[name]
    B = inner_map(A.shape[:2])
    g = upstream(INNER_HW)
    dA = np.random.default_rng(5).standard_normal(A.shape)
    ga, _ = _lib.coords_compose_bwd_host(A, B, g, need=(True, False))
    lhs, rhs = float((g * _lib.coords_compose_host(dA, B)).sum()), float((ga * dA).sum())
    print("%s: inner products %.17g, %.17g" % (name, lhs, rhs))
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0)


@pytest.mark.parametrize("name", NAMES)
def test_inner_gradient_against_central_differences(name):
    """h = 1e-6 at every entry at least 1e-3 from a cell boundary and from the clip's ends (compose is pointwise in the inner map, so
    all of them are perturbed at once).  Measured worst error over the four maps (712 entries each): 0.13 % of the bound."""
    A = invert_maps()[name]
    aH, aW = A.shape[:2]
    B = inner_map((aH, aW), spill=0.0)
    g = upstream(INNER_HW)
    far = np.ones(INNER_HW, bool)
    for k, n in ((0, aH), (1, aW)):
        v = B[..., k]
        far &= (np.abs(v - np.round(v)) >= 1e-3) & (v >= 1e-3) & (v <= n - 1 - 1e-3)
    assert int(far.sum()) >= 20
    _, gb = _lib.coords_compose_bwd_host(A, B, g, need=(False, True))
    worst = 0.0
    for k in range(2):
        step = np.zeros(2)
        step[k] = FD_H
        fd = ((_lib.coords_compose_host(A, B + step) - _lib.coords_compose_host(A, B - step)) / (2 * FD_H) * g).sum(-1)
        err = np.abs(fd - gb[..., k])[far]
        bound = FD_TOL * np.maximum(np.abs(gb[..., k])[far], 1.0)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound)
    print("%s: %d entries, worst error %.3g of the bound" % (name, int(far.sum()), worst))


# ---------------------------------------------------------------------------------------------- 3. invert backward
def _inverse(F, tol=1e-9, init=None):
    return _lib.coords_invert_host(np.ascontiguousarray(F), HW, init=init, tol=tol)


def _masked_upstream(G, seed=6):
    return np.where(_valid(G)[..., None], upstream(G.shape[:2], seed), 0.0)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("name", NAMES)
def test_invert_backward_against_autograd_of_the_restatement(name, dt):
    F = invert_maps()[name].astype(dt)
    G = _inverse(F)
    g = _masked_upstream(G)
    assert _valid(G).mean() > 0.5
    got = _lib.coords_invert_bwd_host(F, G, g)
    adj_close(got, invert_grad_ref(F, G, g), "%s %s grad_f" % (name, np.dtype(dt).name))
    assert np.any(got != 0)
    # a float32 copy of the inverse is promoted exactly
    G32 = G.astype(np.float32)
    assert R.same_bits(_lib.coords_invert_bwd_host(F, G32, g), _lib.coords_invert_bwd_host(F, G32.astype(np.float64), g))


@pytest.mark.parametrize("name", NAMES)
def test_invert_backward_against_central_differences(name):
    """Entries of F perturbed by +-h, the host inverse recomputed with tol = 1e-12 from init = G, sum(g dG) / 2h against grad_f at
    the entry.  h = 1e-6 and the bound 1e-5 max(|g|, 1) hold as they stand: the measured worst error over the four maps is 0.09 % of
    the bound (the inverse of a piecewise-bilinear map is smooth in F while no entry of G changes its cell)."""
    F = invert_maps()[name]
    G = _inverse(F, tol=1e-12)
    ok = _valid(G)
    g = _masked_upstream(G)
    gf = _lib.coords_invert_bwd_host(F, G, g)
    touched = np.argwhere(np.abs(gf).sum(-1) > 0)
    rng = np.random.default_rng(7)
    worst = 0.0
    for i, j in touched[rng.choice(len(touched), 6, replace=False)]:
        for k in range(2):
            d = []
            for s in (+1.0, -1.0):
                Fp = F.copy()
                Fp[i, j, k] += s * FD_H
                Gp = _inverse(Fp, tol=1e-12, init=np.where(ok[..., None], G, 0.0))
                assert np.array_equal(_valid(Gp), ok)
                d.append(Gp)
            fd = float(np.where(ok[..., None], g * (d[0] - d[1]), 0.0).sum() / (2 * FD_H))
            bound = FD_TOL * max(abs(gf[i, j, k]), 1.0)
            worst = max(worst, abs(fd - gf[i, j, k]) / bound)
            assert abs(fd - gf[i, j, k]) <= bound, (i, j, k, fd, gf[i, j, k])
    print("%s: worst error %.3g of the bound" % (name, worst))


@pytest.mark.parametrize("name", NAMES)
def test_cancellation_identity(name):
    """G = invert(F): the gradient of compose(F, G) with respect to F, directly (D) and through G (I), vanishes -- both use the same
    J from the same statements, so D + I is the rounding of the 2 x 2 solve"""
    F = invert_maps()[name]
    G = _inverse(F)
    g = _masked_upstream(G)
    D, inner = _lib.coords_compose_bwd_host(F, G, g)
    assert not np.any(inner[~_valid(G)]) and np.all(np.isfinite(inner))
    I = _lib.coords_invert_bwd_host(F, G, inner)
    scale = max(float(np.max(np.abs(D))), 1.0)
    err = float(np.max(np.abs(D + I)))
    print("%s: max |D + I| = %.3g, max |D| = %.3g, bound %.3g" % (name, err, scale, ADJ_TOL * scale))
    assert np.any(D != 0) and err <= ADJ_TOL * scale


# ---------------------------------------------------------------------------------------------- 4. special entries and the contract
def special_compose():
    """(A [6, 7, 2], B [1, 12, 2], g [1, 12, 2]): NaN inner entries (finite and NaN upstream), +-inf and out-of-range rows, rows
    exactly on 0 and n - 1, columns on 0 and n - 1; shared with the GPU suite"""
    A = np.random.default_rng(8).standard_normal((6, 7, 2))
    inf = np.inf
    B = np.array([[[np.nan, 2.3], [2.3, np.nan], [np.nan, np.nan], [-inf, 2.5], [inf, 2.5], [-1.5, 3.25], [5.75, 3.25], [0.0, 1.5],
                   [5.0, 1.5], [2.5, 0.0], [2.5, 6.0], [1.25, inf]]])
    g = np.random.default_rng(9).standard_normal(B.shape)
    g[0, 1] = np.nan
    return A, B, g


def test_special_entries_of_compose_backward():
    A, B, g = special_compose()
    ga, gb = _lib.coords_compose_bwd_host(A, B, g)
    assert not np.any(gb[0, :3]) and np.all(np.isfinite(ga))          # NaN entries: (0, 0) whatever g holds, nothing scattered
    fin = np.arange(3, B.shape[1])
    ra, rb = compose_grads_ref(A, B[:, fin], g[:, fin])
    adj_close(ga, ra, "special grad_outer")
    adj_close(gb[:, fin], rb, "special grad_inner")
    # blocked rows (-inf, +inf, -1.5, 5.75): no row gradient, a column gradient, the outer gradient on the border row's two taps
    for e, row in ((3, 0), (4, 5), (5, 0), (6, 5)):
        assert gb[0, e, 0] == 0.0 and gb[0, e, 1] != 0.0
        only, _ = _lib.coords_compose_bwd_host(A, B[:, e:e + 1], g[:, e:e + 1], need=(True, False))
        hit = np.argwhere(np.abs(only).sum(-1) > 0)
        assert sorted(map(tuple, hit)) == [(row, int(np.floor(B[0, e, 1]))), (row, int(np.floor(B[0, e, 1])) + 1)]
        assert np.allclose(only.sum((0, 1)), g[0, e], rtol=0, atol=1e-15)
    for e in (7, 8, 9, 10):                                            # exactly on 0 and n - 1: the clip passes
        assert gb[0, e, 0] != 0.0 and gb[0, e, 1] != 0.0
    assert gb[0, 11, 1] == 0.0 and gb[0, 11, 0] != 0.0                 # +inf column


def test_identity_map_and_a_nan_corner():
    """t = 0 everywhere: the derivative is that of cell i0 = min(floor(r), n - 2), the outer gradient lands on the entry itself"""
    A = np.random.default_rng(10).standard_normal((5, 6, 2))
    ii, jj = np.meshgrid(np.arange(5.0), np.arange(6.0), indexing="ij")
    B = np.stack([ii, jj], axis=-1)
    g = upstream((5, 6))
    ga, gb = _lib.coords_compose_bwd_host(A, B, g)
    assert R.same_bits(ga, g)                                          # one tap of weight 1 * 1 per entry
    ra, rb = compose_grads_ref(A, B, g)
    adj_close(ga, ra, "identity grad_outer")
    adj_close(gb, rb, "identity grad_inner")
    assert np.all(gb != 0)
    # a NaN corner the forward does not read (its weight is 0) still makes the inner gradient NaN, as autograd of the formula does
    An = A.copy()
    An[2, 3] = np.nan
    assert np.all(np.isfinite(_lib.coords_compose_host(An, B)[2, 2]))
    ga, gb = _lib.coords_compose_bwd_host(An, B, g)
    ra, rb = compose_grads_ref(An, B, g)
    assert np.all(np.isnan(gb[2, 2])) and np.array_equal(np.isnan(gb), np.isnan(rb))
    assert R.same_bits(ga, g)
    fin = ~np.isnan(rb)
    assert float(np.max(np.abs(gb[fin] - rb[fin]))) <= ADJ_TOL * max(float(np.max(np.abs(rb[fin]))), 1.0)


def special_invert():
    """(F [6, 7, 2], G [1, 6, 2], g): F with a constant (folded) cell and a NaN vertex; G with NaN entries, an entry inside the folded
    cell, one inside a cell with the NaN corner, and two ordinary ones; shared with the GPU suite"""
    ii, jj = np.meshgrid(np.arange(6.0), np.arange(7.0), indexing="ij")
    F = np.stack([1.1 * ii + 0.1 * jj, 0.9 * jj - 0.05 * ii], axis=-1)
    F[0:2, 0:2] = F[0, 0]                 # cell (0, 0): constant, det = 0
    F[4, 5] = np.nan                      # cells (3..4, 4..5) have a NaN corner
    G = np.array([[[np.nan, 1.0], [np.nan, np.nan], [0.5, 0.5], [3.5, 4.5], [2.25, 2.5], [1.5, 5.75]]])
    g = np.random.default_rng(11).standard_normal(G.shape)
    g[0, 1] = np.nan
    return F, G, g


def test_special_entries_of_invert_backward():
    F, G, g = special_invert()
    for e in range(4):                    # NaN entries of G, the folded cell, the NaN corner: nothing
        assert not np.any(_lib.coords_invert_bwd_host(F, G[:, e:e + 1], g[:, e:e + 1])), e
    got = _lib.coords_invert_bwd_host(F, G, g)
    assert np.all(np.isfinite(got)) and np.any(got != 0)
    Ff = np.where(np.isnan(F), 0.0, F)
    adj_close(got, invert_grad_ref(Ff, G[:, 4:], g[:, 4:]), "special grad_f")


def test_accumulate_contract_and_null_halves():
    """dyadic positions, integer upstream and integer pre-fill: every product and sum is exact, so a pre-filled buffer gains exactly
    the gradient whatever the order of the scatter"""
    rng = np.random.default_rng(12)
    A = rng.integers(-8, 9, (6, 7, 2)).astype(np.float64)
    B = np.stack([rng.integers(-4, 24, INNER_HW) / 4.0, rng.integers(-4, 28, INNER_HW) / 4.0], axis=-1)
    g = rng.integers(-5, 6, INNER_HW + (2,)).astype(np.float64)
    ga, gb = _lib.coords_compose_bwd_host(A, B, g)
    pa, pb = rng.integers(-9, 10, A.shape).astype(np.float64), rng.integers(-9, 10, B.shape).astype(np.float64)
    qa, qb = _lib.coords_compose_bwd_host(A, B, g, pa.copy(), pb.copy())
    assert R.same_bits(qa, pa + ga) and R.same_bits(qb, pb + gb) and np.any(ga != 0) and np.any(gb != 0)
    # null halves: the other half is what the full call gives, a skipped buffer is not touched
    only_a, none_b = _lib.coords_compose_bwd_host(A, B, g, need=(True, False))
    none_a, only_b = _lib.coords_compose_bwd_host(A, B, g, need=(False, True))
    assert none_a is None and none_b is None and R.same_bits(only_a, ga) and R.same_bits(only_b, gb)
    # invert: F = 2 u + const is exactly invertible at dyadic positions; v = -g / 2 is exact
    ii, jj = np.meshgrid(np.arange(6.0), np.arange(7.0), indexing="ij")
    F = np.stack([2.0 * ii + 1.0, 2.0 * jj - 3.0], axis=-1)
    G = np.stack([rng.integers(0, 21, INNER_HW) / 4.0, rng.integers(0, 25, INNER_HW) / 4.0], axis=-1)
    gf = _lib.coords_invert_bwd_host(F, G, g)
    pf = rng.integers(-9, 10, F.shape).astype(np.float64)
    assert R.same_bits(_lib.coords_invert_bwd_host(F, G, g, pf.copy()), pf + gf) and np.any(gf != 0)
    assert float(np.abs(gf.sum((0, 1)) + g.sum((0, 1)) / 2.0).max()) == 0.0


def _p(a):
    return None if a is None else a.ctypes.data


def test_refusals_write_nothing():
    L = _lib.lib()
    A, B, g = np.zeros((6, 7, 2)), np.ones((4, 5, 2)), np.ones((4, 5, 2))
    ga, gb = np.full((6, 7, 2), -7.0), np.full((4, 5, 2), -7.0)
    big = np.full((6 * 7 + 4 * 5) * 2 + 2, -7.0)

    def compose(a=A, adt=F64, sa=14, aH=6, aW=7, b=B, bdt=F64, sb=10, go=g, oH=4, oW=5, pa=ga, pb=gb):
        ptr = lambda x: x if isinstance(x, (int, type(None))) else _p(x)
        return L.lerf_coords_compose_bwd_host(ptr(a), adt, sa, aH, aW, ptr(b), bdt, sb, ptr(go), oH, oW, ptr(pa), ptr(pb))

    assert compose() == 0
    ga[:], gb[:] = -7.0, -7.0
    bad = [dict(a=None), dict(b=None), dict(go=None), dict(pa=None, pb=None), dict(aH=1), dict(aW=1), dict(aH=0), dict(oH=0), dict(oW=0),
           dict(sa=13), dict(sa=12), dict(sb=9), dict(sb=8), dict(adt=99), dict(bdt=99), dict(a=_p(A) + 8), dict(b=_p(B) + 8),
           dict(go=_p(g) + 8), dict(pa=_p(ga) + 8), dict(pb=_p(gb) + 8),
           dict(pa=A), dict(pb=B), dict(pb=g), dict(pa=_p(big), pb=_p(big) + 16 * 10), dict(pa=_p(big) + 16 * 10, pb=_p(big)),
           dict(a=_p(big), pa=_p(big) + 16 * 41), dict(b=_p(big) + 16 * 41, pa=_p(big)), dict(go=_p(big) + 16 * 19, pb=_p(big))]
    for kw in bad:
        assert compose(**kw) == EINVAL, kw
    assert (ga == -7.0).all() and (gb == -7.0).all() and (big == -7.0).all() and not A.any() and (B == 1.0).all()

    gf = np.full((6, 7, 2), -7.0)

    def invert(f=A, fdt=F64, sf=14, fH=6, fW=7, gg=B, gdt=F64, sg=10, go=g, oH=4, oW=5, pf=gf):
        ptr = lambda x: x if isinstance(x, (int, type(None))) else _p(x)
        return L.lerf_coords_invert_bwd_host(ptr(f), fdt, sf, fH, fW, ptr(gg), gdt, sg, ptr(go), oH, oW, ptr(pf))

    assert invert() == 0 and (gf == -7.0).all()                        # F is constant: every cell is folded
    bad = [dict(f=None), dict(gg=None), dict(go=None), dict(pf=None), dict(fH=1), dict(fW=1), dict(oH=0), dict(oW=0), dict(sf=13), dict(sf=12),
           dict(sg=9), dict(fdt=99), dict(gdt=99), dict(f=_p(A) + 8), dict(gg=_p(B) + 8), dict(go=_p(g) + 8), dict(pf=_p(gf) + 8),
           dict(pf=A), dict(gg=_p(big) + 16 * 41, pf=_p(big)), dict(go=_p(big) + 16 * 41, pf=_p(big))]
    for kw in bad:
        assert invert(**kw) == EINVAL, kw
    assert (gf == -7.0).all() and (big == -7.0).all()
    # the wrappers turn the code into ValueError
    with pytest.raises(ValueError, match="lerf_coords_compose_bwd_host"):
        _lib.coords_compose_bwd_host(np.zeros((1, 7, 2)), B, g)
    with pytest.raises(ValueError, match="lerf_coords_invert_bwd_host"):
        _lib.coords_invert_bwd_host(np.zeros((6, 1, 2)), B, g)
    with pytest.raises(ValueError, match="grad_out"):
        _lib.coords_compose_bwd_host(A, B, g.astype(np.float32))
