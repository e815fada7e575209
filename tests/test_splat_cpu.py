"""CPU-only: the forward warp by summation splatting through its host twins (lerf_splat_host, lerf_splat_bwd_host: the kernels' own
statements of csrc/lerf_splat_point.h under the host runner).  The references import nothing of the library (tests/splat_ref.py: numpy
float64 statement by statement, and the same forward in torch float64 for autograd):

  1. the exports;
  2. the host twins against the restatement bit for bit, forward and backward, each half alone equal to the half of the full call;
  3. exact cases: the identity, an integer translation, the frame's edges, non-finite entries;
  4. mass, the adjoint identity, grad_F against central differences and all three gradients against autograd;
  5. the accumulate contract, and a batch against its single-set calls;
  6. every refusal leaves a sentinel-filled arena untouched;
  7. the modes of coords.splat on numpy.

The cases the GPU suite runs against these host twins are built here (CASES, make_case(), special_map(), inside_map())."""
import os
import re

import numpy as np
import pytest
import torch

import splat_ref as SR
from conftest import REPO
from test_coords_grad_cpu import ADJ_TOL, FD_H, FD_TOL

from lerf_pytorch_amd import _lib, coords

EINVAL = -1
F32, F64 = _lib.LERF_F32, _lib.LERF_F64
NAMES = ("lerf_splat", "lerf_splat_host", "lerf_splat_bwd", "lerf_splat_bwd_host")
f32, f64 = np.float32, np.float64
# (source hw, output hw, C, B (0: the single form), per-sample map, T, map dtype, norm plane, weight): every seam once -- several 4 x 64
# blocks ragged on both axes, frames unequal to the source, both C, a shared and a per-sample map, both T, both map dtypes, 1 x 1
CASES = [
    ((23, 31), (29, 37), 1, 0, False, f32, f32, False, False),
    ((23, 31), (29, 37), 3, 3, False, f64, f64, True, True),
    ((23, 31), (29, 37), 3, 3, True, f32, f64, True, False),
    ((70, 130), (64, 150), 3, 0, False, f32, f32, True, True),
    ((70, 130), (64, 150), 1, 3, True, f64, f32, False, True),
    ((70, 130), (64, 150), 3, 3, False, f32, f64, True, True),
    ((1, 1), (29, 37), 3, 3, True, f64, f64, True, True),
    ((1, 1), (1, 1), 1, 0, False, f32, f32, True, False),
]
IDS = ["%dx%d-%dx%d-C%d-B%d%s-%s-%s%s%s" % (c[0] + c[1] + (c[2], c[3], "m" if c[4] else "", c[5].__name__[5:], c[6].__name__[5:],
                                                          "-norm" if c[7] else "", "-w" if c[8] else "")) for c in CASES]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def special_map(hw, ohw, dt, seed=0):
    """a forward map [H, W, 2] of `dt`: the source frame scaled onto the output frame plus a smooth flow that carries a margin of it
    outside, with the special entries -- NaN, +-inf, 1e300, -0.5, oH - 1 exactly, oH - 0.5, integers -- on a stride-5 walk"""
    H, W = hw
    oH, oW = ohw
    i, j = np.meshgrid(np.arange(H, dtype=f64), np.arange(W, dtype=f64), indexing="ij")
    F = np.stack([(i + 0.37) * (oH + 2.0) / H - 1.5 + 1.3 * np.sin(0.31 * j + 0.2 * seed), (j + 0.61) * (oW + 3.0) / W - 2.0 + 1.7 * np.cos(0.23 * i + seed)], -1)
    sp = [(np.nan, 3.0), (2.0, np.nan), (np.inf, 1.0), (1.0, -np.inf), (1e300, 2.0), (2.0, -1e300), (-0.5, 4.25), (3.5, -0.5), (oH - 1.0, 5.5),
          (4.0, oW - 1.0), (oH - 0.5, 2.0), (1.5, oW - 0.5), (3.0, 7.0), (0.0, 0.0), (oH - 1.0, oW - 1.0), (-1.0, 2.0), (float(oH), 3.5)]
    if H * W == 1:                                                  # the single pixel lands inside whatever the frame, on four taps or on one
        F[0, 0] = (0.25 * (oH - 1) - 0.25, 0.5 * (oW - 1) - 0.375)
    flat = F.reshape(-1, 2)
    n = min(len(sp), flat.shape[0] // 5)
    if n:                                                           # 1 x 1: a plain entry (its special values: the single-entry test)
        flat[0:5 * n:5] = sp[:n]
    with np.errstate(over="ignore"):
        return F.astype(dt)


def inside_map(hw, ohw, seed=0, away=1e-3):
    """a float64 map whose positions lie inside [away, n - 1 - away] on both axes and at least `away` from every integer"""
    rng = np.random.default_rng(100 + seed)
    F = np.stack([rng.uniform(0.0, ohw[0] - 1.0, hw), rng.uniform(0.0, ohw[1] - 1.0, hw)], -1)
    F = np.floor(F) + np.clip(F - np.floor(F), 0.01, 0.99)
    return F


def make_case(case, seed=0):
    """(X, F, M) of a case: X [(B,) C, H, W] of T, F [(B,) H, W, 2] (shared: [H, W, 2]), M of T or None"""
    hw, ohw, C, B, per_sample, T, TF, norm, weighted = case
    rng = np.random.default_rng(seed)
    lead = (B,) if B else ()
    X = rng.standard_normal(lead + (C,) + hw).astype(T)
    F = np.stack([special_map(hw, ohw, TF, s) for s in range(B)]) if per_sample else special_map(hw, ohw, TF)
    M = rng.uniform(0.25, 2.0, lead + hw).astype(T) if weighted else None
    return X, F, M


def as_batch(X, F, M):
    return (X, F, M) if X.ndim == 4 else (X[None], F, None if M is None else M[None])


def upstream(case, seed=1):
    hw, ohw, C, B, per_sample, T, TF, norm, weighted = case
    return np.random.default_rng(seed).standard_normal(((B,) if B else ()) + (C + norm,) + ohw).astype(T)


# ---------------------------------------------------------------------------------------------- 1. exports
def test_exports_and_abi_version():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "lerf_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lerf_[a-z0-9_]+)\s*\(", src))
    for n in NAMES:
        assert n in declared and n in _lib.EXPORTS and hasattr(_lib.lib(), n), n
    assert _lib.lib().lerf_abi_version() == 7


# ---------------------------------------------------------------------------------------------- 2. the host twins are the restatement
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_host_twin_is_the_restatement_bit_for_bit(case):
    X, F, M = make_case(case)
    ohw, norm = case[1], case[7]
    keep = [a.copy() for a in (X, F)]
    got = _lib.splat_host(X, F, ohw, M, norm)
    ref, n, mag = SR.splat(*as_batch(X, F, M), ohw, norm)
    assert same_bits(got, ref.reshape(got.shape))
    assert int(n.sum()) > 0 and np.isfinite(got).all()
    assert same_bits(X, keep[0]) and same_bits(F, keep[1])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward_host_twin_is_the_restatement_bit_for_bit(case):
    X, F, M = make_case(case)
    norm = case[7]
    G = upstream(case)
    Xb, Fb, Mb = as_batch(X, F, M)
    need = (True, M is not None, True)
    gx, gm, gf = _lib.splat_bwd_host(X, F, G, M, norm, need)
    rx, rm, rf = SR.splat_bwd(Xb, Fb, Mb, G.reshape((Xb.shape[0],) + G.shape[-3:]), norm, need)
    if case[3] and F.ndim == 3:
        rf = rf.sum(0)
    assert same_bits(gx, rx.reshape(gx.shape)) and same_bits(gf, rf.reshape(gf.shape)) and gf.dtype == np.float64
    assert (gm is None) == (M is None) and (gm is None or same_bits(gm, rm.reshape(gm.shape)))
    # each half alone is the half of the full call, and the restatement agrees with itself on that
    for k in range(3):
        if not need[k]:
            continue
        one = tuple(i == k for i in range(3))
        alone = _lib.splat_bwd_host(X, F, G, M, norm, one)
        assert [a is None for a in alone] == [not w for w in one]
        assert same_bits(alone[k], (gx, gm, gf)[k])


# ---------------------------------------------------------------------------------------------- 3. exact cases
@pytest.mark.parametrize("T", [f32, f64])
@pytest.mark.parametrize("TF", [f32, f64])
def test_identity_and_integer_translation_are_exact(T, TF):
    H, W, C = 23, 31, 3
    X = np.random.default_rng(2).standard_normal((C, H, W)).astype(T)
    ident = coords.from_flow(np.zeros((H, W, 2))).astype(TF)
    assert same_bits(_lib.splat_host(X, ident, (H, W)), X)
    acc = _lib.splat_host(X, ident, (H, W), norm=True)
    assert same_bits(acc[:C], X) and (acc[C] == 1).all()
    dr, dc = 3, -11                                          # a third of the frame's columns leave on the left
    out = _lib.splat_host(X, (ident + np.array([dr, dc])).astype(TF), (H, W))
    want = np.zeros_like(X)
    want[:, dr:, :W + dc] = X[:, :H - dr, -dc:]
    assert same_bits(out, want)


@pytest.mark.parametrize("T", [f32, f64])
def test_frame_edges_and_non_finite_entries(T):
    oH, oW = 29, 37
    x = np.array([[[8.0]]], T)

    def land(r, c, norm=False):
        return _lib.splat_host(x, np.array([[[r, c]]], f64), (oH, oW), norm=norm)

    a = land(oH - 1.0, 5.0)
    assert a[0, oH - 1, 5] == 8 and np.count_nonzero(a) == 1             # the last row is inside the frame
    a = land(oH - 0.5, 5.0)
    assert a[0, oH - 1, 5] == 4 and np.count_nonzero(a) == 1             # half its mass is lost
    a = land(-0.5, 5.0)
    assert a[0, 0, 5] == 4 and np.count_nonzero(a) == 1                  # half is kept
    a = land(3.0, oW - 0.5, norm=True)
    assert a[0, 3, oW - 1] == 4 and a[1, 3, oW - 1] == 0.5 and np.count_nonzero(a) == 2
    a = land(-0.5, -0.5)
    assert a[0, 0, 0] == 2 and np.count_nonzero(a) == 1
    for r, c in ((-1.0, 3.0), (float(oH), 3.0), (3.0, -1.0), (3.0, float(oW)), (-7.25, 2.0), (2.0, 1e9)):
        assert np.count_nonzero(land(r, c, True)) == 0, (r, c)
    G = np.full((2, oH, oW), np.nan, T)
    w = np.array([[2.0]], T)
    for r, c in ((np.nan, 3.0), (3.0, np.nan), (np.inf, 3.0), (3.0, -np.inf), (1e300, 3.0), (3.0, -1e300), (np.nan, np.inf)):
        F = np.array([[[r, c]]], f64)
        assert np.count_nonzero(land(r, c, True)) == 0, (r, c)
        gx, gm, gf = _lib.splat_bwd_host(x, F, G, w, True)
        if np.isfinite(r) and np.isfinite(c):                 # 1e300: finite, every tap dropped -- zeros by the sums, not by the select
            assert (gx == 0).all() and (gm == 0).all() and (gf == 0).all()
        else:                                                 # exact zeros under a NaN-filled G
            assert not bits(gx).any() and not bits(gm).any() and not bits(gf).any(), (r, c)


# ---------------------------------------------------------------------------------------------- 4. mass, adjoint, gradients
def float64_case(B=0, C=3, hw=(23, 31), ohw=(29, 37), seed=0):
    rng = np.random.default_rng(seed)
    lead = (B,) if B else ()
    X = rng.standard_normal(lead + (C,) + hw)
    F = np.stack([inside_map(hw, ohw, s) for s in range(B)]) if B else inside_map(hw, ohw, seed)
    M = rng.uniform(0.25, 2.0, lead + hw)
    G = rng.standard_normal(lead + (C + 1,) + ohw)
    return X, F, M, G


def test_mass_is_kept_inside_the_frame():
    X, F, M, _ = float64_case()
    acc = _lib.splat_host(X, F, (29, 37), M, True)
    for k in range(3):
        want, scale = (M * X[k]).sum(), np.abs(M * X[k]).sum()
        assert abs(acc[k].sum() - want) <= 1e-12 * scale
    assert abs(acc[3].sum() - M.sum()) <= 1e-12 * M.sum()


@pytest.mark.parametrize("B", [0, 3])
def test_adjoint_identity(B):
    X, F, M, G = float64_case(B)
    F = special_map((23, 31), (29, 37), f64) if B else F           # the batch shares one map with dropped taps and special entries
    acc = _lib.splat_host(X, F, (29, 37), M, True)
    gx, gm, _ = _lib.splat_bwd_host(X, F, G, M, True)
    Xb, Fb, Mb = as_batch(X, F, M)
    _, _, mag = SR.splat(Xb, Fb, Mb, (29, 37), True)
    bound = 1e-12 * (mag.reshape(G.shape) * np.abs(G)).sum()
    lhs = (acc * G).sum()
    C = X.shape[-3]
    Gx = np.take(G, range(C), axis=-3)
    # <splat(X), G[:C]> = <X, grad_X>; the norm plane does not depend on X
    lhs_x = (np.take(acc, range(C), axis=-3) * Gx).sum()
    assert abs(lhs_x - (X * gx).sum()) <= bound
    assert abs(lhs - (M * gm).sum()) <= bound                       # the whole accumulator is linear in M


def test_grad_map_against_central_differences():
    X, F, M, G = float64_case()
    frac = F - np.floor(F)
    away = 1e-3
    assert (np.minimum(frac, 1 - frac) >= away).all()               # at least 1e-3 from every integer position ...
    assert (F >= away).all() and (F[..., 0] <= 28 - away).all() and (F[..., 1] <= 36 - away).all()        # ... and from the frame's edge
    _, _, gf = _lib.splat_bwd_host(X, F, G, M, True)

    def loss(Fm):
        return float((_lib.splat_host(X, Fm, (29, 37), M, True) * G).sum())

    rng = np.random.default_rng(5)
    for _ in range(12):
        i, j, k = int(rng.integers(23)), int(rng.integers(31)), int(rng.integers(2))
        Fp, Fn = F.copy(), F.copy()
        Fp[i, j, k] += FD_H
        Fn[i, j, k] -= FD_H
        fd = (loss(Fp) - loss(Fn)) / (2 * FD_H)
        assert abs(fd - gf[i, j, k]) <= FD_TOL * max(abs(gf[i, j, k]), 1.0), (i, j, k, fd, gf[i, j, k])


@pytest.mark.parametrize("B,special", [(0, False), (3, False), (0, True)])
def test_gradients_against_autograd_of_the_restatement(B, special):
    X, F, M, G = float64_case(B)
    if special:
        F = special_map((23, 31), (29, 37), f64)
        with np.errstate(invalid="ignore"):
            frac = F - np.floor(F)
        F = np.where((frac == 0) & np.isfinite(F), F + 0.25, F)      # integer positions are one-sided here and two-sided nowhere: moved
    gx, gm, gf = _lib.splat_bwd_host(X, F, G, M, True)
    tx, tf, tm = (torch.tensor(a, requires_grad=True) for a in (X, F, M))
    (SR.torch_splat(tx, tf, tm, (29, 37), True) * torch.tensor(G)).sum().backward()
    for got, ref in ((gx, tx.grad), (gm, tm.grad), (gf, tf.grad)):
        ref = ref.numpy()
        assert np.abs(got - ref).max() <= ADJ_TOL * max(np.abs(ref).max(), 1.0)
    if special:
        bad = ~np.isfinite(F).all(-1)
        assert bad.any() and not gf[bad].any() and not gx[:, bad].any() and not gm[bad].any()


def test_one_sided_derivative_at_integer_positions():
    """at an integer position grad_F is the derivative of the cell [f, f + 1]: the forward difference of the loss, not the backward one"""
    x, G = np.array([[[1.0]]]), np.arange(20.0).reshape(1, 4, 5) ** 2
    F = np.array([[[2.0, 3.0]]])
    _, _, gf = _lib.splat_bwd_host(x, F, G, None, False, (False, False, True))
    assert gf[0, 0, 0] == G[0, 3, 3] - G[0, 2, 3] and gf[0, 0, 1] == G[0, 2, 4] - G[0, 2, 3]
    F = np.array([[[3.0, 4.0]]])                                     # the last row and column: the cell beyond is outside, S = 0 there
    _, _, gf = _lib.splat_bwd_host(x, F, G, None, False, (False, False, True))
    assert gf[0, 0, 0] == -G[0, 3, 4] and gf[0, 0, 1] == -G[0, 3, 4]


# ---------------------------------------------------------------------------------------------- 5. accumulate, batch
@pytest.mark.parametrize("T", [f32, f64])
def test_two_calls_into_one_accumulator(T):
    case = ((23, 31), (29, 37), 3, 0, False, T, f64, True, True)
    X1, F1, M1 = make_case(case, 0)
    X2, F2, M2 = make_case(case, 1)
    F2 = special_map((23, 31), (29, 37), f64, 3)
    acc = _lib.splat_host(X1, F1, (29, 37), M1, True)
    first = acc.copy()
    assert _lib.splat_host(X2, F2, (29, 37), M2, True, acc=acc) is acc
    ref = SR.splat_one(X2, F2, M2, (29, 37), True, acc=first.copy())[0]
    assert same_bits(acc, ref)
    two = first.astype(f64) + _lib.splat_host(X2, F2, (29, 37), M2, True).astype(f64)
    u = 2.0 ** (-24 if T == f32 else -53)
    _, n2, mag2 = SR.splat_one(X2, F2, M2, (29, 37), True)
    assert (np.abs(acc - two) <= 2 * (n2 + 1) * u * (mag2 + np.abs(first))).all()      # the sum of two calls, up to the order of the adds


@pytest.mark.parametrize("case", [c for c in CASES if c[3]], ids=[i for c, i in zip(CASES, IDS) if c[3]])
def test_a_batch_is_its_single_set_calls_bit_for_bit(case):
    X, F, M = make_case(case)
    ohw, norm = case[1], case[7]
    G = upstream(case)
    acc = _lib.splat_host(X, F, ohw, M, norm)
    need = (True, M is not None, True)
    gx, gm, gf = _lib.splat_bwd_host(X, F, G, M, norm, need)
    gf_sets = []
    for s in range(case[3]):
        Fs, Ms = (F if F.ndim == 3 else F[s]), (None if M is None else M[s])
        assert same_bits(acc[s], _lib.splat_host(X[s], Fs, ohw, Ms, norm))
        sx, sm, sf = _lib.splat_bwd_host(X[s], Fs, G[s], Ms, norm, need)
        assert same_bits(gx[s], sx) and (gm is None or same_bits(gm[s], sm))
        gf_sets.append(sf)
    assert same_bits(gf, np.stack(gf_sets).sum(0) if F.ndim == 3 else np.stack(gf_sets))


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_every_refusal_leaves_the_arena_untouched():
    L = _lib.lib()
    C, H, W, oH, oW, B = 2, 3, 4, 5, 6, 2
    n, on = H * W, oH * oW
    arena = np.full(8192, -7.0)
    base = arena.ctypes.data
    assert base % 16 == 0
    X, F, M, ACC, G, GX, GM, GF = (base + 8 * k for k in (0, 256, 512, 768, 2048, 3072, 3584, 4096))

    def fwd(x=X, dt=F64, c=C, h=H, w=W, xset=C * n, f=F, fdt=F64, frow=2 * W, fset=2 * n, m=M, mset=n, acc=ACC, norm=1, oh=oH, ow=oW,
            aset=(C + 1) * on, n_sets=B):
        return L.lerf_splat_host(x, dt, c, h, w, xset, f, fdt, frow, fset, m, mset, acc, norm, oh, ow, aset, n_sets)

    def bwd(x=X, dt=F64, c=C, h=H, w=W, xset=C * n, f=F, fdt=F64, frow=2 * W, fset=2 * n, m=M, mset=n, g=G, norm=1, oh=oH, ow=oW,
            gset=(C + 1) * on, gx=GX, gxset=C * n, gm=GM, gmset=n, gf=GF, gfset=2 * n, n_sets=B):
        return L.lerf_splat_bwd_host(x, dt, c, h, w, xset, f, fdt, frow, fset, m, mset, g, norm, oh, ow, gset, gx, gxset, gm, gmset, gf, gfset, n_sets)

    common = [dict(x=None), dict(f=None), dict(x=X + 4), dict(f=F + 8), dict(m=M + 4), dict(dt=0), dict(dt=3), dict(fdt=0), dict(fdt=3),
              dict(frow=2 * W + 1), dict(frow=2 * W - 2), dict(c=0), dict(c=-1), dict(h=0), dict(w=0), dict(oh=0), dict(ow=0), dict(norm=2),
              dict(norm=-1), dict(n_sets=0), dict(n_sets=65536), dict(xset=-C * n), dict(fset=2 * n + 1), dict(fset=2 * n - 2), dict(xset=C * n - 1),
              dict(mset=n - 1), dict(xset=0), dict(mset=0), dict(h=262141)]
    for kw in common + [dict(acc=None), dict(acc=ACC + 4), dict(aset=(C + 1) * on - 1), dict(aset=0), dict(acc=X), dict(acc=M), dict(acc=F),
                        dict(acc=X + 8 * (B * C * n - 1)), dict(acc=F - 8 * (B * (C + 1) * on - 1))]:
        assert fwd(**kw) == EINVAL, kw
    for kw in common + [dict(g=None), dict(g=G + 4), dict(gset=(C + 1) * on - 1), dict(gx=None, gm=None, gf=None), dict(gx=GX + 4), dict(gm=GM + 4),
                        dict(gf=GF + 8), dict(gxset=C * n - 1), dict(gmset=n - 1), dict(gfset=2 * n - 2), dict(gfset=2 * n + 1), dict(gfset=0),
                        dict(gx=X), dict(gx=F), dict(gx=M), dict(gx=G), dict(gm=X), dict(gm=F), dict(gm=M), dict(gm=G), dict(gf=X), dict(gf=F),
                        dict(gf=M), dict(gf=G), dict(gx=GM), dict(gx=GF), dict(gm=GF), dict(gm=GX + 8 * (B * C * n - 1)),
                        dict(gf=G + 8 * (B * (C + 1) * on - 2))]:
        assert bwd(**kw) == EINVAL, kw
    assert (arena == -7.0).all()
    # the same arena takes the good calls: the table refuses nothing it should accept
    arena[:3072] = 0.5
    assert fwd() == 0 and fwd(fset=0) == 0 and fwd(m=None, mset=0) == 0 and fwd(norm=0, aset=C * on) == 0
    assert fwd(n_sets=1, xset=0, fset=0, mset=0, aset=0) == 0
    assert bwd() == 0 and bwd(gx=None) == 0 and bwd(gm=None) == 0 and bwd(gf=None) == 0 and bwd(fset=0, m=None) == 0
    assert (arena[3072 + B * C * n:3584] == -7.0).all() and (arena[3584 + B * n:4096] == -7.0).all() and (arena[4096 + 2 * B * n:] == -7.0).all()
    assert not (arena[3072:3072 + B * C * n] == -7.0).any() and not (arena[4096:4096 + 2 * B * n] == -7.0).any()
    # the wrappers
    x, f = np.zeros((2, H, W)), np.zeros((H, W, 2))
    for bad in (dict(src=x[0]), dict(src=x.astype(np.int32)), dict(fmap=f[:2]), dict(fmap=np.zeros((3, H, W, 2))), dict(weight=np.ones((H, W), f32)),
                dict(weight=np.ones((W, H))), dict(out_hw=(0, 4))):
        kw = dict(src=x, fmap=f, out_hw=(oH, oW), weight=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            _lib.splat_on(_lib._HOST, kw["src"], kw["fmap"], kw["out_hw"], kw["weight"])
    with pytest.raises(ValueError, match="acc"):
        _lib.splat_host(x, f, (oH, oW), acc=np.zeros((2, oH, oW), f32))
    with pytest.raises(ValueError, match="grad"):
        _lib.splat_bwd_host(x, f, np.zeros((3, oH, oW)))
    with pytest.raises(ValueError, match="weight"):
        _lib.splat_bwd_host(x, f, np.zeros((2, oH, oW)), need=(True, True, True))
    with pytest.raises(ValueError, match="at least one"):
        _lib.splat_bwd_host(x, f, np.zeros((2, oH, oW)), need=(False, False, False))


def test_python_refusals():
    x, f = np.zeros((2, 3, 4)), np.zeros((3, 4, 2))
    with pytest.raises(ValueError, match="mode"):
        coords.splat(x, f, (5, 6), mode="max")
    with pytest.raises(ValueError, match="average"):
        coords.splat(x, f, (5, 6), weight=np.ones((3, 4)), mode="average")
    for mode in ("linear", "softmax"):
        with pytest.raises(ValueError, match="needs a weight"):
            coords.splat(x, f, (5, 6), mode=mode)
    with pytest.raises(ValueError, match="map"):
        coords.splat(x, np.zeros((4, 3, 2)), (5, 6))
    with pytest.raises(ValueError, match="weight"):
        coords.splat(x, f, (5, 6), weight=np.ones((2, 3, 4)))
    with pytest.raises(ValueError, match="out_hw"):
        coords.splat(x, f, (5, 0))
    with pytest.raises(ValueError, match="no autograd"):
        coords.splat(torch.zeros((2, 3, 4), requires_grad=True), f, (5, 6))
    with torch.no_grad():
        assert coords.splat(torch.zeros((2, 3, 4), requires_grad=True), f, (5, 6)).shape == (2, 5, 6)


# ---------------------------------------------------------------------------------------------- 7. the modes
@pytest.mark.parametrize("B", [0, 3])
def test_modes_on_numpy(B):
    X, F, M, _ = float64_case(B)
    F = special_map((23, 31), (29, 37), f64)
    ohw, eps = (29, 37), 1e-7
    Xb, Fb, Mb = as_batch(X, F, M)
    ones = SR.splat(Xb, Fb, None, ohw, True)[0].reshape(X.shape[:-3] + (4,) + ohw)
    lin = SR.splat(Xb, Fb, Mb, ohw, True)[0].reshape(ones.shape)
    C = 3
    assert same_bits(coords.splat(X, F, ohw), ones[..., :C, :, :])
    assert same_bits(coords.splat(X, F, ohw, weight=M), lin[..., :C, :, :])
    out, norm = coords.splat(X, F, ohw, mode="average", return_norm=True)
    assert same_bits(out, ones[..., :C, :, :] / (ones[..., C:, :, :] + eps)) and same_bits(norm, ones[..., C, :, :])
    holes = norm == 0                                                # norm == 0 is the hole mask: nothing landed, the quotient is 0 / eps
    assert holes.any() and not (out * holes[..., None, :, :]).any()
    out, norm = coords.splat(X, F, ohw, weight=M, mode="linear", return_norm=True)
    assert same_bits(out, lin[..., :C, :, :] / (lin[..., C:, :, :] + eps)) and same_bits(norm, lin[..., C, :, :])
    # softmax: m = exp(w - max over the sample); a constant added to the weight cancels
    w = np.log(M)
    out = coords.splat(X, F, ohw, weight=w, mode="softmax")
    m = np.exp(w - w.max(axis=(-2, -1), keepdims=True))
    sm = SR.splat(Xb, Fb, m.reshape(Mb.shape), ohw, True)[0].reshape(ones.shape)
    assert same_bits(out, sm[..., :C, :, :] / (sm[..., C:, :, :] + eps))
    shifted = coords.splat(X, F, ohw, weight=w + 1024.0, mode="softmax")           # exact in float64: the shifted weights differ by the same bits
    assert np.abs(shifted - out).max() <= 1e-12 * np.abs(out).max()
    with np.errstate(invalid="ignore"):                               # eps = 0: a hole is 0 / 0
        far = coords.splat(X, F, ohw, weight=w + 1e4, mode="softmax", eps=0.0)        # exp(1e4) alone would overflow
        ref0 = coords.splat(X, F, ohw, weight=w, mode="softmax", eps=0.0)
    ok = np.isfinite(ref0)
    assert ok.any() and np.abs(far[ok] - ref0[ok]).max() <= 1e-9 * np.abs(ref0[ok]).max()
    wn = w.copy()
    wn[..., 0, 0] = np.nan                                           # a NaN weight counts as -inf: that pixel has no importance
    out_n, norm_n = coords.splat(X, F, ohw, weight=wn, mode="softmax", return_norm=True)
    assert np.isfinite(out_n).all() and np.isfinite(norm_n).all()
    # float32 sources give float32; a float32 tensor on the host goes the same way
    o32 = coords.splat(X.astype(f32), F, ohw, mode="average")
    assert o32.dtype == f32
    t32 = coords.splat(torch.from_numpy(X.astype(f32)), torch.from_numpy(F), ohw, mode="average")
    assert same_bits(np.asarray(t32), o32)
