"""The forward warp by summation splatting on the device (entry_kernel<SplatOp> and entry_kernel<SplatBwdOp> of csrc/lerf_coords.hip behind
ops.splat / ops.splat_bwd and coords.splat / coords.splat_torch), against the host twins that tests/test_splat_cpu.py pins to the
restatement:

  1. the backward is the host twin's by bit pattern, twice in a row; exact zeros at non-finite entries under a NaN-filled upstream;
  2. the forward within the bound of a reordered sum, per element:  |device - host| <= 2 n[q] u sum|term|,  u = 2^-24 (float32) or 2^-53
     (float64), n[q] and sum|term| from the restatement (tests/splat_ref.py) -- each of the two sums carries a rounding error of at most
     (n - 1) u sum|term| to first order -- and exactly where n[q] <= 1; the same under contention (a 70 x 130 source into an 8 x 8 patch);
  3. the forward exactly where every partial sum is exact in any order (integer maps, small-integer src and weight);
  4. the accumulate contract; the padding of a strided map untouched; operands unmodified;
  5. splat_torch end to end against float64 autograd of the restatement on the same device, and the skipped halves;
  6. the occluded two-layer scene through reproject_torch -> splat_torch(mode="softmax");
  7. the Python-level refusals launch nothing.
"""
import numpy as np
import pytest

import splat_ref as SR
from test_coords_grad_cpu import ADJ_TOL
from test_coords_reproject_cpu import occluded_scene
from test_splat_cpu import CASES, IDS, as_batch, bits, f32, f64, make_case, same_bits, special_map, upstream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def _dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def unit(T):
    return 2.0 ** (-24 if T == f32 else -53)


# ---------------------------------------------------------------------------------------------- 1. backward
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward_is_the_host_twin_by_bit_pattern_twice(torch, case):
    from lerf_pytorch_amd import _lib, ops
    X, F, M = make_case(case)
    G, norm = upstream(case), case[7]
    need = (True, M is not None, True)
    ref = _lib.splat_bwd_host(X, F, G, M, norm, need)
    dX, dF, dM, dG = (_dev(torch, a) for a in (X, F, M, G))
    for _ in range(2):
        got = ops.splat_bwd(dX, dF, dG, dM, norm, need)
        for g, r in zip(got, ref):
            assert (g is None) == (r is None) and (g is None or same_bits(_np(g), r))
    for k in range(3):
        if need[k]:
            one = tuple(i == k for i in range(3))
            alone = ops.splat_bwd(dX, dF, dG, dM, norm, one)
            assert [a is None for a in alone] == [not w for w in one] and same_bits(_np(alone[k]), ref[k])
    for d, h in ((dX, X), (dF, F), (dM, M), (dG, G)):
        assert h is None or same_bits(_np(d), h)


@pytest.mark.parametrize("T", [f32, f64])
def test_non_finite_entries_get_exact_zeros_under_a_nan_upstream(torch, T):
    from lerf_pytorch_amd import ops
    hw, ohw = (23, 31), (29, 37)
    rng = np.random.default_rng(8)
    X, M = rng.standard_normal((3,) + hw).astype(T), rng.uniform(0.25, 2.0, hw).astype(T)
    F = special_map(hw, ohw, f64)
    bad = ~np.isfinite(F).all(-1)
    assert bad.sum() == 4                                            # NaN in r, NaN in c, +inf, -inf (1e300 is finite: its taps are dropped)
    G = np.full((4,) + ohw, np.nan, T)
    gx, gm, gf = (_np(t) for t in ops.splat_bwd(_dev(torch, X), _dev(torch, F), _dev(torch, G), _dev(torch, M), True))
    assert not bits(gx[:, bad]).any() and not bits(gm[bad]).any() and not bits(gf[bad]).any()
    landed = ~bad & (F[..., 0] > 0) & (F[..., 0] < 28) & (F[..., 1] > 0) & (F[..., 1] < 36)
    assert np.isnan(gx[:, landed]).all() and np.isnan(gm[landed]).all()                  # a NaN upstream at a finite entry propagates


# ---------------------------------------------------------------------------------------------- 2. forward, the bound of a reordered sum
def check_reordered(got, host, n, mag, T):
    got, host = got.astype(f64).reshape(n.shape), host.astype(f64).reshape(n.shape)
    err = np.abs(got - host)
    bound = 2.0 * n * unit(T) * mag
    print("max err %.3e, max bound %.3e, max n %d, elements with n <= 1: %d" % (err.max(), bound.max(), n.max(), int((n <= 1).sum())))
    assert (err <= bound).all()
    assert (err[n <= 1] == 0).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_within_the_bound_of_a_reordered_sum(torch, case):
    from lerf_pytorch_amd import _lib, ops
    X, F, M = make_case(case)
    ohw, norm, T = case[1], case[7], case[5]
    host = _lib.splat_host(X, F, ohw, M, norm)
    _, n, mag = SR.splat(*as_batch(X, F, M), ohw, norm)
    dX, dF, dM = (_dev(torch, a) for a in (X, F, M))
    got = ops.splat(dX, dF, ohw, dM, norm)
    assert got.shape == host.shape and got.dtype == dX.dtype
    check_reordered(_np(got), host, n, mag, T)
    for d, h in ((dX, X), (dF, F), (dM, M)):
        assert h is None or same_bits(_np(d), h)


@pytest.mark.parametrize("T", [f32, f64])
def test_forward_under_contention(torch, T):
    """a 70 x 130 source into an 8 x 8 patch of a 64 x 150 frame: about 570 adders per element"""
    from lerf_pytorch_amd import _lib, ops
    H, W, ohw = 70, 130, (64, 150)
    rng = np.random.default_rng(7)
    X = rng.standard_normal((3, H, W)).astype(T)
    M = rng.uniform(0.25, 2.0, (H, W)).astype(T)
    i, j = np.meshgrid(np.arange(H, dtype=f64), np.arange(W, dtype=f64), indexing="ij")
    F = np.stack([20.3 + i * (7.0 / H), 41.7 + j * (7.0 / W)], -1)
    host = _lib.splat_host(X, F, ohw, M, True)
    _, n, mag = SR.splat_one(X, F, M, ohw, True)
    assert n.max() > 400 and (n > 0).sum() == 4 * 9 * 9
    got = ops.splat(_dev(torch, X), _dev(torch, F), ohw, _dev(torch, M), True)
    check_reordered(_np(got), host, n, mag, T)


# ---------------------------------------------------------------------------------------------- 3. forward, exact
@pytest.mark.parametrize("T,TF", [(f32, f32), (f64, f64), (f32, f64)])
def test_forward_is_exact_on_integer_maps(torch, T, TF):
    """integer-valued maps, small-integer src and weight: every partial sum is an integer below 2^24, exact in any order"""
    from lerf_pytorch_amd import _lib, coords, ops
    H, W, ohw, B = 70, 130, (64, 150), 3
    rng = np.random.default_rng(3)
    X = rng.integers(-8, 9, (B, 3, H, W)).astype(T)
    M = rng.integers(1, 5, (B, H, W)).astype(T)
    ident = coords.from_flow(np.zeros((H, W, 2)))
    F = np.stack([ident + np.array([-3.0, 63.0]),                    # a translation that pushes a third of the frame out on the right
                  np.floor(ident / 4.0) + np.array([5.0, 7.0]),      # 16 sources per target
                  ident[::-1, ::-1] - np.array([10.0, 0.0])])        # a flip, rows pushed out at the top
    F[1, 3, 5], F[1, 4, 6], F[1, 5, 7], F[2, 0, 0], F[2, 1, 1] = (np.nan, 1.0), (np.inf, 2.0), (3.0, -np.inf), (1e300, 1.0), (2.0, -1e300)
    with np.errstate(over="ignore"):
        F = F.astype(TF)                                             # 1e300 -> inf in float32
    host = _lib.splat_host(X, F, ohw, M, True)
    assert np.array_equal(host, np.round(host)) and np.abs(host).max() < 2 ** 24 and host[1].max() >= 16
    got = ops.splat(_dev(torch, X), _dev(torch, F), ohw, _dev(torch, M), True)
    assert torch.equal(got.cpu(), torch.from_numpy(host))
    one = ops.splat(_dev(torch, X[0]), _dev(torch, F[0]), ohw, None, False)
    assert torch.equal(one.cpu(), torch.from_numpy(_lib.splat_host(X[0], F[0], ohw)))
    want = np.zeros((3,) + ohw, T)
    want[:, :, 63:] = X[0][:, 3:67, :87]
    assert np.array_equal(_np(one), want)


# ---------------------------------------------------------------------------------------------- 4. accumulate, padding, operands
def test_accumulate_contract_and_strided_map(torch):
    from lerf_pytorch_amd import _lib, ops
    H, W, ohw, B = 23, 31, (29, 37), 3
    rng = np.random.default_rng(4)
    X = rng.integers(-8, 9, (B, 3, H, W)).astype(f32)
    with np.errstate(over="ignore"):
        F = np.stack([np.round(special_map((H, W), ohw, f64, s)) for s in range(B)]).astype(f32)   # integer positions, NaN / inf kept
    acc0 = rng.integers(-4, 5, (B, 4) + ohw).astype(f32)
    host = _lib.splat_host(X, F, ohw, None, True, acc=acc0.copy())
    buf = torch.full((B, H, W + 3, 2), -7.0, dtype=torch.float32, device="cuda")
    dF = buf[:, :, :W]
    dF.copy_(_dev(torch, F))
    assert dF.stride(1) == 2 * (W + 3) and not dF.is_contiguous()
    dX, acc = _dev(torch, X), _dev(torch, acc0)
    out = ops.splat(dX, dF, ohw, None, True, acc=acc)
    assert out is acc and torch.equal(acc.cpu(), torch.from_numpy(host))                          # exact: integers
    assert bool((buf[:, :, W:] == -7.0).all()) and same_bits(_np(dF.contiguous()), F) and same_bits(_np(dX), X)
    G = _dev(torch, rng.standard_normal((B, 4) + ohw).astype(f32))
    gx, _, gf = ops.splat_bwd(dX, dF, G, None, True, (True, False, True))
    hx, _, hf = _lib.splat_bwd_host(X, F, _np(G), None, True, (True, False, True))
    assert same_bits(_np(gx), hx) and same_bits(_np(gf), hf)
    assert bool((buf[:, :, W:] == -7.0).all()) and same_bits(_np(dF.contiguous()), F)


# ---------------------------------------------------------------------------------------------- 5. splat_torch
def test_splat_torch_against_autograd_of_the_restatement(torch):
    from lerf_pytorch_amd import coords
    H, W, ohw, B = 23, 31, (29, 37), 3
    rng = np.random.default_rng(5)
    X = rng.standard_normal((B, 3, H, W))
    F = np.stack([special_map((H, W), ohw, f64, s) for s in range(B)])
    with np.errstate(invalid="ignore"):
        F = np.where((F == np.floor(F)) & np.isfinite(F), F + 0.25, F)                             # autograd is two-sided nowhere: no integers
    Wt = rng.uniform(-1.0, 1.0, (B, H, W))
    G = _dev(torch, rng.standard_normal((B, 3) + ohw))

    def leaves():
        return [_dev(torch, a).requires_grad_(True) for a in (X, Wt, F)]

    for mode in ("linear", "softmax"):
        x, w, f = leaves()
        imp = torch.exp(w) if mode == "linear" else w
        out = coords.splat_torch(x, f, ohw, weight=imp, mode=mode)
        (out * G).sum().backward()
        rx, rw, rf = leaves()
        m = torch.exp(rw) if mode == "linear" else torch.exp(rw - rw.detach().amax(dim=(-2, -1), keepdim=True))
        acc = SR.torch_splat(rx, rf, m, ohw, True)
        ref = acc[:, :3] / (acc[:, 3:] + 1e-7)
        (ref * G).sum().backward()
        assert float((out - ref).detach().abs().max()) <= ADJ_TOL * max(float(ref.detach().abs().max()), 1.0)
        for got, want in ((x.grad, rx.grad), (w.grad, rw.grad), (f.grad, rf.grad)):
            assert float((got - want).abs().max()) <= ADJ_TOL * max(float(want.abs().max()), 1.0), mode
        bad = ~torch.isfinite(f.detach()).all(-1)
        assert bool(bad.any()) and not bool(f.grad[bad].any())
    # each skipped half returns None; a shared map gathers the sum over the samples
    for k in range(3):
        ls = [_dev(torch, a) for a in (X, np.exp(Wt), F)]
        ls[k].requires_grad_(True)
        coords.splat_torch(ls[0], ls[2], ohw, weight=ls[1]).sum().backward()
        assert [t.grad is None for t in ls] == [i != k for i in range(3)]
    f1 = _dev(torch, F[0]).requires_grad_(True)
    x = _dev(torch, X)
    coords.splat_torch(x, f1, ohw, mode="average").square().sum().backward()
    rf = _dev(torch, F[0]).requires_grad_(True)
    acc = SR.torch_splat(x, rf, None, ohw, True)
    (acc[:, :3] / (acc[:, 3:] + 1e-7)).square().sum().backward()
    assert f1.grad.shape == (H, W, 2) and float((f1.grad - rf.grad).abs().max()) <= ADJ_TOL * max(float(rf.grad.abs().max()), 1.0)
    with torch.no_grad():                                            # no graph: the plain kernel, what splat runs (two runs of a float sum:
        a = coords.splat_torch(x, f1, ohw, mode="average")           # equal up to the order of the adds, test 2's bound; float64 here)
    b = coords.splat(x, f1.detach(), ohw, mode="average")
    assert not a.requires_grad and float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())


# ---------------------------------------------------------------------------------------------- 6. the occluded scene
def test_softmax_splat_of_the_occluded_scene(torch):
    """The two-layer scene of the reproject / raster tests with INTEGER displacements (t_x = -0.5: the background, depth 8, moves 2 px,
    the square of depth 2 moves 8 px), so every landing is one pixel.  weight = -beta z with beta dz = 42: where both layers land,
    out - x_f = (m_b (x_b - x_f) - eps x_f) / (1 + m_b + eps) with m_b = exp(-beta dz); where the background lands alone,
    out = x_b / (1 + eps / m_b).  So |out - ref| <= exp(-beta dz) max|x_b - x_f| + (eps / norm) |ref|, plus a few ulp.  eps = 1e-30:
    the default 1e-7 is far above the background's own importance exp(-42) and would swallow it."""
    from lerf_pytorch_amd import coords
    d, K, _ = occluded_scene()
    t = np.array([-0.5, 0.0, 0.0])
    hw, beta, eps = (24, 32), 7.0, 1e-30
    assert beta * (8.0 - 2.0) >= 40
    img = np.random.default_rng(6).uniform(0.5, 1.5, (3,) + hw)
    depth = _dev(torch, d).requires_grad_(True)
    Kd, td, x = _dev(torch, K), _dev(torch, t), _dev(torch, img)
    m, z = coords.reproject_torch(depth, Kd, Kd, None, td, return_depth=True)
    assert np.array_equal(_np(m), np.round(_np(m)))
    out, norm = coords.splat_torch(x, m, hw, weight=-beta * z.double(), mode="softmax", eps=eps, return_norm=True)
    fg = np.zeros(hw, bool)
    fg[8:16, 12:20] = True
    ref, landed = np.zeros_like(img), np.zeros(hw, bool)
    landed[:, :30] = ~fg[:, 2:]
    ref[:, :, :30] = np.where(landed[:, :30], img[:, :, 2:], 0.0)
    ref[:, 8:16, 4:12], landed[8:16, 4:12] = img[:, 8:16, 12:20], True
    nrm = _np(norm)
    assert np.array_equal(nrm == 0, ~landed)
    G = coords.invert_raster(m.detach(), hw, depth=z.detach(), max_span=4, orient=1)
    assert np.array_equal(nrm == 0, np.isnan(_np(G)[..., 0]))        # exactly the entries the hard chain leaves NaN
    rel = eps / np.where(landed, nrm, 1.0)                           # a hole holds exactly 0: ref is 0 there and so must out be
    bound = np.where(landed, np.exp(-beta * 6.0) * 1.0 + (rel + 8 * 2.0 ** -53) * np.abs(ref), 0.0)
    err = np.abs(_np(out) - ref)
    print("max err %.3e, max bound %.3e" % (err.max(), bound.max()))
    assert (err <= bound).all()
    out.sum().backward()
    g = _np(depth.grad)
    assert np.isfinite(g).all() and np.abs(g[fg]).max() > 0


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_python_level_refusals_launch_nothing(torch, monkeypatch):
    from lerf_pytorch_amd import _lib, coords, ops
    L = _lib.lib()
    launched = []
    for name in ("lerf_splat", "lerf_splat_bwd", "lerf_splat_host", "lerf_splat_bwd_host"):
        monkeypatch.setattr(L, name, lambda *a, _n=name: launched.append(_n) or 0)
    xh, fh, wh = np.zeros((2, 3, 4)), np.zeros((3, 4, 2)), np.ones((3, 4))
    xd, fd, wd = (_dev(torch, a) for a in (xh, fh, wh))
    for call in (lambda: coords.splat(xd, fh, (5, 6)),                                            # mixed operands
                 lambda: coords.splat(xh, fd, (5, 6)),
                 lambda: coords.splat(xd, fd, (5, 6), weight=wh),
                 lambda: coords.splat(xd.clone().requires_grad_(True), fd, (5, 6)),              # no autograd
                 lambda: coords.splat(xd, fd.clone().requires_grad_(True), (5, 6)),
                 lambda: coords.splat(xd, fd, (5, 6), mode="max"),
                 lambda: coords.splat(xd, fd, (5, 6), weight=wd, mode="average"),
                 lambda: coords.splat(xd, fd, (5, 6), mode="softmax"),
                 lambda: coords.splat(xd, fd[:2], (5, 6)),
                 lambda: coords.splat(xd, fd, (0, 6)),
                 lambda: coords.splat_torch(xh, fd, (5, 6)),                                       # host operands
                 lambda: coords.splat_torch(xd, fd.cpu(), (5, 6)),
                 lambda: coords.splat_torch(xd.to(torch.int32), fd, (5, 6)),
                 lambda: coords.splat_torch(xd, fd, (5, 6), mode="linear"),
                 lambda: ops.splat(xd, fd, (5, 6), wd.float()),                                     # the weight's dtype
                 lambda: ops.splat(xd, fd, (5, 6), acc=torch.zeros((2, 5, 6), device="cuda")),     # the accumulator's dtype
                 lambda: ops.splat(xd, fd, (5, 6), acc=torch.zeros((3, 5, 6), dtype=torch.float64, device="cuda")),
                 lambda: ops.splat_bwd(xd, fd, torch.zeros((3, 5, 6), dtype=torch.float64, device="cuda")),
                 lambda: ops.splat_bwd(xd, fd, torch.zeros((2, 5, 6), dtype=torch.float64, device="cuda"), need=(False, False, False)),
                 lambda: ops.splat_bwd(xd, fd, torch.zeros((2, 5, 6), dtype=torch.float64, device="cuda"), need=(True, True, False))):
        with pytest.raises(ValueError):
            call()
    assert launched == []
