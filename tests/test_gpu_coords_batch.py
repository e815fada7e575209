"""The batched forms of the chained coordinate-map operations on the device (entry_kernel<OP>, cell_kernel<RasterOp> and the two passes
of the mesh adjoint of csrc/lerf_coords.hip with the set on blockIdx.z, behind ops.coords_* and coords.*).  B = 3 throughout; the tiles
are 23 x 31 and 70 x 130 (blocks are 64 x 4 entries: both cross the block seams on both axes).  The cases are the ones
tests/test_coords_batch_cpu.py settles on the host twins: a clean sample, one with NaN, +-inf and 1e300 entries, one that folds.

  1. bit-equal forms: every batched device entry point equals its batched host twin and three single-map device calls by bit pattern --
     mesh (bilinear, bicubic), compose, invert, invert_raster (G and keys), grad_inner of compose; the mesh adjoint (which has no host
     twin) equals three single-map device calls; the contended minifying map gives the same bits in two runs.  One exception, on
     the sample with special entries only and against the HOST only: a NaN produced by arithmetic has the platform's sign bit
     (same_as_host below); device against device is by bits throughout;
  2. the atomic scatters grad_outer and grad_f within ADJ_TOL of the host twin, of the sum of single-map calls, with a shared outer
     map too, and of float64 autograd of the restatement;
  3. the differentiable twins on a batch give the per-sample results and gradients; three squarings of a batched flow through
     compose_torch into a batched remap class;
  4. strides: sentinel padding between sets and rows is untouched after every device call.
"""
import numpy as np
import pytest

import coords_ref as R
from test_coords_batch_cpu import B, F64, cast, compose_case, invert_case, mesh_case, padded, raster_case, upstream_case
from test_coords_grad_cpu import ADJ_TOL, compose_grads_ref, inner_map, invert_grad_ref, upstream
from test_coords_raster_cpu import minify_map
from test_gpu_remap_grad import _classes, _map_close, _operands

pytestmark = pytest.mark.gpu

HWS = [(23, 31), (70, 130)]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _keys(t):
    return _np(t).view(np.uint64)


def same_as_host(got, host):
    """device against host twin, sample by sample of a batch whose sample 1 holds the special entries: bit patterns on the samples
    whose operands are finite; on sample 1 the same NaN positions and the same bits everywhere else.  A NaN that ARITHMETIC produces
    (inf - inf, 0 * inf in the mesh's weighted sum or in a Jacobian) carries the sign bit on the host's x86 and not on the GPU; the
    kernels' own NaN results (compose, invert, the rasteriser) are one constant and compare by bits like everything else."""
    if not (R.same_bits(got[0], host[0]) and R.same_bits(got[2], host[2])):
        return False
    nan = np.isnan(host[1])
    return bool(np.array_equal(np.isnan(got[1]), nan)) and R.same_bits(np.where(nan, 0, got[1]), np.where(nan, 0, host[1]))


def adj_close(got, ref, what):
    scale = max(float(np.max(np.abs(ref))), 1.0)
    err = float(np.max(np.abs(got - ref)))
    print("%s: max error %.3g, scale %.3g, relative %.3g, bound %.3g" % (what, err, scale, err / scale, ADJ_TOL * scale))
    assert np.isfinite(err) and err <= ADJ_TOL * scale, what


def smooth_outer(hw, seed):
    """a smooth map with a non-singular Jacobian in every cell (what the autograd restatement of invert needs)"""
    ii, jj = np.meshgrid(np.arange(hw[0], dtype=np.float64), np.arange(hw[1], dtype=np.float64), indexing="ij")
    return np.stack([1.3 * ii + 0.2 * jj + 0.4 * np.sin(jj / 5.0 + seed), 0.8 * jj - 0.1 * ii + 0.3 * np.cos(ii / 4.0 + seed)], axis=-1)


# ---------------------------------------------------------------------------------------------- 1. bit-equal forms
@pytest.mark.parametrize("interp", ["bilinear", "bicubic"])
@pytest.mark.parametrize("hw", HWS)
def test_mesh_batch_is_bit_equal(torch, hw, interp):
    from lerf_pytorch_amd import _lib, ops
    for cdt, odt in ((np.float64, np.float64), (np.float32, np.float64), (np.float64, np.float32)):
        ctrl = cast(mesh_case(), cdt)
        host = _lib.coords_mesh_host(ctrl, hw, interp, odt)
        cd = _dev(torch, ctrl)
        got = ops.coords_mesh(cd, hw, interp, dtype=getattr(torch, np.dtype(odt).name))
        assert tuple(got.shape) == (B,) + hw + (2,) and same_as_host(_np(got), host)
        for s in range(B):
            assert R.same_bits(_np(ops.coords_mesh(cd[s], hw, interp, dtype=got.dtype)), _np(got[s])), s


@pytest.mark.parametrize("hw", HWS)
def test_compose_batch_is_bit_equal(torch, hw):
    from lerf_pytorch_amd import _lib, ops
    A, Bm = compose_case(hw)
    for adt, bdt in ((np.float64, np.float64), (np.float32, np.float64), (np.float64, np.float32)):
        a, b = cast(A, adt), cast(Bm, bdt)
        ad, bd = _dev(torch, a), _dev(torch, b)
        got = ops.coords_compose(ad, bd)
        assert got.dtype == bd.dtype and R.same_bits(_np(got), _lib.coords_compose_host(a, b, bdt))        # C's dtype: the inner map's
        shared = ops.coords_compose(ad[0], bd)                                     # one outer map for every sample
        assert R.same_bits(_np(shared), _lib.coords_compose_host(a[0], b, bdt))
        for s in range(B):
            assert R.same_bits(_np(ops.coords_compose(ad[s], bd[s])), _np(got[s])), s
            assert R.same_bits(_np(ops.coords_compose(ad[0], bd[s])), _np(shared[s])), s


@pytest.mark.parametrize("hw", HWS)
def test_invert_batch_is_bit_equal(torch, hw):
    from lerf_pytorch_amd import _lib, ops
    F, init = invert_case(hw)
    Fd, initd = _dev(torch, F), _dev(torch, init)
    for start, startd, iters in ((None, None, 16), (init, initd, 4), (None, None, 1)):
        got = ops.coords_invert(Fd, hw, init=startd, max_iter=iters)
        assert R.same_bits(_np(got), _lib.coords_invert_host(F, hw, init=start, max_iter=iters))
        for s in range(B):
            one = ops.coords_invert(Fd[s], hw, init=None if startd is None else startd[s], max_iter=iters)
            assert R.same_bits(_np(one), _np(got[s])), s
    shared = ops.coords_invert(Fd[0], hw, init=initd, dtype=torch.float32)         # one map, a start per sample
    assert R.same_bits(_np(shared), _lib.coords_invert_host(F[0], hw, init=init, dtype=np.float32))


@pytest.mark.parametrize("hw", HWS)
def test_raster_batch_is_bit_equal(torch, hw):
    from lerf_pytorch_amd import _lib, ops
    F, depth = raster_case(hw)
    Fd, dd = _dev(torch, F), _dev(torch, depth)
    for d, ddev in ((None, None), (depth, dd), (depth[0], dd[0])):                 # no depth, one per sample, one shared plane
        hG, hK = _lib.coords_invert_raster_host(F, hw, depth=d, return_keys=True)
        G, K = ops.coords_invert_raster(Fd, hw, depth=ddev, return_keys=True)
        assert tuple(K.shape) == (B,) + hw and R.same_bits(_np(G), hG) and np.array_equal(_keys(K), hK)
        for s in range(B):
            g, k = ops.coords_invert_raster(Fd[s], hw, depth=None if ddev is None else (ddev[s] if ddev.ndim == 3 else ddev), return_keys=True)
            assert R.same_bits(_np(g), _np(G[s])) and torch.equal(k, K[s]), s


def test_the_contended_minifying_batch_gives_the_same_bits_in_two_runs(torch):
    from lerf_pytorch_amd import _lib, ops
    F = np.stack([np.ascontiguousarray(minify_map((70, 130))), np.ascontiguousarray(minify_map((70, 130)))[::-1].copy(), 0.3 * minify_map((70, 130))])
    depth = np.random.default_rng(5).uniform(1.0, 2.0, (B, 70, 130)).astype(np.float32)
    Fd, dd = _dev(torch, F), _dev(torch, depth)
    host = _lib.coords_invert_raster_host(F, (18, 33), depth=depth, return_keys=True)
    a = ops.coords_invert_raster(Fd, (18, 33), depth=dd, return_keys=True)
    b = ops.coords_invert_raster(Fd, (18, 33), depth=dd, return_keys=True)
    for G, K in (a, b):
        assert R.same_bits(_np(G), host[0]) and np.array_equal(_keys(K), host[1])
    assert not np.isnan(host[0][0, 1:-1, 1:-1]).any()                              # some sixteen cells land on every pixel


@pytest.mark.parametrize("interp", ["bilinear", "bicubic"])
@pytest.mark.parametrize("hw", HWS)
def test_mesh_adjoint_batch_equals_single_calls(torch, hw, interp):
    from lerf_pytorch_amd import ops
    import torch.nn.functional as Fn
    g = upstream_case(hw)
    g[1] = np.nan_to_num(g[1])
    gd = _dev(torch, g)
    for ghw in ((4, 5), (2, 2)):                                                   # 2 x 2: every vertex reaches the whole map
        got = ops.coords_mesh_bwd(gd, ghw, interp)
        assert tuple(got.shape) == (B,) + ghw + (2,)
        for s in range(B):
            assert torch.equal(ops.coords_mesh_bwd(gd[s], ghw, interp), got[s]), s
        assert torch.equal(ops.coords_mesh_bwd(gd, ghw, interp), got)                 # fixed summation order: two runs agree
        acc = torch.full_like(got, 0.5)
        assert ops.coords_mesh_bwd(gd, ghw, interp, grad_ctrl=acc).data_ptr() == acc.data_ptr()
        adj_close(_np(acc), 0.5 + _np(got), "mesh adjoint accumulates")
    c = torch.zeros((B, 2, 4, 5), dtype=torch.float64, device="cuda", requires_grad=True)      # the transpose, by autograd of torch's upsample
    up = Fn.interpolate(c, size=hw, mode=interp, align_corners=True)
    ref, = torch.autograd.grad((up * gd.permute(0, 3, 1, 2)).sum(), c)
    adj_close(_np(ops.coords_mesh_bwd(gd, (4, 5), interp)), _np(ref.permute(0, 2, 3, 1)), "mesh adjoint vs autograd of F.interpolate")


# ---------------------------------------------------------------------------------------------- 2. the adjoints
@pytest.mark.parametrize("hw", HWS)
def test_compose_backward_batch(torch, hw):
    from lerf_pytorch_amd import _lib, ops
    A, Bm = compose_case(hw)
    g = upstream_case(hw)
    Ad, Bd, gd = _dev(torch, A), _dev(torch, Bm), _dev(torch, g)
    finite = lambda a: np.nan_to_num(a, nan=0.0, posinf=0.0, neginf=0.0)
    ha, hb = _lib.coords_compose_bwd_host(A, Bm, g)
    ga, gb = ops.coords_compose_bwd(Ad, Bd, gd)
    assert same_as_host(_np(gb), hb)                                               # one writer per entry: bit-equal
    assert np.array_equal(np.isfinite(_np(ga)), np.isfinite(ha))
    adj_close(finite(_np(ga)), finite(ha), "batched grad_outer vs host twin %s" % (hw,))
    for s in range(B):
        a1, b1 = ops.coords_compose_bwd(Ad[s], Bd[s], gd[s])
        assert torch.equal(torch.nan_to_num(b1), torch.nan_to_num(gb[s])) and torch.equal(torch.isnan(b1), torch.isnan(gb[s]))
        adj_close(finite(_np(ga[s])), finite(_np(a1)), "batched grad_outer vs single call %d" % s)
    # a shared outer map: one buffer gains the sum over the samples (samples 0 and 2: finite operands)
    keep = [0, 2]
    A0, Bk, gk = A[0], Bm[keep], g[keep]
    sa, sb = ops.coords_compose_bwd(Ad[0], _dev(torch, Bk), _dev(torch, gk))
    hsa, hsb = _lib.coords_compose_bwd_host(A0, Bk, gk)
    assert tuple(sa.shape) == A0.shape and R.same_bits(_np(sb), hsb)
    adj_close(_np(sa), hsa, "shared grad_outer vs host twin")
    total = sum(_np(ops.coords_compose_bwd(Ad[0], Bd[s], gd[s], need=(True, False))[0]) for s in keep)
    adj_close(_np(sa), total, "shared grad_outer vs the sum of single calls")
    ra = sum(compose_grads_ref(A0, Bm[s], g[s])[0] for s in keep)
    adj_close(_np(sa), ra, "shared grad_outer vs autograd of the restatement")
    r0a, r0b = compose_grads_ref(A[0], Bm[0], g[0])
    adj_close(_np(ga[0]), r0a, "grad_outer of sample 0 vs autograd")
    adj_close(_np(gb[0]), r0b, "grad_inner of sample 0 vs autograd")


@pytest.mark.parametrize("hw", HWS)
def test_invert_backward_batch(torch, hw):
    from lerf_pytorch_amd import _lib, ops
    F, _ = invert_case(hw)
    F[1:] = [smooth_outer(F.shape[1:3], 1), smooth_outer(F.shape[1:3], 2)]          # maps autograd of the restatement can follow
    Fd = _dev(torch, F)
    Gd = ops.coords_invert(Fd, hw)
    G = _np(Gd)
    g = np.where(np.isnan(G), 0.0, np.stack([upstream(hw, seed=50 + s) for s in range(B)]))
    gd = _dev(torch, g)
    gf = ops.coords_invert_bwd(Fd, Gd, gd)
    adj_close(_np(gf), _lib.coords_invert_bwd_host(F, G, g), "batched grad_f vs host twin %s" % (hw,))
    for s in range(B):
        adj_close(_np(gf[s]), _np(ops.coords_invert_bwd(Fd[s], Gd[s], gd[s])), "batched grad_f vs single call %d" % s)
        adj_close(_np(gf[s]), invert_grad_ref(F[s], G[s], g[s]), "batched grad_f vs autograd of the restatement %d" % s)
    assert all(bool((gf[s] != 0).any()) for s in range(B))
    # the special sample: NaN entries of the inverse and of F contribute nothing, on the device as on the host
    F2, _ = invert_case(hw)
    G2 = _lib.coords_invert_host(F2, hw)
    g2 = upstream_case(hw)
    g2[1] = np.nan_to_num(g2[1])
    got, ref = _np(ops.coords_invert_bwd(_dev(torch, F2), _dev(torch, G2), _dev(torch, g2))), _lib.coords_invert_bwd_host(F2, G2, g2)
    assert np.array_equal(np.isfinite(got), np.isfinite(ref))
    adj_close(np.nan_to_num(got, posinf=0.0, neginf=0.0), np.nan_to_num(ref, posinf=0.0, neginf=0.0), "special samples vs host twin")


# ---------------------------------------------------------------------------------------------- 3. the differentiable twins
def test_twins_on_a_batch_give_the_per_sample_results_and_gradients(torch):
    from lerf_pytorch_amd import coords
    hw, ahw = (23, 31), (12, 17)
    As = np.stack([smooth_outer(ahw, s) for s in range(B)])
    Bs = np.stack([inner_map(ahw, hw, seed=20 + s) for s in range(B)])
    gs = _dev(torch, np.stack([upstream(hw, 30 + s) for s in range(B)]))
    for shared in (False, True):
        la, lb = _dev(torch, As[0] if shared else As).requires_grad_(True), _dev(torch, Bs).requires_grad_(True)
        out = coords.compose_torch(la, lb)
        out.backward(gs)
        wa = np.zeros(la.shape)
        for n in range(B):
            a1, b1 = _dev(torch, As[0] if shared else As[n]).requires_grad_(True), _dev(torch, Bs[n]).requires_grad_(True)
            o1 = coords.compose_torch(a1, b1)
            assert torch.equal(o1.detach(), out[n].detach())
            o1.backward(gs[n])
            assert torch.equal(b1.grad, lb.grad[n])
            if shared:
                wa += _np(a1.grad)
            else:
                wa[n] = _np(a1.grad)
        adj_close(_np(la.grad), wa, "compose_torch grad_outer, shared=%s" % shared)
    Fs = np.stack([smooth_outer((hw[0] + 6, hw[1] + 9), s) for s in range(B)])
    lf = _dev(torch, Fs).requires_grad_(True)
    inv = coords.invert_torch(lf, hw)
    w = torch.where(torch.isnan(inv.detach()), torch.zeros_like(inv), gs)
    torch.nansum(inv * w).backward()
    for n in range(B):
        f1 = _dev(torch, Fs[n]).requires_grad_(True)
        i1 = coords.invert_torch(f1, hw)
        assert R.same_bits(_np(i1), _np(inv[n]))
        torch.nansum(i1 * w[n]).backward()
        adj_close(_np(lf.grad[n]), _np(f1.grad), "invert_torch grad_f %d" % n)
    for interp in ("bilinear", "bicubic"):
        for dt in (torch.float64, torch.float32):
            lc = _dev(torch, mesh_case()[[0, 2, 0]]).to(dt).requires_grad_(True)
            m = coords.from_mesh_torch(lc, hw, interp)
            assert tuple(m.shape) == (B,) + hw + (2,) and m.dtype == dt and m.requires_grad
            m.backward(gs.to(dt))
            assert tuple(lc.grad.shape) == tuple(lc.shape) and lc.grad.dtype == dt
            for n in range(B):
                c1 = lc.detach()[n].clone().requires_grad_(True)
                m1 = coords.from_mesh_torch(c1, hw, interp)
                assert torch.equal(m1.detach(), m[n].detach())
                m1.backward(gs[n].to(dt))
                assert torch.equal(c1.grad, lc.grad[n])                            # fixed summation order: bit-equal
    assert same_as_host(_np(coords.from_mesh(_dev(torch, mesh_case()), hw, "bicubic")), coords.from_mesh(mesh_case(), hw, "bicubic"))


def test_three_squarings_of_a_batched_flow_into_a_batched_remap(torch):
    from lerf_pytorch_amd import coords
    T = _classes()
    hw, P = (23, 31), 2
    x, _ = _operands(torch, "cubic", in_hw=hw, planes=B * P)
    x4 = x.view((B, P) + hw)
    gen = torch.Generator(device="cuda").manual_seed(11)
    v = (torch.rand((B,) + hw + (2,), generator=gen, device="cuda", dtype=torch.float64) - 0.5) * 0.6
    Gw = torch.rand((B, P) + hw, generator=gen, device="cuda", dtype=torch.float64)

    def loss_of(vel, images, weights):
        phi = coords.from_flow_torch(vel / 8.0)
        for _ in range(3):                                                         # scaling and squaring: phi <- phi o phi
            phi = coords.compose_torch(phi, phi)
        w = T.BicubicRemap2dTorch().enable_backward()
        w.set_shape([images.shape[0], P] + list(hw), phi)
        return (torch.nan_to_num(w.warp(images), nan=0.0) * weights).sum(), phi

    leaf = v.clone().requires_grad_(True)
    loss, phi = loss_of(leaf, x4, Gw)
    assert tuple(phi.shape) == (B,) + hw + (2,) and phi.requires_grad
    loss.backward()
    assert tuple(leaf.grad.shape) == tuple(v.shape) and bool((leaf.grad != 0).any())
    total = 0.0
    for n in range(B):
        l1 = v[n].clone().requires_grad_(True)
        loss1, phi1 = loss_of(l1, x4[n:n + 1], Gw[n:n + 1])
        assert torch.equal(phi1.detach(), phi[n].detach())
        loss1.backward()
        total += float(loss1.detach())
        _map_close(_np(leaf.grad[n]), _np(l1.grad), "three squarings, sample %d" % n)
    assert abs(float(loss.detach()) - total) <= 1e-9 * max(abs(total), 1.0)


# ---------------------------------------------------------------------------------------------- 4. strides on the device
def _dev_padded(torch, a, sentinel=-7.0):
    """padded() on the device: (buffer, the strided view that holds `a`)"""
    buf, view = padded(a, sentinel=sentinel)
    n, h, w = a.shape[:3]
    dbuf = torch.from_numpy(buf).cuda()
    return dbuf, dbuf[::2, 2:2 + h, 3:3 + w]


def _dev_untouched(torch, dbuf, view):
    keep = view.clone()
    view[...] = -7.0
    ok = bool((dbuf == -7.0).all())
    view[...] = keep
    return ok


@pytest.mark.parametrize("hw", HWS)
def test_padding_between_sets_and_rows_is_untouched(torch, hw):
    from lerf_pytorch_amd import _lib, ops
    zeros = np.zeros((B,) + hw + (2,))
    origin, full = (3, 7), (hw[0] + 5, hw[1] + 9)
    # mesh: a tile at an origin, written into a strided batch view
    ctrl = mesh_case()
    buf, out = _dev_padded(torch, zeros)
    assert ops.coords_mesh(_dev(torch, ctrl), hw, "bicubic", out=out, origin=origin, full_hw=full).data_ptr() == out.data_ptr()
    whole = _lib.coords_mesh_host(ctrl, full, "bicubic")
    assert same_as_host(_np(out), np.ascontiguousarray(whole[:, 3:3 + hw[0], 7:7 + hw[1]])) and _dev_untouched(torch, buf, out)
    # compose: every operand a strided view (NaN in the gaps of the inputs: a read outside a view would show)
    A, Bm = compose_case(hw)
    (_, a), (_, b) = _dev_padded(torch, A, np.nan), _dev_padded(torch, Bm, np.nan)
    buf, out = _dev_padded(torch, cast(zeros, np.float32))
    ops.coords_compose(a, b, out=out)
    assert R.same_bits(_np(out), _lib.coords_compose_host(A, Bm, np.float32)) and _dev_untouched(torch, buf, out)
    # invert: a tile of the whole inverse
    F, init = invert_case(full)
    tile = np.ascontiguousarray(init[:, 3:3 + hw[0], 7:7 + hw[1]])
    (_, f), (_, i) = _dev_padded(torch, F, np.nan), _dev_padded(torch, tile, np.nan)
    buf, out = _dev_padded(torch, zeros)
    ops.coords_invert(f, hw, init=i, out=out, origin=origin, max_iter=4)
    assert R.same_bits(_np(out), _lib.coords_invert_host(F, hw, init=tile, origin=origin, max_iter=4)) and _dev_untouched(torch, buf, out)
    # raster: a tile; the keys are dense per sample
    F, depth = raster_case(full)
    (_, f) = _dev_padded(torch, F, np.nan)
    buf, out = _dev_padded(torch, zeros)
    _, K = ops.coords_invert_raster(f, hw, depth=_dev(torch, depth), out=out, origin=origin, return_keys=True)
    hG, hK = _lib.coords_invert_raster_host(F, hw, depth=depth, origin=origin, return_keys=True)
    assert R.same_bits(_np(out), hG) and np.array_equal(_keys(K), hK) and _dev_untouched(torch, buf, out)
    # the adjoints through the C entry points: set strides larger than a set on every gradient, sentinel in the gaps
    A, Bm = compose_case(hw)
    g = upstream_case(hw)
    na, nb, pad = 2 * A.shape[1] * A.shape[2], 2 * hw[0] * hw[1], 6
    gbuf, gabuf, gbbuf = np.full((B, nb + pad), -7.0), np.full((B, na + pad), -7.0), np.full((B, nb + pad), -7.0)
    gbuf[:, :nb], gabuf[:, :na], gbbuf[:, :nb] = g.reshape(B, nb), 0.0, 0.0
    Ad, Bd, gd, gad, gbd = (_dev(torch, t) for t in (A, Bm, gbuf, gabuf, gbbuf))
    L, st = _lib.lib(), _lib.current_stream(Ad.device)
    rc = L.lerf_coords_compose_bwd_batched(Ad.data_ptr(), F64, 2 * A.shape[2], A.shape[1], A.shape[2], Bd.data_ptr(), F64, 2 * hw[1], gd.data_ptr(),
                                           hw[0], hw[1], gad.data_ptr(), gbd.data_ptr(), B, na, nb, nb + pad, na + pad, nb + pad, st)
    assert rc == 0
    ha, hb = _lib.coords_compose_bwd_host(A, Bm, g)
    assert same_as_host(_np(gbd)[:, :nb].reshape(Bm.shape), hb)
    assert np.array_equal(np.isfinite(_np(gad)[:, :na].reshape(A.shape)), np.isfinite(ha))
    adj_close(np.nan_to_num(_np(gad)[:, :na].reshape(A.shape), posinf=0, neginf=0), np.nan_to_num(ha, posinf=0, neginf=0), "padded grad_outer")
    assert bool((gad[:, na:] == -7.0).all()) and bool((gbd[:, nb:] == -7.0).all()) and bool((gd[:, nb:] == -7.0).all())
    F, _ = invert_case(hw)
    G = _lib.coords_invert_host(F, hw)
    g[1] = np.nan_to_num(g[1])
    gbuf[:, :nb] = g.reshape(B, nb)
    nf = 2 * F.shape[1] * F.shape[2]
    gfbuf = np.full((B, nf + pad), -7.0)
    gfbuf[:, :nf] = 0.0
    Fd, Gd, gd, gfd = (_dev(torch, t) for t in (F, G, gbuf, gfbuf))
    rc = L.lerf_coords_invert_bwd_batched(Fd.data_ptr(), F64, 2 * F.shape[2], F.shape[1], F.shape[2], Gd.data_ptr(), F64, 2 * hw[1], gd.data_ptr(), hw[0],
                                          hw[1], gfd.data_ptr(), B, nf, nb, nb + pad, nf + pad, st)
    assert rc == 0
    ref = _lib.coords_invert_bwd_host(F, G, g)
    got = _np(gfd)[:, :nf].reshape(F.shape)
    assert np.array_equal(np.isfinite(got), np.isfinite(ref))
    adj_close(np.nan_to_num(got, posinf=0, neginf=0), np.nan_to_num(ref, posinf=0, neginf=0), "padded grad_f")
    assert bool((gfd[:, nf:] == -7.0).all())
    # the mesh adjoint: padded set strides on grad_map and grad_ctrl
    gh, gw = 4, 5
    nc = 2 * gh * gw
    gcbuf = np.full((B, nc + pad), -7.0)
    gcbuf[:, :nc] = 0.0
    gcd = _dev(torch, gcbuf)
    need = B * int(L.lerf_coords_mesh_bwd_workspace_bytes(gh, gw, hw[0], hw[1]))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc = L.lerf_coords_mesh_bwd_batched(gd.data_ptr(), hw[0], hw[1], 1, gh, gw, gcd.data_ptr(), ws.data_ptr(), need, B, nb + pad, nc + pad, st)
    assert rc == 0
    ref = ops.coords_mesh_bwd(_dev(torch, g), (gh, gw), "bicubic")
    assert torch.equal(gcd[:, :nc].reshape(B, gh, gw, 2), ref) and bool((gcd[:, nc:] == -7.0).all()) and bool((gd[:, nb:] == -7.0).all())
