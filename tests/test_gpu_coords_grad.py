"""The adjoints of compose and invert on the device (entry_kernel<ComposeBwdOp>, entry_kernel<InvertBwdOp> of csrc/lerf_coords.hip behind
ops.coords_compose_bwd / coords_invert_bwd and coords.compose_torch / invert_torch / invert_flow_torch).  The bounds are the ones
tests/test_coords_grad_cpu.py settles on the host twins:

  5. parity: grad_b bit-equal to the host twin and from run to run; grad_a / grad_f (float64 atomic adds) within ADJ_TOL of the host
     twin and of autograd of the restatement -- ragged shapes, more than one block, many entries per cell, the contention case,
     dtype mixes, strided tile views inside NaN-filled buffers, the special entries;
  6. the accumulate contract and the null halves;
  7. the differentiable twins: bit equality under no_grad, gradient dtypes, compose_torch(phi, phi), the batch forms,
     invert_flow_torch, the refusals;
  8. autograd end to end through the remap, from a flow (compose) and from a control mesh (invert), against the chained
     restatements; the cancellation identity through autograd.
"""
import math

import numpy as np
import pytest

import coords_grad_ref as GR
import coords_ref as R
import remap_grad_ref
from test_coords_grad_cpu import ADJ_TOL, compose_grads_ref, inner_map, invert_grad_ref, special_compose, special_invert, upstream
from test_coords_invert_cpu import HW, _valid, invert_maps
from test_gpu_remap_grad import _close, _make, _classes, _operands

pytestmark = pytest.mark.gpu

HWS = [(37, 53), (70, 130), (1, 9)]          # inner map and gradient: 70 x 130 is more than one 4 x 64 block each way, ragged edges
OUTER_HWS = [(12, 17), (37, 53), (70, 130)]  # 12 x 17: many entries per cell


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def outer_map(hw, seed=1):
    """a smooth map of shape hw with a non-singular Jacobian in every cell: a stretched, sheared grid plus a gentle sinusoid"""
    ii, jj = np.meshgrid(np.arange(hw[0], dtype=np.float64), np.arange(hw[1], dtype=np.float64), indexing="ij")
    return np.stack([1.3 * ii + 0.2 * jj + 0.4 * np.sin(jj / 5.0 + seed), 0.8 * jj - 0.1 * ii + 0.3 * np.cos(ii / 4.0 + seed)], axis=-1)


def adj_close(got, ref, what):
    scale = max(float(np.max(np.abs(ref))), 1.0)
    err = float(np.max(np.abs(got - ref)))
    print("%s: max error %.3g, scale %.3g, relative %.3g, bound %.3g" % (what, err, scale, err / scale, ADJ_TOL * scale))
    assert np.isfinite(err) and err <= ADJ_TOL * scale, what


# ---------------------------------------------------------------------------------------------- 5. parity
@pytest.mark.parametrize("ahw", OUTER_HWS)
@pytest.mark.parametrize("hw", HWS)
def test_compose_backward_parity(torch, hw, ahw):
    from lerf_pytorch_amd import _lib, ops
    A, B, g = outer_map(ahw), inner_map(ahw, hw), upstream(hw)
    ha, hb = _lib.coords_compose_bwd_host(A, B, g)
    ga, gb = ops.coords_compose_bwd(_dev(torch, A), _dev(torch, B), _dev(torch, g))
    assert ga.dtype == torch.float64 and gb.dtype == torch.float64 and tuple(ga.shape) == ahw + (2,) and tuple(gb.shape) == hw + (2,)
    assert R.same_bits(_np(gb), hb)
    adj_close(_np(ga), ha, "compose %s in %s grad_outer vs host" % (hw, ahw))
    ra, rb = compose_grads_ref(A, B, g)
    adj_close(_np(ga), ra, "compose %s in %s grad_outer vs autograd" % (hw, ahw))
    adj_close(_np(gb), rb, "compose %s in %s grad_inner vs autograd" % (hw, ahw))
    ga2, gb2 = ops.coords_compose_bwd(_dev(torch, A), _dev(torch, B), _dev(torch, g))
    assert torch.equal(gb2, gb)                                       # one writer per entry: bit-equal from run to run
    adj_close(_np(ga2), _np(ga), "compose grad_outer, second run")


@pytest.mark.parametrize("fhw", OUTER_HWS)
@pytest.mark.parametrize("hw", HWS)
def test_invert_backward_parity(torch, hw, fhw):
    """any finite G serves: the gradient of the implicit function does not depend on the target the solver was given"""
    from lerf_pytorch_amd import _lib, ops
    F, G, g = outer_map(fhw), inner_map(fhw, hw, spill=0.5), upstream(hw)
    host = _lib.coords_invert_bwd_host(F, G, g)
    got = ops.coords_invert_bwd(_dev(torch, F), _dev(torch, G), _dev(torch, g))
    assert got.dtype == torch.float64 and tuple(got.shape) == fhw + (2,) and np.any(host != 0)
    adj_close(_np(got), host, "invert %s in %s grad_f vs host" % (hw, fhw))
    adj_close(_np(got), invert_grad_ref(F, G, g), "invert %s in %s grad_f vs autograd" % (hw, fhw))


@pytest.mark.parametrize("name", ["barrel", "homography", "mesh", "flow"])
def test_invert_backward_at_the_inverse_the_kernel_returned(torch, name):
    from lerf_pytorch_amd import _lib, ops
    F = invert_maps()[name]
    Gd = ops.coords_invert(_dev(torch, F), HW)
    G = _np(Gd)
    g = np.where(_valid(G)[..., None], upstream(HW, 6), 0.0)
    got = ops.coords_invert_bwd(_dev(torch, F), Gd, _dev(torch, g))
    adj_close(_np(got), _lib.coords_invert_bwd_host(F, G, g), "%s grad_f vs host" % name)
    adj_close(_np(got), invert_grad_ref(F, G, g), "%s grad_f vs autograd" % name)


def test_contention_all_entries_in_one_cell(torch):
    """a constant inner map of 70 x 130: 9 100 entries, four addresses"""
    from lerf_pytorch_amd import ops
    hw, ahw, pos = (70, 130), (12, 17), (4.25, 9.625)
    A, g = outer_map(ahw), upstream(hw)
    B = np.broadcast_to(np.array(pos), hw + (2,)).copy()
    ga, gb = ops.coords_compose_bwd(_dev(torch, A), _dev(torch, B), _dev(torch, g))
    want = np.zeros(ahw + (2,))
    tot = [math.fsum(g[..., k].ravel()) for k in range(2)]
    for a, wr in ((0, 0.75), (1, 0.25)):
        for b, wc in ((0, 0.375), (1, 0.625)):
            want[4 + a, 9 + b] = [wr * wc * tot[0], wr * wc * tot[1]]
    adj_close(_np(ga), want, "contention grad_outer vs the closed form")
    assert int((np.abs(_np(ga)).sum(-1) > 0).sum()) == 4
    # the same cell of F, every entry: the scatter of v = -J^-T g
    F = outer_map(ahw)
    got = ops.coords_invert_bwd(_dev(torch, F), _dev(torch, B), _dev(torch, g))
    adj_close(_np(got), invert_grad_ref(F, B, g), "contention grad_f vs autograd")
    assert int((np.abs(_np(got)).sum(-1) > 0).sum()) == 4


def test_dtype_mixes_and_strided_views(torch):
    from lerf_pytorch_amd import _lib, ops
    hw, ahw = (37, 53), (12, 17)
    A, B, g = outer_map(ahw), inner_map(ahw, hw), upstream(hw)
    gd = _dev(torch, g)
    nan = float("nan")
    for adt in (np.float64, np.float32):
        for bdt in (np.float64, np.float32):
            Ax, Bx = A.astype(adt), B.astype(bdt)
            ha, hb = _lib.coords_compose_bwd_host(Ax, Bx, g)
            hf = _lib.coords_invert_bwd_host(Ax, Bx, g)
            # dense operands, then tile views inside NaN-filled buffers: a read outside the view would poison the sums
            wa = torch.full((ahw[0] + 2, ahw[1] + 3, 2), nan, dtype=_dev(torch, Ax).dtype, device="cuda")
            wb = torch.full((hw[0] + 1, hw[1] + 5, 2), nan, dtype=_dev(torch, Bx).dtype, device="cuda")
            wa[1:ahw[0] + 1, 2:ahw[1] + 2], wb[1:, 3:hw[1] + 3] = _dev(torch, Ax), _dev(torch, Bx)
            for a, b in ((_dev(torch, Ax), _dev(torch, Bx)), (wa[1:ahw[0] + 1, 2:ahw[1] + 2], wb[1:, 3:hw[1] + 3])):
                ga, gb = ops.coords_compose_bwd(a, b, gd)
                assert R.same_bits(_np(gb), hb), (adt, bdt)
                adj_close(_np(ga), ha, "mix %s %s grad_outer" % (np.dtype(adt).name, np.dtype(bdt).name))
                adj_close(_np(ops.coords_invert_bwd(a, b, gd)), hf, "mix %s %s grad_f" % (np.dtype(adt).name, np.dtype(bdt).name))


def test_special_entries_equal_the_host_twin(torch):
    from lerf_pytorch_amd import _lib, ops
    A, B, g = special_compose()
    ha, hb = _lib.coords_compose_bwd_host(A, B, g)
    ga, gb = ops.coords_compose_bwd(_dev(torch, A), _dev(torch, B), _dev(torch, g))
    assert R.same_bits(_np(gb), hb) and not np.any(_np(gb)[0, :3])
    adj_close(_np(ga), ha, "special grad_outer")
    # the identity map with a NaN corner: a NaN inner gradient at the entries whose cell holds it, the host twin's bits
    An = np.random.default_rng(10).standard_normal((5, 6, 2))
    An[2, 3] = np.nan
    ii, jj = np.meshgrid(np.arange(5.0), np.arange(6.0), indexing="ij")
    ident, gi = np.stack([ii, jj], axis=-1), upstream((5, 6))
    ha, hb = _lib.coords_compose_bwd_host(An, ident, gi)
    ga, gb = ops.coords_compose_bwd(_dev(torch, An), _dev(torch, ident), _dev(torch, gi))
    assert R.same_bits(_np(gb), hb) and np.all(np.isnan(_np(gb)[2, 2])) and R.same_bits(_np(ga), gi)
    F, G, g = special_invert()
    hf = _lib.coords_invert_bwd_host(F, G, g)
    got = ops.coords_invert_bwd(_dev(torch, F), _dev(torch, G), _dev(torch, g))
    adj_close(_np(got), hf, "special grad_f")
    for e in range(4):
        assert not bool(ops.coords_invert_bwd(_dev(torch, F), _dev(torch, G[:, e:e + 1]), _dev(torch, g[:, e:e + 1])).any())


# ---------------------------------------------------------------------------------------------- 6. the contract
def test_accumulate_contract_and_null_halves(torch):
    """dyadic positions, integer upstream and pre-fill: every product and sum is exact whatever the order of the atomic adds"""
    from lerf_pytorch_amd import _lib, ops
    rng = np.random.default_rng(12)
    hw = (70, 130)
    A = rng.integers(-8, 9, (6, 7, 2)).astype(np.float64)
    B = np.stack([rng.integers(-4, 24, hw) / 4.0, rng.integers(-4, 28, hw) / 4.0], axis=-1)
    g = rng.integers(-5, 6, hw + (2,)).astype(np.float64)
    ha, hb = _lib.coords_compose_bwd_host(A, B, g)
    Ad, Bd, gd = _dev(torch, A), _dev(torch, B), _dev(torch, g)
    ga, gb = ops.coords_compose_bwd(Ad, Bd, gd)
    assert R.same_bits(_np(ga), ha) and R.same_bits(_np(gb), hb)
    pa, pb = rng.integers(-9, 10, A.shape).astype(np.float64), rng.integers(-9, 10, B.shape).astype(np.float64)
    qa, qb = _dev(torch, pa), _dev(torch, pb)
    ra, rb = ops.coords_compose_bwd(Ad, Bd, gd, grad_outer=qa, grad_inner=qb)
    assert ra.data_ptr() == qa.data_ptr() and rb.data_ptr() == qb.data_ptr()
    assert R.same_bits(_np(qa), pa + ha) and R.same_bits(_np(qb), pb + hb)
    qa, qb = _dev(torch, pa), _dev(torch, pb)
    only_a, none_b = ops.coords_compose_bwd(Ad, Bd, gd, grad_outer=qa, grad_inner=qb, need=(True, False))
    assert none_b is None and R.same_bits(_np(only_a), pa + ha) and R.same_bits(_np(qb), pb)
    qa, qb = _dev(torch, pa), _dev(torch, pb)
    none_a, only_b = ops.coords_compose_bwd(Ad, Bd, gd, grad_outer=qa, grad_inner=qb, need=(False, True))
    assert none_a is None and R.same_bits(_np(only_b), pb + hb) and R.same_bits(_np(qa), pa)
    ii, jj = np.meshgrid(np.arange(6.0), np.arange(7.0), indexing="ij")
    F = np.stack([2.0 * ii + 1.0, 2.0 * jj - 3.0], axis=-1)
    G = np.stack([rng.integers(0, 21, hw) / 4.0, rng.integers(0, 25, hw) / 4.0], axis=-1)
    hf = _lib.coords_invert_bwd_host(F, G, g)
    pf = rng.integers(-9, 10, F.shape).astype(np.float64)
    qf = _dev(torch, pf)
    assert ops.coords_invert_bwd(_dev(torch, F), _dev(torch, G), gd, grad_f=qf).data_ptr() == qf.data_ptr()
    assert R.same_bits(_np(qf), pf + hf) and np.any(hf != 0)


def test_ops_refusals_write_nothing(torch):
    from lerf_pytorch_amd import ops
    z = lambda *s, dt=torch.float64: torch.full(s, -7.0, dtype=dt, device="cuda")
    A, B, g = z(6, 7, 2), z(4, 5, 2), z(4, 5, 2)
    for call in (lambda: ops.coords_compose_bwd(z(1, 7, 2), B, g), lambda: ops.coords_compose_bwd(z(6, 1, 2), B, g),
                 lambda: ops.coords_compose_bwd(A, B, g, need=(False, False)), lambda: ops.coords_compose_bwd(A, B, g, grad_outer=A),
                 lambda: ops.coords_compose_bwd(A, B, g, grad_inner=B), lambda: ops.coords_compose_bwd(A, B, g, grad_inner=g),
                 lambda: ops.coords_compose_bwd(A, B, z(4, 5, 2, dt=torch.float32)), lambda: ops.coords_compose_bwd(A, B, z(4, 6, 2)),
                 lambda: ops.coords_compose_bwd(A, B, g, grad_outer=z(6, 7, 2, dt=torch.float32)), lambda: ops.coords_compose_bwd(A.cpu(), B, g),
                 lambda: ops.coords_compose_bwd(A[:, ::2], B, g),
                 lambda: ops.coords_invert_bwd(z(1, 7, 2), B, g), lambda: ops.coords_invert_bwd(A, B, g, grad_f=A),
                 lambda: ops.coords_invert_bwd(A, B, g, grad_f=z(6, 6, 2)), lambda: ops.coords_invert_bwd(A, B, z(4, 5, 2, dt=torch.float32)),
                 lambda: ops.coords_invert_bwd(A, B.cpu(), g)):
        with pytest.raises(ValueError):
            call()
    assert all(bool((t == -7.0).all()) for t in (A, B, g))


# ---------------------------------------------------------------------------------------------- 7. the differentiable twins
def test_twins_forward_is_the_plain_kernel_and_gradient_dtypes(torch):
    from lerf_pytorch_amd import coords
    ahw, hw = (12, 17), (37, 53)
    A, B = _dev(torch, outer_map(ahw)), _dev(torch, inner_map(ahw, hw))
    F = _dev(torch, invert_maps()["barrel"])
    la, lb, lf = A.clone().requires_grad_(True), B.clone().requires_grad_(True), F.clone().requires_grad_(True)
    with torch.no_grad():
        assert torch.equal(coords.compose_torch(la, lb), coords.compose(A, B))
        got, want = coords.invert_torch(lf, HW), coords.invert(F, HW)
        assert R.same_bits(_np(got), _np(want))
    assert torch.equal(coords.compose_torch(A, B, dtype=np.float32), coords.compose(A, B, dtype=np.float32))     # no leaf: plain
    assert not coords.compose_torch(A, B).requires_grad and not coords.invert_torch(F, HW).requires_grad
    out = coords.compose_torch(la, lb)
    assert out.requires_grad and torch.equal(out.detach(), coords.compose(A, B))
    inv = coords.invert_torch(lf, HW)
    assert inv.requires_grad and R.same_bits(_np(inv), _np(coords.invert(F, HW)))
    g = _dev(torch, upstream(hw))
    # a float32 operand's gradient is the float64 gradient rounded once: half a unit of 2^-23 of its magnitude on top of ADJ_TOL
    TOL_OF = {torch.float64: ADJ_TOL, torch.float32: ADJ_TOL + 2.0 ** -24}
    for adt in (torch.float64, torch.float32):
        for bdt in (torch.float64, torch.float32):
            la, lb = A.to(adt).clone().requires_grad_(True), B.to(bdt).clone().requires_grad_(True)
            out = coords.compose_torch(la, lb)
            assert out.dtype == bdt
            out.backward(g.to(bdt))
            assert la.grad.dtype == adt and lb.grad.dtype == bdt and tuple(la.grad.shape) == tuple(la.shape)
            ra, rb = compose_grads_ref(_np(la), _np(lb), _np(g.to(bdt).double()))
            for got, ref, dt_ in ((la.grad, ra, adt), (lb.grad, rb, bdt)):
                assert float(np.max(np.abs(_np(got) - ref))) <= TOL_OF[dt_] * max(float(np.max(np.abs(ref))), 1.0)
            # only one operand requires grad: the other half is skipped and the remaining one is unchanged
            oa, ob = A.to(adt).clone().requires_grad_(True), B.to(bdt).clone().requires_grad_(True)
            coords.compose_torch(oa, lb.detach()).backward(g.to(bdt))
            coords.compose_torch(la.detach(), ob).backward(g.to(bdt))
            assert torch.equal(ob.grad, lb.grad)
            assert float((oa.grad - la.grad).abs().max()) <= TOL_OF[adt] * max(float(la.grad.abs().max()), 1.0)
    for fdt in (torch.float64, torch.float32):
        lf = F.to(fdt).clone().requires_grad_(True)
        inv = coords.invert_torch(lf, HW, dtype=np.float64)
        w = torch.where(torch.isnan(inv.detach()), torch.zeros_like(inv), _dev(torch, upstream(HW, 6)))
        torch.nansum(inv * w).backward()
        assert lf.grad.dtype == fdt
        ref = invert_grad_ref(_np(lf), _np(inv), _np(w))
        assert float(np.max(np.abs(_np(lf.grad) - ref))) <= TOL_OF[fdt] * max(float(np.max(np.abs(ref))), 1.0)
    # init is a constant
    init = (coords.invert(F, HW).nan_to_num(11.0) + 0.25).requires_grad_(True)
    lf = F.clone().requires_grad_(True)
    torch.nansum(coords.invert_torch(lf, HW, init=init)).backward()
    assert init.grad is None and lf.grad is not None


def test_compose_torch_of_the_same_tensor_twice(torch):
    """scaling and squaring: phi <- phi o phi receives the sum of the outer and the inner gradient"""
    from lerf_pytorch_amd import coords, ops
    hw = (37, 53)
    ii, jj = np.meshgrid(np.arange(hw[0], dtype=np.float64), np.arange(hw[1], dtype=np.float64), indexing="ij")
    phi0 = np.stack([ii + 0.7 * np.sin(jj / 6.0) + 0.31, jj + 0.9 * np.cos(ii / 5.0) - 0.17], axis=-1)
    g = upstream(hw)
    phi = _dev(torch, phi0).requires_grad_(True)
    coords.compose_torch(phi, phi).backward(_dev(torch, g))
    ra, rb = compose_grads_ref(phi0, phi0, g)
    adj_close(_np(phi.grad), ra + rb, "compose_torch(phi, phi)")
    ga, gb = ops.coords_compose_bwd(phi.detach(), phi.detach(), _dev(torch, g))
    adj_close(_np(phi.grad), _np(ga + gb), "compose_torch(phi, phi) vs the two halves")


def test_batch_forms_equal_the_per_sample_calls(torch):
    from lerf_pytorch_amd import coords
    ahw, hw, Bn = (12, 17), (37, 53), 3
    As = np.stack([outer_map(ahw, s) for s in range(Bn)])
    Bs = np.stack([inner_map(ahw, hw, seed=20 + s) for s in range(Bn)])
    gs = np.stack([upstream(hw, 30 + s) for s in range(Bn)])
    for shared in (False, True):
        la = _dev(torch, As[0] if shared else As).requires_grad_(True)
        lb = _dev(torch, Bs).requires_grad_(True)
        out = coords.compose_torch(la, lb)
        assert tuple(out.shape) == (Bn,) + hw + (2,)
        out.backward(_dev(torch, gs))
        wa = np.zeros(As[0].shape) if shared else np.zeros(As.shape)
        for n in range(Bn):
            a1 = _dev(torch, As[0] if shared else As[n]).requires_grad_(True)
            b1 = _dev(torch, Bs[n]).requires_grad_(True)
            o1 = coords.compose_torch(a1, b1)
            assert torch.equal(o1.detach(), out[n].detach())
            o1.backward(_dev(torch, gs[n]))
            assert torch.equal(b1.grad, lb.grad[n])
            if shared:
                wa += _np(a1.grad)
            else:
                wa[n] = _np(a1.grad)
        adj_close(_np(la.grad), wa, "batch grad_outer, shared=%s" % shared)
    Fs = np.stack([invert_maps()[k] for k in ("barrel", "mesh", "flow")])
    lf = _dev(torch, Fs).requires_grad_(True)
    start = coords.invert(_dev(torch, Fs), HW).nan_to_num(11.0) + 0.25
    for init in (None, start):
        lf.grad = None
        inv = coords.invert_torch(lf, HW, init=init)
        assert tuple(inv.shape) == (Bn,) + HW + (2,)
        w = torch.where(torch.isnan(inv.detach()), torch.zeros_like(inv), _dev(torch, np.stack([upstream(HW, 40 + s) for s in range(Bn)])))
        torch.nansum(inv * w).backward()
        for n in range(Bn):
            f1 = _dev(torch, Fs[n]).requires_grad_(True)
            i1 = coords.invert_torch(f1, HW, init=None if init is None else init[n])
            assert R.same_bits(_np(i1), _np(inv[n]))
            torch.nansum(i1 * w[n]).backward()
            adj_close(_np(lf.grad[n]), _np(f1.grad), "batch grad_f %d" % n)


def test_invert_flow_torch(torch):
    from lerf_pytorch_amd import coords
    from test_coords_invert_cpu import F_HW, _flow
    flow = _flow()
    with torch.no_grad():
        assert R.same_bits(_np(coords.invert_flow_torch(_dev(torch, flow))), _np(coords.invert_flow(_dev(torch, flow))))
    lf = _dev(torch, flow).requires_grad_(True)
    b = coords.invert_flow_torch(lf)
    assert b.requires_grad and R.same_bits(_np(b), _np(coords.invert_flow(_dev(torch, flow))))
    ok = ~torch.isnan(b.detach())
    w = torch.where(ok, _dev(torch, upstream(F_HW, 6)), torch.zeros_like(b))
    torch.nansum(b * w).backward()
    ident = coords.from_flow(np.zeros(F_HW + (2,)))
    ref = invert_grad_ref(ident + flow, _np(b) + ident, _np(w))
    adj_close(_np(lf.grad), ref, "invert_flow_torch")
    assert lf.grad.dtype == torch.float64 and bool((lf.grad != 0).any())


def test_twin_refusals(torch):
    from lerf_pytorch_amd import coords
    A, B = _dev(torch, outer_map((6, 7))), _dev(torch, inner_map((6, 7), (4, 5)))
    bad = [lambda: coords.compose_torch(_np(A), B), lambda: coords.compose_torch(A, _np(B)), lambda: coords.compose_torch(A.cpu(), B),
           lambda: coords.compose_torch(A, B.cpu()), lambda: coords.compose_torch(A.long(), B), lambda: coords.compose_torch(A, B.int()),
           lambda: coords.compose_torch(A[..., 0], B), lambda: coords.compose_torch(A, B[None, None]),
           lambda: coords.compose_torch(torch.stack([A, A]), B), lambda: coords.compose_torch(torch.stack([A, A]), torch.stack([B, B, B])),
           lambda: coords.compose_torch(A.half(), B),
           lambda: coords.compose_torch(A[:1].clone().requires_grad_(True), B),                                 # 1 x 7: no cell
           lambda: coords.invert_torch(_np(A), (4, 5)), lambda: coords.invert_torch(A.cpu(), (4, 5)), lambda: coords.invert_torch(A.long(), (4, 5)),
           lambda: coords.invert_torch(A, (4, 5), init=_np(B)), lambda: coords.invert_torch(A, (4, 5), init=B.cpu()),
           lambda: coords.invert_torch(A, (4, 5), init=B[:3]), lambda: coords.invert_torch(A, (0, 5)), lambda: coords.invert_torch(A[0], (4, 5)),
           lambda: coords.invert_flow_torch(_np(B)), lambda: coords.invert_flow_torch(B.cpu()), lambda: coords.invert_flow_torch(B.long())]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="different devices"):
            coords.compose_torch(A, B.to("cuda:1"))
    # the plain entry points keep refusing, and name the twin
    with pytest.raises(ValueError, match="autograd.*compose_torch"):
        coords.compose(A.clone().requires_grad_(True), B)
    with pytest.raises(ValueError, match="autograd.*invert_torch"):
        coords.invert(A.clone().requires_grad_(True), (4, 5))


# ---------------------------------------------------------------------------------------------- 8. autograd end to end
IN_HW, OUT_HW, A_HW = (40, 48), (9, 11), (12, 14)
FLOW_SEED, MESH_SEED = 0, 0


def _away_from_integers(v, lo, hi):
    return bool(np.all((np.abs(v - np.round(v)) > 1e-3) & (v > lo + 1e-3) & (v < hi - 1e-3)))


def flow_case(seed=FLOW_SEED):
    """(outer [A_HW] into the frame, flow [OUT_HW], pads, ok): ok says that identity + flow stays > 1e-3 off every cell boundary of
    the outer map and the composed map > 1e-3 off every discontinuity of the remap -- decided by the restatements alone"""
    rng = np.random.default_rng(seed)
    a, b = np.meshgrid(np.linspace(2.2, IN_HW[0] - 3.3, A_HW[0]), np.linspace(1.7, IN_HW[1] - 2.9, A_HW[1]), indexing="ij")
    outer = np.stack([a, b], axis=-1) + rng.normal(0, 0.5, A_HW + (2,))
    flow = rng.normal(0, 0.4, OUT_HW + (2,)) + np.array([1.3, 1.4])
    ii, jj = np.meshgrid(np.arange(OUT_HW[0], dtype=np.float64), np.arange(OUT_HW[1], dtype=np.float64), indexing="ij")
    inner = np.stack([ii, jj], axis=-1) + flow
    cm = R.compose(outer, inner)
    pads = remap_grad_ref.pads_of(cm, IN_HW, 2)
    ok = _away_from_integers(inner[..., 0], 0, A_HW[0] - 1) and _away_from_integers(inner[..., 1], 0, A_HW[1] - 1) \
        and float(remap_grad_ref.margins("gauss", 2, cm, pads, IN_HW).min()) > 1e-3
    return outer, flow, pads, ok


def mesh_case(seed=MESH_SEED):
    """(ctrl [3, 4] of a map F [IN_HW] into the output frame, G = the restated Newton fixed point's start from the host inverse, pads,
    ok): ok says that every target is reached and G stays > 1e-3 off every cell boundary of F and every discontinuity of the remap"""
    from lerf_pytorch_amd import _lib
    rng = np.random.default_rng(seed)
    a, b = np.meshgrid(np.linspace(-1.6, OUT_HW[0] + 0.7, 3), np.linspace(-1.4, OUT_HW[1] + 0.6, 4), indexing="ij")
    ctrl = np.stack([a, b], axis=-1) + rng.normal(0, 0.3, (3, 4, 2))
    F = R.mesh(ctrl, IN_HW, "bilinear")
    G = _lib.coords_invert_host(np.ascontiguousarray(F), OUT_HW)
    if np.isnan(G).any():
        return ctrl, G, (0, 0), False
    pads = remap_grad_ref.pads_of(G, IN_HW, 2)
    ok = _away_from_integers(G[..., 0], 0, IN_HW[0] - 1) and _away_from_integers(G[..., 1], 0, IN_HW[1] - 1) \
        and float(remap_grad_ref.margins("gauss", 2, G, pads, IN_HW).min()) > 1e-3
    return ctrl, G, pads, ok


@pytest.mark.parametrize("dt", ["float64", "float32"])
def test_autograd_from_a_flow_through_compose_to_the_loss(torch, dt):
    from lerf_pytorch_amd import coords
    T = _classes()
    outer0, flow0, pads, ok = flow_case()
    assert ok
    x, hs = _operands(torch, "gauss", planes=2)
    tdt = getattr(torch, dt)
    flow, outer = _dev(torch, flow0).to(tdt).requires_grad_(True), _dev(torch, outer0).to(tdt).requires_grad_(True)
    cm = coords.compose_torch(outer, coords.from_flow_torch(flow))
    assert cm.requires_grad and cm.dtype == tdt and tuple(cm.shape) == OUT_HW + (2,)
    w = _make(T, "gauss", 2, "constant").enable_backward()
    w.set_shape([1, 2] + list(IN_HW), cm)
    loss = (w.warp(x[None], *[h[None] for h in hs]) ** 2).sum()
    loss.backward()
    assert flow.grad.dtype == tdt and outer.grad.dtype == tdt
    fr, orf = flow.detach().clone().requires_grad_(True), outer.detach().clone().requires_grad_(True)
    cr = GR.compose_ref(orf, coords.from_flow_torch(fr)).to(tdt)
    ref = (remap_grad_ref.restated_remap("gauss", 2, "constant", cr, pads, x, hs, 10.0) ** 2).sum()
    gf, go = torch.autograd.grad(ref, (fr, orf))
    print("loss %.9g (restatement %.9g), max |grad| flow %.3g, outer %.3g" % (float(loss.detach()), float(ref.detach()), float(gf.abs().max()),
                                                                              float(go.abs().max())))
    _close(_np(flow.grad), _np(gf))
    _close(_np(outer.grad), _np(go))
    assert bool((flow.grad != 0).any()) and bool((outer.grad != 0).any())


@pytest.mark.parametrize("dt", ["float64", "float32"])
def test_autograd_from_a_control_mesh_through_invert_to_the_loss(torch, dt):
    from lerf_pytorch_amd import coords
    T = _classes()
    c, _, pads, ok = mesh_case()
    assert ok
    x, hs = _operands(torch, "gauss", planes=2)
    tdt = getattr(torch, dt)
    ctrl = _dev(torch, c).to(tdt).requires_grad_(True)
    G = coords.invert_torch(coords.from_mesh_torch(ctrl, IN_HW), OUT_HW)
    assert G.requires_grad and G.dtype == tdt and tuple(G.shape) == OUT_HW + (2,) and not bool(torch.isnan(G).any())
    w = _make(T, "gauss", 2, "constant").enable_backward()
    w.set_shape([1, 2] + list(IN_HW), G)
    loss = (w.warp(x[None], *[h[None] for h in hs]) ** 2).sum()
    loss.backward()
    assert ctrl.grad.dtype == tdt and tuple(ctrl.grad.shape) == (3, 4, 2)
    cr = ctrl.detach().clone().requires_grad_(True)
    Gr = GR.invert_ift_ref(R.mesh_torch(cr, IN_HW, "bilinear").to(tdt), G.detach()).to(tdt)
    ref = (remap_grad_ref.restated_remap("gauss", 2, "constant", Gr, pads, x, hs, 10.0) ** 2).sum()
    gref, = torch.autograd.grad(ref, cr)
    print("loss %.9g (restatement %.9g), max |grad| %.3g" % (float(loss.detach()), float(ref.detach()), float(gref.abs().max())))
    _close(_np(ctrl.grad), _np(gref))
    assert bool((ctrl.grad != 0).any())


@pytest.mark.parametrize("name", ["barrel", "homography", "mesh", "flow"])
def test_cancellation_identity_through_autograd(torch, name):
    """d/dF nansum(compose_torch(F, invert_torch(F)) * W) = D + I vanishes by the bound the CPU suite settled"""
    from lerf_pytorch_amd import coords, ops
    F = _dev(torch, invert_maps()[name]).requires_grad_(True)
    W = _dev(torch, upstream(HW, 6))
    G = coords.invert_torch(F, HW)
    torch.nansum(coords.compose_torch(F, G) * W).backward()
    Wm = torch.where(torch.isnan(G.detach()), torch.zeros_like(W), W)
    D, _ = ops.coords_compose_bwd(F.detach(), G.detach(), Wm, need=(True, False))
    scale = max(float(D.abs().max()), 1.0)
    err = float(F.grad.abs().max())
    print("%s: max |D + I| = %.3g, max |D| = %.3g, relative %.3g, bound %.3g" % (name, err, scale, err / scale, ADJ_TOL * scale))
    assert bool((D != 0).any()) and err <= ADJ_TOL * scale
