"""Every instantiation of entry_kernel<OP> (csrc/lerf_coords.hip) launched once: each model, interpolation and dtype mix of BuildOp,
BuildDevOp, MeshOp, ComposeOp, InvertOp, ComposeBwdOp and InvertBwdOp is its own instantiation of one kernel template, and its host
twin runs the same functor in a plain loop.  Tiles of 5 x 67 (one full and one partial 4 x 64 block in both directions) and 1 x 1,
written through a strided view of row stride 2 * (oW + 3) at origin (3, 7) where the operation takes one:

  - maps and grad_inner are bit-equal to the host twin (the int64 / int32 patterns, so NaN entries count);
  - the padding columns of the strided view are untouched;
  - the two atomic scatters (grad_outer, grad_f) are within ADJ_TOL * max(max |host|, 1) of the host twin, the bound
    tests/test_gpu_coords_grad.py holds them to.

The arithmetic itself is judged by the CPU tests, which compare the host twins with the restatements of tests/coords*_ref.py.
"""
import itertools
import math

import numpy as np
import pytest

from test_coords_grad_cpu import ADJ_TOL

pytestmark = pytest.mark.gpu

HWS = [(5, 67), (1, 1)]
ORIGIN = (3, 7)
PAD = 3
SENTINEL = -7.0
DTS = [np.float32, np.float64]

_M = [1.02, 0.03, -2.5, -0.02, 0.98, 1.5, 1e-4, -2e-4, 1.0]
_K = [1.0 / 35, 0, -27.5 / 35, 0, 1.0 / 33, -16.0 / 33, 0.001, -0.0005, 1]
PARAMS = {
    "homography": _M,
    "radial": [30.0, 40.0, 45.0, 50.0, 35.5, 45.5, 0.08, -0.02],
    "brown": _K + [61.5, 58.75, 25.25, 17.5, 0.05, -0.012, 0.001, -0.002, 0.004, 0.01, -0.003, 0.0005],
    "fisheye": _K + [61.5, 58.75, 25.25, 17.5, 0.05, -0.012, 0.004, -0.0009],
    "equirect": [1.0 / 64, 0, -26.0 / 64, 0, 0, -1, 0, 1.0 / 64, -18.0 / 64, 192 / (2 * math.pi), 96 / math.pi, 95.5, 47.5],   # through a pole
}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _same(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(_bits(got), _bits(ref)), what


def _buffers(torch, hw, dt, sets=None):
    """a sentinel-filled host buffer and its device copy, [oH, oW + PAD, 2] (a leading [sets] when given)"""
    host = np.full(((hw[0], hw[1] + PAD, 2) if sets is None else (sets, hw[0], hw[1] + PAD, 2)), SENTINEL, dtype=dt)
    return host, torch.from_numpy(host.copy()).cuda()


def _check(dev_buf, host_buf, hw, what):
    got = dev_buf.cpu().numpy()
    assert dev_buf.stride(-3) == 2 * (hw[1] + PAD)
    _same(got[..., :hw[1], :], host_buf[..., :hw[1], :], what)
    assert np.all(got[..., hw[1]:, :] == SENTINEL) and np.all(host_buf[..., hw[1]:, :] == SENTINEL), what + ": padding written"


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _outer(dt):
    """A [4, 6, 2]: what compose samples"""
    ii, jj = np.meshgrid(np.arange(4.0), np.arange(6.0), indexing="ij")
    return np.stack([3.0 * ii + 0.5 * jj + 0.1 * ii * jj, 2.0 * jj - 0.25 * ii], axis=-1).astype(dt)


def _inner(hw, dt):
    """B [oH, oW, 2]: positions inside, on the border of and outside a 4 x 6 map, with inf and NaN entries"""
    k = np.arange(hw[0] * hw[1]).reshape(hw)
    ii, jj = np.meshgrid(np.arange(hw[0], dtype=np.float64), np.arange(hw[1], dtype=np.float64), indexing="ij")
    r = np.where(k % 11 == 3, np.nan, np.where(k % 13 == 5, -np.inf, np.where(k % 7 == 2, 3.0, 0.9 * ii - 0.5)))
    c = np.where(k % 17 == 4, np.inf, np.where(k % 5 == 1, 5.0, 0.11 * jj - 0.75))
    if k.size == 1:
        r, c = np.full(hw, 1.25), np.full(hw, 2.5)               # the 1 x 1 tile: inside a cell, so that both gradients are live
    return np.stack([r, c], axis=-1).astype(dt)


def _forward(hw, dt):
    """F [oH + 8, oW + 12, 2]: a sheared grid that covers the targets ORIGIN + (i, j) of the tile, one NaN corner"""
    ii, jj = np.meshgrid(np.arange(hw[0] + 8.0), np.arange(hw[1] + 12.0), indexing="ij")
    F = np.stack([0.9 * ii + 0.05 * jj - 1.0, 1.1 * jj + 0.1 * ii - 2.0], axis=-1)
    if hw[0] > 1:
        F[6, 30, 0] = np.nan
    return F.astype(dt)


def _upstream(hw):
    k = np.arange(hw[0] * hw[1] * 2, dtype=np.float64).reshape(hw + (2,))
    return np.sin(0.37 * k) + 0.25


def _adj_close(got, ref, what):
    scale = max(float(np.max(np.abs(ref))), 1.0)
    err = float(np.max(np.abs(got - ref)))
    print("%s: max error %.3g, scale %.3g, bound %.3g" % (what, err, scale, ADJ_TOL * scale))
    assert np.isfinite(err) and err <= ADJ_TOL * scale, what


@pytest.mark.parametrize("hw", HWS)
def test_build_every_model_and_dtype(torch, hw):
    from lerf_pytorch_amd import _lib, ops
    for model, dt in itertools.product(PARAMS, DTS):
        host, dev = _buffers(torch, hw, dt)
        _lib.coords_build_host(model, PARAMS[model], hw, out=host[:, :hw[1]], origin=ORIGIN)
        ops.coords_build(model, PARAMS[model], hw, out=dev[:, :hw[1]], origin=ORIGIN)
        _check(dev, host, hw, "build %s %s" % (model, np.dtype(dt)))


@pytest.mark.parametrize("hw", HWS)
def test_build_from_device_parameters_two_sets(torch, hw):
    from lerf_pytorch_amd import _lib, ops
    for model, dt in itertools.product(PARAMS, DTS):
        p = np.stack([np.asarray(PARAMS[model], np.float64)] * 2)
        p[1, 2] += 0.125                                       # a translation (radial: the outer half-diagonal): another map
        host, dev = _buffers(torch, hw, dt, sets=2)
        for s in range(2):
            _lib.coords_build_host(model, p[s], hw, out=host[s, :, :hw[1]], origin=ORIGIN)
        ops.coords_build_params(model, _dev(torch, p), hw, out=dev[:, :, :hw[1]], origin=ORIGIN)
        _check(dev, host, hw, "build_dev %s %s" % (model, np.dtype(dt)))
        assert not np.array_equal(_bits(host[0]), _bits(host[1]))


@pytest.mark.parametrize("hw", HWS)
def test_mesh_every_interp_and_dtype_mix(torch, hw):
    from lerf_pytorch_amd import _lib, ops
    aa, bb = np.meshgrid(np.arange(3.0), np.arange(4.0), indexing="ij")
    ctrl64 = np.stack([10.0 * aa + 0.25 * bb * bb, 7.0 * bb - 0.5 * aa * aa], axis=-1)
    full_hw = (hw[0] + 5, hw[1] + 8)                           # the tile sits inside a larger map
    for interp, tc, to in itertools.product(["bilinear", "bicubic"], DTS, DTS):
        ctrl = ctrl64.astype(tc)
        host, dev = _buffers(torch, hw, to)
        _lib.coords_mesh_host(ctrl, hw, interp, out=host[:, :hw[1]], origin=ORIGIN, full_hw=full_hw)
        ops.coords_mesh(_dev(torch, ctrl), hw, interp, out=dev[:, :hw[1]], origin=ORIGIN, full_hw=full_hw)
        _check(dev, host, hw, "mesh %s %s -> %s" % (interp, np.dtype(tc), np.dtype(to)))


@pytest.mark.parametrize("hw", HWS)
def test_compose_every_dtype_mix(torch, hw):
    from lerf_pytorch_amd import _lib, ops
    for ta, tb, to in itertools.product(DTS, DTS, DTS):
        A, B = _outer(ta), _inner(hw, tb)
        host, dev = _buffers(torch, hw, to)
        _lib.coords_compose_host(A, B, out=host[:, :hw[1]])
        ops.coords_compose(_dev(torch, A), _dev(torch, B), out=dev[:, :hw[1]])
        _check(dev, host, hw, "compose %s(%s) -> %s" % (np.dtype(ta), np.dtype(tb), np.dtype(to)))


@pytest.mark.parametrize("hw", HWS)
def test_invert_every_dtype_mix_with_and_without_init(torch, hw):
    from lerf_pytorch_amd import _lib, ops
    ii, jj = np.meshgrid(np.arange(hw[0], dtype=np.float64), np.arange(hw[1], dtype=np.float64), indexing="ij")
    init64 = np.stack([4.0 + ii, 8.0 + 0.9 * jj], axis=-1)
    if hw[0] > 1:
        init64[2, 5, 0], init64[3, 40, 1] = np.nan, 1e30
    for tf, ti, to in itertools.product(DTS, [None] + DTS, DTS):
        F = _forward(hw, tf)
        init = None if ti is None else init64.astype(ti)
        host, dev = _buffers(torch, hw, to)
        _lib.coords_invert_host(F, hw, init=init, out=host[:, :hw[1]], origin=ORIGIN)
        ops.coords_invert(_dev(torch, F), hw, init=None if init is None else _dev(torch, init), out=dev[:, :hw[1]], origin=ORIGIN)
        _check(dev, host, hw, "invert %s, init %s -> %s" % (np.dtype(tf), ti and np.dtype(ti), np.dtype(to)))
        assert np.isfinite(host[0, 0]).all()                   # the targets are reached: the loop ran to its tolerance


@pytest.mark.parametrize("hw", HWS)
def test_compose_backward_every_dtype_mix(torch, hw):
    from lerf_pytorch_amd import _lib, ops
    g = _upstream(hw)
    for ta, tb in itertools.product(DTS, DTS):
        A, B = _outer(ta), _inner(hw, tb)
        ha, hb = _lib.coords_compose_bwd_host(A, B, g)
        ga, gb = ops.coords_compose_bwd(_dev(torch, A), _dev(torch, B), _dev(torch, g))
        _same(gb.cpu().numpy(), hb, "compose_bwd %s(%s) grad_inner" % (np.dtype(ta), np.dtype(tb)))
        _adj_close(ga.cpu().numpy(), ha, "compose_bwd %s(%s) %s grad_outer" % (np.dtype(ta), np.dtype(tb), hw))
        assert np.any(ha != 0) and np.any(hb != 0)


@pytest.mark.parametrize("hw", HWS)
def test_invert_backward_every_dtype_mix(torch, hw):
    from lerf_pytorch_amd import _lib, ops
    g = _upstream(hw)
    for tf, tg in itertools.product(DTS, DTS):
        F = _forward(hw, tf)
        G = _lib.coords_invert_host(F, hw, origin=ORIGIN).astype(tg)
        hf = _lib.coords_invert_bwd_host(F, G, g)
        gf = ops.coords_invert_bwd(_dev(torch, F), _dev(torch, G), _dev(torch, g))
        _adj_close(gf.cpu().numpy(), hf, "invert_bwd %s, %s %s grad_f" % (np.dtype(tf), np.dtype(tg), hw))
        assert np.any(hf != 0)
