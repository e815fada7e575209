"""The map inverse on the device (entry_kernel<InvertOp> of csrc/lerf_coords.hip behind ops.coords_invert and coords.invert):

  8. bit equality with the host twin on the maps of the residual contract: every dtype combination, with and without init, strided
     tile views inside sentinel-filled buffers, a 1 x 1 and a 1 x 53 output;
  9. the special entries (NaN in F, NaN / +-inf in init, a fold, a constant map, max_iter = 1): the host twin's bits.  Every
     operand is read inside its own bounds whatever it holds (tests/test_coords_invert_cpu.py builds them);
 10. coords.invert / invert_flow on device tensors equal their host forms; a batch of three maps equals three single calls;
 11. the engine: remap through compose(F, invert(F)) masks exactly the entries the inverse leaves NaN, and the composition is the
     identity within tol elsewhere.
"""
import numpy as np
import pytest

import coords_ref as R
from test_coords_invert_cpu import F_HW, HW, TOL, _flow, _targets, _valid, invert_maps, special_cases

pytestmark = pytest.mark.gpu

NAMES = ["barrel", "pincushion", "homography", "mesh", "flow"]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


@pytest.fixture(scope="module")
def maps():
    return invert_maps()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tdt(torch, dt):
    return torch.float32 if np.dtype(dt) == np.float32 else torch.float64


def _start(G):
    """a start a little off the solution, finite everywhere"""
    return np.where(np.isnan(G), 11.0, G) + 0.25


# ---------------------------------------------------------------------------------------------- 8. bit equality
@pytest.mark.parametrize("name", NAMES)
def test_invert_is_bit_equal_to_its_host_twin(torch, maps, name):
    from lerf_pytorch_amd import _lib, ops
    F = maps[name]
    start = _start(_lib.coords_invert_host(F, HW))
    for fdt in (np.float64, np.float32):
        Ff = F.astype(fdt)
        for idt in (None, np.float64, np.float32):
            init = None if idt is None else start.astype(idt)
            for odt in (np.float64, np.float32):
                host = _lib.coords_invert_host(Ff, HW, init=init, dtype=odt)
                got = ops.coords_invert(_dev(torch, Ff), HW, init=None if init is None else _dev(torch, init), dtype=_tdt(torch, odt))
                assert got.is_cuda and R.same_bits(got.cpu().numpy(), host), (fdt, idt, odt)
    assert ops.coords_invert(_dev(torch, F.astype(np.float32)), HW).dtype == torch.float32      # the default dtype is f's


@pytest.mark.parametrize("name", ["barrel", "mesh"])
def test_strided_tiles_and_small_outputs(torch, maps, name):
    from lerf_pytorch_amd import _lib, ops
    F = maps[name]
    whole = _lib.coords_invert_host(F, HW)
    start = _start(whole)
    whole_i = _lib.coords_invert_host(F, HW, init=start)
    wf = torch.full((F_HW[0], F_HW[1] + 3, 2), float("nan"), dtype=torch.float64, device="cuda")
    wi = torch.full((HW[0], HW[1] + 2, 2), float("nan"), dtype=torch.float64, device="cuda")
    wf[:, 2:F_HW[1] + 2], wi[:, 1:HW[1] + 1] = _dev(torch, F), _dev(torch, start)
    for dt in (np.float64, np.float32):
        for init, want in ((None, whole), (wi[5:16, 8:31], whole_i)):
            buf = torch.full((HW[0], HW[1] + 3, 2), -7.0, dtype=_tdt(torch, dt), device="cuda")
            ops.coords_invert(wf[:, 2:F_HW[1] + 2], (11, 23), init=init, out=buf[5:16, 7:30], origin=(5, 7))
            b = buf.cpu().numpy()
            assert R.same_bits(np.ascontiguousarray(b[5:16, 7:30]), want[5:16, 7:30].astype(dt))
            b[5:16, 7:30] = -7.0
            assert (b == -7.0).all()
    Fd = _dev(torch, F)
    for hw, origin in (((1, 1), (0, 0)), ((1, 1), (17, 29)), ((1, 53), (0, 0)), ((1, 53), (21, 2))):
        host = _lib.coords_invert_host(F, hw, origin=origin)
        assert R.same_bits(host, whole[origin[0]:origin[0] + hw[0], origin[1]:origin[1] + hw[1]])
        assert R.same_bits(ops.coords_invert(Fd, hw, origin=origin).cpu().numpy(), host)


# ---------------------------------------------------------------------------------------------- 9. special entries
def test_special_entries_equal_the_host_twin(torch):
    from lerf_pytorch_amd import _lib, ops
    for name, (F, init, max_iter) in special_cases().items():
        host = _lib.coords_invert_host(F, HW, init=init, max_iter=max_iter)
        got = ops.coords_invert(_dev(torch, F), HW, init=None if init is None else _dev(torch, init), max_iter=max_iter)
        assert R.same_bits(got.cpu().numpy(), host), name
    F, init, _ = special_cases()["init_nan_inf"]
    for idt in (np.float32,):                                         # +-inf and NaN survive the float32 round trip
        host = _lib.coords_invert_host(F, HW, init=init.astype(idt))
        assert R.same_bits(ops.coords_invert(_dev(torch, F), HW, init=_dev(torch, init.astype(idt))).cpu().numpy(), host)


# ---------------------------------------------------------------------------------------------- 10. coords.invert on device tensors
def test_coords_invert_on_device_tensors(torch, maps):
    from lerf_pytorch_amd import coords
    F = maps["barrel"]
    host = coords.invert(F, HW)
    got = coords.invert(_dev(torch, F), HW)
    assert got.is_cuda and got.dtype == torch.float64 and R.same_bits(got.cpu().numpy(), host)
    start = _start(host)
    got = coords.invert(_dev(torch, F), HW, init=_dev(torch, start), max_iter=12, tol=1e-8, dtype=np.float32)
    assert got.dtype == torch.float32 and R.same_bits(got.cpu().numpy(), coords.invert(F, HW, init=start, max_iter=12, tol=1e-8, dtype=np.float32))
    batch = np.stack([maps["barrel"], maps["mesh"], maps["flow"]])
    got = coords.invert(_dev(torch, batch), HW)
    assert tuple(got.shape) == (3,) + HW + (2,)
    for n in range(3):
        assert R.same_bits(got[n].cpu().numpy(), coords.invert(_dev(torch, batch[n]), HW).cpu().numpy())
        assert R.same_bits(got[n].cpu().numpy(), coords.invert(batch[n], HW))
    flow = _flow()
    b = coords.invert_flow(_dev(torch, flow))
    assert b.is_cuda and R.same_bits(b.cpu().numpy(), coords.invert_flow(flow))
    # refusals of the device forms
    dev, host_t = _dev(torch, F), torch.from_numpy(F)
    for a, i in ((dev, start), (F, _dev(torch, start)), (host_t, _dev(torch, start))):
        with pytest.raises(ValueError, match="mixed"):
            coords.invert(a, HW, init=i)
    leaf = dev.clone().requires_grad_(True)
    with pytest.raises(ValueError, match="autograd"):
        coords.invert(leaf, HW)
    with pytest.raises(ValueError, match="autograd"):
        coords.invert(dev, HW, init=_dev(torch, start).requires_grad_(True))
    with torch.no_grad():
        assert R.same_bits(coords.invert(leaf, HW).cpu().numpy(), host)


def test_ops_refusals_leave_out_untouched(torch):
    from lerf_pytorch_amd import ops
    f = torch.zeros((4, 5, 2), dtype=torch.float64, device="cuda")
    out = torch.full((6, 8, 2), -7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="lerf_coords_invert"):
        ops.coords_invert(f, (6, 8), out=out, max_iter=0)
    with pytest.raises(ValueError, match="lerf_coords_invert"):
        ops.coords_invert(f, (6, 8), out=out, tol=float("nan"))
    with pytest.raises(ValueError, match="lerf_coords_invert"):
        ops.coords_invert(f, (6, 8), out=out, origin=(0, -1))
    with pytest.raises(ValueError, match="lerf_coords_invert"):
        ops.coords_invert(f[:1], (6, 8), out=out)
    with pytest.raises(ValueError, match="lerf_coords_invert"):
        ops.coords_invert(out, (6, 8), out=out)                       # out IS f
    with pytest.raises(ValueError, match="lerf_coords_invert"):
        ops.coords_invert(f, (6, 8), init=out, out=out)               # out IS init
    with pytest.raises(ValueError, match="init must have out's shape"):
        ops.coords_invert(f, (6, 8), init=f, out=out)
    with pytest.raises(ValueError, match="column stride"):
        ops.coords_invert(out[:, ::2], (6, 8))
    assert bool((out == -7.0).all())


# ---------------------------------------------------------------------------------------------- 11. end to end
def test_engine_remap_through_a_map_composed_with_its_inverse(torch):
    import lerf_pytorch_amd as L
    from lerf_pytorch_amd import coords
    img = np.random.default_rng(0).integers(0, 256, HW + (3,), dtype=np.uint8)
    F = coords.radial(HW, F_HW, -0.18, 0.02, device="cuda")
    G = coords.invert(F, HW)
    nan = torch.isnan(G).any(dim=-1)
    assert 0.1 < float(nan.double().mean()) < 0.5                    # the barrel map leaves the frame's corners unreached
    C = coords.compose(F, G)
    q = _dev(torch, _targets(HW))
    err = float((C - q).abs()[~nan].max())
    print("max |compose(F, invert(F)) - identity| = %.3g (tol %.3g)" % (err, TOL))
    assert err <= TOL and bool(torch.isnan(C[nan]).all())
    # border=0: the white frame has no black rim, so the mask is false only where the remap reads no source at all
    out, mask = L.LerfEngine.shipped("lerf-g").remap(img, C, border=0)
    assert out.shape == HW + (3,) and mask.shape == HW + (3,)
    assert np.array_equal(~mask, np.broadcast_to(nan.cpu().numpy()[..., None], mask.shape))
    assert not out[nan.cpu().numpy()].any()                          # a NaN entry reads nothing: the uint8 output is 0 there
