"""One coordinate map per sample (lerf_remap_batched / lerf_remap_packed_batched / lerf_remap_bwd_batched): a call with B
maps and P planes per map returns what B calls with one map each return.

The batch is B = 3 maps -- remap_ref.sinus_flow, remap_ref.folded and the seeded scatter of test_gpu_remap_grad.py -- in that
order and with the scatter first, P = 2 planes per map, frames (40, 48), maps (33, 37).  Their derived low pads differ inside
the batch (S = 2: (1,0), (1,0), (0,0); S = 4: (2,0), (2,1), (0,0); asserted in test_remap_batch_cpu.py), so a batched call
that takes its pads, or anything else, from map 0 fails here.

  1. forward, planar: bit-equal to the concatenation of the single-map calls (NaN positions included) for every kind, pad mode,
     map dtype and output dtype; a strided view of a wider buffer; special entries (NaN, +-inf, 1e300), entry [0, 0] = NaN in
     one sample only;
  2. packed stage outputs (the per-pixel RGB S = 2 kernel with the frame on the grid, and the general packed kernel) and
     LerfEngine.remap, byte for byte against the per-frame loop;
  3. backward: the per-plane map gradient bit-equal to the single-map calls and from run to run; image and hyper gradients
     against the float64 restatement per sample by the GRAD_RTOL rule (float atomics sum in arrival order: equality with the
     loop is not claimed); both accumulation paths;
  4. the torch twins with a 4-D leaf map, coords.from_flow_torch of a batched flow;  5. refusals on the device path.

No map value can form an address outside the operands (lerf_remap.hip: the clip comes before any conversion to int), so the
special entries are values like any other; nothing here provokes a fault."""
import ctypes as C

import numpy as np
import pytest

import remap_ref
from test_gpu_warp_grad import _close
from test_gpu_remap_grad import (IN_HW, OUT_HW, KIND_S, KIND_MAPS, WB_LDS, _block_windows, _classes, _make, _map_close, _max_sigma,
                                 _operands, _run_ref, _same_bits, _scatter, _upstream)

pytestmark = pytest.mark.gpu

B, P = 3, 2
PAD_MODES = ["constant", "replicate", "reflect", "circular"]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def _maps(scatter_first=False, in_hw=IN_HW, out_hw=OUT_HW):
    m = [remap_ref.sinus_flow(in_hw, out_hw), remap_ref.folded(in_hw, out_hw), _scatter(in_hw, out_hw)]
    return np.ascontiguousarray(np.stack(m[2:] + m[:2] if scatter_first else m))


def _special(cm):
    """the special entries of the existing tests inside a batch, a different set per sample; never entry [0, 0]"""
    cm = cm.copy()
    H, W = IN_HW
    cm[0, 5, 5, 0] = np.nan
    cm[0, 6, 7] = (np.inf, -np.inf)
    cm[1, 20, 21, 1] = np.nan
    cm[1, 7, 8] = (-1e300, 1e300)
    cm[1, 14, 15, 0] = float(H)
    cm[2, 8, 9] = (np.nan, np.nan)
    cm[2, 10, 11] = (-np.inf, W + 0.5)
    return cm


def _geo(ops, _lib, cm, S, pad="constant", in_hw=IN_HW):
    return ops.RemapGeometry(in_hw, cm, S, pad_mode=_lib.pad_mode_code(pad, _lib.TORCH_PAD_MODES))


def _planar_batched_vs_loop(torch, kind, pad, cm_t, x, hs, out):
    """one batched call against the B single-map calls; cm_t: device tensor [B, oH, oW, 2] (any strides the geometry takes)"""
    from lerf_pytorch_amd import _lib, ops
    S = KIND_S[kind]
    got = ops.remap_planar(x, hs, _geo(ops, _lib, cm_t, S, pad), kind, _max_sigma(kind), out=out)
    want = torch.cat([ops.remap_planar(x[b * P:(b + 1) * P], [h[b * P:(b + 1) * P] for h in hs], _geo(ops, _lib, cm_t[b], S, pad), kind,
                                       _max_sigma(kind), out=out) for b in range(B)])
    assert got.dtype == want.dtype and tuple(got.shape) == (B * P,) + OUT_HW
    assert _same_bits(torch, got, want), "%s %s %s: %d values differ" % (kind, pad, out, int((got != want).sum()))
    return got


# ---------------------------------------------------------------------------------------------- 1. forward, planar
@pytest.mark.parametrize("pad", PAD_MODES)
@pytest.mark.parametrize("kind", list(KIND_S))
def test_planar_forward_equals_the_single_map_calls(torch, kind, pad):
    x, hs = _operands(torch, kind, planes=B * P)
    for first in (False, True):
        cm = _special(_maps(first))
        for dt in (torch.float64, torch.float32):
            cm_t = torch.from_numpy(cm).cuda().to(dt)
            for out in ("f64", "f32"):
                got = _planar_batched_vs_loop(torch, kind, pad, cm_t, x, hs, out)
                nan_px = torch.from_numpy(np.isnan(cm).any(-1)).cuda().repeat_interleave(P, 0)
                assert bool(torch.isnan(got[nan_px]).all())             # a NaN entry of sample b: NaN in b's planes
    # the same maps from the host (uploaded once): the same bits
    from lerf_pytorch_amd import _lib, ops
    host = ops.remap_planar(x, hs, _geo(ops, _lib, cm, KIND_S[kind], pad), kind, _max_sigma(kind), out="f64")
    dev = ops.remap_planar(x, hs, _geo(ops, _lib, torch.from_numpy(cm).cuda(), KIND_S[kind], pad), kind, _max_sigma(kind), out="f64")
    assert _same_bits(torch, host, dev)


@pytest.mark.parametrize("kind", ["gauss", "cubic", "nearest"])
def test_a_batch_that_is_a_strided_view_of_a_wider_buffer(torch, kind):
    oH, oW = OUT_HW
    x, hs = _operands(torch, kind, planes=B * P)
    for dt in (torch.float64, torch.float32):
        wide = torch.full((B, oH + 2, oW + 5, 2), 1e300 if dt == torch.float64 else 1e30, dtype=dt, device="cuda")
        wide[:, :oH, :oW] = torch.from_numpy(_maps()).cuda().to(dt)
        view = wide[:, :oH, :oW]
        assert view.stride(1) > 2 * oW and view.stride(0) > oH * view.stride(1)
        got = _planar_batched_vs_loop(torch, kind, "constant", view, x, hs, "f64")
        dense = _planar_batched_vs_loop(torch, kind, "constant", view.contiguous(), x, hs, "f64")
        assert _same_bits(torch, got, dense)


@pytest.mark.parametrize("kind,pad", [("gauss", "constant"), ("linear", "reflect"), ("cubic", "constant"), ("lanczos3", "circular")])
def test_first_entry_nan_in_one_sample_only(torch, kind, pad):
    """entry [0, 0] carries a map's pads: NaN clips to 0, so THAT sample's pads become (ceil(S/2), ceil(S/2)) and the others keep theirs"""
    from lerf_pytorch_amd import ops
    S = KIND_S[kind]
    cm = _maps()
    cm[1, 0, 0] = np.nan
    pads = ops.RemapGeometry(IN_HW, cm, S).pads()
    assert tuple(pads[1]) == ((S + 1) // 2, (S + 1) // 2) and tuple(pads[0]) != tuple(pads[1]) != tuple(pads[2])
    x, hs = _operands(torch, kind, planes=B * P)
    for dt in (torch.float64, torch.float32):
        got = _planar_batched_vs_loop(torch, kind, pad, torch.from_numpy(cm).cuda().to(dt), x, hs, "f64")
        assert bool(torch.isnan(got[P:2 * P, 0, 0]).all())


# ---------------------------------------------------------------------------------------------- 2. packed stage outputs, engine
FRAME_HW = (24, 20)


@pytest.fixture(scope="module")
def engines(torch):
    import lerf_pytorch_amd as L
    return {"gauss": L.LerfEngine.shipped("lerf-g"), "linear": L.LerfEngine.shipped("lerf-l")}


@pytest.fixture(scope="module")
def packed3(torch, engines):
    """three 24 x 20 noise frames through stages_packed, once per (kind, channels), left unchanged"""
    from lerf_pytorch_amd import ops
    cache = {}

    def get(kind, Cn):
        if (kind, Cn) not in cache:
            imgs = np.random.default_rng(20 + Cn).integers(0, 256, (B,) + FRAME_HW + (Cn,), dtype=np.uint8)
            cache[(kind, Cn)] = (torch.from_numpy(imgs).cuda(), ops.stages_packed(torch.from_numpy(imgs).cuda(), engines[kind].luts))
        return cache[(kind, Cn)]
    return get


# (33, 37): one 256-pixel segment per row; (5, 300): a ragged second segment; (1030, 3): >= 1024 blocks per frame, the
# XCD-contiguous block order of warp_px_block
@pytest.mark.parametrize("out_hw", [(33, 37), (5, 300), (1030, 3)])
@pytest.mark.parametrize("kind", ["gauss", "linear"])
def test_packed_batched_equals_the_per_frame_loop(torch, engines, packed3, kind, out_hw):
    from lerf_pytorch_amd import ops
    for Cn, S in ((3, 2), (1, 2), (4, 2), (3, 4)):                         # RGB S = 2: the per-pixel kernel; else the general one
        _, packed = packed3(kind, Cn)
        for first in (False, True):
            cm = _maps(first, FRAME_HW, out_hw)
            cm[0, 1, 1, 0] = np.nan
            cm[2, 2, 0] = (np.inf, -1e300)
            for dt in (np.float64, np.float32):
                cm_t = torch.from_numpy(cm.astype(dt)).cuda()
                geo = ops.RemapGeometry(FRAME_HW, cm_t, S)
                for out in ("u8", "f32"):
                    for ms in ((10.0, 16.0) if out == "u8" and Cn == 3 else (10.0,)):     # production / general uint8 arithmetic
                        got = ops.remap_packed(packed, geo, kind, ms, out=out)
                        want = torch.stack([ops.remap_packed(packed[f], ops.RemapGeometry(FRAME_HW, cm_t[f], S), kind, ms, out=out)
                                            for f in range(B)])
                        assert got.dtype == want.dtype and tuple(got.shape) == (B,) + out_hw + (Cn,)
                        assert _same_bits(torch, got.float(), want.float()), (Cn, S, first, dt, out, ms, int((got != want).sum()))
                        assert bool((got[0, 1, 1] == 0).all()) if out == "u8" else bool(torch.isnan(got[0, 1, 1]).all())


@pytest.mark.parametrize("out", ["u8", "f32"])
@pytest.mark.parametrize("kind", ["gauss", "linear"])
def test_engine_remap_of_a_batch(torch, engines, packed3, kind, out):
    eng = engines[kind]
    frames, _ = packed3(kind, 3)
    cm = _maps(False, FRAME_HW, OUT_HW)
    cm[1, 3, 4] = np.nan
    cm_t = torch.from_numpy(cm).cuda()
    loop = [eng.remap(frames[f], cm_t[f], out=out) for f in range(B)]
    o, m = eng.remap(frames, cm_t, out=out)                                # one map per frame
    assert tuple(o.shape) == tuple(m.shape) == (B,) + OUT_HW + (3,) and m.dtype == torch.bool and o.dtype == loop[0][0].dtype
    for f in range(B):
        assert _same_bits(torch, o[f].float(), loop[f][0].float()) and torch.equal(m[f], loop[f][1]), f
    assert not torch.equal(m[0], m[2])                                     # the masks are per map
    o_np, m_np = eng.remap(frames.cpu().numpy(), cm, out=out)              # numpy in, numpy out
    assert np.array_equal(o_np, o.cpu().numpy(), equal_nan=True) and np.array_equal(m_np, m.cpu().numpy())
    # a shared 3-D map: the existing shared-map launch
    loop = [eng.remap(frames[f], cm_t[0], out=out) for f in range(B)]
    o, m = eng.remap(frames, cm_t[0], out=out)
    assert tuple(o.shape) == tuple(m.shape) == (B,) + OUT_HW + (3,)
    for f in range(B):
        assert _same_bits(torch, o[f].float(), loop[f][0].float()) and torch.equal(m[f], loop[f][1]), f
    assert eng.remap(frames, cm_t, return_mask=False)[1] is None
    with pytest.raises(ValueError):
        eng.remap(frames[:2], cm_t)                                        # 2 frames, 3 maps
    with pytest.raises(ValueError):
        eng.remap(frames[0], cm_t)                                         # one frame, a batch of maps


# ---------------------------------------------------------------------------------------------- 3. backward
def _bwd(torch, ops, geo, kind, x, hs, G):
    grads = [torch.zeros_like(x) for _ in range(1 + len(hs))]
    gc = torch.zeros((x.shape[0],) + geo.out_hw + (2,), dtype=torch.float64, device="cuda")
    ops.remap_bwd_planar(x, hs, geo, kind, _max_sigma(kind), G, grads, gc)
    return grads, gc


@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("kind", ["gauss", "linear", "cubic"])
def test_backward_equals_the_single_map_calls_and_the_restatement(torch, kind, first):
    from lerf_pytorch_amd import ops
    S = KIND_S[kind]
    x, hs = _operands(torch, kind, planes=B * P)
    G = _upstream(torch, B * P, OUT_HW)
    cm = _maps(first)
    cm[0, 5, 5, 0] = np.nan                                                # a masked pixel in one sample
    cm[1, 6, 7] = (np.inf, -1e300)                                         # the clip blocks the map gradient there
    for dt in (torch.float64, torch.float32):
        cm_t = torch.from_numpy(cm).cuda().to(dt)
        geo = ops.RemapGeometry(IN_HW, cm_t, S)
        grads, gc = _bwd(torch, ops, geo, kind, x, hs, G)
        grads2, gc2 = _bwd(torch, ops, geo, kind, x, hs, G)
        assert _same_bits(torch, gc, gc2) and bool((torch.nan_to_num(gc) != 0).any())                    # bit-equal from run to run
        nan_px = torch.from_numpy(np.isnan(cm).any(-1)).cuda()
        for b in range(B):
            sl = slice(b * P, (b + 1) * P)
            one = ops.RemapGeometry(IN_HW, cm_t[b], S)
            _, gcb = _bwd(torch, ops, one, kind, x[sl], [h[sl] for h in hs], G[sl])
            assert _same_bits(torch, gc[sl], gcb), "sample %d: the per-plane map gradient differs from the single-map call" % b
            Gr = G[sl].clone()
            Gr[:, nan_px[b]] = 0                                           # the restatement reads a NaN entry as 0
            ref, rgrads, rgc = _run_ref(torch, kind, S, "constant", cm_t[b], one.pads(), x[sl], [h[sl] for h in hs], Gr)
            for a, r in zip(grads, rgrads):
                _close(a[sl].cpu().numpy(), r.cpu().numpy())
            if dt == torch.float64:
                _map_close(gc[sl].sum(0).cpu().numpy(), rgc.cpu().numpy(), "%s sample %d" % (kind, b))
            else:                                                          # what _RemapFn hands a float32 map
                _close(gc[sl].sum(0).to(dt).cpu().numpy(), rgc.cpu().numpy())


def test_both_accumulation_paths_inside_one_batch(torch):
    """52 x 52 frames as in test_gpu_remap_grad.py: the scatter's block windows span the frame (2704 floats per map > the LDS
    window's 2048 for gauss: global atomics), the sinus map's fit (LDS window) -- in ONE launch"""
    from lerf_pytorch_amd import ops
    in_hw, kind, S = (52, 52), "gauss", 2
    cap = WB_LDS // KIND_MAPS[kind]
    cm = _maps(False, in_hw, OUT_HW)
    areas = [_block_windows(ops.RemapGeometry(in_hw, cm[b], S), S) for b in range(B)]
    assert max(areas[0]) <= cap and max(areas[2]) == 52 * 52 > cap
    x, hs = _operands(torch, kind, in_hw, planes=B * P)
    G = _upstream(torch, B * P, OUT_HW)
    cm_t = torch.from_numpy(cm).cuda()
    geo = ops.RemapGeometry(in_hw, cm_t, S)
    grads, gc = _bwd(torch, ops, geo, kind, x, hs, G)
    for b in range(B):
        sl = slice(b * P, (b + 1) * P)
        one = ops.RemapGeometry(in_hw, cm_t[b], S)
        _, gcb = _bwd(torch, ops, one, kind, x[sl], [h[sl] for h in hs], G[sl])
        assert _same_bits(torch, gc[sl], gcb)
        ref, rgrads, rgc = _run_ref(torch, kind, S, "constant", cm_t[b], one.pads(), x[sl], [h[sl] for h in hs], G[sl])
        for a, r in zip(grads, rgrads):
            _close(a[sl].cpu().numpy(), r.cpu().numpy())
        _map_close(gc[sl].sum(0).cpu().numpy(), rgc.cpu().numpy(), "52x52 sample %d" % b)


# ---------------------------------------------------------------------------------------------- 4. twins
def test_twin_with_a_4d_leaf_map(torch):
    T = _classes()
    kind, S = "gauss", 2
    x, hs = _operands(torch, kind, planes=B * P)
    x4, h4 = x.view((B, P) + IN_HW), [h.view((B, P) + IN_HW) for h in hs]
    G = _upstream(torch, B * P, OUT_HW).view((B, P) + OUT_HW)
    cm = _maps()
    for dt in (torch.float64, torch.float32):
        leaf = torch.from_numpy(cm).cuda().to(dt).requires_grad_(True)
        w = _make(T, kind, S, "constant").enable_backward()
        w.set_shape([B, P] + list(IN_HW), leaf)
        xl = x4.clone().requires_grad_(True)
        out = w.warp(xl, *h4)
        assert out.dtype == torch.float64 and out.requires_grad and tuple(out.shape) == (B, P) + OUT_HW
        out.backward(G)
        assert leaf.grad.dtype == dt and tuple(leaf.grad.shape) == (B,) + OUT_HW + (2,)
        assert tuple(xl.grad.shape) == tuple(xl.shape) and bool((xl.grad != 0).any())
        for b in range(B):
            lb = torch.from_numpy(cm[b]).cuda().to(dt).requires_grad_(True)
            wb = _make(T, kind, S, "constant").enable_backward()
            wb.set_shape([1, P] + list(IN_HW), lb)
            ob = wb.warp(x4[b:b + 1], *[h[b:b + 1] for h in h4])
            assert _same_bits(torch, ob, out[b:b + 1].detach())
            ob.backward(G[b:b + 1])
            assert lb.grad.dtype == dt and bool((lb.grad != 0).any())
            _map_close(leaf.grad[b].cpu().numpy(), lb.grad.cpu().numpy(), "twin %s sample %d" % (dt, b))
    with pytest.raises(ValueError, match="one map per sample"):
        w.set_shape([2, P] + list(IN_HW), leaf)
    w.set_shape([B, P] + list(IN_HW), leaf)
    with pytest.raises(ValueError, match="batch"):
        w.warp(x4[:2], *[h[:2] for h in h4])


def test_batched_flow_receives_its_gradient(torch):
    from lerf_pytorch_amd import coords
    T = _classes()
    x, _ = _operands(torch, "cubic", planes=B * P)
    gen = torch.Generator(device="cuda").manual_seed(3)
    flow = (torch.rand((B,) + OUT_HW + (2,), generator=gen, device="cuda", dtype=torch.float64) * 4 - 1).requires_grad_(True)
    cm = coords.from_flow_torch(flow)
    assert tuple(cm.shape) == (B,) + OUT_HW + (2,) and cm.requires_grad
    w = T.BicubicRemap2dTorch().enable_backward()
    w.set_shape([B, P] + list(IN_HW), cm)
    out = w.warp(x.view((B, P) + IN_HW))
    torch.nan_to_num(out, nan=0.0).sum().backward()
    assert tuple(flow.grad.shape) == tuple(flow.shape) and flow.grad.dtype == torch.float64
    assert all(bool((torch.nan_to_num(flow.grad[b]) != 0).any()) for b in range(B))


# ---------------------------------------------------------------------------------------------- 5. refusals on the device path
def test_refusals_on_the_device_path(torch):
    from lerf_pytorch_amd import _lib, ops
    cm_t = torch.from_numpy(_maps()).cuda()
    geo = ops.RemapGeometry(IN_HW, cm_t, 2)
    x, hs = _operands(torch, "gauss", planes=4)                            # 4 planes for 3 maps
    with pytest.raises(ValueError, match="planes for 3 maps"):
        ops.remap_planar(x, hs, geo, "gauss", 10.0, out="f64")
    with pytest.raises(ValueError, match="planes for 3 maps"):
        ops.remap_bwd_planar(x, hs, geo, "gauss", 10.0, _upstream(torch, 4, OUT_HW), [torch.zeros_like(x)])
    with pytest.raises(ValueError, match="frames for 3 maps"):
        ops.remap_packed(torch.zeros((2,) + IN_HW + (3,), dtype=torch.int32, device="cuda"), geo)
    with pytest.raises(ValueError, match="one per map"):
        ops.remap_hwc_u8(torch.zeros((2,) + IN_HW + (3,), dtype=torch.uint8, device="cuda"), None, ops.RemapGeometry(IN_HW, cm_t, 1), "nearest")
    # the C entry point itself, device operands: refused before anything is launched, nothing written
    out = torch.full((4,) + OUT_HW, 3.0, dtype=torch.float64, device="cuda")
    g, _keep = geo.struct(x.device)
    pf, po = ops._planes_chw(x), ops._planes_chw(out)
    ph, _k = ops._hyper_planes(hs, "planar", 3)
    call = lambda planes, n_maps, stride, ppm: _lib.lib().lerf_remap_batched(
        C.byref(pf), ph, IN_HW[0], IN_HW[1], planes, C.byref(g), n_maps, stride, ppm, _lib.KINDS["gauss"], 10.0, C.byref(po),
        _lib.current_stream())
    stride = geo.map_stride(x.device)
    assert call(4, 3, stride, 1) == -1 and call(4, 3, stride, 2) == -1 and call(4, 0, stride, 4) == -1
    assert call(4, 2, stride + 1, 2) == -1 and call(4, 2, stride - 2, 2) == -1
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    assert call(4, 2, stride, 2) == 0                                      # and a well-formed call runs: 2 maps, 2 planes each
    torch.cuda.synchronize()
    assert bool((out != 3.0).any())
    # a device-resident map serves its own device only
    with pytest.raises(ValueError, match="lives on"):
        geo.struct(torch.device("cuda", torch.cuda.current_device() + 1))
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="lives on"):
            ops.remap_planar(x[:3].to("cuda:1"), [h[:3].to("cuda:1") for h in hs], geo, "gauss", 10.0, out="f64")
    # strides a device batch may not have
    oH, oW = OUT_HW
    flat = torch.zeros(B * oH * oW * 2 + 8, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="batch stride"):
        ops.RemapGeometry(IN_HW, flat.as_strided((B, oH, oW, 2), (oH * oW * 2 + 1, oW * 2, 2, 1)), 2)       # odd
    with pytest.raises(ValueError, match="batch stride"):
        ops.RemapGeometry(IN_HW, flat.as_strided((B, oH, oW, 2), (oH * oW * 2 - 2, oW * 2, 2, 1)), 2)       # overlapping maps
