"""GPU tests of the remap (warp by a dense coordinate map): lerf_remap / lerf_remap_packed through ops, LerfEngine.remap and the
class twins.

  1. a homography's map reproduces the homographic warp bit for bit (every packed kernel, the direct kernel, the engine);
  2. arbitrary maps against the float64 oracle, whose geometry is replaced by its map-fed restatement (tests/remap_ref.py):
     uint8 bytes exactly, float32 within test_gpu_parity.F32_TOL, NaN at the same positions -- the standard of
     test_warp_packed_paths_vs_oracle;
  3. launch-shape edges of the per-pixel kernel; 4. explicit pads (tiles of a map); 5. non-finite coordinates (values only);
  6. the fixed kinds and the class twins.
"""
import numpy as np
import pytest

import remap_ref
from test_gpu_parity import F32_TOL

pytestmark = pytest.mark.gpu

IN_HW, OUT_HW = (52, 52), (60, 70)
CASES = [(3, 2, 10.0), (3, 2, 16.0), (1, 2, 10.0), (3, 4, 10.0)]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


@pytest.fixture(scope="module")
def engines(torch):
    import lerf_pytorch_amd as L
    return {"gauss": L.LerfEngine.shipped("lerf-g"), "linear": L.LerfEngine.shipped("lerf-l")}


@pytest.fixture(scope="module")
def stages(torch, engines):
    """packed stage outputs of seeded noise through the shipped LUTs, computed once per (kind, C, seed, frame size) and left
    unchanged: (images uint8 [2,H,W,C], packed int32 [2,H,W,C] on the device)"""
    from lerf_pytorch_amd import ops
    cache = {}

    def get(kind, C, seed, hw=IN_HW):
        key = (kind, C, seed, hw)
        if key not in cache:
            imgs = np.random.default_rng(seed).integers(0, 256, (2,) + tuple(hw) + (C,), dtype=np.uint8)
            cache[key] = (imgs, ops.stages_packed(torch.from_numpy(imgs).cuda(), engines[kind].luts))
        return cache[key]
    return get


def _same(torch, a, b):
    """torch.equal with NaN == NaN"""
    if a.is_floating_point():
        assert torch.equal(torch.isnan(a), torch.isnan(b))
        a, b = torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0)
    assert torch.equal(a, b), "%d of %d values differ" % (int((a != b).sum()), a.numel())


def _vs_oracle(oracle, got, ref, out):
    """the standard of tests/test_gpu_parity.py:485-492"""
    if out == "u8":
        want = oracle.to_u8(np.nan_to_num(ref, nan=0.0))
        assert np.array_equal(got, want), "%d of %d bytes differ" % ((got != want).sum(), want.size)
    else:
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        ok = ~np.isnan(ref)
        err = np.max(np.abs(got[ok] - ref[ok]))
        print("float32 error %.3g (bound %.3g)" % (err, F32_TOL))
        assert err <= F32_TOL, err


@pytest.fixture
def map_oracle(oracle, monkeypatch):
    """the float64 oracle with its geometry read from a map: warp_u8 / warp_params_f32 take the map as `matrix`"""
    monkeypatch.setattr(oracle, "warp_geometry", remap_ref.map_geometry)
    return oracle


# ------------------------------------------------------------------------------------------------ 1. homography equivalence
@pytest.mark.parametrize("out", ["u8", "f32"])
@pytest.mark.parametrize("C,S,max_sigma", CASES)
@pytest.mark.parametrize("kind", ["gauss", "linear"])
def test_remap_of_a_homography_map_equals_the_warp(torch, golden, engines, stages, kind, C, S, max_sigma, out):
    from lerf_pytorch_amd import coords, ops
    M = golden("g4_warp.npz")["isc/matrix"]
    _, packed = stages(kind, C, 100 * C + S + int(max_sigma))
    luts = engines[kind].luts
    wgeo = ops.WarpGeometry(IN_HW, M, OUT_HW, S)
    rgeo = ops.RemapGeometry(IN_HW, coords.from_homography(M, OUT_HW), S)
    assert rgeo.pads() == (wgeo.struct.pad_r_lo, wgeo.struct.pad_c_lo)
    _same(torch, ops.remap_packed(packed, rgeo, kind, max_sigma, out=out), ops.warp_packed(packed, wgeo, kind, max_sigma, out=out))
    feat, hq = ops.unpack_stages(packed[1], luts.oC)
    _same(torch, ops.remap_hwc_u8(feat, hq, rgeo, kind, max_sigma, out=out), ops.warp_hwc_u8(feat, hq, wgeo, kind, max_sigma, out=out))


@pytest.mark.parametrize("out", ["u8", "f32"])
@pytest.mark.parametrize("kind", ["gauss", "linear"])
def test_engine_remap_equals_engine_warp(torch, golden, engines, kind, out):
    from lerf_pytorch_amd import coords
    M = golden("g4_warp.npz")["isc/matrix"]
    img = torch.from_numpy(np.random.default_rng(5).integers(0, 256, IN_HW + (3,), dtype=np.uint8)).cuda()
    eng = engines[kind]
    a, ma = eng.remap(img, coords.from_homography(M, OUT_HW), out=out)
    b, mb = eng.warp(img, M, OUT_HW, out=out)
    _same(torch, a, b)
    assert ma.dtype == torch.bool and torch.equal(ma, mb) and bool(ma.any()) and not bool(ma.all())
    # numpy in -> numpy out, no mask; the module-level entry point
    import lerf_pytorch_amd as L
    if kind == "gauss" and out == "u8":
        o, m = L.remap(img.cpu().numpy(), coords.from_homography(M, OUT_HW))
        assert isinstance(o, np.ndarray) and np.array_equal(o, a.cpu().numpy()) and np.array_equal(m, ma.cpu().numpy())
        assert eng.remap(img, coords.from_homography(M, OUT_HW), return_mask=False)[1] is None


# ------------------------------------------------------------------------------------------------ 2. arbitrary maps vs the oracle
def _map(name, in_hw=IN_HW, out_hw=OUT_HW):
    from lerf_pytorch_amd import coords
    if name == "radial":
        return coords.radial(in_hw, out_hw, 0.35, 0.1)          # the corners leave the frame: clipped
    if name == "sinus":
        return remap_ref.sinus_flow(in_hw, out_hw)
    return remap_ref.folded(in_hw, out_hw)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["gauss", "linear"])
@pytest.mark.parametrize("name", ["radial", "sinus", "folded"])
def test_arbitrary_maps_vs_oracle(torch, map_oracle, engines, stages, name, kind, dtype):
    from lerf_pytorch_amd import ops
    cm = _map(name).astype(dtype)
    cm64 = cm.astype(np.float64)                                 # what the oracle is fed: the float32 values, promoted
    luts = engines[kind].luts
    if name == "sinus":
        assert map_oracle.warp_geometry(cm64, IN_HW, OUT_HW, 2)["pad"][0] > 0      # non-zero low pads
    for C, S, max_sigma in ((3, 2, 10.0), (1, 4, 10.0)):         # the per-pixel kernel (PROD / exact) and the per-channel one
        _, packed = stages(kind, C, 7 + C)
        geo = ops.RemapGeometry(IN_HW, cm, S)
        feat, hq = (t.cpu().numpy() for t in ops.unpack_stages(packed[0], luts.oC))
        ref = map_oracle.warp_u8(feat, hq, cm64, OUT_HW, S, max_sigma, kind)
        for out in ("u8", "f32"):
            _vs_oracle(map_oracle, ops.remap_packed(packed[0], geo, kind, max_sigma, out=out).cpu().numpy(), ref, out)
        # the direct kernel on the unpacked planes (float64 arithmetic for float outputs)
        f, h = ops.unpack_stages(packed[0], luts.oC)
        _vs_oracle(map_oracle, ops.remap_hwc_u8(f, h, geo, kind, max_sigma, out="u8").cpu().numpy(), ref, "u8")
        got64 = ops.remap_hwc_u8(f, h, geo, kind, max_sigma, out="f64").cpu().numpy()
        assert np.array_equal(np.isnan(got64), np.isnan(ref))
        assert np.max(np.abs(got64[~np.isnan(ref)] - ref[~np.isnan(ref)])) <= 1e-9        # test_gpu_parity's float64 bound


# ------------------------------------------------------------------------------------------------ 3. launch-shape edges
@pytest.mark.parametrize("in_hw,out_hw", [((52, 52), (9, 300)),       # a ragged second 256-pixel segment
                                          ((52, 52), (1100, 8)),      # >= 1024 blocks: the XCD-contiguous block order
                                          ((70, 130), (60, 70))])     # the source crosses the 64-pixel tiles of stages_packed
def test_per_pixel_kernel_launch_shapes(torch, map_oracle, engines, stages, in_hw, out_hw):
    from lerf_pytorch_amd import ops
    luts = engines["gauss"].luts
    _, packed = stages("gauss", 3, 11, in_hw)
    cm = remap_ref.sinus_flow(in_hw, out_hw)
    geo = ops.RemapGeometry(in_hw, cm, 2)
    both = ops.remap_packed(packed, geo, "gauss", 10.0, out="u8")
    feat, hq = (t.cpu().numpy() for t in ops.unpack_stages(packed[0], luts.oC))
    _vs_oracle(map_oracle, both[0].cpu().numpy(), map_oracle.warp_u8(feat, hq, cm, out_hw, 2, 10.0, "gauss"), "u8")
    # two frames sharing one map, against each frame alone
    for n in range(2):
        assert torch.equal(both[n], ops.remap_packed(packed[n], geo, "gauss", 10.0, out="u8"))
    # a device-resident map with a row stride larger than 2 * oW (float64 and float32): the same bytes
    for dt in (torch.float64, torch.float32):
        wide = torch.full((out_hw[0], out_hw[1] + 5, 2), float("nan"), dtype=dt, device="cuda")
        wide[:, :out_hw[1]] = torch.from_numpy(cm).cuda().to(dt)
        view = wide[:, :out_hw[1]]
        assert view.stride(0) > 2 * out_hw[1]
        dense = ops.RemapGeometry(in_hw, view.contiguous(), 2)
        for out in ("u8", "f32"):
            _same(torch, ops.remap_packed(packed, ops.RemapGeometry(in_hw, view, 2), "gauss", 10.0, out=out),
                  ops.remap_packed(packed, dense, "gauss", 10.0, out=out))
        if dt == torch.float64:
            assert torch.equal(ops.remap_packed(packed, dense, "gauss", 10.0, out="u8"), both)


# ------------------------------------------------------------------------------------------------ 4. explicit pads
@pytest.mark.parametrize("kind", ["gauss", "linear"])
def test_rows_of_a_map_with_the_whole_maps_pads(torch, engines, stages, kind):
    from lerf_pytorch_amd import ops
    luts = engines[kind].luts
    _, packed = stages(kind, 3, 10)
    cm = remap_ref.sinus_flow(IN_HW, OUT_HW)
    whole = ops.RemapGeometry(IN_HW, cm, 2)
    assert whole.pads()[0] > 0
    i0, i1 = 13, 41
    feat, hq = ops.unpack_stages(packed[0], luts.oC)
    for part in (ops.RemapGeometry(IN_HW, cm[i0:i1], 2, pads=whole.pads()), whole.rows(i0, i1),
                 ops.RemapGeometry(IN_HW, torch.from_numpy(cm).cuda()[i0:i1], 2, pads=whole.pads())):
        assert part.out_hw == (i1 - i0, OUT_HW[1]) and part.pads() == whole.pads()
        for out in ("u8", "f32"):
            _same(torch, ops.remap_packed(packed, part, kind, 10.0, out=out), ops.remap_packed(packed, whole, kind, 10.0, out=out)[:, i0:i1])
            _same(torch, ops.remap_hwc_u8(feat, hq, part, kind, 10.0, out=out), ops.remap_hwc_u8(feat, hq, whole, kind, 10.0, out=out)[i0:i1])


# ------------------------------------------------------------------------------------------------ 5. non-finite coordinates
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_non_finite_coordinates(torch, engines, stages, dtype):
    """values only: NaN entries give 0 / NaN, everything else is untouched by them (the kernel's address guard is by
    construction: clip before any conversion to int, lerf_host_geometry.h clip_coord)"""
    from lerf_pytorch_amd import ops
    rng = np.random.default_rng(3)
    clean = remap_ref.sinus_flow(IN_HW, OUT_HW).astype(dtype)
    idx = rng.permutation(OUT_HW[0] * OUT_HW[1] - 1)[:90] + 1              # never entry (0, 0): it carries the pads
    ii, jj = np.unravel_index(idx, OUT_HW)
    clean[ii[60:70], jj[60:70], 0] = np.inf
    clean[ii[70:80], jj[70:80], 1] = -np.inf
    clean[ii[80:90], jj[80:90]] = (-np.inf, np.inf)
    dirty = clean.copy()
    dirty[ii[:20], jj[:20], 0] = np.nan                                    # row, column, both
    dirty[ii[20:40], jj[20:40], 1] = np.nan
    dirty[ii[40:60], jj[40:60]] = np.nan
    clean[ii[:60], jj[:60]] = 5.0                                          # any finite value
    nan = torch.from_numpy(np.isnan(dirty).any(-1)).cuda()
    assert int(nan.sum()) == 60

    def check(a, b, pix):                                                  # a: dirty map, b: clean map; pix: [.., oH, oW, ..] -> mask
        m = pix(nan)
        if a.is_floating_point():
            assert bool(torch.isnan(a[m.expand_as(a)]).all())
        else:
            assert int(a[m.expand_as(a)].max()) == 0
        _same(torch, torch.where(m.expand_as(a), torch.zeros_like(a), a), torch.where(m.expand_as(b), torch.zeros_like(b), b))

    for kind in ("gauss", "linear"):
        luts = engines[kind].luts
        for C, S in ((3, 2), (1, 4)):
            _, packed = stages(kind, C, 7 + C)
            gd, gc = ops.RemapGeometry(IN_HW, dirty, S), ops.RemapGeometry(IN_HW, clean, S)
            for out in ("u8", "f32"):
                check(ops.remap_packed(packed, gd, kind, 10.0, out=out), ops.remap_packed(packed, gc, kind, 10.0, out=out),
                      lambda m: m[None, :, :, None])
            feat, hq = ops.unpack_stages(packed[0], luts.oC)
            for out in ("u8", "f32", "f64"):
                check(ops.remap_hwc_u8(feat, hq, gd, kind, 10.0, out=out), ops.remap_hwc_u8(feat, hq, gc, kind, 10.0, out=out),
                      lambda m: m[:, :, None])
    planes = torch.rand((2,) + IN_HW, device="cuda") * 255
    for k in ("nearest", "cubic", "lanczos3"):
        S = {"nearest": 1, "cubic": 4, "lanczos3": 6}[k]
        check(ops.remap_planar(planes, [], ops.RemapGeometry(IN_HW, dirty, S), k, 1.0, out="f64"),
              ops.remap_planar(planes, [], ops.RemapGeometry(IN_HW, clean, S), k, 1.0, out="f64"), lambda m: m[None])


# ------------------------------------------------------------------------------------------------ 6. fixed kinds, class twins
def test_fixed_kind_twins_equal_the_warp_classes(torch, golden):
    from lerf_pytorch_amd import coords
    from lerf_pytorch_amd.resize_right import resize_right2d_numpy as RN, resize_right2d_torch as RT
    M = golden("g4_warp.npz")["isc/matrix"]
    cm = coords.from_homography(M, OUT_HW)
    x = np.random.default_rng(1).random((3,) + IN_HW).astype(np.float32) * 255
    xt = torch.from_numpy(x).cuda()[None]
    for name in ("Nearest", "Bicubic"):
        for pad_mode in ("constant", "reflect"):
            w = getattr(RN, name + "Warp2dNumpy")(pad_mode=pad_mode)
            w.set_shape([3] + list(IN_HW), M, [3] + list(OUT_HW))
            r = getattr(RN, name + "Remap2dNumpy")(pad_mode=pad_mode)
            r.set_shape([3] + list(IN_HW), cm)
            assert r.out_shape == [3] + list(OUT_HW) and r.support_sz == w.support_sz
            a, b = np.asarray(r.warp(x)), np.asarray(w.warp(x))       # (a lazy.DeviceArray when lazy results are on)
            assert a.dtype == np.float64 and a.shape == (3,) + OUT_HW and np.array_equal(a, b, equal_nan=True)
            wt = getattr(RT, name + "Warp2dTorch")(pad_mode=pad_mode)
            wt.set_shape([1, 3] + list(IN_HW), M, [1, 3] + list(OUT_HW))
            rt = getattr(RT, name + "Remap2dTorch")(pad_mode=pad_mode)
            rt.set_shape([1, 3] + list(IN_HW), torch.from_numpy(cm).cuda())
            at, bt = rt.warp(xt), wt.warp(xt)
            assert at.dtype == torch.float64 and tuple(at.shape) == (1, 3) + OUT_HW
            _same(torch, at, bt)
            assert np.array_equal(at[0].cpu().numpy(), a, equal_nan=True)


def test_learned_twins_equal_the_warp_classes_and_are_forward_only(torch, golden):
    from lerf_pytorch_amd import coords
    from lerf_pytorch_amd.resize_right import resize_right2d_numpy as RN, resize_right2d_torch as RT
    M = golden("g4_warp.npz")["isc/matrix"]
    cm = coords.from_homography(M, OUT_HW)
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.rand((1, 3) + IN_HW, device="cuda", generator=g) * 255
    h = [torch.rand((1, 3) + IN_HW, device="cuda", generator=g) for _ in range(3)]
    w = RT.SteeringGaussianWarp2dTorch(support_sz=4, max_sigma=10)
    w.set_shape([1, 3] + list(IN_HW), M, [1, 3] + list(OUT_HW))
    r = RT.SteeringGaussianRemap2dTorch(support_sz=4, max_sigma=10)
    r.set_shape([1, 3] + list(IN_HW), cm)
    _same(torch, r.warp(x, *h), w.warp(x, *h))
    wl = RT.AmplifiedLinearWarp2dTorch()
    wl.set_shape([1, 3] + list(IN_HW), M, [1, 3] + list(OUT_HW))
    rl = RT.AmplifiedLinearRemap2dTorch()
    rl.set_shape([1, 3] + list(IN_HW), cm)
    _same(torch, rl.warp(x, h[0]), wl.warp(x, h[0]))
    # the numpy twins
    xn, hn = x[0].cpu().numpy(), [t[0].cpu().numpy() for t in h]
    wn = RN.SteeringGaussianWarp2dNumpy(support_sz=2)
    wn.set_shape([3] + list(IN_HW), M, [3] + list(OUT_HW))
    rn = RN.SteeringGaussianRemap2dNumpy(support_sz=2)
    rn.set_shape([3] + list(IN_HW), cm)
    assert np.array_equal(np.asarray(rn.warp(xn, *hn)), np.asarray(wn.warp(xn, *hn)), equal_nan=True)
    wa = RN.AmplifiedLinearWarp2dNumpy()
    wa.set_shape([3] + list(IN_HW), M, [3] + list(OUT_HW))
    ra = RN.AmplifiedLinearRemap2dNumpy()
    ra.set_shape([3] + list(IN_HW), cm)
    assert np.array_equal(np.asarray(ra.warp(xn, hn[0])), np.asarray(wa.warp(xn, hn[0])), equal_nan=True)
    # forward only: an input that requires grad is an error, not a detached result
    xg = x.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="forward-only"):
        r.warp(xg, *h)
    hg = h[0].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="forward-only"):
        rl.warp(x, hg)
    with torch.no_grad():
        _same(torch, r.warp(xg, *h), w.warp(x, *h))


def test_remap_rejects_what_it_cannot_run(torch, engines, stages):
    from lerf_pytorch_amd import ops
    _, packed = stages("gauss", 3, 10)
    cm = remap_ref.sinus_flow(IN_HW, OUT_HW)
    with pytest.raises(ValueError):
        ops.remap_packed(packed, ops.RemapGeometry((40, 52), cm, 2))                      # another frame size
    with pytest.raises(ValueError):
        ops.RemapGeometry(IN_HW, torch.from_numpy(cm).cuda()[:, ::2], 2)                  # column stride 4
    with pytest.raises(ValueError):
        ops.RemapGeometry(IN_HW, torch.from_numpy(cm).cuda().half(), 2)
    with pytest.raises(Exception):
        ops.remap_packed(packed, ops.RemapGeometry(IN_HW, cm, 2, pad_mode=2))             # packed maps: constant padding only
