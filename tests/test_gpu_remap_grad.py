"""Autograd through the remap: lerf_remap_bwd (csrc/lerf_remap_bwd.hip) behind ops.remap_bwd_planar and the *Remap2dTorch
classes after enable_backward() (`_RemapFn`).

  1. every g24 case (the reference's own torch warp gradients) through the remap twin on the map of its homography: forward
     to 1e-9, gradients by the GRAD_RTOL rule of test_gpu_warp_grad.py, the same NaNs;
  2. image, hyper-parameter and MAP gradients against the float64 autograd restatement (tests/remap_grad_ref.py, anchored by
     tests/test_remap_grad_cpu.py): every kind, the four pad modes, a smooth, a folded and a scattered map, float64 and float32
     maps.  The float64 map gradient is one thread's float64 sum per element: bound MAP_TOL * max(max|ref|, 1);
  3. both accumulation paths (LDS window / global atomics), decided per block from the host geometry in the test;
  4. NaN, +-inf, out-of-range and border entries; 5. determinism of the map gradient; 6. the C contract (NULL subsets,
     accumulation, refusals, a row tile); 7. the opt-in switch; 8. a flow fitted by SGD against the same loop on the restatement.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import remap_ref
import remap_grad_ref
from test_gpu_warp_grad import _close, _g24_leaves, _g24_out

pytestmark = pytest.mark.gpu

IN_HW, OUT_HW = (40, 48), (33, 37)
MAP_TOL = 1e-9            # the forward's own float64 bound, scaled like the other gradients
WB_LDS, WB = 8192, 16     # csrc/lerf_warp_bwd_kernels.h: floats of LDS window per block, block edge
KIND_S = {"gauss": 2, "linear": 2, "nearest": 1, "cubic": 4, "bilinear": 2, "lanczos2": 4, "lanczos3": 6}
KIND_MAPS = {"gauss": 4, "linear": 2}
TWIN = {"gauss": "SteeringGaussian", "linear": "AmplifiedLinear", "nearest": "Nearest", "cubic": "Bicubic", "bilinear": "Bilinear",
        "lanczos2": "Lanczos2", "lanczos3": "Lanczos3"}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def _classes():
    from lerf_pytorch_amd.resize_right import resize_right2d_torch as T
    return T


def _make(T, kind, S, pad_mode, dev="cuda"):
    """the remap twin of `kind`; S = None: the class's default support (what the warp twins of the g24 cases were built with)"""
    cls = getattr(T, TWIN[kind] + "Remap2dTorch")
    kw = {} if S is None else {"support_sz": S}
    if kind == "gauss":
        kw["max_sigma"] = 10
    return cls(device=dev, pad_mode=pad_mode, **kw)


def _max_sigma(kind):
    return 10.0 if kind == "gauss" else 1.0


def _scatter(in_hw, out_hw, seed=9):
    """seeded uniform scatter over [-3, H + 3] x [-3, W + 3]: entries outside the clip, every block's window the whole frame"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-3, in_hw[0] + 3, out_hw), rng.uniform(-3, in_hw[1] + 3, out_hw)], axis=-1)


def _map(name, in_hw=IN_HW, out_hw=OUT_HW):
    if name == "sinus":
        return remap_ref.sinus_flow(in_hw, out_hw)
    if name == "folded":
        return remap_ref.folded(in_hw, out_hw)
    return _scatter(in_hw, out_hw)


def _operands(torch, kind, in_hw=IN_HW, planes=2, seed=7):
    """float32 [planes, H, W] leaves: the image in [0, 255]; hyper maps as in test_gpu_warp_grad's window test (sigma <= 3 keeps
    every Gaussian weight sum away from underflow)"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand((planes,) + tuple(in_hw), generator=gen, device="cuda") * 255
    hs = []
    if kind in ("gauss", "linear"):
        hs.append(torch.rand((planes,) + tuple(in_hw), generator=gen, device="cuda"))
    if kind == "gauss":
        hs += [torch.rand((planes,) + tuple(in_hw), generator=gen, device="cuda") * 0.3 for _ in range(2)]
    return x, hs


def _upstream(torch, planes, out_hw, seed=8):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn((planes,) + tuple(out_hw), generator=gen, device="cuda", dtype=torch.float64)


def _run_ops(torch, kind, S, pad_mode, cm, x, hs, G, in_hw=IN_HW, want_coords=True, pads=None):
    """the kernel through ops: (forward float64, [gx, gh...] float32, grad_coords float64 [N, oH, oW, 2] or None, geometry)"""
    from lerf_pytorch_amd import _lib, ops
    geo = ops.RemapGeometry(in_hw, cm, S, pad_mode=_lib.pad_mode_code(pad_mode, _lib.TORCH_PAD_MODES), pads=pads)
    out = ops.remap_planar(x, hs, geo, kind, _max_sigma(kind), out="f64")
    grads = [torch.zeros_like(x) for _ in range(1 + len(hs))]
    gc = torch.zeros((x.shape[0],) + geo.out_hw + (2,), dtype=torch.float64, device="cuda") if want_coords else None
    ops.remap_bwd_planar(x, hs, geo, kind, _max_sigma(kind), G, grads, gc)
    return out, grads, gc, geo


def _run_ref(torch, kind, S, pad_mode, cm_t, pads, x, hs, G):
    """the restatement on fresh leaves: (forward, [gx, gh...], map gradient summed over the planes, in the map's dtype)"""
    xr = x.detach().clone().requires_grad_(True)
    hr = [h.detach().clone().requires_grad_(True) for h in hs]
    cr = cm_t.detach().clone().requires_grad_(True)
    ref = remap_grad_ref.restated_remap(kind, S, pad_mode, cr, pads, xr, hr, _max_sigma(kind))
    got = torch.autograd.grad((ref * G).sum(), [xr] + hr + [cr], allow_unused=True)
    got = [torch.zeros_like(t) if g is None else g for g, t in zip(got, [xr] + hr + [cr])]      # box: no path to the map
    return ref.detach(), got[:-1], got[-1]


def _map_close(ours, ref, what=""):
    """float64 map gradient: MAP_TOL * max(max|ref|, 1), the same NaN positions; prints the measured error"""
    ours, ref = np.asarray(ours, np.float64), np.asarray(ref, np.float64)
    assert ours.shape == ref.shape
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(ours), nan), "NaN positions differ (%d vs %d)" % (int(np.isnan(ours).sum()), int(nan.sum()))
    if nan.all():
        return 0.0
    scale = max(float(np.max(np.abs(ref[~nan]))), 1.0)
    err = float(np.max(np.abs(ours[~nan] - ref[~nan])))
    print("map gradient %s: max error %.3g, scale %.3g, bound %.3g" % (what, err, scale, MAP_TOL * scale))
    assert err <= MAP_TOL * scale, "max |ours - ref| = %g > %g" % (err, MAP_TOL * scale)
    return err / scale


def _same_bits(torch, a, b):
    """torch.equal with NaN == NaN (a pixel whose weights all vanish has a NaN gradient in every run)"""
    return bool(torch.equal(torch.isnan(a), torch.isnan(b))) and bool(torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0)))


def _forward_close(out, ref):
    np.testing.assert_allclose(out.cpu().numpy(), ref.cpu().numpy(), rtol=0, atol=1e-9, equal_nan=True)


# ---------------------------------------------------------------------------------------------- 1. the reference's gradients
def test_golden_forward_and_gradients_through_the_map_of_the_homography(torch, golden):
    from lerf_pytorch_amd import coords
    T = _classes()
    g, g4, g13 = golden("g24_warp_grads.npz"), golden("g4_warp.npz"), golden("g13_torch_warp.npz")
    dev = torch.device("cuda")
    for c in g["cases"]:
        kind, S, pad = str(g[c + "/kind"]), int(g[c + "/S"]), str(g[c + "/pad_mode"])
        xl, hl = _g24_leaves(torch, g4, c, g, dev)
        B, Cn = xl.shape[:2]
        ref = _g24_out(g, g13, c)
        oH, oW = ref.shape[2:]
        w = _make(T, kind, S if kind == "gauss" else None, pad, dev).enable_backward()
        w.set_shape([B, Cn, 52, 52], coords.from_homography(g[c + "/matrix"], (oH, oW)))
        out = w.warp(xl, *hl)
        assert out.dtype == torch.float64 and out.requires_grad
        np.testing.assert_allclose(out.detach().cpu().numpy(), ref, rtol=0, atol=1e-9, equal_nan=True, err_msg=c)
        (out * torch.tensor(g[c + "/Gi"] / 2.0, device=dev)).sum().backward()
        assert xl.grad.dtype == torch.float32 and tuple(xl.grad.shape) == tuple(xl.shape)
        _close(xl.grad.cpu().numpy(), g[c + "/gx"])
        for k, h in enumerate(hl):
            assert h.grad.dtype == torch.float32 and tuple(h.grad.shape) == tuple(h.shape)
            _close(h.grad.cpu().numpy(), g[c + "/gh"][k])


# ---------------------------------------------------------------------------------------------- 2. map gradient vs restatement
CASES = [("gauss", 2, "constant"), ("gauss", 4, "constant"), ("gauss", 2, "replicate"), ("gauss", 2, "reflect"), ("gauss", 2, "circular"),
         ("linear", 2, "constant"), ("cubic", 4, "constant"), ("bilinear", 2, "constant"), ("lanczos2", 4, "constant"),
         ("lanczos3", 6, "constant"), ("nearest", 1, "constant")]


@pytest.mark.parametrize("name", ["sinus", "folded", "scatter"])
@pytest.mark.parametrize("kind,S,pad", CASES)
def test_gradients_against_restatement(torch, kind, S, pad, name):
    x, hs = _operands(torch, kind)
    G = _upstream(torch, 2, OUT_HW)
    for dt in (torch.float64, torch.float32):
        cm_t = torch.from_numpy(_map(name)).cuda().to(dt)
        out, grads, gc, geo = _run_ops(torch, kind, S, pad, cm_t, x, hs, G)
        ref, rgrads, rgc = _run_ref(torch, kind, S, pad, cm_t, geo.pads(), x, hs, G)
        _forward_close(out, ref)
        for a, b in zip(grads, rgrads):
            _close(a.cpu().numpy(), b.cpu().numpy())
        if kind == "nearest":
            assert not bool(gc.any()) and not bool(rgc.any())                    # box has no gradient: identically 0
        elif dt == torch.float64:
            _map_close(gc.sum(0).cpu().numpy(), rgc.cpu().numpy(), "%s S=%d %s %s" % (kind, S, pad, name))
        else:                                                                    # what _RemapFn hands a float32 map
            assert rgc.dtype == torch.float32
            _close(gc.sum(0).to(dt).cpu().numpy(), rgc.cpu().numpy())
        if kind != "nearest" and name != "scatter":
            assert bool((gc != 0).any())


# ---------------------------------------------------------------------------------------------- 3. both accumulation paths
def _block_windows(geo, S):
    """per 16 x 16 block of the output, the area (rows x columns) of the window its taps' clamped source pixels span: what
    warp_bwd_body reduces in LDS, from the host mirror of the kernels' geometry (axis_tap: the padded tap index clamped to
    [0, n - 1], shifted back by the low pad, clamped into the frame)"""
    gr, gc, lr, lc, pads = geo.host_geometry()
    H, W = geo.in_hw
    first = lambda l, n, p: np.clip(np.clip(l, 0, n - 1) - p, 0, n - 1)
    r0, r1 = first(lr, H, pads[0]), first(lr + S - 1, H, pads[0])
    c0, c1 = first(lc, W, pads[1]), first(lc + S - 1, W, pads[1])
    oH, oW = geo.out_hw
    areas = []
    for i in range(0, oH, WB):
        for j in range(0, oW, WB):
            b = (slice(i, i + WB), slice(j, j + WB))
            areas.append(int(r1[b].max() - r0[b].min() + 1) * int(c1[b].max() - c0[b].min() + 1))
    return areas


@pytest.mark.parametrize("kind,name,fits", [("gauss", "scatter", False), ("cubic", "scatter", True), ("gauss", "sinus", True)])
def test_lds_window_and_global_atomic_paths(torch, kind, name, fits):
    in_hw, out_hw, S = (52, 52), (33, 37), KIND_S[kind]
    cap = WB_LDS // KIND_MAPS.get(kind, 1)
    cm = _map(name, in_hw, out_hw)
    x, hs = _operands(torch, kind, in_hw)
    G = _upstream(torch, 2, out_hw)
    out, grads, gc, geo = _run_ops(torch, kind, S, "constant", cm, x, hs, G, in_hw)
    areas = _block_windows(geo, S)
    assert len(areas) == 3 * 3
    if fits:
        assert max(areas) <= cap, (max(areas), cap)
    else:
        assert max(areas) == 52 * 52 > cap                                       # 2704 > 2048: every tap adds to global memory
    cm_t = torch.from_numpy(cm).cuda()
    ref, rgrads, rgc = _run_ref(torch, kind, S, "constant", cm_t, geo.pads(), x, hs, G)
    _forward_close(out, ref)
    for a, b in zip(grads, rgrads):
        _close(a.cpu().numpy(), b.cpu().numpy())
    _map_close(gc.sum(0).cpu().numpy(), rgc.cpu().numpy(), "%s %s 52x52" % (kind, name))


def test_constant_region_of_the_folded_map(torch):
    """the lower right quarter of `folded` reads ONE source position: every pixel of its blocks adds to the same window elements"""
    cm = _map("folded")
    oH, oW = OUT_HW
    assert np.all(cm[oH // 2:, oW // 2:] == cm[-1, -1])
    x, hs = _operands(torch, "gauss")
    G = _upstream(torch, 2, OUT_HW)
    G[:, :oH // 2] = 0
    G[:, :, :oW // 2] = 0
    out, grads, gc, geo = _run_ops(torch, "gauss", 2, "constant", cm, x, hs, G)
    assert min(_block_windows(geo, 2)) <= 4 < WB_LDS // 4                        # a block of the quarter: one 2 x 2 window
    ref, rgrads, rgc = _run_ref(torch, "gauss", 2, "constant", torch.from_numpy(cm).cuda(), geo.pads(), x, hs, G)
    _forward_close(out, ref)
    for a, b in zip(grads, rgrads):
        assert int((b != 0).sum()) <= 2 * 4                                      # 2 planes x the 2 x 2 taps
        _close(a.cpu().numpy(), b.cpu().numpy())
    _map_close(gc.sum(0).cpu().numpy(), rgc.cpu().numpy(), "folded, constant quarter")
    assert not bool(gc[:, :oH // 2].any()) and bool((gc[:, oH // 2:, oW // 2:] != 0).any())


# ---------------------------------------------------------------------------------------------- 4. special entries
def test_special_entries(torch):
    H, W = IN_HW
    inf = float("inf")
    clean = _map("sinus")
    special = {(5, 5): (np.nan, None), (20, 21): (None, np.nan), (6, 7): (inf, None), (8, 9): (None, -inf), (10, 11): (-0.5, None),
               (12, 13): (0.0, None), (14, 15): (float(H), None), (16, 17): (H + 0.5, None), (18, 19): (None, float(W)),
               (22, 23): (None, W + 0.5), (24, 25): (-inf, inf)}
    dirty = clean.copy()
    for (i, j), (r, c) in special.items():
        if r is not None:
            dirty[i, j, 0] = r
        if c is not None:
            dirty[i, j, 1] = c
    spec = np.zeros(OUT_HW, bool)
    for i, j in special:
        spec[i, j] = True
    nan_px = np.isnan(dirty).any(-1)
    assert int(nan_px.sum()) == 2 and not spec[0, 0]
    x, hs = _operands(torch, "gauss")
    G = _upstream(torch, 2, OUT_HW)
    # ---- the special map against the restatement (which reads a NaN entry as 0: its pixels' upstream gradient is zeroed there)
    out, grads, gc, geo = _run_ops(torch, "gauss", 2, "constant", dirty, x, hs, G)
    assert bool(torch.isnan(out[:, torch.from_numpy(nan_px).cuda()]).all())
    Gr = G.clone()
    Gr[:, torch.from_numpy(nan_px).cuda()] = 0
    ref, rgrads, rgc = _run_ref(torch, "gauss", 2, "constant", torch.from_numpy(dirty).cuda(), geo.pads(), x, hs, Gr)
    for a, b in zip(grads, rgrads):
        _close(a.cpu().numpy(), b.cpu().numpy())                                 # no NaN the restatement lacks, none missing
    gcs, rg = gc.sum(0).cpu().numpy(), rgc.cpu().numpy()
    _map_close(gcs, rg, "special entries")
    assert not np.isnan(gc.cpu().numpy()).any()
    for (i, j), (r, c) in special.items():
        for k, v in ((0, r), (1, c)):
            if v is None:
                continue
            if np.isnan(v):
                assert not gc[:, i, j].any(), (i, j)                             # a masked pixel: both coordinates, every plane
            elif v in (0.0, float(H), float(W)):                                 # the clip passes at its borders
                assert abs(gcs[i, j, k] - rg[i, j, k]) <= MAP_TOL * max(abs(rg).max(), 1.0), (i, j, k)
            else:                                                                # +-inf and out of range: the clip blocks
                assert not gc[:, i, j, k].any(), (i, j, k)
    # ---- the other pixels do not see them: zero upstream gradient at the special pixels, special vs ordinary entries.  This shows
    # isolation for a zero upstream gradient only (with a non-zero one the two maps legitimately differ: an infinite or
    # out-of-range entry is clipped onto the border and contributes there); what the special pixels contribute under a non-zero
    # upstream gradient is held to the restatement by the comparison above
    Gz = G.clone()
    Gz[:, torch.from_numpy(spec).cuda()] = 0
    _, ga, gca, _ = _run_ops(torch, "gauss", 2, "constant", dirty, x, hs, Gz)
    _, gb, gcb, _ = _run_ops(torch, "gauss", 2, "constant", clean, x, hs, Gz)
    for a, b in zip(ga, gb):
        _close(a.cpu().numpy(), b.cpu().numpy())
    assert torch.equal(gca, gcb) and not bool(gca[:, torch.from_numpy(spec).cuda()].any())


# ---------------------------------------------------------------------------------------------- 5. determinism
@pytest.mark.parametrize("name", ["sinus", "scatter"])
def test_map_gradient_is_bit_equal_from_run_to_run(torch, name):
    x, hs = _operands(torch, "gauss")
    G = _upstream(torch, 2, OUT_HW)
    a = _run_ops(torch, "gauss", 2, "constant", _map(name), x, hs, G)[2]
    b = _run_ops(torch, "gauss", 2, "constant", _map(name), x, hs, G)[2]
    assert torch.equal(a, b) and bool((a != 0).any())


# ---------------------------------------------------------------------------------------------- 6. C contract
def _contract_setup(torch):
    from lerf_pytorch_amd import ops
    x, hs = _operands(torch, "gauss")
    G = _upstream(torch, 2, OUT_HW)
    geo = ops.RemapGeometry(IN_HW, _map("sinus"), 2)
    return ops, x, hs, G, geo


def test_null_subsets_and_accumulation(torch):
    ops, x, hs, G, geo = _contract_setup(torch)
    shape_c = (2,) + OUT_HW + (2,)
    full = [torch.zeros_like(x) for _ in range(4)]
    full_c = torch.zeros(shape_c, dtype=torch.float64, device="cuda")
    ops.remap_bwd_planar(x, hs, geo, "gauss", 10.0, G, full, full_c)
    assert all(bool(t.abs().sum() > 0) for t in full) and bool(full_c.abs().sum() > 0)
    for keep in itertools.product((False, True), repeat=5):
        part = [torch.zeros_like(x) if k else None for k in keep[:4]]
        part_c = torch.zeros(shape_c, dtype=torch.float64, device="cuda") if keep[4] else None
        ops.remap_bwd_planar(x, hs, geo, "gauss", 10.0, G, part, part_c)
        for p, f in zip(part, full):
            if p is not None:
                _close(p.cpu().numpy(), f.cpu().numpy())
        if part_c is not None:
            assert torch.equal(part_c, full_c)
    base = [torch.full_like(x, 3.0) for _ in range(4)]
    base_c = torch.full(shape_c, 3.0, dtype=torch.float64, device="cuda")
    ops.remap_bwd_planar(x, hs, geo, "gauss", 10.0, G, base, base_c)
    for b, f in zip(base, full):
        _close((b - 3.0).cpu().numpy(), f.cpu().numpy())
    _map_close((base_c - 3.0).cpu().numpy(), full_c.cpu().numpy(), "accumulated onto 3.0")
    # the fixed kinds: the image and the map, no hyper maps
    only = [torch.zeros_like(x)]
    only_c = torch.zeros(shape_c, dtype=torch.float64, device="cuda")
    ops.remap_bwd_planar(x, [], ops.RemapGeometry(IN_HW, _map("sinus"), 4), "cubic", 1.0, G, only, only_c)
    assert bool((only[0] != 0).any()) and bool((only_c != 0).any())          # (cubic has NaN pixels at the clamped last rows)


def test_refused_arguments_write_nothing(torch):
    from lerf_pytorch_amd import _lib
    ops, x, hs, G, geo = _contract_setup(torch)
    lib = _lib.lib()
    bufs = [torch.full_like(x, 3.0) for _ in range(4)]
    buf_c = torch.full((2,) + OUT_HW + (2,), 3.0, dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)

    def call(feat=x, h=hs, N=2, kind="gauss", G_=G, geo_null=False, **fields):
        s, keep = geo.struct(x.device)
        for k, v in fields.items():
            setattr(s, k, v)
        code = _lib.KINDS[kind] if isinstance(kind, str) else kind
        return lib.lerf_remap_bwd(p(feat), p(h[0]), p(h[1]), p(h[2]), N, IN_HW[0], IN_HW[1], None if geo_null else C.byref(s), code, 10.0,
                                  p(G_), p(bufs[0]), p(bufs[1]), p(bufs[2]), p(bufs[3]), p(buf_c), _lib.current_stream())
    EINVAL, EUNSUPPORTED = -1, -2
    assert call(feat=None) == EINVAL
    assert call(G_=None) == EINVAL
    assert call(geo_null=True) == EINVAL
    assert call(coords=None) == EINVAL
    assert call(coords_dtype=_lib.LERF_U8) == EINVAL
    assert call(pad_mode=7) == EINVAL and call(pad_mode=-1) == EINVAL
    assert call(row_stride=2 * OUT_HW[1] - 2) == EINVAL and call(row_stride=2 * OUT_HW[1] + 1) == EINVAL
    assert call(pad_r_lo=-2) == EINVAL and call(pad_c_lo=99) == EINVAL
    assert call(kind=7) == EUNSUPPORTED and call(kind=-1) == EUNSUPPORTED
    assert call(S=0) == EUNSUPPORTED and call(S=99) == EUNSUPPORTED
    assert call(N=65536) == EINVAL and call(N=0) == EINVAL                       # the grid caps
    assert call(out_h=65535 * WB + 1, row_stride=2 * OUT_HW[1]) == EINVAL
    assert call(h=[hs[0], None, hs[2]]) == EINVAL and call(h=[None, hs[1], hs[2]]) == EINVAL
    assert call(h=[None, None, None], kind="linear") == EINVAL
    torch.cuda.synchronize()
    assert all(bool((b == 3.0).all()) for b in bufs) and bool((buf_c == 3.0).all())
    assert call() == 0                                                           # and the same call, unaltered, runs
    torch.cuda.synchronize()
    assert all(bool((b != 3.0).any()) for b in bufs) and bool((buf_c != 3.0).any())


@pytest.mark.parametrize("on_device", [False, True])
def test_row_tile_with_the_whole_maps_pads(torch, on_device):
    from lerf_pytorch_amd import ops
    x, hs = _operands(torch, "gauss")
    G = _upstream(torch, 2, OUT_HW)
    cm = _map("sinus")
    whole = ops.RemapGeometry(IN_HW, torch.from_numpy(cm).cuda() if on_device else cm, 2)
    assert whole.pads()[0] > 0
    i0, i1 = 13, 30                                                              # ragged against the 16-row blocks
    part = whole.rows(i0, i1)
    assert part.out_hw == (i1 - i0, OUT_HW[1]) and part.pads() == whole.pads()
    Gw = torch.zeros_like(G)
    Gw[:, i0:i1] = G[:, i0:i1]
    gw = [torch.zeros_like(x) for _ in range(4)]
    gcw = torch.zeros((2,) + OUT_HW + (2,), dtype=torch.float64, device="cuda")
    ops.remap_bwd_planar(x, hs, whole, "gauss", 10.0, Gw, gw, gcw)
    gp = [torch.zeros_like(x) for _ in range(4)]
    gcp = torch.zeros((2, i1 - i0, OUT_HW[1], 2), dtype=torch.float64, device="cuda")
    ops.remap_bwd_planar(x, hs, part, "gauss", 10.0, G[:, i0:i1], gp, gcp)
    assert torch.equal(gcp, gcw[:, i0:i1]) and bool((gcp != 0).any())
    for a, b in zip(gp, gw):
        _close(a.cpu().numpy(), b.cpu().numpy())


# ---------------------------------------------------------------------------------------------- 7. the switch
def test_backward_is_opt_in_and_the_plain_paths_are_unchanged(torch):
    from lerf_pytorch_amd import ops
    T = _classes()
    x, hs = _operands(torch, "gauss")
    x4, h4 = x[None], [h[None] for h in hs]
    cm = _map("sinus")
    fresh = T.SteeringGaussianRemap2dTorch(support_sz=2, max_sigma=10)
    fresh.set_shape([1, 2] + list(IN_HW), cm)
    plain = fresh.warp(x4, *h4)
    assert plain.grad_fn is None and not plain.requires_grad
    xg = x4.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="forward-only"):
        fresh.warp(xg, *h4)
    on = T.SteeringGaussianRemap2dTorch(support_sz=2, max_sigma=10).enable_backward()
    on.set_shape([1, 2] + list(IN_HW), cm)
    assert torch.equal(on.warp(x4, *h4), plain) and on.warp(x4, *h4).grad_fn is None          # no leaf requires grad
    with torch.no_grad():
        assert torch.equal(on.warp(xg, *h4), plain) and torch.equal(fresh.warp(xg, *h4), plain)
    out = on.warp(xg, *h4)
    assert out.requires_grad and out.dtype == torch.float64 and torch.equal(out.detach(), plain)
    out.sum().backward()
    assert xg.grad.dtype == torch.float32 and tuple(xg.grad.shape) == tuple(xg.shape)
    # a map held as numpy gets no gradient and the call works; a fresh class with a map that requires grad refuses
    leaf = torch.from_numpy(cm).cuda().requires_grad_(True)
    fresh.set_shape([1, 2] + list(IN_HW), leaf)
    with pytest.raises(NotImplementedError, match="forward-only"):
        fresh.warp(x4, *h4)
    with torch.no_grad():
        assert torch.equal(fresh.warp(x4, *h4), plain)
    direct = ops.remap_planar(x, hs, on.geo, "gauss", 10, out="f64")
    assert torch.equal(plain[0], direct)
    # a HOST tensor that requires grad would be uploaded as data: refused, not silently detached (numpy stays data)
    on.set_shape([1, 2] + list(IN_HW), torch.from_numpy(cm).requires_grad_(True))
    with pytest.raises(ValueError, match="host"):
        on.warp(x4, *h4)
    with torch.no_grad():
        assert torch.equal(on.warp(x4, *h4), plain)
    # the kernels read the map in place: a leaf map modified between warp() and backward() is an error autograd reports
    leaf2 = torch.from_numpy(cm).cuda().requires_grad_(True)
    on.set_shape([1, 2] + list(IN_HW), leaf2)
    out2 = on.warp(x4, *h4)
    with torch.no_grad():
        leaf2.add_(0.25)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out2.sum().backward()


@pytest.mark.parametrize("kind", ["gauss", "cubic"])
def test_map_as_a_leaf_dtypes_shapes_and_views(torch, kind):
    T = _classes()
    S = KIND_S[kind]
    x, hs = _operands(torch, kind)
    G = _upstream(torch, 2, OUT_HW)
    cm = _map("sinus")
    oH, oW = OUT_HW
    ref64 = None
    for dt in (torch.float64, torch.float32):
        for view in (False, True):
            if view:                                                             # rows of a wider buffer: a strided tile view
                leaf = torch.full((oH, oW + 5, 2), 1.0, dtype=dt, device="cuda")
                with torch.no_grad():
                    leaf[:, :oW] = torch.from_numpy(cm).cuda().to(dt)
                leaf.requires_grad_(True)
                m = leaf[:, :oW]
                assert m.stride(0) > 2 * oW
            else:
                leaf = torch.from_numpy(cm).cuda().to(dt).requires_grad_(True)
                m = leaf
            xl = x[None].clone().requires_grad_(True)
            hl = [h[None].clone().double().requires_grad_(True) for h in hs]     # a float64 leaf gets a float64 gradient
            w = _make(T, kind, S, "constant").enable_backward()
            w.set_shape([1, 2] + list(IN_HW), m)
            out = w.warp(xl, *hl)
            assert out.dtype == torch.float64 and out.requires_grad and tuple(out.shape) == (1, 2) + OUT_HW
            out.backward(G[None])
            assert leaf.grad.dtype == dt and tuple(leaf.grad.shape) == tuple(leaf.shape)
            assert xl.grad.dtype == torch.float32 and tuple(xl.grad.shape) == tuple(xl.shape)
            for h in hl:
                assert h.grad.dtype == torch.float64 and tuple(h.grad.shape) == tuple(h.shape)
            gm = leaf.grad[:, :oW]
            if view:
                assert not bool(leaf.grad[:, oW:].any())
            assert bool((gm != 0).any())
            if dt == torch.float64 and not view:
                ref64 = gm.clone()
            elif dt == torch.float64:
                assert _same_bits(torch, gm, ref64)                                    # the view is the same map: the same bits
    # the map gradient alone: only the map requires grad
    leaf = torch.from_numpy(cm).cuda().requires_grad_(True)
    w = _make(T, kind, S, "constant").enable_backward()
    w.set_shape([1, 2] + list(IN_HW), leaf)
    out = w.warp(x[None], *[h[None] for h in hs])
    assert out.requires_grad
    out.backward(G[None])
    assert _same_bits(torch, leaf.grad, ref64)


# ---------------------------------------------------------------------------------------------- 8. a fit
FIT_LR, FIT_STEPS, FIT_EDGE = 0.1, 20, 6     # the step size gives the restatement a final / initial loss of 0.21 (CPU, float64)


def _fit(torch, dev, forward):
    """plain SGD on a flow from zero towards the constant shift (1.3, -0.7); the loss is the mean squared error over the
    interior (the frame's last rows and columns have no finite bicubic value: the field of view is clamped in padded
    coordinates), and only the interior flow moves"""
    from lerf_pytorch_amd import coords
    n = 48
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    img = (100 + 50 * np.sin(2 * np.pi * ii / 24) + 40 * np.cos(2 * np.pi * jj / 16) + 30 * np.sin(2 * np.pi * (ii + jj) / 32)).astype(np.float32)
    x = torch.from_numpy(img)[None].to(dev)
    e = slice(FIT_EDGE, n - FIT_EDGE)
    shift = torch.zeros((n, n, 2), dtype=torch.float64, device=dev)
    shift[..., 0], shift[..., 1] = 1.3, -0.7
    with torch.no_grad():
        target = forward(x, coords.from_flow_torch(shift))
    flow = torch.zeros((n, n, 2), dtype=torch.float64, device=dev, requires_grad=True)
    losses = []
    for step in range(FIT_STEPS + 1):
        loss = ((forward(x, coords.from_flow_torch(flow)) - target)[:, e, e] ** 2).mean()
        losses.append(float(loss.detach()))
        if step == FIT_STEPS:
            break
        g, = torch.autograd.grad(loss, flow)
        with torch.no_grad():
            flow[e, e] -= FIT_LR * g[e, e]
    assert np.isfinite(losses).all()
    return losses[-1] / losses[0]


def test_a_flow_fitted_by_sgd_follows_the_restatement(torch):
    T = _classes()

    def gpu_forward(x, cm):
        w = T.BicubicRemap2dTorch().enable_backward()
        w.set_shape([1, 1, 48, 48], cm)
        return w.warp(x[None])[0]

    def ref_forward(x, cm):
        return remap_grad_ref.restated_remap("cubic", 4, "constant", cm, remap_grad_ref.pads_of(cm, (48, 48), 4), x, [], 1.0)
    ref_ratio = _fit(torch, torch.device("cpu"), ref_forward)
    assert ref_ratio < 0.5, ref_ratio
    gpu_ratio = _fit(torch, torch.device("cuda"), gpu_forward)
    print("final / initial loss: restatement %.6g, GPU %.6g" % (ref_ratio, gpu_ratio))
    assert abs(gpu_ratio - ref_ratio) <= 0.05 * ref_ratio, (gpu_ratio, ref_ratio)
