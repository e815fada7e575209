"""GPU: resize_right.resize on the MI355X (csrc/lerf_rr.hip) against the reference's own results
(tests/golden/g29_rr.npz, tests/golden/gen_rr_golden.py) and against the shipped Set5 LR folders, which the reference's
resize made.

Tolerances.
  * Set5 bytes: 0 differing bytes.
  * numpy cases: 1e-9 absolute on the 0..255 range (the project's float64 bound).  Bit equality is asserted in addition for
    every numpy case except 1-D inputs with 8 or more taps: the kernel adds the taps in order, as numpy does when it
    reduces a non-last axis; a 1-D input makes the tap axis the last, contiguous one, where numpy sums pairwise.
  * torch float32 cases: twice the largest |reference float32 - reference float64| gap of the case's class, recorded by
    the generator (a different float32 summation order may land on either side).  Class sweep/box is the exception: the
    box kernel is discontinuous, so its recorded gap (230) measures which PIXEL a float32 grid selects, not a rounding
    error.  The tables here are the reference's float32 tables bit for bit (tests/test_rr_cpu.py), so what remains is the
    float32 sum of at most `taps` products of values up to 255: (taps + 1) * 255 * 2^-23.
  * torch float64 cases: the float32 tables promoted, float64 sums: 1e-9 absolute, as for numpy.
  * gradients: float32 twice the recorded gap of the reference's float32 autograd against its float64 autograd;
    float64 1e-9; the dot-product identity to 1e-9 relative.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import ASSETS, DATA, GOLDEN

sys.path.insert(0, GOLDEN)
import gen_rr_golden as G                                                     # noqa: E402

import lerf_pytorch_amd as L                                                  # noqa: E402,F401
from lerf_pytorch_amd import lazy                                             # noqa: E402
from lerf_pytorch_amd.resize_right import interp_methods as IM                # noqa: E402
from lerf_pytorch_amd.resize_right import resize_right as R                   # noqa: E402
from lerf_pytorch_amd.resize_right.resize_right import resize, resize_to_uint8   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64_TOL = 1e-9


@pytest.fixture(scope="module")
def g29():
    g = np.load(os.path.join(GOLDEN, "g29_rr.npz"))
    return g, json.loads(str(g["cases"]))


def kwargs_of(c):
    kw = dict(c["kw"])
    name = kw.pop("interp_method", "cubic")
    kw["interp_method"] = G.gauss5 if name == "gauss5" else getattr(IM, name)
    return kw


def host(a):
    return np.asarray(a)


# ---------------------------------------------------------------- 1. Set5 bytes
def _set5():
    for s in (2, 3, 4):
        for f in sorted(os.listdir(os.path.join(DATA, "HR"))):
            yield s, f


def _modcrop(a, s):
    H, W = a.shape[:2]
    return a[:H - H % s, :W - W % s]


@pytest.mark.parametrize("s,f", list(_set5()))
def test_set5_lr_bytes(s, f):
    hr = np.array(Image.open(os.path.join(DATA, "HR", f)))
    want = np.array(Image.open(os.path.join(DATA, "LR_bicubic", "rrLR_X%d.00_%d.00" % (s, s), f)))
    x = np.ascontiguousarray(_modcrop(hr, s)).astype(np.float64)
    keep = x.copy()
    got = host(np.round(np.clip(resize(x, scale_factors=[1 / s, 1 / s]), 0, 255)).astype(np.uint8))
    assert got.shape == want.shape and got.dtype == np.uint8
    print("%s x%d: %d differing bytes (resize + host rounding)" % (f, s, int((got != want).sum())))
    assert int((got != want).sum()) == 0
    fused = host(resize_to_uint8(x, scale_factors=[1 / s, 1 / s]))
    print("%s x%d: %d differing bytes (uint8 epilogue)" % (f, s, int((fused != want).sum())))
    assert fused.dtype == np.uint8 and int((fused != want).sum()) == 0
    assert np.array_equal(x, keep)
    lazy.set_enabled(False)                      # plain numpy results: the same bytes
    try:
        plain = resize(x, scale_factors=[1 / s, 1 / s])
    finally:
        lazy.set_enabled(True)
    assert isinstance(plain, np.ndarray) and plain.dtype == np.float64
    assert np.array_equal(np.round(np.clip(plain, 0, 255)).astype(np.uint8), want)


# ---------------------------------------------------------------- 2. numpy cases
def _taps_of_last_pass(c):
    kw = kwargs_of(c)
    scales, sizes = R._scales_and_sizes(c["shape"], kw.get("out_shape"), kw.get("scale_factors"), False, True)
    plan = R._plan(c["shape"], scales, sizes, kw["interp_method"], kw.get("support_sz"), kw.get("antialiasing", True), 0, True)
    return max(t.taps for _, t in plan)


def test_numpy_cases(g29):
    g, cases = g29
    n = bit = 0
    for i, c in enumerate(cases):
        if c["fw"] != "np":
            continue
        x = G.make_input(1000 + i, c["shape"], c["dtype"])
        keep = x.copy()
        got = host(resize(x, **kwargs_of(c)))
        ref = g["out_%d" % i]
        assert got.dtype == np.dtype(c["out_dtype"]) == np.float64 and got.shape == ref.shape, (i, c)
        err = float(np.max(np.abs(got - ref)))
        assert err <= F64_TOL, (i, c, err)
        if not (len(c["shape"]) == 1 and _taps_of_last_pass(c) >= 8):
            assert got.tobytes() == ref.tobytes(), (i, c, err)
            bit += 1
        assert np.array_equal(x, keep)
        n += 1
    print("numpy cases: %d, bit-equal asserted for %d" % (n, bit))
    assert n > 90 and bit >= n - 3


# ---------------------------------------------------------------- 3. torch cases
def _class_tolerances(g, cases):
    tol = {}
    for i, c in enumerate(cases):
        if "gap_%d" % i in g.files:
            tol[c["cls"]] = max(tol.get(c["cls"], 0.0), 2.0 * float(g["gap_%d" % i]))
    return tol


def _box_tolerance(c):
    kw = kwargs_of(c)
    scales, sizes = R._scales_and_sizes(c["shape"], kw.get("out_shape"), kw.get("scale_factors"), False, False)
    plan = R._plan(c["shape"], scales, sizes, kw["interp_method"], kw.get("support_sz"), kw.get("antialiasing", True), 0, False)
    return sum((t.taps + 1) for _, t in plan) * 255.0 * 2.0 ** -23


def test_torch_cases(g29):
    g, cases = g29
    tol = _class_tolerances(g, cases)
    worst = {}
    n = 0
    for i, c in enumerate(cases):
        if c["fw"] != "torch":
            continue
        x = torch.from_numpy(G.make_input(1000 + i, c["shape"], c["dtype"])).to(DEV)
        keep = x.clone()
        got = resize(x, **kwargs_of(c))
        ref = g["out_%d" % i]
        assert got.is_cuda and str(got.dtype) == "torch." + c["out_dtype"] and tuple(got.shape) == ref.shape, (i, c)
        err = float(np.max(np.abs(got.double().cpu().numpy() - ref.astype(np.float64))))
        if c["dtype"] == "float64":
            bound = F64_TOL
        elif c["cls"] == "sweep/box":
            bound = _box_tolerance(c)
        else:
            bound = tol[c["cls"]]
        worst[c["cls"]] = max(worst.get(c["cls"], (0.0, 0.0)), (err, bound))
        assert err <= bound, (i, c, err, bound)
        assert torch.equal(x, keep)
        n += 1
    for k in sorted(worst):
        print("torch class %-16s worst error %.3e (bound %.3e)" % (k, worst[k][0], worst[k][1]))
    assert n > 80


# ---------------------------------------------------------------- 4. gradients
def test_gradients_against_reference_autograd(g29):
    g, cases = g29
    ggaps = [float(g[k]) for k in g.files if k.startswith("ggap_")]
    tol32 = 2.0 * max(ggaps)
    n = 0
    for i, c in enumerate(cases):
        if "grad_%d" % i not in g.files:
            continue
        x = torch.from_numpy(G.make_input(1000 + i, c["shape"], c["dtype"])).to(DEV).requires_grad_(True)
        out = resize(x, **kwargs_of(c))
        y = torch.from_numpy(G.make_input(5000 + i, tuple(out.shape), c["dtype"]) / 255.0).to(x.dtype).to(DEV)
        (out * y).sum().backward()
        ref = g["grad_%d" % i]
        assert x.grad.dtype == x.dtype and tuple(x.grad.shape) == ref.shape
        err = float(np.max(np.abs(x.grad.double().cpu().numpy() - ref.astype(np.float64))))
        bound = F64_TOL if c["dtype"] == "float64" else tol32
        print("gradient case %d (%s %s): error %.3e (bound %.3e)" % (i, c["cls"], c["dtype"], err, bound))
        assert err <= bound, (i, c, err, bound)
        n += 1
    assert n == 6


def test_backward_is_deterministic_and_the_adjoint():
    rng = np.random.default_rng(11)
    for trial in range(12):
        nd = int(rng.integers(1, 5))
        shape = [int(rng.integers(1, 40)) for _ in range(nd)]
        k = int(rng.integers(1, min(nd, 3) + 1))
        scales = [float(rng.choice([0.125, 0.3, 0.5, 0.77, 1.0, 1.5, 2.0, 3.3])) for _ in range(k)]
        pad = str(rng.choice(["constant", "replicate", "reflect", "circular"]))
        if pad == "reflect" and min(shape) < 2:
            pad = "replicate"
        method = [IM.cubic, IM.lanczos3, IM.linear][trial % 3]
        x = torch.from_numpy(rng.normal(size=shape)).to(DEV).requires_grad_(True)
        out = resize(x, scale_factors=scales, interp_method=method, pad_mode=pad)
        if out is x:
            continue
        y = torch.from_numpy(rng.normal(size=tuple(out.shape))).to(DEV)
        (gx,) = torch.autograd.grad(out, x, y, retain_graph=True)
        (gx2,) = torch.autograd.grad(out, x, y)
        assert torch.equal(gx, gx2)
        lhs, rhs = float((out.detach() * y).sum()), float((x.detach() * gx).sum())
        scale = float(out.detach().abs().mul(y.abs()).sum()) + 1e-300
        assert abs(lhs - rhs) <= 1e-9 * scale, (shape, scales, pad, lhs, rhs)


# ---------------------------------------------------------------- 5. layouts, streams, edges
def test_non_contiguous_input_and_non_default_stream():
    rng = np.random.default_rng(5)
    base = torch.from_numpy(rng.uniform(0, 255, (2, 20, 24, 3)).astype(np.float32)).to(DEV)
    x = base.permute(0, 3, 1, 2)                                       # NCHW view of NHWC storage
    assert not x.is_contiguous()
    want = resize(x.contiguous(), scale_factors=[0.5, 1.5])
    assert torch.equal(resize(x, scale_factors=[0.5, 1.5]), want)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        got = resize(x, scale_factors=[0.5, 1.5])
    st.synchronize()
    assert torch.equal(got, want)
    xs = x[:, :, ::2, 1:-1]
    assert torch.equal(resize(xs, scale_factors=[2, 2]), resize(xs.contiguous(), scale_factors=[2, 2]))


def test_batch_independence():
    rng = np.random.default_rng(6)
    x = torch.from_numpy(rng.uniform(0, 255, (5, 3, 17, 70)).astype(np.float32)).to(DEV)
    for sf in ([0.4, 0.4], [2.0, 3.0], [1, 0.125]):
        full = resize(x, scale_factors=sf, interp_method=IM.lanczos3)
        for b in range(5):
            assert torch.equal(full[b:b + 1], resize(x[b:b + 1], scale_factors=sf, interp_method=IM.lanczos3))


def test_wide_rows_and_the_lds_window_fallback():
    """inner >= 1024 exercises the wide kernel's four elements per lane; a last-dim pass whose segment exceeds the LDS window
    (x1/32 Lanczos-3: 192 taps, 256 outputs per workgroup) takes the global-memory path.  Same numbers either way: compare
    with the transposed problem, which runs through the other lane mapping."""
    rng = np.random.default_rng(7)
    a = rng.uniform(0, 255, (40, 1500))
    r0 = host(resize(a, scale_factors=[0.5, 1]))                        # wide: inner = 1500
    r1 = host(resize(np.ascontiguousarray(a.T), scale_factors=[1, 0.5])).T      # narrow: inner = 1
    assert np.array_equal(r0, r1)
    b = rng.uniform(0, 255, (70, 9000))
    n0 = host(resize(b, scale_factors=[1, 1 / 32], interp_method=IM.lanczos3))
    n1 = host(resize(np.ascontiguousarray(b.T), scale_factors=[1 / 32, 1], interp_method=IM.lanczos3)).T
    assert n0.shape == (70, 282) and np.array_equal(n0, n1)


def test_edges_one_pixel_dims_and_wide_taps():
    x = np.array([[7.0, 9.0, 250.0]])
    out = host(resize(x, scale_factors=[3, 2], pad_mode="edge"))         # a 1-pixel dim, up-scaled under an edge pad
    # every row is the same weighted mean of the one source row; the weights differ per row, so only to rounding
    assert out.shape == (3, 6) and np.allclose(out[0], out[1], rtol=0, atol=F64_TOL) and np.allclose(out[1], out[2], rtol=0, atol=F64_TOL)
    assert np.allclose(out[0], host(resize(x[0], scale_factors=[2], pad_mode="edge")), rtol=0, atol=F64_TOL)
    five = np.array([10.0, 20.0, 30.0, 40.0, 50.0])
    one = host(resize(five, scale_factors=[0.125], pad_mode="wrap"))     # 32 taps over 5 pixels, n_out == 1
    assert one.shape == (1,)
    tab = R.axis_table(5, 1, 0.125, IM.cubic, 4, True, 4, True)
    want = 0.0
    for k in range(tab.taps):
        want = want + tab.w[0, k] * five[(int(tab.left[0]) + k) % 5]
    assert one[0] == want
    u8 = np.arange(24, dtype=np.uint8).reshape(4, 6)
    assert np.array_equal(host(resize(u8, [2, 2])), host(resize(u8.astype(np.float64), [2, 2])))
    t = torch.arange(24, dtype=torch.uint8, device=DEV).reshape(1, 4, 6)
    assert resize(t, 2).dtype == torch.float32
    assert torch.equal(resize(t, 2), resize(t.float(), 2))
    with pytest.raises(Exception, match="GPU"):
        resize(torch.zeros(1, 4, 4), 2)


def test_uint8_epilogue_equals_numpy_rounding():
    rng = np.random.default_rng(8)
    for shape, sf in (((33, 47, 3), [1 / 3, 1 / 3]), ((33, 47), [0.5, 2]), ((20, 31, 3), [1 / 1.5, 1 / 2]), ((9, 9, 3), [1, 0.5])):
        x = rng.uniform(-40, 300, shape)
        lazy.set_enabled(False)
        try:
            f = resize(x, scale_factors=sf)
            u = resize_to_uint8(x, scale_factors=sf)
        finally:
            lazy.set_enabled(True)
        assert u.dtype == np.uint8 and np.array_equal(u, np.round(np.clip(f, 0, 255)).astype(np.uint8))


# ---------------------------------------------------------------- 6. make_lr and the harness
def test_make_lr_reproduces_set5_and_the_harness_scores_it(tmp_path, capsys):
    from lerf_pytorch_amd.resample import eval_harness as EH
    from lerf_pytorch_amd.resample import make_lr as ML
    root = tmp_path / "bench"
    os.makedirs(root / "Set5")
    os.symlink(os.path.join(DATA, "HR"), root / "Set5" / "HR")
    ML.main(["--testDir", str(root), "--datasets", "Set5", "--scales", "2x2", "3x3", "4x4", "1.5x2"])
    for s in (2, 3, 4):
        made = root / "Set5" / "LR_bicubic" / ("rrLR_X%d.00_%d.00" % (s, s))
        shipped = os.path.join(DATA, "LR_bicubic", "rrLR_X%d.00_%d.00" % (s, s))
        assert sorted(os.listdir(made)) == sorted(os.listdir(shipped))
        for f in os.listdir(shipped):
            a, b = np.array(Image.open(made / f)), np.array(Image.open(os.path.join(shipped, f)))
            assert a.shape == b.shape and np.array_equal(a, b), (s, f)
    with pytest.raises(FileExistsError):
        ML.main(["--testDir", str(root), "--scales", "2x2"])
    ML.main(["--testDir", str(root), "--scales", "2x2", "--force"])
    capsys.readouterr()
    tables = []
    for test_dir in (str(root), os.path.dirname(DATA)):
        EH.main(["sr", "--testDir", test_dir, "-e", os.path.join(ASSETS, "lerf-g"), "--scales", "2x2"])
        tables.append(capsys.readouterr().out)
    assert tables[0] == tables[1] and tables[0].split()[:2] == ["Scale", "2.0x2.0"] and "35.71/0.9475" in tables[0]
    # a pair that was not shipped: made above, scored here
    hr = np.array(Image.open(os.path.join(DATA, "HR", "woman.png")))
    lr = np.array(Image.open(root / "Set5" / "LR_bicubic" / "rrLR_X1.50_2.00" / "woman.png"))
    assert lr.shape == (int(np.ceil(hr.shape[0] / 1.5)), int(np.ceil(hr.shape[1] / 2)), 3)
    EH.main(["sr", "--testDir", str(root), "-e", os.path.join(ASSETS, "lerf-g"), "--scales", "1.5x2"])
    line = capsys.readouterr().out.splitlines()
    assert line[0].split() == ["Scale", "1.5x2.0"]
    # no reference figure exists for this pair; a sane score lies between the x4 table entry (30.15 dB, a harder problem
    # in both directions) and 45 dB, above which an up-scaling result would be implausibly close to lossless
    psnr = float(line[1].split()[1].split("/")[0])
    assert 30.15 < psnr < 45.0
