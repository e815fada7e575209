"""The trainable hyper-networks on the GPU (lerf_srnet.hip: lerf_srnet_fwd_f32 / lerf_srnet_bwd_f32, and SRNetsSWF2 on
top of them), against float64 restatements and against the reference's own SRNetsSWF2 (tests/golden/g26_srnets.npz).

Tolerances.
  forward: the first-order float32 bound of test_gpu_transfer_paths.py, |y - y64| <= gamma_969 * M6 + 2^-22, M6 the
    pre-tanh sum of the absolute network (oracle.srnet_forward(..., absolute=True)); sech^2 <= 1 is not exploited.
  backward: each weight tensor's gradient and the image gradient within 1e-4 of the largest entry of that tensor in
    the float64 autograd restatement (float32 products, sums over up to 17 k positions in tile / slab order: a few
    1e-6 relative in practice; a wrong layout or a lost tile is off by O(1e-2) or more).
  golden: net outputs within 2e-5 (float32 against the reference's float32 CPU convolutions); integer predict planes
    equal except at rounding ties, which flip by exactly one step and are counted (<= 1 % of the plane); loss within
    1e-3 relative; the sampled parameter gradients within 2e-3 of the largest sampled entry of that parameter.
"""
import ctypes as C
import os
import types

import numpy as np
import pytest

from conftest import ASSETS, DATA

pytestmark = pytest.mark.gpu
REACH = {"s": 1, "d": 2, "y": 2, "c": 3, "t": 3}
PATTERN = {"s": [(0, 0), (0, 1), (1, 0), (1, 1)], "d": [(0, 0), (0, 2), (2, 0), (2, 2)],
           "y": [(0, 0), (1, 1), (1, 2), (2, 1)], "c": [(0, 0), (0, 1), (0, 2), (0, 3)],
           "t": [(0, 0), (1, 1), (2, 2), (3, 3)]}
LAYERS = ["conv1.conv", "conv2.conv1.conv", "conv3.conv1.conv", "conv4.conv1.conv", "conv5.conv1.conv", "conv6.conv"]
KEY = "s2_cr1"


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def _weights(rng, outC):
    """Kaiming-normal SRNet weights (Conv's init) with small random biases, as state_dict arrays under KEY"""
    d = {}
    for li, name in enumerate(LAYERS):
        fan_in = 4 if li == 0 else li * 64
        n_out = outC if li == 5 else 64
        d["%s.model.%s.weight" % (KEY, name)] = (rng.standard_normal((n_out, fan_in)) * np.sqrt(2.0 / fan_in)).astype(np.float32)
        d["%s.model.%s.bias" % (KEY, name)] = (0.05 * rng.standard_normal(n_out)).astype(np.float32)
    return d


def _pack(d):
    return np.concatenate([d["%s.model.%s.%s" % (KEY, n, t)].reshape(-1) for n in LAYERS for t in ("weight", "bias")])


def _tuples(img, mode, h, w):
    """[n_planes*h*w, 4] pattern pixels of every output position (plane-major, then row, column)"""
    return np.stack([img[:, dy:dy + h, dx:dx + w].reshape(-1) for dy, dx in PATTERN[mode]], axis=1)


def _fwd(torch, flat, outC, mode, img, h, w, bd):
    L = __import__("lerf_pytorch_amd")._lib
    out = torch.empty((img.shape[0], outC, h, w), dtype=torch.float32, device="cuda")
    rc = L.lib().lerf_srnet_fwd_f32(C.c_void_p(flat.data_ptr()), outC, mode.encode(), C.c_void_p(img.data_ptr()), img.shape[0],
                                    h, w, bd, C.c_void_p(out.data_ptr()), L.current_stream())
    return rc, out


def _bwd(torch, flat, outC, mode, img, g, h, w, bd, gw, gx, ws=None, nbytes=None):
    L = __import__("lerf_pytorch_amd")._lib
    lib = L.lib()
    if ws is None:
        nbytes = lib.lerf_srnet_bwd_workspace_bytes(outC, img.shape[0], h, w)
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device="cuda")
    return lib.lerf_srnet_bwd_f32(C.c_void_p(flat.data_ptr()), outC, mode.encode(), C.c_void_p(img.data_ptr()),
                                  C.c_void_p(g.data_ptr()), img.shape[0], h, w, bd, C.c_void_p(gw.data_ptr() if gw is not None else None),
                                  C.c_void_p(gx.data_ptr() if gx is not None else None), C.c_void_p(ws.data_ptr()), nbytes,
                                  L.current_stream())


def _autograd64(torch, d, mode, img, G, h, w):
    """float64 torch restatement of SRNet.forward + autograd: returns (y [P,oC,h,w], {layer: (gW, gb)}, g_img)"""
    P = img.shape[0]
    x = torch.tensor(img, dtype=torch.float64, requires_grad=True)
    t = torch.stack([x[:, dy:dy + h, dx:dx + w].reshape(-1) for dy, dx in PATTERN[mode]], dim=1)
    ps = []
    for name in LAYERS:
        W = torch.tensor(d["%s.model.%s.weight" % (KEY, name)], dtype=torch.float64, requires_grad=True)
        b = torch.tensor(d["%s.model.%s.bias" % (KEY, name)], dtype=torch.float64, requires_grad=True)
        ps.append((W, b))
    a = torch.relu(t @ ps[0][0].reshape(64, -1).T + ps[0][1])
    for W, b in ps[1:5]:
        a = torch.cat([a, torch.relu(a @ W.T + b)], dim=1)
    y = torch.tanh(a @ ps[5][0].T + ps[5][1])                      # [P*h*w, oC]
    y = y.reshape(P, h, w, -1).permute(0, 3, 1, 2)
    (y * torch.tensor(G, dtype=torch.float64)).sum().backward()
    return y.detach().numpy(), [(W.grad.numpy(), b.grad.numpy()) for W, b in ps], x.grad.numpy()


def _case(rng, mode, outC, P, h, w, extra):
    bd = REACH[mode] + extra
    img = rng.random((P, h + bd, w + bd)).astype(np.float32)
    return bd, img


@pytest.mark.parametrize("outC", [1, 2, 3])
@pytest.mark.parametrize("mode", list("sdyct"))
def test_forward_against_float64(torch, oracle, mode, outC):
    rng = np.random.default_rng(100 + 10 * outC + "sdyct".index(mode))
    d = _weights(rng, outC)
    flat = torch.tensor(_pack(d), device="cuda")
    for P, h, w, extra in ((3, 13, 17, 0), (2, 9, 31, 2), (1, 1, 1, 1)):
        bd, img = _case(rng, mode, outC, P, h, w, extra)
        rc, out = _fwd(torch, flat, outC, mode, torch.tensor(img, device="cuda"), h, w, bd)
        assert rc == 0
        y64, M6 = oracle.srnet_forward(d, KEY, _tuples(img, mode, h, w), absolute=True)
        u = 2.0 ** -24
        bound = 969 * u / (1 - 969 * u) * M6 + 2.0 ** -22
        got = out.cpu().numpy().transpose(0, 2, 3, 1).reshape(-1, outC)
        assert np.all(np.abs(got - y64) <= bound), (mode, outC, P, h, w, float(np.max(np.abs(got - y64))))


@pytest.mark.parametrize("mode,outC,P,h,w,extra", [("s", 3, 2, 11, 13, 0), ("d", 1, 1, 7, 9, 1), ("y", 2, 3, 10, 5, 0),
                                                  ("c", 3, 1, 33, 19, 2), ("t", 1, 2, 15, 15, 0),
                                                  ("c", 3, 3, 77, 75, 0)])      # 542 tiles: several tiles per slab
def test_backward_against_float64(torch, mode, outC, P, h, w, extra):
    rng = np.random.default_rng(300 + P * h * w)
    d = _weights(rng, outC)
    bd, img = _case(rng, mode, outC, P, h, w, extra)
    G = rng.standard_normal((P, outC, h, w)).astype(np.float32)
    flat = torch.tensor(_pack(d), device="cuda")
    gw = torch.zeros_like(flat)
    gx = torch.zeros((P, h + bd, w + bd), dtype=torch.float32, device="cuda")
    assert _bwd(torch, flat, outC, mode, torch.tensor(img, device="cuda"), torch.tensor(G, device="cuda"), h, w, bd, gw, gx) == 0
    _, grads, gimg = _autograd64(torch, d, mode, img, G, h, w)
    got = gw.cpu().numpy()
    off = 0
    for li, (gW, gb) in enumerate(grads):
        for ref in (gW.reshape(-1), gb):
            part = got[off:off + ref.size]
            off += ref.size
            scale = max(np.abs(ref).max(), 1e-30)
            assert np.max(np.abs(part - ref)) <= 1e-4 * scale, ("layer", li + 1, float(np.max(np.abs(part - ref)) / scale))
    assert off == got.size
    gxn = gx.cpu().numpy()
    assert np.max(np.abs(gxn - gimg)) <= 1e-4 * np.abs(gimg).max()
    assert np.all(gxn[gimg == 0] == 0)


def test_backward_contract(torch):
    """bitwise repeatable; accumulates into grad_weights / grad_img; NULL grad_img; workspace size; error codes"""
    L = __import__("lerf_pytorch_amd")._lib
    lib = L.lib()
    rng = np.random.default_rng(5)
    outC, mode, P, h, w = 3, "t", 2, 40, 23
    bd = REACH[mode]
    d = _weights(rng, outC)
    img = torch.tensor(rng.random((P, h + bd, w + bd)).astype(np.float32), device="cuda")
    G = torch.tensor(rng.standard_normal((P, outC, h, w)).astype(np.float32), device="cuda")
    flat = torch.tensor(_pack(d), device="cuda")
    nbytes = lib.lerf_srnet_bwd_workspace_bytes(outC, P, h, w)
    assert nbytes > 0
    runs = []
    for _ in range(2):
        gw, gx = torch.zeros_like(flat), torch.zeros_like(img)
        assert _bwd(torch, flat, outC, mode, img, G, h, w, bd, gw, gx) == 0
        runs.append((gw.cpu().numpy(), gx.cpu().numpy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    # accumulation into non-zero buffers
    gw0 = rng.standard_normal(flat.numel()).astype(np.float32)
    gx0 = rng.standard_normal(tuple(img.shape)).astype(np.float32)
    gw, gx = torch.tensor(gw0, device="cuda"), torch.tensor(gx0, device="cuda")
    assert _bwd(torch, flat, outC, mode, img, G, h, w, bd, gw, gx) == 0
    assert np.array_equal(gw.cpu().numpy(), gw0 + runs[0][0]) and np.array_equal(gx.cpu().numpy(), gx0 + runs[0][1])
    # NULL grad_img: the same weight gradient
    gw = torch.zeros_like(flat)
    assert _bwd(torch, flat, outC, mode, img, G, h, w, bd, gw, None) == 0
    assert np.array_equal(gw.cpu().numpy(), runs[0][0])
    # workspace one byte too small
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    assert _bwd(torch, flat, outC, mode, img, G, h, w, bd, gw, None, ws, nbytes - 1) == -1
    assert _bwd(torch, flat, outC, mode, img, G, h, w, bd, gw, None, ws, nbytes) == 0
    # bad mode, outC, bd
    assert _bwd(torch, flat, outC, "q", img, G, h, w, bd, gw, None) == -1
    assert _fwd(torch, flat, outC, "q", img, h, w, bd)[0] == -1
    assert _bwd(torch, flat, outC, mode, img, G, h + 1, w + 1, bd - 1, gw, None) == -1
    assert _fwd(torch, flat, outC, mode, img, h + 1, w + 1, bd - 1)[0] == -1
    for bad in (0, 5):
        assert lib.lerf_srnet_bwd_workspace_bytes(bad, P, h, w) == 0
        assert _bwd(torch, flat, bad, mode, img, G, h, w, bd, gw, None, ws, nbytes) == -2
        assert _fwd(torch, flat, bad, mode, img, h, w, bd)[0] == -2
    torch.cuda.synchronize()


def _opt(**kw):
    o = types.SimpleNamespace(nf=64, modes="sct", modes2="sct", stages=2, norm=255)
    o.__dict__.update(kw)
    return o


def _model(torch, name=None, seed=None):
    from lerf_pytorch_amd.resample.model import SRNetsSWF2
    if seed is not None:
        torch.manual_seed(seed)
    m = SRNetsSWF2(_opt(), inC=1, outC=1 if name == "lerf-l" else 3)
    if name is not None:
        m.load_state_dict({k: torch.from_numpy(v) for k, v in np.load(os.path.join(ASSETS, name, "srnets_weights.npz")).items()})
    return m.cuda()


@pytest.mark.parametrize("name", ["lerf-g", "lerf-l"])
def test_golden_parity_with_reference(torch, golden, name):
    import torch.nn.functional as F
    from lerf_pytorch_amd.resize_right.resize_right2d_torch import AmplifiedLinearResize2dTorch, SteeringGaussianResize2dTorch
    g = golden("g26_srnets.npz")
    p = name + "/"
    m = _model(torch, name)
    x = torch.tensor(g[p + "x"], device="cuda")
    lb = torch.tensor(g[p + "lb"], device="cuda")
    with torch.no_grad():                                       # the nets on the reference's rotation-0 inputs
        for key in ["s1_%sr0" % md for md in "sct"] + ["s2_%sr%d" % (md, r) for md in "sct" for r in (0, 1)]:
            stage, mode, r = int(key[1]), key[3], int(key[5])
            src = x if stage == 1 else torch.tensor(g[p + "s1"], device="cuda") / 255.0
            pad = REACH[mode]
            y = m(F.pad(src, (0, pad, 0, pad), mode="replicate"), stage, mode, r).cpu().numpy()
            assert np.max(np.abs(y - g[p + "net/" + key])) <= 2e-5, key
    ties = 0
    with torch.no_grad():
        s1 = m.predict(x, stage=1).cpu().numpy()
        s2 = m.predict(torch.tensor(g[p + "s1"], device="cuda") / 255.0, stage=2).cpu().numpy()
    # integer planes: s1 in 0..255, s2 * 255 (the division by norm itself may round differently on the device: 1 ulp)
    for got, ref, mul in ((s1, g[p + "s1"], 1.0), (s2, g[p + "s2"], 255.0)):
        assert np.max(np.abs(got * mul - np.round(got * mul))) <= 1e-4 and np.max(np.abs(ref * mul - np.round(ref * mul))) <= 1e-4
        diff = np.abs(np.round(got * mul) - np.round(ref * mul))
        assert diff.max() <= 1, name
        ties += int(np.sum(diff > 0))
        assert np.sum(diff > 0) <= 0.01 * diff.size, (name, int(np.sum(diff > 0)))
    print("%s: %d rounding ties in the predict planes" % (name, ties))
    feat = m.predict(x, stage=1)
    hyper = m.predict(feat / 255.0, stage=2)
    if name == "lerf-g":
        rz = SteeringGaussianResize2dTorch(support_sz=2, device=torch.device("cuda"), max_sigma=10)
        rz.set_shape([2, 1, 12, 12], scale_factors=2)
        pred = rz.resize(feat, hyper[:, :1], hyper[:, 1:2], hyper[:, 2:])
    else:
        rz = AmplifiedLinearResize2dTorch(support_sz=2, device=torch.device("cuda"))
        rz.set_shape([2, 1, 12, 12], scale_factors=2)
        pred = rz.resize(feat, hyper)
    loss = F.mse_loss(torch.clamp(pred, 0, 255) / 255.0, lb)
    loss.backward()
    assert abs(loss.item() - float(g[p + "loss"][0])) <= 1e-3 * float(g[p + "loss"][0])
    n = 0
    for pname, prm in m.named_parameters():
        idx, val = g[p + "grad/" + pname + "/idx"], g[p + "grad/" + pname + "/val"]
        got = prm.grad.reshape(-1).cpu().numpy()[idx]
        scale = max(np.abs(val).max(), 1e-12)
        assert np.max(np.abs(got - val)) <= 2e-3 * scale, (pname, float(np.max(np.abs(got - val)) / scale))
        n += 1
    assert n == 108


def test_weight_round_trip(torch, tmp_path):
    """shipped npz -> SRNetsSWF2 -> export_srnets -> transfer: byte-equal LUTs to transferring the shipped file"""
    from lerf_pytorch_amd.resample import transfer_to_lut as T
    from lerf_pytorch_amd.resample.model import export_srnets
    m = _model(torch, "lerf-g")
    path = export_srnets(m, str(tmp_path))
    assert path == os.path.join(str(tmp_path), "srnets_weights.npz")
    a = T.transfer(T.load_weights(str(tmp_path)))
    b = T.transfer(T.load_weights(os.path.join(ASSETS, "lerf-g")))
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)


def _set5_batch(torch):
    from PIL import Image
    lrs, hrs = [], []
    for n in ("baby", "bird", "head", "woman"):
        hr = np.array(Image.open(os.path.join(DATA, "HR", n + ".png")).convert("L")).astype(np.float32) / 255.0
        lr = np.array(Image.open(os.path.join(DATA, "LR_bicubic", "rrLR_X2.00_2.00", n + ".png")).convert("L")).astype(np.float32) / 255.0
        y, x = lr.shape[0] // 2 - 12, lr.shape[1] // 2 - 12
        lrs.append(lr[y:y + 24, x:x + 24])
        hrs.append(hr[2 * y:2 * y + 48, 2 * x:2 * x + 48])
    return (torch.tensor(np.stack(lrs)[:, None], device="cuda"), torch.tensor(np.stack(hrs)[:, None], device="cuda"))


def _train(torch, m, im, lb, steps, lr):
    from lerf_pytorch_amd.resample.model import lutft_step
    from lerf_pytorch_amd.resize_right.resize_right2d_torch import SteeringGaussianResize2dTorch
    r = SteeringGaussianResize2dTorch(support_sz=2, device=torch.device("cuda"), max_sigma=10)
    r.set_shape(list(im.shape), scale_factors=2)
    opt_G = torch.optim.Adam(m.parameters(), lr=lr, betas=(0.9, 0.999), eps=1e-8)
    return [float(lutft_step(m, r, im, lb, opt_G).detach()) for _ in range(steps)]


def test_end_to_end_training_transfer_and_sr(torch, tmp_path):
    """20 Adam steps of lutft_step from the shipped lerf-g nets on Set5 crops (x2), export, transfer, SR with the LUTs;
    the same from Kaiming initialisation lowers the loss"""
    import lerf_pytorch_amd as L
    from PIL import Image
    from lerf_pytorch_amd.resample import transfer_to_lut as T
    from lerf_pytorch_amd.resample.model import export_srnets
    im, lb = _set5_batch(torch)
    m = _model(torch, "lerf-g")
    losses = _train(torch, m, im, lb, 20, 1e-4)
    print("fine-tune losses", losses[0], losses[-1])
    assert all(np.isfinite(losses)) and losses[-1] <= losses[0], losses
    export_srnets(m, str(tmp_path))
    T.main(["-e", str(tmp_path)])
    eng = L.LerfEngine(L.LutSet.from_dir(str(tmp_path), linear=False, lut_name="LUT"))
    lr = np.array(Image.open(os.path.join(DATA, "LR_bicubic", "rrLR_X2.00_2.00", "baby.png")))
    hr = np.array(Image.open(os.path.join(DATA, "HR", "baby.png")))
    out = eng.sr(lr, 2)
    assert out.shape == (2 * lr.shape[0], 2 * lr.shape[1], 3)
    psnr = L.metrics.psnr_y(hr, out, 2)
    print("Set5 baby x2 PSNR with the transferred LUTs: %.2f dB" % psnr)
    assert np.isfinite(psnr) and psnr > 20
    k = _model(torch, None, seed=0)
    losses = _train(torch, k, im, lb, 20, 1e-3)
    print("from Kaiming initialisation", losses[0], losses[-1])
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
