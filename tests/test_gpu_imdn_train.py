"""Training LeRF-Net on the GPU (lerf_imdn_bwd.hip: lerf_imdn_fwd_train_f32 / lerf_imdn_bwd_f32, and
resample.model.IMDN2.enable_backward on top of them).

Tolerances.
  float64: per parameter tensor and for grad_x, e = max |t - t64| / max |t64| against float64 torch autograd on the CPU
    (imdn_grad_ref.net_grads, pinned to the reference by test_imdn_grad_cpu.py).  The same figure e_stock is taken for
    stock float32 torch autograd of imdn_ref64.torch_imdn_rtc on the GPU -- the reference's own arithmetic -- and the
    HIP backward must satisfy e_hip <= 4 e_stock + 1e-6: the factor 4 is the margin for another float32 summation order
    (slab split-K against MIOpen's) over at most 782 pixels (in this file: at most 25 tiles, one per slab;
    test_gpu_imdn_train_tiles.py has the batches of more tiles than slabs, up to 5 400 pixels, under the same rule) and
    28 convolutions.  So that the comparison means something,
    e_stock <= 1e-3 for every tensor, and with post != 0 no float64 raw output lies within 1e-4 of +-1 (no float32 run
    can flip the clamp mask); the seeds are chosen for that, and both are asserted.
  golden (g28_imdn_grads.npz, the reference's float32 CPU run of train_model.py:418-441): the terms of the same
    comparison in test_gpu_srnet.py: loss within 1e-3 relative, each recorded gradient within 2e-3 of its golden's
    largest entry.
  determinism, batch independence, fwd_train against fwd, no_grad against the inference path: bitwise.
"""
import ctypes as C
import os
import types

import numpy as np
import pytest

import imdn_grad_ref as GR
import imdn_ref64 as R

pytestmark = pytest.mark.gpu

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "Set5")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def _lib():
    return __import__("lerf_pytorch_amd")._lib


def _flat(torch, sd, prefix):
    return torch.from_numpy(np.concatenate([v.reshape(-1) for k, v in sd.items() if k.startswith(prefix)])).cuda()


def _unflat(sd, prefix, flat):
    """packed gradient -> {key: array}"""
    out, o = {}, 0
    for k in GR.net_keys(sd, prefix):
        out[k] = flat[o:o + sd[k].size].reshape(sd[k].shape)
        o += sd[k].size
    assert o == flat.size
    return out


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else None)


def _fwd_train(torch, flat, nf, in_nc, out_nc, xt, post, saved_bytes=None, out=None):
    """lerf_imdn_fwd_train_f32 -> (rc, out, saved)"""
    L = _lib()
    lib = L.lib()
    B, _, H, W = xt.shape
    need = lib.lerf_imdn_saved_bytes(nf, in_nc, out_nc, B, H, W)
    saved = torch.empty((max(need, 1),), dtype=torch.uint8, device="cuda")
    if out is None:
        out = torch.empty((B, out_nc, H, W), dtype=torch.float32, device="cuda")
    rc = lib.lerf_imdn_fwd_train_f32(_ptr(flat), nf, in_nc, out_nc, _ptr(xt), B, H, W, post, _ptr(saved),
                                     need if saved_bytes is None else saved_bytes, _ptr(out), L.current_stream())
    torch.cuda.synchronize()
    return rc, out, saved


def _bwd(torch, flat, nf, in_nc, out_nc, xt, post, saved, G, gw, gx, saved_bytes=None, ws_bytes=None):
    L = _lib()
    lib = L.lib()
    B, _, H, W = xt.shape
    need = lib.lerf_imdn_bwd_workspace_bytes(nf, in_nc, out_nc, B, H, W)
    ws = torch.empty((max(need, 1),), dtype=torch.uint8, device="cuda")
    rc = lib.lerf_imdn_bwd_f32(_ptr(flat), nf, in_nc, out_nc, _ptr(xt), B, H, W, post, _ptr(saved),
                               saved.numel() if saved_bytes is None else saved_bytes, _ptr(G), _ptr(gw), _ptr(gx), _ptr(ws),
                               need if ws_bytes is None else ws_bytes, L.current_stream())
    torch.cuda.synchronize()
    return rc


def _case(torch, nf, in_nc, out_nc, B, H, W, seed):
    sd = R.weight_rule(nf, in_nc, out_nc // in_nc, seed)
    rng = np.random.default_rng(seed + 1)
    x = (3 * rng.random((B, in_nc, H, W))).astype(np.float32)        # [0, 3): enough outputs leave [-1, 1] to exercise the mask
    G = rng.standard_normal((B, out_nc, H, W)).astype(np.float32)
    return sd, x, G


def _run(torch, sd, nf, in_nc, out_nc, x, G, post, want_gx=True):
    """forward + backward through the C ABI -> (out, packed gradient, grad_x) as tensors"""
    flat = _flat(torch, sd, "stage2.")
    xt, Gt = torch.from_numpy(x).cuda(), torch.from_numpy(G).cuda()
    rc, out, saved = _fwd_train(torch, flat, nf, in_nc, out_nc, xt, post)
    assert rc == 0
    gw = torch.full_like(flat, float("nan"))
    gx = torch.full_like(xt, float("nan")) if want_gx else None
    assert _bwd(torch, flat, nf, in_nc, out_nc, xt, post, saved, Gt, gw, gx) == 0
    return out, gw, gx


# nf, in_nc, out_nc, B, H, W, post, seed
CASES = [(16, 1, 1, 3, 1, 1, 0, 81),          # every tap but the centre is out of bounds
         (16, 3, 3, 2, 17, 23, 1, 82),        # 782 pixels: ragged tiles, an image boundary
         (32, 1, 3, 1, 33, 65, 2, 83),        # two column blocks
         (48, 3, 9, 1, 9, 40, 2, 114),         # three column blocks, r = 36
         (64, 3, 9, 2, 5, 7, 1, 85)]          # four column blocks


@pytest.mark.parametrize("cfg", CASES, ids=lambda c: "x".join(map(str, c[:7])))
def test_backward_matches_float64(torch, cfg):
    nf, in_nc, out_nc, B, H, W, post, seed = cfg
    sd, x, G = _case(torch, nf, in_nc, out_nc, B, H, W, seed)
    y64, g64, gx64 = GR.net_grads(torch, sd, "stage2.", x, G, post, torch.float64)
    if post:
        assert np.abs(np.abs(y64) - 1).min() > 1e-4, "a raw output within 1e-4 of +-1: choose another seed"
        assert 0.02 <= float((np.abs(y64) > 1).mean()) <= 0.5, "the clamp mask is not exercised: choose another seed"
    _, gs, gxs = GR.net_grads(torch, sd, "stage2.", x, G, post, torch.float32, "cuda")
    _, gw, gx = _run(torch, sd, nf, in_nc, out_nc, x, G, post)
    gh = _unflat(sd, "stage2.", gw.cpu().numpy())
    worst = (0.0, 0.0, "")
    fails = []
    for k, t, ts, t64 in [(k, gh[k], gs[k], g64[k]) for k in g64] + [("grad_x", gx.cpu().numpy(), gxs, gx64)]:
        e_hip, e_stock = GR.rel_err(t, t64), GR.rel_err(ts, t64)
        assert e_stock <= 1e-3, (k, e_stock)
        if e_hip > worst[0]:
            worst = (e_hip, e_stock, k)
        if not e_hip <= 4 * e_stock + 1e-6:
            fails.append((k, e_hip, e_stock))
    print("%s: worst e_hip %.3g (e_stock %.3g) at %s" % (cfg[:7], worst[0], worst[1], worst[2]))
    assert not fails, fails


def test_deterministic_and_batch_independent(torch):
    nf, in_nc, out_nc, B, H, W, post, seed = 32, 3, 3, 2, 19, 21, 1, 111
    sd, x, G = _case(torch, nf, in_nc, out_nc, B, H, W, seed)
    _, gw_a, gx_a = _run(torch, sd, nf, in_nc, out_nc, x, G, post)
    _, gw_b, gx_b = _run(torch, sd, nf, in_nc, out_nc, x, G, post)
    assert torch.equal(gw_a, gw_b) and torch.equal(gx_a, gx_b)
    assert bool(torch.isfinite(gw_a).all()) and bool(torch.isfinite(gx_a).all())
    _, _, gx_1 = _run(torch, sd, nf, in_nc, out_nc, x[1:2], G[1:2], post)
    assert torch.equal(gx_1[0], gx_a[1]), "grad_x of image 1 differs from the image run alone"


def test_contract(torch):
    L = _lib()
    lib = L.lib()
    nf, in_nc, out_nc, B, H, W, seed = 16, 3, 3, 2, 11, 18, 132
    sd, x, G = _case(torch, nf, in_nc, out_nc, B, H, W, seed)
    flat = _flat(torch, sd, "stage2.")
    xt, Gt = torch.from_numpy(x).cuda(), torch.from_numpy(G).cuda()
    # the saving forward's out is lerf_imdn_fwd_f32's, bit for bit
    for post in (0, 1, 2):
        nbytes = lib.lerf_imdn_workspace_bytes(nf, B, H, W)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
        ref = torch.empty((B, out_nc, H, W), dtype=torch.float32, device="cuda")
        assert lib.lerf_imdn_fwd_f32(_ptr(flat), nf, in_nc, out_nc, _ptr(xt), B, H, W, post, _ptr(ws), nbytes, _ptr(ref),
                                     L.current_stream()) == 0
        rc, out, _ = _fwd_train(torch, flat, nf, in_nc, out_nc, xt, post)
        assert rc == 0 and torch.equal(out, ref), post
    # unsupported configurations
    for bad in ((24, 3, 3), (16, 2, 3), (16, 3, 5)):
        assert lib.lerf_imdn_saved_bytes(*bad, B, H, W) == 0 and lib.lerf_imdn_bwd_workspace_bytes(*bad, B, H, W) == 0
        big = torch.empty((1 << 22,), dtype=torch.uint8, device="cuda")
        o = torch.empty((B, 9, H, W), dtype=torch.float32, device="cuda")
        assert lib.lerf_imdn_fwd_train_f32(_ptr(flat), *bad, _ptr(xt), B, H, W, 0, _ptr(big), big.numel(), _ptr(o),
                                           L.current_stream()) == -2
        assert lib.lerf_imdn_bwd_f32(_ptr(flat), *bad, _ptr(xt), B, H, W, 0, _ptr(big), big.numel(), _ptr(o), _ptr(flat.clone()),
                                     None, _ptr(big), big.numel(), L.current_stream()) == -2
    # invalid arguments leave sentinel-filled outputs untouched
    post = 2
    need = lib.lerf_imdn_saved_bytes(nf, in_nc, out_nc, B, H, W)
    sentinel = torch.full((B, out_nc, H, W), 7.0, device="cuda")
    rc, out, _ = _fwd_train(torch, flat, nf, in_nc, out_nc, xt, post, saved_bytes=need - 1, out=sentinel.clone())
    assert rc == -1 and torch.equal(out, sentinel)
    rc, out, _ = _fwd_train(torch, flat, nf, in_nc, out_nc, xt, 3, out=sentinel.clone())
    assert rc == -1 and torch.equal(out, sentinel)
    rc, out, saved = _fwd_train(torch, flat, nf, in_nc, out_nc, xt, post)
    assert rc == 0
    sw, sx = torch.full_like(flat, 7.0), torch.full_like(xt, 7.0)
    wneed = lib.lerf_imdn_bwd_workspace_bytes(nf, in_nc, out_nc, B, H, W)
    for kw in ({"saved_bytes": need - 1}, {"ws_bytes": wneed - 1}):
        gw, gx = sw.clone(), sx.clone()
        assert _bwd(torch, flat, nf, in_nc, out_nc, xt, post, saved, Gt, gw, gx, **kw) == -1
        assert torch.equal(gw, sw) and torch.equal(gx, sx)
    gw, gx = sw.clone(), sx.clone()
    assert _bwd(torch, flat, nf, in_nc, out_nc, xt, 3, saved, Gt, gw, gx) == -1
    assert torch.equal(gw, sw) and torch.equal(gx, sx)
    # overwritten and fully written: two different sentinels end in the same gradient; a null grad_x is accepted
    runs = []
    for fill, with_gx in ((7.0, True), (-3.0e30, False), (float("nan"), True)):
        gw = torch.full_like(flat, fill)
        gx = torch.full_like(xt, fill) if with_gx else None
        assert _bwd(torch, flat, nf, in_nc, out_nc, xt, post, saved, Gt, gw, gx) == 0
        runs.append((gw, gx))
    assert bool(torch.isfinite(runs[2][0]).all()) and bool(torch.isfinite(runs[2][1]).all())
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][0], runs[2][0]) and torch.equal(runs[0][1], runs[2][1])
    _, g64, gx64 = GR.net_grads(torch, sd, "stage2.", x, G, post, torch.float64)
    gh = _unflat(sd, "stage2.", runs[0][0].cpu().numpy())
    assert max(GR.rel_err(gh[k], g64[k]) for k in g64) <= 1e-4 and GR.rel_err(runs[0][1].cpu().numpy(), gx64) <= 1e-4


def _imdn2(torch, nf, sd=None, seed=None):
    from lerf_pytorch_amd.resample.model import IMDN2
    if seed is not None:
        torch.manual_seed(seed)
    m = IMDN2(types.SimpleNamespace(nf=nf, norm=255), inC=3, outC=3)
    if sd is not None:
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.cuda()


def test_enable_backward_switch(torch):
    m = _imdn2(torch, 16, seed=3)
    x = torch.rand((2, 3, 9, 11), device="cuda")
    assert m.enable_backward() is m and m.stage1.enable_backward() is m.stage1
    loss = (m.predict(x, stage=1) / 255.0).mean() + m.predict(x, stage=2).square().mean() + m.stage2(x).mean()
    loss.backward()
    for name, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name
    xr = x.clone().requires_grad_()
    m.predict(xr, stage=2).sum().backward()
    assert xr.grad is not None and float(xr.grad.abs().max()) > 0
    with torch.no_grad():
        on = [m.predict(x, stage=1), m.predict(x, stage=2)]
    assert not on[0].requires_grad
    m.enable_backward(False)
    with pytest.raises(NotImplementedError):
        m.predict(x, stage=1)
    with pytest.raises(NotImplementedError):
        m.stage2(x.clone().requires_grad_())
    with torch.no_grad():
        off = [m.predict(x, stage=1), m.predict(x, stage=2)]
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    # norm // 2 != 127 composes torch ops on the raw output
    m.norm = 100
    m.enable_backward()
    m.zero_grad()
    m.predict(x, stage=1).sum().backward()
    assert float(m.stage1.model[0].weight.grad.abs().max()) > 0


@pytest.mark.parametrize("c", ["a", "b"])
def test_golden_parity_with_reference(torch, golden, c):
    from lerf_pytorch_amd.resample.model import lutft_step
    from lerf_pytorch_amd.resize_right.resize_right2d_torch import SteeringGaussianResize2dTorch
    g = golden("g28_imdn_grads.npz")
    nf, inC, outC, B, H, W, seed = [int(v) for v in g[c + "/cfg"]]
    m = _imdn2(torch, nf, R.weight_rule(nf, inC, outC, seed)).enable_backward()
    im, lb = torch.tensor(g[c + "/im"], device="cuda"), torch.tensor(g[c + "/lb"], device="cuda")
    rz = SteeringGaussianResize2dTorch(support_sz=2, device=torch.device("cuda"), max_sigma=10)
    rz.set_shape([B, 1, H, W], scale_factors=2)
    loss = lutft_step(m, rz, im, lb, featC=3, inC=3)
    ref = float(g[c + "/loss"][0])
    print("case %s: loss %.7f, golden %.7f" % (c, loss.item(), ref))
    assert abs(loss.item() - ref) <= 1e-3 * ref
    n, worst = 0, (0.0, "")
    params = dict(m.named_parameters())
    for k in [k for k in g.files if k.startswith(c + "/grad/")]:
        val = g[k]
        got = params[k[len(c + "/grad/"):]].grad.cpu().numpy()
        e = float(np.abs(got - val).max() / max(np.abs(val).max(), 1e-12))
        worst = max(worst, (e, k))
        assert e <= 2e-3, (k, e)
        n += 1
    print("case %s: %d gradients, worst %.3g of the golden's max at %s" % (c, n, worst[0], worst[1]))
    assert n == (112 if c == "a" else 59)


def _set5_batch(torch):
    from PIL import Image
    lrs, hrs = [], []
    for n in ("baby", "bird", "head", "woman"):
        hr = np.array(Image.open(os.path.join(DATA, "HR", n + ".png")).convert("RGB")).astype(np.float32) / 255.0
        lr = np.array(Image.open(os.path.join(DATA, "LR_bicubic", "rrLR_X2.00_2.00", n + ".png")).convert("RGB")).astype(np.float32) / 255.0
        y, x = lr.shape[0] // 2 - 12, lr.shape[1] // 2 - 12
        lrs.append(lr[y:y + 24, x:x + 24].transpose(2, 0, 1))
        hrs.append(hr[2 * y:2 * y + 48, 2 * x:2 * x + 48].transpose(2, 0, 1))
    return torch.tensor(np.stack(lrs), device="cuda"), torch.tensor(np.stack(hrs), device="cuda")


def test_end_to_end_training_and_round_trip(torch, tmp_path):
    """8 Adam steps of lutft_step on Set5 crops (x2) from the default initialisation, then export_imdn2 -> load_imdn2"""
    from lerf_pytorch_amd.resample import model as M
    from lerf_pytorch_amd.resize_right.resize_right2d_torch import SteeringGaussianResize2dTorch
    im, lb = _set5_batch(torch)
    m = _imdn2(torch, 16, seed=0).enable_backward()
    r = SteeringGaussianResize2dTorch(support_sz=2, device=torch.device("cuda"), max_sigma=10)
    r.set_shape([im.shape[0], 1, im.shape[2], im.shape[3]], scale_factors=2)
    opt_G = torch.optim.Adam(m.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    losses = [float(M.lutft_step(m, r, im, lb, opt_G, featC=3, inC=3).detach()) for _ in range(8)]
    print("losses", losses[0], losses[-1])
    assert all(np.isfinite(losses)) and losses[-1] <= losses[0], losses
    m2 = M.load_imdn2(_imdn2(torch, 16, seed=1), M.export_imdn2(m, str(tmp_path))).cuda()
    with torch.no_grad():
        for stage in (1, 2):
            assert torch.equal(m.predict(im, stage=stage), m2.predict(im, stage=stage))
