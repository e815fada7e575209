"""LeRF-Net on the GPU (lerf_imdn.hip: lerf_imdn_fwd_f32, and resample.model.IMDN2 on top of it), against the float64
restatement in imdn_ref64.py, against the reference's own IMDN2 (tests/golden/g27_imdn.npz) and against stock PyTorch
convolutions.

Tolerances.
  float64: the raw output within 1e-4 * max(1, max|y64|).  Every conv is a float32 dot product of up to 576 terms
    (exact products, float32 sums), 27 of them in sequence with residual adds; the relative error that reaches the output
    is a few 1e-6 in practice, so 1e-4 leaves a wide margin, while a wrong tap, channel offset, split or residual is off
    by O(1e-2) or more.  post 1 scales that bound by 127 (plus one float32 ulp of 254), post 2 by 1/2.
  golden: the raw outputs within 2e-5 (float32 against the reference's float32 CPU convolutions), p1 within 127 * 2e-5,
    p2 (computed on the golden p1) within 1e-5.
  stock torch: within 1e-3 * max(1, max|y|) (MIOpen may pick Winograd or FFT convolutions, whose rounding differs).
  batch independence and run-to-run: bitwise.
"""
import ctypes as C
import types

import numpy as np
import pytest

import imdn_ref64 as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def _lib():
    return __import__("lerf_pytorch_amd")._lib


def _flat(torch, sd, prefix):
    return torch.from_numpy(np.concatenate([v.reshape(-1) for k, v in sd.items() if k.startswith(prefix)])).cuda()


def _fwd(torch, flat, nf, in_nc, out_nc, x, post=0, ws_bytes=None, out=None):
    """lerf_imdn_fwd_f32 on a numpy or cuda x -> (rc, out tensor)"""
    L = _lib()
    lib = L.lib()
    xt = torch.as_tensor(x, dtype=torch.float32).cuda().contiguous()
    B, _, H, W = xt.shape
    need = lib.lerf_imdn_workspace_bytes(nf, B, H, W)
    nbytes = need if ws_bytes is None else ws_bytes
    ws = torch.empty((max(need, 1),), dtype=torch.uint8, device="cuda")
    if out is None:
        out = torch.empty((B, out_nc, H, W), dtype=torch.float32, device="cuda")
    rc = lib.lerf_imdn_fwd_f32(C.c_void_p(flat.data_ptr()), nf, in_nc, out_nc, C.c_void_p(xt.data_ptr()), B, H, W, post,
                               C.c_void_p(ws.data_ptr()), nbytes, C.c_void_p(out.data_ptr()), L.current_stream())
    torch.cuda.synchronize()
    return rc, out


SHAPES = [(64, 3, 3, 2, 17, 23), (16, 1, 3, 1, 33, 65), (64, 3, 1, 1, 1, 1), (16, 3, 3, 1, 40, 9), (64, 3, 3, 1, 130, 257)]


@pytest.mark.parametrize("cfg", SHAPES, ids=lambda c: "x".join(map(str, c)))
def test_forward_matches_float64(torch, cfg):
    nf, inC, outC, B, H, W = cfg
    sd = R.weight_rule(nf, inC, outC, 31)
    x = np.random.default_rng(32).random((B, inC, H, W)).astype(np.float32)
    for stage, out_nc in ((1, inC), (2, inC * outC)):
        prefix = "stage%d." % stage
        y64 = R.imdn_rtc(sd, prefix, x)
        tol = 1e-4 * max(1.0, float(np.abs(y64).max()))
        flat = _flat(torch, sd, prefix)
        rc, y = _fwd(torch, flat, nf, inC, out_nc, x, 0)
        assert rc == 0
        err = np.abs(y.cpu().numpy().astype(np.float64) - y64).max()
        assert err <= tol, "stage %d raw: max |dy| %.3g > %.3g" % (stage, err, tol)
        rc, p = _fwd(torch, flat, nf, inC, out_nc, x, stage)
        assert rc == 0
        scale = 127.0 if stage == 1 else 0.5
        err = np.abs(p.cpu().numpy().astype(np.float64) - R.post(y64, stage)).max()
        assert err <= scale * tol + 2 ** -16, "stage %d post: max |dp| %.3g" % (stage, err)


@pytest.mark.parametrize("i", range(4))
def test_reference_golden(torch, golden, i):
    g = golden("g27_imdn.npz")
    nf, inC, outC, B, H, W, seed = [int(v) for v in g["%d/cfg" % i]]
    sd = R.weight_rule(nf, inC, outC, seed)
    x = g["%d/x" % i]
    f1, f2 = _flat(torch, sd, "stage1."), _flat(torch, sd, "stage2.")
    _, y1 = _fwd(torch, f1, nf, inC, inC, x)
    _, y2 = _fwd(torch, f2, nf, inC, inC * outC, x)
    assert np.abs(y1.cpu().numpy() - g["%d/y1" % i]).max() <= 2e-5
    assert np.abs(y2.cpu().numpy() - g["%d/y2" % i]).max() <= 2e-5
    from lerf_pytorch_amd.resample.model import IMDN2
    m = IMDN2(types.SimpleNamespace(nf=nf, norm=255), inC=inC, outC=outC)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m.cuda()
    with torch.no_grad():
        p1 = m.predict(torch.from_numpy(x).cuda(), stage=1)
        p2 = m.predict(torch.from_numpy(g["%d/p1" % i]).cuda() / 255.0, stage=2)
    assert np.abs(p1.cpu().numpy() - g["%d/p1" % i]).max() <= 127 * 2e-5
    assert np.abs(p2.cpu().numpy() - g["%d/p2" % i]).max() <= 1e-5


def test_batch_independent_and_deterministic(torch):
    nf, inC, outC = 32, 3, 3
    sd = R.weight_rule(nf, inC, outC, 41)
    flat = _flat(torch, sd, "stage2.")
    x = np.random.default_rng(42).random((3, inC, 37, 29)).astype(np.float32)
    _, a = _fwd(torch, flat, nf, inC, inC * outC, x, 2)
    _, b = _fwd(torch, flat, nf, inC, inC * outC, x, 2)
    assert torch.equal(a, b)
    for k in range(3):
        _, s = _fwd(torch, flat, nf, inC, inC * outC, x[k:k + 1], 2)
        assert torch.equal(s[0], a[k]), "image %d of the batch differs from the image run alone" % k


def test_matches_stock_torch(torch):
    nf, inC, outC = 64, 3, 3
    sd = R.weight_rule(nf, inC, outC, 51)
    x = torch.rand((1, inC, 256, 256), generator=torch.Generator().manual_seed(52)).cuda()
    sdt = {k: torch.from_numpy(v).cuda() for k, v in sd.items()}
    for stage, out_nc in ((1, inC), (2, inC * outC)):
        prefix = "stage%d." % stage
        with torch.no_grad():
            ref = R.torch_imdn_rtc(sdt, prefix, x)
        _, y = _fwd(torch, _flat(torch, sd, prefix), nf, inC, out_nc, x)
        tol = 1e-3 * max(1.0, float(ref.abs().max()))
        assert float((y - ref).abs().max()) <= tol


def test_unsupported_and_invalid(torch):
    lib = _lib().lib()
    x = np.random.default_rng(0).random((1, 3, 8, 8)).astype(np.float32)
    sd = R.weight_rule(16, 3, 3, 61)
    flat = _flat(torch, sd, "stage1.")
    assert lib.lerf_imdn_weight_floats(24, 3, 3) == 0 and lib.lerf_imdn_weight_floats(16, 2, 3) == 0
    assert lib.lerf_imdn_weight_floats(16, 3, 3) == flat.numel()
    assert _fwd(torch, flat, 24, 3, 3, x, ws_bytes=1 << 20)[0] == -2
    assert _fwd(torch, flat, 16, 2, 3, x[:, :2], ws_bytes=1 << 20)[0] == -2
    assert _fwd(torch, flat, 16, 3, 5, x, ws_bytes=1 << 20)[0] == -2
    sentinel = torch.full((1, 3, 8, 8), 7.0, device="cuda")
    need = lib.lerf_imdn_workspace_bytes(16, 1, 8, 8)
    rc, out = _fwd(torch, flat, 16, 3, 3, x, ws_bytes=need - 1, out=sentinel.clone())
    assert rc == -1 and torch.equal(out, sentinel)
    rc, out = _fwd(torch, flat, 16, 3, 3, x, post=3, out=sentinel.clone())
    assert rc == -1 and torch.equal(out, sentinel)
    rc, out = _fwd(torch, flat, 16, 3, 3, x, out=sentinel.clone())
    assert rc == 0 and not torch.equal(out, sentinel)


def test_autograd_is_refused(torch):
    from lerf_pytorch_amd.resample.model import IMDN2
    m = IMDN2(types.SimpleNamespace(nf=16, norm=255), inC=3, outC=3).cuda()
    x = torch.rand((1, 3, 8, 8), device="cuda")
    with pytest.raises(NotImplementedError):
        m.predict(x, stage=1)
    with pytest.raises(NotImplementedError):
        m.stage2(x.requires_grad_())
    with torch.no_grad():
        assert m.predict(x, stage=2).shape == (1, 9, 8, 8)


def test_load_state_dict_from_golden_keys(torch, golden, tmp_path):
    from lerf_pytorch_amd.resample import model as M
    g = golden("g27_imdn.npz")
    nf, inC, outC = 16, 1, 3
    names = [s.split(":")[0] for s in g["keys/%d/%d/%d" % (nf, inC, outC)]]
    sd = R.weight_rule(nf, inC, outC, 71)
    assert list(sd) == names
    m = M.IMDN2(types.SimpleNamespace(nf=nf, norm=255), inC=inC, outC=outC)
    m.load_state_dict({k: torch.from_numpy(sd[k]) for k in names}, strict=True)
    m2 = M.load_imdn2(M.IMDN2(types.SimpleNamespace(nf=nf, norm=255), inC=inC, outC=outC), M.export_imdn2(m, str(tmp_path)))
    torch.save(m.state_dict(), str(tmp_path / "Model_000001.pth"))
    m3 = M.load_imdn2(M.IMDN2(types.SimpleNamespace(nf=nf, norm=255), inC=inC, outC=outC), str(tmp_path / "Model_000001.pth"))
    x = torch.rand((1, 1, 21, 19), device="cuda")
    with torch.no_grad():
        outs = [mm.cuda().predict(x, stage=2) for mm in (m, m2, m3)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
