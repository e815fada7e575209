"""CPU-only: the remap backward's C ABI surface, the anchoring of the restatement the GPU tests measure the map gradient against
(tests/remap_grad_ref.py), and the class surface that needs no device.

  1. lerf_remap_bwd is declared, exported, resolves and has argtypes;
  2. the restatement's forward equals the oracle's remap forward (the oracle with its geometry read from the map,
     remap_ref.map_geometry) to 1e-9 -- gauss and linear, S 2 and 4, the four pad modes, a smooth and a folded map;
  3. the restatement's autograd map gradient equals central finite differences (h = 1e-6) of that oracle forward at ~20 pixels
     per case chosen at least 1e-3 from every discontinuity.  Bound 1e-5 * max(|g|, 1): the truncation term is at most
     h^2 sigma^3 255 ~ 3e-7 at sigma = 10, the rounding term 255 * 2^-52 / h ~ 6e-8 -- more than an order below it;
  4. the new numpy / torch twins exist; the torch ones carry the opt-in switch (off by default).
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO

import lerf_pytorch_amd as L
from lerf_pytorch_amd import _lib

import remap_ref
import remap_grad_ref

IN_HW, OUT_HW = (40, 48), (33, 37)
FD_H, FD_MARGIN, FD_PIXELS = 1e-6, 1e-3, 20
MAPS = {"sinus": remap_ref.sinus_flow, "folded": remap_ref.folded}
CASES = [(kind, S, pad, name) for kind in ("gauss", "linear") for S in (2, 4)
         for pad in ("constant", "replicate", "reflect", "circular") for name in ("sinus", "folded")]


def test_remap_bwd_symbol_declared_exported_and_resolves():
    src = open(os.path.join(REPO, "include", "lerf_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(lerf_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(L.LIB_PATH)
    n = "lerf_remap_bwd"
    assert n in declared, "%s is not declared in include/lerf_hip.h" % n
    assert n in _lib.EXPORTS
    assert hasattr(lib, n), "liblerf_hip.so does not export %s" % n
    assert len(getattr(_lib.lib(), n).argtypes) == 17
    assert lib.lerf_abi_version() == 7


@pytest.fixture(scope="module")
def operands():
    """float32 planes shared by every case, computed once: image in [0, 255], hyper maps in [0, 1]"""
    rng = np.random.default_rng(11)
    x = (rng.random((2,) + IN_HW) * 255).astype(np.float32)
    hs = [rng.random((2,) + IN_HW).astype(np.float32) for _ in range(3)]
    G = rng.standard_normal((2,) + OUT_HW)
    return x, hs, G


def _oracle_forward(oracle, kind, S, pad, cm, x, hs, max_sigma):
    nh = 3 if kind == "gauss" else 1
    p = list(hs[:nh]) + [None] * (3 - nh)
    return oracle.warp_params_f32(x, p[0], p[1], p[2], cm, OUT_HW, S, max_sigma, kind, pad_mode=remap_grad_ref.NP_PAD[pad])


@pytest.mark.parametrize("kind,S,pad,name", CASES)
def test_restatement_forward_and_map_gradient(oracle, monkeypatch, operands, kind, S, pad, name):
    import torch
    monkeypatch.setattr(oracle, "warp_geometry", remap_ref.map_geometry)
    x, hs, G = operands
    max_sigma = 10 if kind == "gauss" else 1
    nh = 3 if kind == "gauss" else 1
    cm = MAPS[name](IN_HW, OUT_HW)
    geo = remap_ref.map_geometry(cm, IN_HW, OUT_HW, S)
    pads = (geo["pad"][0], geo["pad"][2])
    # ---- forward: restatement == oracle
    ref = _oracle_forward(oracle, kind, S, pad, cm, x, hs, max_sigma)
    ct = torch.tensor(cm, requires_grad=True)
    out = remap_grad_ref.restated_remap(kind, S, pad, ct, pads, torch.from_numpy(x), [torch.from_numpy(h) for h in hs[:nh]], max_sigma)
    np.testing.assert_allclose(out.detach().numpy(), ref, rtol=0, atol=1e-9, equal_nan=True)
    # ---- map gradient: autograd of the restatement == central differences of the oracle forward.  One entry moves one
    # output pixel, so all entries are moved at once, one coordinate at a time
    (out * torch.from_numpy(G)).sum().backward()
    g = ct.grad.numpy()
    fd = np.zeros_like(g)
    for k in range(2):
        e = np.zeros(2)
        e[k] = FD_H
        moved = []
        for sgn in (1, -1):
            m = cm + sgn * e
            m[0, 0] = cm[0, 0]                   # entry (0, 0) carries the pads: it stays, and is never among the chosen pixels
            assert remap_ref.map_geometry(m, IN_HW, OUT_HW, S)["pad"] == geo["pad"]
            moved.append(m)
        up = _oracle_forward(oracle, kind, S, pad, moved[0], x, hs, max_sigma)
        dn = _oracle_forward(oracle, kind, S, pad, moved[1], x, hs, max_sigma)
        fd[..., k] = (G * (up - dn)).sum(0) / (2 * FD_H)
    margin = remap_grad_ref.margins(kind, S, cm, pads, IN_HW)
    margin[0, 0] = 0.0
    margin[np.isnan(ref).any(0)] = 0.0           # a pixel whose weights all vanish (0 / 0) has no finite gradient to compare
    ok = np.argwhere(margin >= FD_MARGIN)
    assert len(ok) >= FD_PIXELS
    pick = ok[np.random.default_rng(S + len(name)).permutation(len(ok))[:FD_PIXELS]]
    assert all(margin[i, j] >= FD_MARGIN for i, j in pick)
    worst = 0.0
    for i, j in pick:
        for k in range(2):
            err, bound = abs(g[i, j, k] - fd[i, j, k]), 1e-5 * max(abs(g[i, j, k]), 1.0)
            worst = max(worst, err / bound)
            assert err <= bound, "pixel (%d, %d) coordinate %d: autograd %.12g, differences %.12g" % (i, j, k, g[i, j, k], fd[i, j, k])
    print("%s S=%d %s %s: worst error / bound = %.3g over %d pixels" % (kind, S, pad, name, worst, len(pick)))
    assert np.any(g[pick[:, 0], pick[:, 1]] != 0)


def test_fixed_kernel_derivative_conventions():
    """what autograd gives for the forms of interp_methods.py, which fixed_kernel_1d_deriv (csrc/lerf_taps.h) restates: |x|' at 0
    is 0, the hat's kink at 0 gives -1, the Lanczos quotient is smooth through 0, box has no gradient"""
    import torch
    from lerf_pytorch_amd.resize_right import interp_methods as im
    x = torch.tensor([0.0, -0.5, 0.5, 1.0, -1.0, 1.5], dtype=torch.float64, requires_grad=True)

    def d(f):
        y = f(x)
        if not y.requires_grad:
            return None
        return torch.autograd.grad(y.sum(), x)[0].numpy()
    assert d(im.cubic)[0] == 0.0
    np.testing.assert_allclose(d(im.cubic)[1:3], [1.375, -1.375], rtol=1e-15)         # sign(x) (4.5 a^2 - 5 a) at a = 0.5
    np.testing.assert_array_equal(d(im.linear), [-1.0, 1.0, -1.0, -1.0, 1.0, 0.0])
    assert d(im.lanczos2)[0] == 0.0 and d(im.lanczos3)[0] == 0.0
    assert d(im.box) is None


def test_new_twins_exist_and_backward_is_opt_in():
    from lerf_pytorch_amd.resize_right import resize_right2d_numpy as RN, resize_right2d_torch as RT
    from lerf_pytorch_amd import coords
    for name, S in (("Bilinear", 2), ("Lanczos2", 4), ("Lanczos3", 6)):
        for mod, suffix in ((RN, "Numpy"), (RT, "Torch")):
            cls = getattr(mod, name + "Remap2d" + suffix)
            twin = getattr(mod, name + "Warp2d" + suffix)
            assert cls().support_sz == twin().support_sz == S
    for name in ("Nearest", "SteeringGaussian", "AmplifiedLinear", "Bicubic", "Bilinear", "Lanczos2", "Lanczos3"):
        r = getattr(RT, name + "Remap2dTorch")()
        assert r._backward is False
        assert r.enable_backward() is r and r._backward is True
        assert getattr(RT, name + "Remap2dTorch")()._backward is False         # per instance, not per class
    import torch
    f = torch.zeros((5, 6, 2), dtype=torch.float64, requires_grad=True)
    m = coords.from_flow_torch(f)
    assert m.requires_grad and m.dtype == torch.float64 and tuple(m.shape) == (5, 6, 2)
    assert np.array_equal(m.detach().numpy(), coords.from_flow(np.zeros((5, 6, 2))))
    m[2, 3, 1].backward()
    assert float(f.grad[2, 3, 1]) == 1.0 and float(f.grad.abs().sum()) == 1.0
    assert coords.from_flow_torch(torch.zeros((5, 6, 2))).dtype == torch.float32
    with pytest.raises(ValueError):
        coords.from_flow_torch(np.zeros((5, 6, 2)))
    with pytest.raises(ValueError):
        coords.from_flow_torch(torch.zeros((5, 6)))
