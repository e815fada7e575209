"""The error-bound material of the float64 oracle (CPU only): the per-entry term counts and magnitude sums of
oracle.swf2lut_interp(..., bounds=True), and the absolute network of oracle.srnet_forward(..., absolute=True).  The GPU
tests of the fine-tuning and transfer kernels (tests/test_gpu_train_paths.py, tests/test_gpu_transfer_paths.py) scale
their per-entry tolerances with these, so they are pinned here against brute-force restatements."""
import numpy as np
import pytest

L4 = 17 ** 4
STRIDES = (17 ** 3, 17 ** 2, 17, 1)
PATTERN = {"s": ((0, 0), (0, 1), (1, 0), (1, 1)), "d": ((0, 0), (0, 2), (2, 0), (2, 2)),
           "y": ((0, 0), (1, 1), (1, 2), (2, 1)), "c": ((0, 0), (0, 1), (0, 2), (0, 3)),
           "t": ((0, 0), (1, 1), (2, 2), (3, 3))}
LSB_MODE = {"s": "s", "d": "d", "y": "y", "c": "y", "t": "y"}
PAD = {"s": 1, "d": 2, "y": 2, "c": 3, "t": 3}


def _brute(weight, outC, mode, img, bd, G):
    """pixel by pixel: the 4-simplex walk of one pixel and every term it contributes (float64 Python loops)"""
    B, Cn, hp, wp = img.shape
    h, w = hp - bd, wp - bd
    rq = np.round(weight.astype(np.float32) * np.float32(127))
    P = np.clip(rq, -127, 127).astype(np.float64)
    gate = (rq >= -127) & (rq <= 127)
    gw, gw_n, gw_a = (np.zeros(weight.shape) for _ in range(3))
    gi, gi_n, gi_a = (np.zeros(img.shape) for _ in range(3))
    pm, pl = PATTERN[mode], PATTERN[LSB_MODE[mode]]
    for b in range(B):
        for c in range(Cn):
            for y in range(h):
                for x in range(w):
                    m = [int(img[b, c, y + dy, x + dx]) // 16 for dy, dx in pm]
                    f = [int(img[b, c, y + dy, x + dx]) % 16 for dy, dx in pl]
                    axes = sorted(range(4), key=lambda k: (f[k], k), reverse=True)       # later axis first on ties
                    fs = [f[k] for k in axes] + [0]
                    idx = [sum(m[k] * STRIDES[k] for k in range(4))]
                    for k in axes:
                        idx.append(idx[-1] + STRIDES[k])
                    wts = [16 - fs[0]] + [fs[n] - fs[n + 1] for n in range(4)]
                    g = [float(G[b, c * outC + oc, y, x]) / 16 for oc in range(outC)]
                    for n in range(5):
                        for oc in range(outC):
                            if wts[n] != 0 and gate[idx[n], oc]:
                                t = g[oc] * wts[n] * 127
                                gw[idx[n], oc] += t
                                gw_n[idx[n], oc] += 1
                                gw_a[idx[n], oc] += abs(t)
                    for n in range(4):
                        ly, lx = pl[axes[n]]
                        for oc in range(outC):
                            t = g[oc] * (P[idx[n + 1], oc] - P[idx[n], oc])
                            gi[b, c, y + ly, x + lx] += t
                            gi_n[b, c, y + ly, x + lx] += 1
                            gi_a[b, c, y + ly, x + lx] += abs(t)
    return gw, gi, {"gw_count": gw_n, "gw_abs": gw_a, "gimg_count": gi_n, "gimg_abs": gi_a}


def _weights(rng, outC):
    return np.clip(rng.standard_normal((L4, outC)).astype(np.float32) * 0.5, -1.3, 1.3)      # straddles the clamp gate


def _monotone_weights(outC):
    """a LUT non-decreasing along every axis: P(a,b,c,d) = clip(round(127 (a+b+c+d)/32 - 127)), so P_{n+1} >= P_n"""
    a = np.stack(np.meshgrid(*([np.arange(17)] * 4), indexing="ij"), -1).reshape(-1, 4).sum(1)
    w = (a / 32.0 - 1.0).astype(np.float32)
    return np.repeat(w[:, None], outC, 1) * np.linspace(1.0, 1.2, outC, dtype=np.float32)


@pytest.mark.parametrize("mode,outC,shape,bd_extra", [("s", 1, (1, 1, 3, 4), 0), ("t", 3, (1, 2, 2, 3), 1),
                                                      ("c", 3, (2, 1, 3, 2), 0), ("y", 1, (1, 1, 1, 5), 2),
                                                      ("d", 3, (1, 1, 4, 3), 0)])
def test_counts_and_sums_match_brute_force(oracle, mode, outC, shape, bd_extra):
    rng = np.random.default_rng(ord(mode) + outC)
    bd = PAD[mode] + bd_extra
    B, Cn, h, w = shape
    img = rng.integers(0, 256, (B, Cn, h + bd, w + bd)).astype(np.float32)
    img[0, 0, 0, :] = 255                                                                   # ties and the top corner
    wt = _weights(rng, outC)
    G = rng.standard_normal((B, Cn * outC, h, w)).astype(np.float32)
    _, gw, gi, st = oracle.swf2lut_interp(wt, outC, mode, img, bd, G, bounds=True)
    bgw, bgi, bst = _brute(wt, outC, mode, img, bd, G)
    np.testing.assert_allclose(gw, bgw, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(gi, bgi, rtol=1e-12, atol=1e-12)
    for k in ("gw_count", "gimg_count"):
        assert np.array_equal(st[k], bst[k]), k
    for k in ("gw_abs", "gimg_abs"):
        np.testing.assert_allclose(st[k], bst[k], rtol=1e-12, atol=0)
    # no term -> exactly zero, in both the gradients and the magnitude sums
    assert np.all(gw[st["gw_count"] == 0] == 0) and np.all(st["gw_abs"][st["gw_count"] == 0] == 0)
    assert np.all(gi[st["gimg_count"] == 0] == 0) and np.all(st["gimg_abs"][st["gimg_count"] == 0] == 0)
    if bd_extra:                                                                          # rows / columns past the reach
        assert np.all(st["gimg_count"][:, :, -bd_extra:, :] == 0) and np.all(st["gimg_count"][:, :, :, -bd_extra:] == 0)


@pytest.mark.parametrize("mode,outC", [("s", 3), ("c", 1), ("t", 3), ("d", 1), ("y", 3)])
def test_abs_sum_dominates_and_is_tight_for_one_signed_terms(oracle, mode, outC):
    rng = np.random.default_rng(11 + ord(mode))
    bd = PAD[mode]
    img = rng.integers(0, 256, (2, 1, 9 + bd, 13 + bd)).astype(np.float32)
    G = rng.standard_normal((2, outC, 9, 13)).astype(np.float32)
    _, gw, gi, st = oracle.swf2lut_interp(_weights(rng, outC), outC, mode, img, bd, G, bounds=True)
    assert np.all(st["gw_abs"] >= np.abs(gw)) and np.all(st["gimg_abs"] >= np.abs(gi))
    assert np.any(st["gw_abs"] > np.abs(gw) * (1 + 1e-9))                                 # mixed signs: strictly larger somewhere
    # G >= 0 and a monotone LUT: every term of every entry has the same sign, so the magnitude sum is the gradient itself
    Gp = np.abs(G)
    _, gw, gi, st = oracle.swf2lut_interp(_monotone_weights(outC), outC, mode, img, bd, Gp, bounds=True)
    np.testing.assert_allclose(st["gw_abs"], gw, rtol=1e-12, atol=0)
    np.testing.assert_allclose(st["gimg_abs"], gi, rtol=1e-12, atol=0)
    assert gi.max() > 0 and gw.max() > 0


def test_bounds_option_leaves_the_results_alone(oracle):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (1, 2, 8, 11)).astype(np.float32)
    wt = _weights(rng, 3)
    G = rng.standard_normal((1, 6, 7, 10)).astype(np.float32)
    a = oracle.swf2lut_interp(wt, 3, "s", img, 1, G)
    b = oracle.swf2lut_interp(wt, 3, "s", img, 1, G, bounds=True)
    assert len(a) == 3 and len(b) == 4
    for x, y in zip(a, b[:3]):
        assert np.array_equal(x, y)


def _srnet(rng, key, outC, nonneg=False):
    d, p, fan = {}, key + ".model.", [4, 64, 128, 192, 256, 320]
    names = ["conv1.conv", "conv2.conv1.conv", "conv3.conv1.conv", "conv4.conv1.conv", "conv5.conv1.conv", "conv6.conv"]
    for li, nm in enumerate(names):
        n_out = outC if li == 5 else 64
        w = rng.standard_normal((n_out, fan[li])) * np.sqrt(2.0 / fan[li])
        b = rng.standard_normal(n_out) * 0.1
        if nonneg:
            w, b = np.abs(w) * 0.05, np.abs(b) * 0.05
        d[p + nm + ".weight"] = w.astype(np.float32).reshape((n_out, 1, 2, 2) if li == 0 else (n_out, fan[li], 1, 1))
        d[p + nm + ".bias"] = b.astype(np.float32)
    return d


def test_absolute_network_equals_plain_for_nonnegative_weights(oracle):
    rng = np.random.default_rng(3)
    w = _srnet(rng, "s2_cr1", 3, nonneg=True)
    x = oracle.transfer_inputs(6)
    y, M6 = oracle.srnet_forward(w, "s2_cr1", x, absolute=True)
    assert np.array_equal(y, oracle.srnet_forward(w, "s2_cr1", x))
    np.testing.assert_allclose(np.tanh(M6), y, rtol=1e-13, atol=0)        # no ReLU is active: |s| = s = M6


def test_absolute_network_dominates(oracle):
    rng = np.random.default_rng(4)
    w = _srnet(rng, "s1_sr0", 2)
    x = oracle.transfer_inputs(6)
    y, M6 = oracle.srnet_forward(w, "s1_sr0", x, absolute=True)
    s = np.arctanh(np.clip(y, -1 + 1e-15, 1 - 1e-15))
    assert M6.shape == y.shape and np.all(M6 >= np.abs(s) * (1 - 1e-9))
    assert np.median(M6 / np.maximum(np.abs(s), 1e-12)) > 1.5                    # signed weights: strictly looser
