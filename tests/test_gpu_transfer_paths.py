"""Net -> LUT transfer (lerf_transfer.hip: lerf_srnet_to_lut) at every interval and output channel count, with synthetic
SRNet weights, against the float64 oracle (oracle.srnet_forward) with a derived per-entry bound.

Bound.  The kernel evaluates, per tuple, conv1 as 4 float32 FMAs from the bias on inputs v / 255 rounded like the oracle's;
the dense layers 2..5 as K = 64, 128, 192, 256 term dot products on the matrix cores (float32 products and sums) plus
the bias; conv6 as 320 FMAs from the bias.  A K-term float32 dot product is within gamma_K * sum |w_i a_i| of the exact
one (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1), gamma_n = n u / (1 - n u),
u = 2^-24; ReLU is 1-Lipschitz, and an error in an activation reaches the pre-tanh sum through at most the absolute
weights of the later layers.  Every partial sum of the forward pass, carried forward through |W|, is bounded by M6,
the pre-tanh sum of the absolute network (oracle.srnet_forward(..., absolute=True)), so to first order

    |s_gpu - s| <= (gamma_5 + gamma_65 + gamma_129 + gamma_193 + gamma_257 + gamma_320) * M6 <= gamma_969 * M6 = bs

(layer 1 counts the input quotient as a fifth rounding; gamma_a + gamma_b <= gamma_{a+b} absorbs the second-order
terms).  tanh is 1-Lipschitz, and by the mean value theorem |tanh(s_gpu) - tanh(s)| <= bs * sech^2(max(|s| - bs, 0));
ocml's tanhf is within 2 ulp, and an ulp of |y| <= 1 is at most 2^-24, so 4 ulp are allowed:

    bound = bs * sech^2(max(|s| - bs, 0)) + 2^-22.

The LUT is rint(clip(y, -1, 1) * 127) with one more rounding of the product (127 u at most), so it equals
rint(clip(y64, -1, 1) * 127) except where y64 * 127 lies within 127 * bound + 127 u of a half-integer; there it may
differ by exactly 1.  M6 is large against |s| when the weights have both signs (the bound then covers every entry:
signed He weights below, reported, not relied on); the one-signed weight sets keep M6 within ~10 |s|, where the bound
is a few hundredths of a LUT step and pins all but a few per cent of the entries exactly."""
import os

import numpy as np
import pytest

from conftest import ASSETS

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LAYERS = ["conv1.conv", "conv2.conv1.conv", "conv3.conv1.conv", "conv4.conv1.conv", "conv5.conv1.conv", "conv6.conv"]
FAN = [4, 64, 128, 192, 256, 320]
GAMMA = 969 * U / (1 - 969 * U)
KEY = "s2_cr1"


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def synthetic(kind, outC, seed):
    """state_dict arrays of one SRNet under KEY (the names pack_srnet_weights reads):
    'he'   He-scaled Gaussian weights, small Gaussian biases;
    'pos'  one-signed He-scaled weights, non-positive hidden biases (ReLU still cuts), conv6 bias centring s near 0;
    'sat'  'pos' with conv6 scaled by 40: |s| >> 1, tanhf returns exactly +-1 on most entries;
    'dead' 'he' with conv1 killed by a bias of -50 and non-positive later biases: every activation is 0, s = b6."""
    from oracle import lerf_oracle as O
    rng = np.random.default_rng(seed)
    d = {}
    for li, nm in enumerate(LAYERS):
        n = outC if li == 5 else 64
        w = rng.standard_normal((n, FAN[li])) * np.sqrt(2.0 / FAN[li])
        b = rng.standard_normal(n) * 0.1
        if kind in ("pos", "sat"):
            w, b = np.abs(w) / np.sqrt(FAN[li]) * (4.0 if li == 5 else 1.0), -np.abs(b)
        if kind == "dead" and li < 5:
            b = np.full(n, -50.0) if li == 0 else -np.abs(b)
        shape = (n, 1, 2, 2) if li == 0 else (n, FAN[li], 1, 1)
        d["%s.model.%s.weight" % (KEY, nm)] = w.astype(np.float32).reshape(shape)
        d["%s.model.%s.bias" % (KEY, nm)] = b.astype(np.float32)
    if kind == "dead":
        d["%s.model.conv6.conv.bias" % KEY] = np.array([0.3, -1.7, 0.05, 2.5][:outC], np.float32)
    if kind in ("pos", "sat"):
        s = np.arctanh(O.srnet_forward(d, KEY, O.transfer_inputs(6)))
        b6 = d["%s.model.conv6.conv.bias" % KEY] - np.median(s, 0)
        if kind == "sat":
            d["%s.model.conv6.conv.weight" % KEY] = d["%s.model.conv6.conv.weight" % KEY] * np.float32(40)
            b6 = b6 * 40
        d["%s.model.conv6.conv.bias" % KEY] = b6.astype(np.float32)
    return d


def shipped_scaled(model, key, scale):
    """shipped weights of one SRNet, renamed to KEY, conv6 scaled: |s| >> 1 on many entries"""
    from lerf_pytorch_amd.resample import transfer_to_lut as T
    w = T.load_weights(os.path.join(ASSETS, model))
    d = {KEY + k[len(key):]: np.asarray(v) for k, v in w.items() if k.startswith(key + ".")}
    for nm in ("weight", "bias"):
        d["%s.model.conv6.conv.%s" % (KEY, nm)] = (d["%s.model.conv6.conv.%s" % (KEY, nm)] * np.float32(scale)).astype(np.float32)
    return d


def weights_of(spec):
    kind, outC, seed = spec
    if kind == "shipped":
        return shipped_scaled("lerf-g", "s2_tr1", 1.0) if seed == 0 else shipped_scaled("lerf-g", "s2_cr1", float(seed))
    return synthetic(kind, outC, seed)


def gpu_transfer(torch, w, interval):
    from lerf_pytorch_amd.resample import transfer_to_lut as T
    lut, y = T.srnet_to_lut(w, KEY, interval, return_float=True)
    torch.cuda.synchronize()
    return lut.cpu().numpy(), y.cpu().numpy()


def check_entries(lut, y, w, x, what):
    """the bars of the module docstring on the rows whose inputs are x; returns the count of rounding-ambiguous entries"""
    from oracle import lerf_oracle as O
    y64, M6 = O.srnet_forward(w, KEY, x, absolute=True)
    s64 = np.arctanh(np.clip(y64, -1 + 1e-16, 1 - 1e-16))
    bs = GAMMA * M6
    bound = bs / np.cosh(np.minimum(np.maximum(np.abs(s64) - bs, 0), 300)) ** 2 + 2.0 ** -22
    err = np.abs(y.astype(np.float64) - y64)
    assert np.all(err <= bound), "%s: %d entries outside the bound, worst excess %g" % (
        what, int((err > bound).sum()), float((err - bound).max()))
    q = np.clip(y64, -1, 1) * 127
    want = np.round(q)
    amb = np.abs(q - np.floor(q) - 0.5) <= 127 * bound + 127 * U
    d = lut.astype(np.int64) - want
    assert np.all(d[~amb] == 0), "%s: %d unambiguous entries differ" % (what, int((d[~amb] != 0).sum()))
    assert np.all(np.abs(d[amb]) <= 1), what
    print("%s: %d of %d entries within the rounding-ambiguity band (%d differ by 1)" % (
        what, int(amb.sum()), amb.size, int((d != 0).sum())))
    return int(amb.sum()), y64


# (interval, weight spec (kind, outC, seed)); every interval's L^4 leaves a partial last workgroup of 64 rows
FULL = []
for _iv, _oc in ((5, 4), (6, 2), (7, 3)):
    FULL += [(_iv, ("he", _oc, _iv)), (_iv, ("pos", 3, _iv)), (_iv, ("pos", 1, 10 + _iv)), (_iv, ("sat", 2, _iv)),
             (_iv, ("dead", 4, _iv)), (_iv, ("shipped", 3, 30))]
FULL += [(4, ("he", 2, 4)), (4, ("he", 4, 4)), (4, ("pos", 2, 4)), (4, ("pos", 4, 14)), (4, ("sat", 4, 24))]


@pytest.mark.parametrize("interval,spec", FULL, ids=["i%d-%s%d-%d" % ((iv,) + sp) for iv, sp in FULL])
def test_every_entry_against_float64(torch, oracle, interval, spec):
    kind, outC, _ = spec
    w = weights_of(spec)
    lut, y = gpu_transfer(torch, w, interval)
    n = (2 ** (8 - interval) + 1) ** 4
    assert lut.shape == (n, outC) and lut.dtype == np.int8 and y.shape == (n, outC)
    x = oracle.transfer_inputs(interval)
    n_amb, y64 = check_entries(lut, y, w, x, "interval %d %s outC %d" % (interval, kind, outC))
    if kind in ("pos", "sat"):
        assert n_amb <= 0.1 * lut.size                       # the bound is tight here: the comparison has teeth
    if kind == "sat":
        sat = np.abs(y64) >= 1 - 1e-12                         # |s| > 14: tanhf is exactly +-1 whatever the rounding
        assert sat.mean() > 0.3
        assert np.all(np.abs(y[sat]) == 1.0) and np.all(np.abs(lut[sat]) == 127)
    if kind == "dead":
        b6 = w["%s.model.conv6.conv.bias" % KEY]
        assert np.all(lut == np.round(np.tanh(b6.astype(np.float64)) * 127).astype(np.int8)[None, :])
        assert np.all(y == y[0][None, :])


@pytest.mark.parametrize("spec", [("shipped", 3, 0), ("pos", 1, 3)], ids=["shipped-s2_tr1", "pos1"])
def test_interval_3_sampled(torch, oracle, spec):
    """interval 3 (33^4 = 1.19 M entries): the GPU computes all of them, the oracle a seeded subset -- the first two and the
    last two workgroups, both rows at a sample of workgroup boundaries, and 50 000 random entries"""
    w = weights_of(spec)
    lut, y = gpu_transfer(torch, w, 3)
    n = 33 ** 4
    assert lut.shape == (n, spec[1])
    rng = np.random.default_rng(33)
    edges = np.concatenate([np.arange(128), np.arange(n - 128, n)])
    bnd = rng.choice(np.arange(1, n // 64 + 1), 400, replace=False) * 64
    idx = np.unique(np.concatenate([edges, bnd - 1, bnd[bnd < n], rng.integers(0, n, 50000)]))
    x = oracle.transfer_inputs(3)[idx]
    check_entries(lut[idx], y[idx], w, x, "interval 3 %s (%d sampled entries)" % (spec[0], idx.size))


@pytest.mark.parametrize("interval,spec", [(5, ("pos", 3, 40)), (6, ("pos", 1, 41))], ids=["i5-oC3", "i6-oC1"])
def test_transferred_lut_drives_four_simplex_interp(torch, oracle, interval, spec):
    """the deploy path at a non-default interval: a LUT transferred at `interval` through FourSimplexInterpFaster equals
    the oracle's integer 4-simplex numerators / 2^interval with the same LUT"""
    from lerf_pytorch_amd.resample.eval_lut_sr import FourSimplexInterpFaster, mode_pad_dict
    lut, _ = gpu_transfer(torch, weights_of(spec), interval)
    oC = spec[1]
    rng = np.random.default_rng(interval)
    img = rng.integers(0, 256, (37, 45, 2)).astype(np.float32)
    img[:3, :5] = 255
    for mode in "sct":
        pad = mode_pad_dict[mode]
        img_in = np.pad(img, ((0, pad), (0, pad), (0, 0)), mode="edge").transpose((2, 0, 1))
        out = FourSimplexInterpFaster(lut.astype(np.float32), img_in, 37, 45, interval, 4, upscale=1, mode=mode, oC=oC)
        num = oracle.lut_interp_numer(lut, img, mode, 0, interval).transpose(2, 3, 0, 1).reshape(2 * oC, 37, 45)
        assert np.array_equal(np.asarray(out), num / float(2 ** interval)), mode
