"""Float64 numpy restatement of the reference's IMDN_RTC / IMDN2 (resample/model.py:434-545) at upscale 1, and the
seeded weight rule of tests/golden/gen_imdn_golden.py (a helper for test_imdn_cpu.py and test_gpu_imdn.py, not a test);
hazards() measures on the same net how close a batch comes to the thresholds of the backward (imdn_grad_ref.py).

Every convolution is zero-padded by (k-1)/2 (PyTorch's Conv2d with padding=(k-1)/2); activations run NHWC in float64."""
import hashlib

import numpy as np

GAIN = 0.5          # weight = normal * GAIN * sqrt(2 / fan_in): keeps most pre-clamp outputs of the 5-module net in (-1, 1)
BIAS_STD = 0.02
MODULES = 5


def state_keys(nf, in_nc, out_nc):
    """[(key, shape)] of one IMDN_RTC in state_dict order (model.0, model.1.sub.{0..4}.c{1..5}, model.1.sub.5, model.2)"""
    d = nf // 4
    r = nf - d
    convs = [("model.0", nf, in_nc, 3)]
    for m in range(MODULES):
        p = "model.1.sub.%d." % m
        convs += [(p + "c1", nf, nf, 3), (p + "c2", nf, r, 3), (p + "c3", nf, r, 3), (p + "c4", d, r, 3), (p + "c5", nf, 4 * d, 1)]
    convs += [("model.1.sub.5", nf, nf, 1), ("model.2", out_nc, nf, 3)]
    out = []
    for name, co, ci, k in convs:
        out += [(name + ".weight", (co, ci, k, k)), (name + ".bias", (co,))]
    return out


def imdn2_keys(nf, inC, outC):
    return ([("stage1." + k, s) for k, s in state_keys(nf, inC, inC)] +
            [("stage2." + k, s) for k, s in state_keys(nf, inC, inC * outC)])


def weight_rule(nf, inC, outC, seed):
    """{key: float32 array} of an IMDN2: keys in state_dict order from one default_rng(seed) stream"""
    rng = np.random.default_rng(seed)
    sd = {}
    for key, shape in imdn2_keys(nf, inC, outC):
        if key.endswith(".weight"):
            fan_in = shape[1] * shape[2] * shape[3]
            sd[key] = (rng.standard_normal(shape) * (GAIN * np.sqrt(2.0 / fan_in))).astype(np.float32)
        else:
            sd[key] = (rng.standard_normal(shape) * BIAS_STD).astype(np.float32)
    return sd


def digest(sd):
    """sha256 over the arrays' bytes in key order"""
    h = hashlib.sha256()
    for k in sd:
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k], dtype=np.float32).tobytes())
    return h.hexdigest()


def _conv(x, w, b):
    """x [B, H, W, Ci] float64, w [Co, Ci, k, k] -> [B, H, W, Co], zero padding (k-1)/2"""
    w = np.asarray(w, np.float64)
    k = w.shape[2]
    p = (k - 1) // 2
    B, H, W, _ = x.shape
    xp = np.pad(x, ((0, 0), (p, p), (p, p), (0, 0))) if p else x
    out = np.broadcast_to(np.asarray(b, np.float64), (B, H, W, w.shape[0])).copy()
    for ky in range(k):
        for kx in range(k):
            out += xp[:, ky:ky + H, kx:kx + W, :] @ w[:, :, ky, kx].T
    return out


def _lrelu(x):
    return np.where(x > 0, x, 0.05 * x)


def _net(sd, prefix, x, seen=None):
    """imdn_rtc's arithmetic; seen(name, z) is handed every LeakyReLU input z [B, H, W, nf] under its conv's name"""
    g = lambda name: (sd[prefix + name + ".weight"], sd[prefix + name + ".bias"])

    def act(h, name):
        z = _conv(h, *g(name))
        if seen is not None:
            seen(name, z)
        return _lrelu(z)

    h = np.transpose(np.asarray(x, np.float64), (0, 2, 3, 1))
    fea = _conv(h, *g("model.0"))
    d = fea.shape[-1] // 4
    h = fea
    for m in range(MODULES):
        p = "model.1.sub.%d." % m
        o1 = act(h, p + "c1")
        o2 = act(o1[..., d:], p + "c2")
        o3 = act(o2[..., d:], p + "c3")
        o4 = _conv(o3[..., d:], *g(p + "c4"))
        h = _conv(np.concatenate([o1[..., :d], o2[..., :d], o3[..., :d], o4], -1), *g(p + "c5")) + h
    y = _conv(_conv(h, *g("model.1.sub.5")) + fea, *g("model.2"))
    return np.transpose(y, (0, 3, 1, 2))


def imdn_rtc(sd, prefix, x):
    """one IMDN_RTC: x [B, in_nc, H, W] (any float) -> [B, out_nc, H, W] float64, sd keys under `prefix`"""
    return _net(sd, prefix, x)


def hazards(sd, prefix, x, exempt=()):
    """how close each image of x [B, in_nc, H, W] comes to a threshold of the backward, in float64 -> (zmin, ymin), [B] each:
    zmin[b] the smallest |z| over every LeakyReLU input (c1, c2, c3 of the five modules, all channels and pixels),
    ymin[b] the smallest | |y| - 1 | over the raw output.  `exempt` leaves out the channels that sit on a threshold on
    purpose: a pair ("model.1.sub.M.cJ", channel) is skipped in zmin, a bare output channel in ymin."""
    skip_z = {}
    for e in exempt:
        if isinstance(e, tuple):
            skip_z.setdefault(e[0], []).append(e[1])
    skip_y = [e for e in exempt if not isinstance(e, tuple)]
    zmin = np.full(np.shape(x)[0], np.inf)

    def seen(name, z):
        keep = np.ones(z.shape[-1], bool)
        keep[skip_z.get(name, [])] = False
        np.minimum(zmin, np.abs(z[..., keep]).min(axis=(1, 2, 3)), out=zmin)

    y = _net(sd, prefix, x, seen)
    keep = np.ones(y.shape[1], bool)
    keep[skip_y] = False
    return zmin, np.abs(np.abs(y[:, keep]) - 1).min(axis=(1, 2, 3))


def post(y, stage, norm=255):
    """IMDN2.predict's clamp and affine on a raw net output"""
    c = np.clip(y, -1, 1)
    return c / 2 + 0.5 if stage == 2 else c * (norm // 2) + (norm // 2)


def torch_imdn_rtc(sd, prefix, x):
    """the same net as stock PyTorch convolutions (F.conv2d: MIOpen on the GPU), in x's dtype and device -- what the
    reference runs; sd values are tensors on x's device"""
    import torch
    import torch.nn.functional as F

    def conv(t, name):
        w = sd[prefix + name + ".weight"]
        return F.conv2d(t, w, sd[prefix + name + ".bias"], padding=(w.shape[2] - 1) // 2)

    act = lambda t: F.leaky_relu(t, 0.05)
    fea = conv(x, "model.0")
    d = fea.shape[1] // 4
    h = fea
    for m in range(MODULES):
        p = "model.1.sub.%d." % m
        o1 = act(conv(h, p + "c1"))
        o2 = act(conv(o1[:, d:], p + "c2"))
        o3 = act(conv(o2[:, d:], p + "c3"))
        o4 = conv(o3[:, d:], p + "c4")
        h = conv(torch.cat([o1[:, :d], o2[:, :d], o3[:, :d], o4], 1), p + "c5") + h
    return conv(conv(h, "model.1.sub.5") + fea, "model.2")
