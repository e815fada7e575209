"""The cases of test_gpu_srnet_paths.py and test_srnet_cases_cpu.py (a helper, not a test): the host rule of
lerf_srnet.hip's backward restated, an SRNet whose forward and backward are exact in float32, Kaiming nets for the
places where nothing is exact, and the float64 autograd restatement all of them are compared with.

The host rule.  srnet_bwd_kernel works on tiles of ROWS = 32 consecutive positions (plane-major, then row, column) and
launches min(tiles, MAX_SLABS = 512) workgroups; workgroup g owns weight-gradient slab g and walks tiles g, g + 512, ...:
the first tile initialises the slab, the later ones read it back and add.

The integer net (integer_net).  Every weight, bias, pixel and cotangent is a small integer, so every product and every
partial sum of the forward and the backward is an integer; as long as the sum of the absolute values of the terms of
every entry stays below 2^24 (integer_bounds), float32 computes them exactly in any order, and the kernel must agree
with float64 autograd bit for bit whatever its tiles, slabs and MFMA blocks do.
  * Neurons come in pairs (2j, 2j + 1) with equal activations: the odd row is the even row with one weight moved
    between two input channels that always carry the same value -- pattern pixels 0/1 or 2/3 for layer 1 (the image
    makes them equal, integer_image), channels (2i, 2i + 1) of the concatenated activations for the hidden layers.
  * W6[c] holds +s on channel 2p and -s on 2p + 1 (s in {1, 2}) and b6 = 0: the conv6 pre-activation is 0 everywhere,
    tanhf(0) = 0, the forward output is all zero and dz6 = grad_out.
  * Because the rows of a pair differ, the +g / -g cotangents of a pair do not cancel: they flow through the moved
    weight into the layers below and into the image.
  * Small integers tie often: many pre-activations are exactly 0 (with a non-zero incoming gradient), and a band of the
    image is black, where every pre-activation is its bias.  relu'(0) = 0, as torch has it.

Every batch and reference is computed once per process and shared read-only."""
import functools

import numpy as np
import torch

ROWS, MAX_SLABS = 32, 512           # lerf_srnet.hip's tile and slab count
NF, ACT = 64, 320
REACH = {"s": 1, "d": 2, "y": 2, "c": 3, "t": 3}
PATTERN = {"s": [(0, 0), (0, 1), (1, 0), (1, 1)], "d": [(0, 0), (0, 2), (2, 0), (2, 2)],
           "y": [(0, 0), (1, 1), (1, 2), (2, 1)], "c": [(0, 0), (0, 1), (0, 2), (0, 3)],
           "t": [(0, 0), (1, 1), (2, 2), (3, 3)]}
LAYERS = ["conv1.conv", "conv2.conv1.conv", "conv3.conv1.conv", "conv4.conv1.conv", "conv5.conv1.conv", "conv6.conv"]
KEY = "s2_cr1"
TENSORS = ["%s%d" % (t, l) for l in range(1, 7) for t in ("W", "b")]      # the 12 tensors in packed order


# ------------------------------------------------------------------------------------------------- the host rule
def n_tiles(P, h, w):
    return (P * h * w + ROWS - 1) // ROWS


def n_slabs(P, h, w):
    return min(n_tiles(P, h, w), MAX_SLABS)


def walk(g, P, h, w):
    """the number of tiles workgroup (= slab) g walks"""
    return len(range(g, n_tiles(P, h, w), n_slabs(P, h, w)))


def last_rows(P, h, w):
    """live rows of the last tile"""
    return P * h * w - (n_tiles(P, h, w) - 1) * ROWS


def straddles(P, h, w):
    """some tile holds positions of two planes"""
    return any(k * h * w % ROWS for k in range(1, P))


CLASSES = ("one position", "one partial tile of 31", "whole tiles only", "a tile straddles two planes", "tiles < 512",
           "tiles == 512", "513..516 tiles: a first walk", "tiles >= 1025: walks of three and of two")


def classes(P, h, w):
    n, t = P * h * w, n_tiles(P, h, w)
    walks = {walk(g, P, h, w) for g in range(n_slabs(P, h, w))}
    c = set()
    if n == 1:
        c.add("one position")
    if n == 31:
        c.add("one partial tile of 31")
    if n % ROWS == 0:
        c.add("whole tiles only")
    if straddles(P, h, w):
        c.add("a tile straddles two planes")
    if 1 < t < MAX_SLABS:
        assert walks == {1}
        c.add("tiles < 512")
    if t == MAX_SLABS:
        assert walks == {1}
        c.add("tiles == 512")
    if MAX_SLABS < t <= MAX_SLABS + 4:
        assert walks == {1, 2}
        c.add("513..516 tiles: a first walk")
    if t >= 2 * MAX_SLABS + 1:
        if walks == {2, 3}:
            c.add("tiles >= 1025: walks of three and of two")
    return c


# name: mode, outC, P, h, w, bd - reach, seed        positions, tiles, rows of the last tile
# The seed is the first multiple of 3 at which census_ok() finds nothing and every sum of absolute terms stays below 2^23
# (a single position seldom ties in all five layers at once, hence the large seed there).
INT_CASES = {
    "one-1": ("s", 3, 1, 1, 1, 0, 10890),        # 1, 1, 1
    "one-31": ("c", 4, 1, 1, 31, 1, 1041),       # 31, 1, 31
    "whole": ("t", 1, 2, 8, 8, 0, 6),            # 128, 4, 32: two whole tiles per plane
    "straddle": ("d", 3, 3, 5, 7, 2, 3),         # 105, 4, 9: tiles 1 and 2 hold two planes each
    "t512": ("c", 1, 1, 128, 128, 0, 6),         # 16384, 512, 32: the last launch without a walk
    "t513": ("s", 4, 2, 59, 139, 1, 3),          # 16402, 513, 18: slab 0 alone walks, a straddling tile
    "t516": ("t", 3, 1, 127, 130, 0, 3),         # 16510, 516, 30: slabs 0..3 walk
    "walk3-s": ("s", 3, 1, 181, 182, 0, 3),      # 32942, 1030, 14: slabs 0..5 walk three tiles, the rest two
    "walk3-t": ("t", 4, 3, 90, 122, 1, 81),      # 32940, 1030, 12: 344 tiles per plane, so the planes alone do not walk
    "walk3-c": ("c", 1, 2, 135, 122, 2, 6),      # 32940, 1030, 12
}
RAND_CASES = {                                # Kaiming weights, random biases, many screened planes: three-tile walks
    "walk3-s": ("s", 3, 915, 6, 6, 0),        # 32940, 1030, 12
    "walk3-t": ("t", 4, 942, 5, 7, 1),        # 32970, 1031, 10: 35 positions per plane, so most tiles hold two planes
}
TIED = ("s", 3, 300, 6, 6, 0)                 # zero biases, a black band in every plane: 10800 positions, 338 tiles
BIAS_P = (0.1, 0.2, 0.35, 0.35)               # the integer net's biases -2, -1, 0, 1: mostly live neurons
Z_WIDTH = 2e-5                                # no pre-activation of a screened batch is closer to 0 (exact zeros apart)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ------------------------------------------------------------------------------------------------- weights
def pack(d):
    return np.concatenate([d["%s.model.%s.%s" % (KEY, n, t)].reshape(-1) for n in LAYERS for t in ("weight", "bias")])


def unpack(flat, outC):
    """packed [weight_floats(outC)] -> the 12 arrays W1 [64, 4], b1, ..., W6 [outC, 320], b6"""
    out, off = [], 0
    for li in range(6):
        n_out, K = (outC if li == 5 else NF), (4 if li == 0 else li * NF)
        out.append(flat[off:off + n_out * K].reshape(n_out, K))
        out.append(flat[off + n_out * K:off + n_out * K + n_out])
        off += n_out * K + n_out
    assert off == flat.size
    return out


def as_dict(tensors):
    d = {}
    for li, name in enumerate(LAYERS):
        d["%s.model.%s.weight" % (KEY, name)] = np.ascontiguousarray(tensors[2 * li], np.float32)
        d["%s.model.%s.bias" % (KEY, name)] = np.ascontiguousarray(tensors[2 * li + 1], np.float32)
    return d


def tensors_of(d):
    return [d["%s.model.%s.%s" % (KEY, n, t)].reshape(-1 if t == "bias" else (d["%s.model.%s.bias" % (KEY, n)].size, -1))
            for n in LAYERS for t in ("weight", "bias")]


def kaiming_net(outC, seed, zero_bias=False):
    """Kaiming-normal weights (_Conv's init); biases 0.05 * normal as in test_gpu_srnet.py, or _Conv's zeros"""
    rng = np.random.default_rng(seed)
    t = []
    for li in range(6):
        fan_in, n_out = (4 if li == 0 else li * NF), (outC if li == 5 else NF)
        t.append(rng.standard_normal((n_out, fan_in)) * np.sqrt(2.0 / fan_in))
        b = 0.05 * rng.standard_normal(n_out)
        t.append(np.zeros(n_out) if zero_bias else b)
    return as_dict(t)


def integer_weights(outC, seed):
    """the integer net's state dict (see the module docstring)"""
    rng = np.random.default_rng(seed)
    t = []
    W1 = np.zeros((NF, 4), np.int64)
    for j in range(NF // 2):
        while True:
            row = rng.integers(-2, 3, 4)
            a = 2 * int(rng.integers(0, 2))                      # the weight moves between pixels 0/1 or 2/3
            e = int(rng.choice([-1, 1]))
            odd = row.copy()
            odd[a] -= e
            odd[a + 1] += e
            if np.abs(odd).max() <= 2 and np.any(row) and np.any(odd):
                break
        W1[2 * j], W1[2 * j + 1] = row, odd
    t += [W1, np.repeat(rng.choice([-2, -1, 0, 1], NF // 2, p=BIAS_P), 2)]
    for layer in range(2, 6):
        K = (layer - 1) * NF
        W = np.zeros((NF, K), np.int64)
        for j in range(NF // 2):
            while True:
                cols = rng.choice(K, 6, replace=False)
                free = [c for c in cols if (c ^ 1) not in cols]  # weights whose partner channel is unused
                if free:
                    break
            W[2 * j, cols] = rng.choice([-1, 1], 6)
            W[2 * j + 1] = W[2 * j]
            for c in rng.permutation(free)[:3]:                  # the odd row: up to three weights moved to the partner channel
                W[2 * j + 1, c ^ 1], W[2 * j + 1, c] = W[2 * j, c], 0
        t += [W, np.repeat(rng.choice([-2, -1, 0, 1], NF // 2, p=BIAS_P), 2)]
    W6 = np.zeros((outC, ACT), np.int64)
    for c in range(outC):
        n = 48 if outC >= 3 else 104                             # the pairs some channel reaches: two thirds of all
        pairs = rng.choice(ACT // 2, n, replace=False)
        s = rng.integers(1, 3, n)
        W6[c, 2 * pairs], W6[c, 2 * pairs + 1] = s, -s
    t += [W6, np.zeros(outC, np.int64)]
    return as_dict(t)


def integer_image(mode, P, h, w, bd, seed):
    """[P, h + bd, w + bd] pixels in 0..3 with pattern pixel 0 equal to pixel 1 and pixel 2 to pixel 3 at every position:
    constant along x for modes s and c, along the diagonals for t, of period 2 in x for d; a band of lines is black"""
    rng = np.random.default_rng(seed)
    H, W = h + bd, w + bd
    yy, xx = np.mgrid[0:H, 0:W]
    if mode in "sc":
        line, n_lines, per = yy, H, 1
    elif mode == "t":
        line, n_lines, per = xx - yy + H - 1, H + W - 1, 1
    elif mode == "d":
        line, n_lines, per = 2 * yy + xx % 2, 2 * H, 2
    else:
        raise ValueError(mode)
    val = rng.integers(0, 4, (P, n_lines))
    if n_lines >= 8 * per:
        val[:, n_lines // 3:n_lines // 2] = 0                    # the black band
    return _frozen(np.ascontiguousarray(val[:, line], np.float32))[0]


@functools.lru_cache(maxsize=None)
def integer_net(outC, mode, seed, shape):
    """-> (state dict, img [P, h + bd, w + bd], grad_out [P, outC, h, w]) for shape = (P, h, w, bd)"""
    P, h, w, bd = shape
    d = integer_weights(outC, seed)
    img = integer_image(mode, P, h, w, bd, seed + 1)
    G = np.random.default_rng(seed + 2).integers(-3, 4, (P, outC, h, w)).astype(np.float32)
    _frozen(G, *d.values())
    return d, img, G


def int_case(name):
    """-> (d, img, G, (mode, outC, P, h, w, bd)) of INT_CASES[name]"""
    mode, outC, P, h, w, extra, seed = INT_CASES[name]
    bd = REACH[mode] + extra
    return integer_net(outC, mode, seed, (P, h, w, bd)) + ((mode, outC, P, h, w, bd),)


def screened_planes(d, mode, P, h, w, bd, seed, black_rows=None):
    """P small planes on which no float32 run can flip a ReLU gate -> (img [P, h + bd, w + bd], kept share).  A float32
    pre-activation differs from the float64 one by a few 1e-6 here, and a batch of 33 000 positions holds about ten
    pre-activations that close to 0: one flipped gate moves grad_img at its position by percents and a weight gradient
    by 1e-3, in stock float32 autograd as well.  So, from default_rng(seed), planes uniform on [0, 1) (rows `black_rows`
    black) are drawn P at a time, and those whose pre-activations all keep |z| > Z_WIDTH in float64 are kept until
    there are P; the pre-activations of all-black positions under zero biases, exact zeros in any arithmetic, are
    exempt.  At most 4 P planes are drawn: fewer than P survivors raise."""
    rng = np.random.default_rng(seed)
    zero_bias = all(not np.any(b) for b in tensors_of(d)[1::2])
    kept, drawn = [], 0
    while sum(len(k) for k in kept) < P:
        if drawn >= 4 * P:
            raise ValueError("only %d of %d planes pass the screen, %d are needed" % (sum(len(k) for k in kept), drawn, P))
        pool = rng.random((P, h + bd, w + bd)).astype(np.float32)
        if black_rows is not None:
            pool[:, black_rows] = 0
        x = tuples(pool, mode, h, w)
        zs, _, _ = activations(d, x)
        zmin = np.min([np.abs(z).min(1) for z in zs], axis=0)
        if zero_bias:
            zmin[~x.any(1)] = np.inf
        kept.append(pool[(zmin > Z_WIDTH).reshape(P, -1).all(1)])
        drawn += P
    n = sum(len(k) for k in kept)
    return np.ascontiguousarray(np.concatenate(kept)[:P]), n / drawn


@functools.lru_cache(maxsize=None)
def rand_case(name):
    """-> (d, img, G, (mode, outC, P, h, w, bd), kept share): Kaiming weights, biases 0.05 * normal, screened planes"""
    mode, outC, P, h, w, extra = RAND_CASES[name]
    bd = REACH[mode] + extra
    i = sorted(RAND_CASES).index(name)
    d = kaiming_net(outC, 2100 + i)
    img, kept = screened_planes(d, mode, P, h, w, bd, 2000 + i)
    G = np.random.default_rng(2050 + i).standard_normal((P, outC, h, w)).astype(np.float32)
    _frozen(img, G, *d.values())
    return d, img, G, (mode, outC, P, h, w, bd), kept


def prefill(shape, seed, integer):
    """a prior content without zeros for an accumulating buffer: integers in +-1..8, or normals"""
    rng = np.random.default_rng(seed)
    if integer:
        return (rng.integers(1, 9, shape) * rng.choice([-1, 1], shape)).astype(np.float32)
    a = rng.standard_normal(shape).astype(np.float32)
    a[a == 0] = 1.0
    return a


def reached(mode, P, h, w, bd):
    """[P, h + bd, w + bd] bool: the pixels some tap of some position reads"""
    m = np.zeros((P, h + bd, w + bd), bool)
    for dy, dx in PATTERN[mode]:
        m[:, dy:dy + h, dx:dx + w] = True
    return m


# ------------------------------------------------------------------------------------------------- the restatement
class _ReluOpenAtZero(torch.autograd.Function):
    """relu with the other convention at the tie: relu'(0) = 1"""

    @staticmethod
    def forward(ctx, z):
        ctx.save_for_backward(z)
        return z.clamp(min=0)

    @staticmethod
    def backward(ctx, g):
        z, = ctx.saved_tensors
        return g * (z >= 0).to(g.dtype)


def autograd(d, mode, img, G, h, w, dtype=torch.float64, device="cpu", open_at_zero=False, internals=False):
    """SRNet.forward restated in torch and differentiated by autograd, in `dtype` on `device`
    -> (y [P, outC, h, w], the 12 gradients in packed order, grad_img), float64 numpy arrays; with internals also the
    pre-activations z_1..z_5 and the gradients arriving at the ReLU outputs, each [positions, 64]"""
    relu = _ReluOpenAtZero.apply if open_at_zero else torch.relu
    P = img.shape[0]
    x = torch.tensor(np.asarray(img), dtype=dtype, device=device, requires_grad=True)
    t = torch.stack([x[:, dy:dy + h, dx:dx + w].reshape(-1) for dy, dx in PATTERN[mode]], dim=1)
    ps = [torch.tensor(a, dtype=dtype, device=device, requires_grad=True) for a in tensors_of(d)]
    zs, outs = [], []
    a = None
    for li in range(5):
        z = (t if li == 0 else a) @ ps[2 * li].T + ps[2 * li + 1]
        o = relu(z)
        if internals:
            o.retain_grad()
        zs.append(z)
        outs.append(o)
        a = o if li == 0 else torch.cat([a, o], dim=1)
    y = torch.tanh(a @ ps[10].T + ps[11]).reshape(P, h, w, -1).permute(0, 3, 1, 2)
    y.backward(torch.tensor(np.asarray(G), dtype=dtype, device=device))
    to64 = lambda v: v.detach().double().cpu().numpy()
    res = (to64(y), [to64(p.grad) for p in ps], to64(x.grad))
    if internals:
        res += ([to64(z) for z in zs], [to64(o.grad) for o in outs])
    return res


@functools.lru_cache(maxsize=None)
def int_reference(name):
    """float64 CPU autograd of int_case(name) -> (y, 12 gradients, grad_img)"""
    d, img, G, (mode, outC, P, h, w, bd) = int_case(name)
    y, gs, gx = autograd(d, mode, img, G, h, w)
    _frozen(y, gx, *gs)
    return y, gs, gx


@functools.lru_cache(maxsize=None)
def rand_reference(name):
    d, img, G, (mode, outC, P, h, w, bd), _ = rand_case(name)
    y, gs, gx = autograd(d, mode, img, G, h, w)
    _frozen(y, gx, *gs)
    return y, gs, gx


def tuples(img, mode, h, w):
    """[P * h * w, 4] pattern pixels of every position"""
    return np.stack([img[:, dy:dy + h, dx:dx + w].reshape(-1) for dy, dx in PATTERN[mode]], axis=1)


def activations(d, x):
    """float64 numpy forward on [N, 4] tuples -> (z_1..z_5 [N, 64] each, act [N, 320], z_6 [N, outC])"""
    ts = [a.astype(np.float64) for a in tensors_of(d)]
    zs, a = [], x.astype(np.float64)
    for li in range(5):
        z = a @ ts[2 * li].T + ts[2 * li + 1]
        zs.append(z)
        a = np.maximum(z, 0) if li == 0 else np.concatenate([a, np.maximum(z, 0)], axis=1)
    return zs, a, a @ ts[10].T + ts[11]


def integer_bounds(d, mode, img, G, h, w):
    """For every entry of every gradient the sum of the absolute values of its terms, the cotangents taken through the
    absolute network (|dz| against |W| down the layers, |dz| against |act| for the weights) -> (the 12 bounds in packed
    order, the bound of grad_img, the largest absolute forward sum).  Every partial sum of the kernel, in any order, is
    an integer no larger than these."""
    P, outC = img.shape[0], G.shape[1]
    x = tuples(img, mode, h, w).astype(np.float64)
    ts = [np.abs(a.astype(np.float64)) for a in tensors_of(d)]
    zs, act, _ = activations(d, x)
    fwd, m = 0.0, np.abs(x)
    for li in range(5):
        mz = m @ ts[2 * li].T + ts[2 * li + 1]
        fwd = max(fwd, mz.max())
        m = mz if li == 0 else np.concatenate([m, mz], axis=1)
    fwd = max(fwd, (m @ ts[10].T + ts[11]).max())
    dz6 = np.abs(np.asarray(G, np.float64)).transpose(0, 2, 3, 1).reshape(-1, outC)
    out = [None] * 12
    out[10], out[11] = dz6.T @ act, dz6.sum(0)
    dact = dz6 @ ts[10]
    for layer in range(5, 1, -1):
        K = (layer - 1) * NF
        dz = dact[:, K:K + NF] * (zs[layer - 1] > 0)
        out[2 * layer - 2], out[2 * layer - 1] = dz.T @ act[:, :K], dz.sum(0)
        dact[:, :K] += dz @ ts[2 * layer - 2]
    dz = dact[:, :NF] * (zs[0] > 0)
    out[0], out[1] = dz.T @ np.abs(x), dz.sum(0)
    dx = (dz @ ts[0]).reshape(P, h, w, 4)
    gimg = np.zeros(img.shape)
    for k, (dy, dxx) in enumerate(PATTERN[mode]):
        gimg[:, dy:dy + h, dxx:dxx + w] += dx[..., k]
    return out, gimg, fwd


def census(d, img, G, geo):
    """what makes an exact comparison on this integer case meaningful, as a dict: test_srnet_cases_cpu.py states the
    conditions.  `open_alone[l - 1]` tells whether relu'(0) = 1 in the gate of layer l alone changes both dW_l and db_l:
    only dz_l changes there, by the incoming gradient at the ties."""
    mode, outC, P, h, w, bd = geo
    y, gs, gx, zs, das = autograd(d, mode, img, G, h, w, internals=True)
    y32, gs32, gx32 = autograd(d, mode, img, G, h, w, dtype=torch.float32)
    _, gso, gxo = autograd(d, mode, img, G, h, w, open_at_zero=True)
    bw, bi, fwd = integer_bounds(d, mode, img, G, h, w)
    _, act, z6 = activations(d, tuples(img, mode, h, w))
    r = reached(mode, P, h, w, bd)
    alone = []
    for l in range(1, 6):
        extra = np.where(zs[l - 1] == 0, das[l - 1], 0.0)
        inp = tuples(img, mode, h, w).astype(np.float64) if l == 1 else act[:, :(l - 1) * NF]
        alone.append(bool(np.any(extra.T @ inp)) and bool(np.any(extra.sum(0))))
    return {
        "float32 equals float64": all(np.array_equal(a, b) for a, b in zip(gs, gs32)) and np.array_equal(gx, gx32)
                                  and np.array_equal(y, y32),
        "forward is zero": not np.any(y) and not np.any(z6),
        "integers": all(np.array_equal(g, np.round(g)) for g in gs + [gx]),
        "largest sum of absolute terms": float(max(max(b.max() for b in bw), bi.max(), fwd)),
        "largest gradient entry": float(max(np.abs(g).max() for g in gs + [gx])),
        "non-zero share": [float((g != 0).mean()) for g in gs],
        "non-zero share of the reached grad_img": float((gx[r] != 0).mean()),
        "unreached grad_img is zero": not np.any(gx[~r]),
        "gates open and closed": [bool((z > 0).any()) and bool((z <= 0).any()) for z in zs],
        "tie share": [float(((z == 0) & (da != 0)).mean()) for z, da in zip(zs, das)],
        "open at zero differs": [not np.array_equal(a, b) for a, b in zip(gs, gso)],
        "open_alone": alone,
    }


def census_ok(c):
    """the conditions of test_srnet_cases_cpu.py on census()'s dict -> the list of those that fail"""
    bad = [k for k in ("float32 equals float64", "forward is zero", "integers", "unreached grad_img is zero") if not c[k]]
    if not c["largest sum of absolute terms"] < 2 ** 24:
        bad.append("a sum of absolute terms reaches 2^24")
    bad += ["%s: %.3f non-zero" % (TENSORS[i], v) for i, v in enumerate(c["non-zero share"]) if v < 0.2]
    if c["non-zero share of the reached grad_img"] < 0.5:
        bad.append("grad_img")
    bad += ["layer %d gates" % (i + 1) for i, v in enumerate(c["gates open and closed"]) if not v]
    bad += ["layer %d ties %.4f" % (i + 1, v) for i, v in enumerate(c["tie share"]) if v < 0.01]
    bad += ["%s under relu'(0) = 1" % TENSORS[i] for i, v in enumerate(c["open at zero differs"][:10]) if not v]
    bad += ["gate %d alone" % (i + 1) for i, v in enumerate(c["open_alone"]) if not v]
    return bad


# ------------------------------------------------------------------------------------------------- real ties
@functools.lru_cache(maxsize=None)
def tied_batch():
    """_Conv's own initialisation (zero biases) on planes with a black band: wherever the four pattern pixels are 0,
    every pre-activation of every layer is exactly 0 in any arithmetic.  screened_planes with rows 2..4 black, so that no
    float32 run can flip a sign elsewhere -> (d, img, G, (mode, outC, P, h, w, bd), tied positions [P * h * w] bool,
    kept share)."""
    mode, outC, P, h, w, extra = TIED
    bd = REACH[mode] + extra
    d = kaiming_net(outC, 2200, zero_bias=True)
    img, kept = screened_planes(d, mode, P, h, w, bd, 2201, black_rows=slice(2, 5))
    G = np.random.default_rng(2202).standard_normal((P, outC, h, w)).astype(np.float32)
    tied = ~tuples(img, mode, h, w).any(1)
    _frozen(img, G, tied, *d.values())
    return d, img, G, (mode, outC, P, h, w, bd), tied, kept


@functools.lru_cache(maxsize=None)
def tied_reference():
    d, img, G, (mode, outC, P, h, w, bd), _, _ = tied_batch()
    y, gs, gx = autograd(d, mode, img, G, h, w)
    _frozen(y, gx, *gs)
    return y, gs, gx


def rel_err(t, t64):
    """max |t - t64| / max |t64| (imdn_grad_ref.rel_err)"""
    return float(np.abs(np.asarray(t, np.float64) - t64).max() / max(np.abs(t64).max(), 1e-300))
