"""The batches of test_gpu_imdn_train_tiles.py and test_imdn_hazard_cpu.py (a helper, not a test): more tiles than
lerf_imdn_bwd.hip has weight-gradient slabs (MAX_SLABS = 256), so that a workgroup of imdn_wgrad_kernel walks several
8 x 16 tiles, built from many tiny images that imdn_grad_ref.screened_batch keeps away from every threshold; and one
net whose weights put chosen channels exactly on the thresholds.

Each batch, its float64 gradients included, is computed once per process and shared read-only."""
import functools

import numpy as np

import imdn_grad_ref as GR
import imdn_ref64 as R

SEED = 401
TH, TW, MAX_SLABS = 8, 16, 256       # lerf_imdn_bwd.hip's tile and slab count
PREFIX = "stage2."

# name: nf, in_nc, out_nc, B, H, W, post      tiles; what the walk meets; kept share of the 4 B pool, clamp share
CASES = {
    "a": (16, 3, 3, 258, 3, 3, 1),    # 258: workgroups 0 and 1 walk two tiles, the rest one; kept 0.897, clamp 0.060
    "b": (64, 3, 9, 257, 2, 3, 2),    # 257: four column blocks, one workgroup has a second tile; kept 0.712, clamp 0.145
    "c": (32, 1, 3, 300, 9, 2, 0),    # 600: three tiles for workgroups 0..87, two for the rest, a seam in y; kept 0.723
    "d": (48, 3, 9, 257, 2, 2, 2),    # 257: r = 36, a ragged third channel block in the slab indices; kept 0.797, clamp 0.072
    "e": (16, 3, 3, 131, 1, 17, 0),   # 262: a seam in x inside every image; kept 0.527
    "f": (16, 1, 1, 180, 1, 17, 0),   # 360: a seam in x with in_nc = out_nc = 1; kept 0.524
}
TIED = (16, 3, 3, 40, 3, 3)           # nf, in_nc, out_nc, B, H, W of the crafted ties, post 1 and 2; kept 0.881, clamp 0.030


def n_tiles(B, H, W):
    return B * ((H + TH - 1) // TH) * ((W + TW - 1) // TW)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def batch(name):
    """-> (sd, x, G, kept share) of CASES[name]"""
    nf, in_nc, out_nc, B, H, W, post = CASES[name]
    assert n_tiles(B, H, W) > MAX_SLABS
    sd = R.weight_rule(nf, in_nc, out_nc // in_nc, SEED)
    x, G, kept = GR.screened_batch(sd, PREFIX, nf, in_nc, out_nc, B, H, W, post, SEED)
    _frozen(*sd.values())
    return sd, x, G, kept


def tied_exempt(nf):
    """the channels tied_weights puts on a threshold, as imdn_ref64.hazards' `exempt`"""
    d = nf // 4
    rows = {"c1": (0, d, nf - 1), "c2": (1, d + 2), "c3": (d - 1, nf - 2)}      # a distilled and a remaining channel each
    return tuple(("model.1.sub.%d.%s" % (m, c), n) for m in (1, 3) for c, ns in rows.items() for n in ns) + (0, 2)


def tied_weights(nf, in_nc, out_nc, seed):
    """weight_rule's net with exact ties: the rows of tied_exempt have zero weights and bias, so their pre-activations are
    0 in every arithmetic, and the upsampler's rows 0 and 2 have zero weights and bias +1 and -1, so y == +-1 there"""
    sd = R.weight_rule(nf, in_nc, out_nc // in_nc, seed)
    for e in tied_exempt(nf):
        if isinstance(e, tuple):
            sd[PREFIX + e[0] + ".weight"][e[1]] = 0
            sd[PREFIX + e[0] + ".bias"][e[1]] = 0
    for n, b in ((0, 1.0), (2, -1.0)):
        sd[PREFIX + "model.2.weight"][n] = 0
        sd[PREFIX + "model.2.bias"][n] = b
    return sd


@functools.lru_cache(maxsize=None)
def tied_batch(post):
    """-> (sd, x, G, kept share) of the crafted ties"""
    nf, in_nc, out_nc, B, H, W = TIED
    sd = tied_weights(nf, in_nc, out_nc, SEED)
    x, G, kept = GR.screened_batch(sd, PREFIX, nf, in_nc, out_nc, B, H, W, post, SEED, tied_exempt(nf))
    _frozen(*sd.values())
    return sd, x, G, kept


@functools.lru_cache(maxsize=None)
def reference(name, post=None):
    """float64 CPU autograd of batch(name), or of tied_batch(post) for name "tied" -> (y64, {key: gradient}, grad_x)"""
    import torch
    if name == "tied":
        sd, x, G, _ = tied_batch(post)
    else:
        sd, x, G, _ = batch(name)
        post = CASES[name][6]
    y64, g64, gx64 = GR.net_grads(torch, sd, PREFIX, x, G, post, torch.float64)
    _frozen(y64, gx64, *g64.values())
    return y64, g64, gx64


def census(out_nc, B, H, W):
    """-> (G, sums): G is zero but for the first pixel of every tile, G[b, tile % out_nc, y0, x0] = tile % 7 + 1 with the
    tiles numbered as lerf_imdn_bwd.hip's tile_origin numbers them (x fastest, then y, then the image); sums[n] is the
    integer sum of G[:, n]: with post 0 the upsampler's bias gradient, exactly, in any summation order"""
    ty, tx = (H + TH - 1) // TH, (W + TW - 1) // TW
    G = np.zeros((B, out_nc, H, W), np.float32)
    sums = np.zeros(out_nc, np.int64)
    for tile in range(B * ty * tx):
        b, y0, x0 = tile // (tx * ty), tile // tx % ty * TH, tile % tx * TW
        G[b, tile % out_nc, y0, x0] = tile % 7 + 1
        sums[tile % out_nc] += tile % 7 + 1
    return G, sums
