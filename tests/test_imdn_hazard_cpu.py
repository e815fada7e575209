"""CPU-only checks of the batches of test_gpu_imdn_train_tiles.py (imdn_tile_cases.py): the hazard screen of
imdn_grad_ref.screened_batch finds enough images in its pool of 4 B, the clamp mask is exercised, and on the screened
batch float32 autograd agrees with float64 as closely as rounding allows -- so the GPU test's rule
e_hip <= 4 e_stock + 1e-6 compares rounding errors and not flipped masks.

Tolerance of float32 against float64 CPU autograd: 1e-5 of each tensor's largest entry, the width of the screen itself
(imdn_grad_ref.Z_WIDTH).  One flipped LeakyReLU sign or clamp bit moves a gradient by 1e-3 to 1e-2 at these sizes; the
largest figure measured on the screened batches is 4.7e-6 (printed per case).
hazards against the brute force: 1e-12 absolute on values of order 1: two float64 summation orders of at most 577 terms
(6e-14 each) carried through 28 convolutions."""
import numpy as np
import pytest

import imdn_grad_ref as GR
import imdn_ref64 as R
import imdn_tile_cases as T

RUNS = [(n, None) for n in T.CASES] + [("tied", 1), ("tied", 2)]


def _batch(name, post):
    return T.tied_batch(post) if name == "tied" else T.batch(name)


@pytest.mark.parametrize("name,post", RUNS, ids=lambda v: str(v))
def test_screened_batch_is_safe_in_float32(name, post):
    import torch
    sd, x, G, kept = _batch(name, post)                                 # raises where the pool does not suffice
    cfg = T.TIED if name == "tied" else T.CASES[name][:6]
    post = post if name == "tied" else T.CASES[name][6]
    nf, in_nc, out_nc, B, H, W = cfg
    assert x.shape == (B, in_nc, H, W) and G.shape == (B, out_nc, H, W) and x.dtype == G.dtype == np.float32
    exempt = T.tied_exempt(nf) if name == "tied" else ()
    zmin, ymin = R.hazards(sd, T.PREFIX, x, exempt)
    assert zmin.min() > GR.Z_WIDTH and (not post or ymin.min() > GR.Y_WIDTH)
    y64, g64, gx64 = T.reference(name, post if name == "tied" else None)
    share = float((np.abs(y64) > 1).mean())
    if post:
        assert 0.02 <= share <= 0.5, share
    _, g32, gx32 = GR.net_grads(torch, sd, T.PREFIX, x, G, post, torch.float32)
    errs = {k: GR.rel_err(g32[k], g64[k]) for k in g64}
    errs["grad_x"] = GR.rel_err(gx32, gx64)
    assert len(errs) == 2 * 28 + 1 and all(np.abs(t).max() > 0 for t in g64.values())
    worst = max(errs, key=errs.get)
    print("%s post %d: kept %.3f, |y| > 1 for %.3f, float32 within %.3g of float64 (%s)" % (name, post, kept, share, errs[worst], worst))
    assert errs[worst] <= 1e-5, (worst, errs[worst])


def test_pool_that_does_not_suffice_raises():
    nf, in_nc, out_nc = 16, 3, 3
    sd = R.weight_rule(nf, in_nc, 1, T.SEED)
    sd["stage2.model.1.sub.0.c1.weight"][5] = 0                         # a pre-activation of exactly 0 in every image
    sd["stage2.model.1.sub.0.c1.bias"][5] = 0
    with pytest.raises(ValueError):
        GR.screened_batch(sd, T.PREFIX, nf, in_nc, out_nc, 2, 3, 3, 1, T.SEED)
    x, _, kept = GR.screened_batch(sd, T.PREFIX, nf, in_nc, out_nc, 2, 3, 3, 1, T.SEED, (("model.1.sub.0.c1", 5),))
    assert x.shape == (2, 3, 3, 3) and kept > 0.25


def _brute_conv(x, w, b):
    """x [H][W][Ci] -> [H][W][Co]: one dot product per output, every out-of-bounds tap skipped"""
    w = np.asarray(w, np.float64)
    Co, Ci, k, _ = w.shape
    H, W, _ = x.shape
    out = np.zeros((H, W, Co))
    for y in range(H):
        for xx in range(W):
            for n in range(Co):
                s = float(b[n])
                for ky in range(k):
                    for kx in range(k):
                        yy, xc = y + ky - k // 2, xx + kx - k // 2
                        if 0 <= yy < H and 0 <= xc < W:
                            s += float(np.dot(x[yy, xc], w[n, :, ky, kx]))
                out[y, xx, n] = s
    return out


def _brute_hazards(sd, prefix, img, exempt):
    """every LeakyReLU input and raw output of one image [in_nc][H][W], gathered as {(conv, channel): values}"""
    g = lambda name: (sd[prefix + name + ".weight"], sd[prefix + name + ".bias"])
    lrelu = lambda z: np.where(z > 0, z, 0.05 * z)
    zs = {}

    def act(h, name):
        z = _brute_conv(h, *g(name))
        for n in range(z.shape[-1]):
            zs[(name, n)] = z[..., n]
        return lrelu(z)

    fea = _brute_conv(np.asarray(img, np.float64).transpose(1, 2, 0), *g("model.0"))
    d = fea.shape[-1] // 4
    h = fea
    for m in range(R.MODULES):
        p = "model.1.sub.%d." % m
        o1 = act(h, p + "c1")
        o2 = act(o1[..., d:], p + "c2")
        o3 = act(o2[..., d:], p + "c3")
        o4 = _brute_conv(o3[..., d:], *g(p + "c4"))
        h = _brute_conv(np.concatenate([o1[..., :d], o2[..., :d], o3[..., :d], o4], -1), *g(p + "c5")) + h
    y = _brute_conv(_brute_conv(h, *g("model.1.sub.5")) + fea, *g("model.2"))
    zmin = min(np.abs(v).min() for k, v in zs.items() if k not in exempt)
    ymin = min(np.abs(np.abs(y[..., n]) - 1).min() for n in range(y.shape[-1]) if n not in exempt)
    return len(zs), zmin, ymin


def test_hazards_agree_with_brute_force():
    nf, in_nc, out_nc = 16, 3, 3
    rng = np.random.default_rng(T.SEED + 2)
    x = (3 * rng.random((3, in_nc, 3, 3))).astype(np.float32)
    plain = R.weight_rule(nf, in_nc, 1, T.SEED)
    tied = T.tied_weights(nf, in_nc, out_nc, T.SEED)
    for sd, exempt in ((plain, ()), (tied, T.tied_exempt(nf)), (tied, ())):
        zmin, ymin = R.hazards(sd, T.PREFIX, x, exempt)
        assert zmin.shape == ymin.shape == (3,)
        n, bz, by = _brute_hazards(sd, T.PREFIX, x[1], exempt)           # image 1: the batch's neighbours must not leak in
        assert n == 15 * nf
        if sd is tied and not exempt:
            assert zmin[1] == 0 and bz == 0 and ymin[1] == 0 and by == 0     # the ties are exact
        else:
            assert zmin[1] > 0 and ymin[1] > 0
            assert abs(zmin[1] - bz) <= 1e-12 and abs(ymin[1] - by) <= 1e-12, (zmin[1], bz, ymin[1], by)
