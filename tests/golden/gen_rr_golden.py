"""Writes tests/golden/g29_rr.npz: outputs of the REFERENCE's resize_right.resize (numpy and torch, on the CPU) for the
cases below, the per-axis tables of one dim of every case, interp_methods values, and input gradients from the reference's
autograd.  Data only: the inputs come from a seeded rule (make_input) that the tests repeat.

    python tests/golden/gen_rr_golden.py --reference <checkout of the reference repository>

Per torch float32 case the file also holds the largest |reference float32 torch result - reference float64 numpy result|
(`gap_<i>`): the reference's own float32 error, from which tests/test_gpu_rr.py derives its float32 tolerance per class.
The largest gap of every class is printed.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
KERNELS = ["cubic", "lanczos2", "lanczos3", "linear", "box"]
SWEEP_SCALES = [0.25, 1 / 3, 0.5, 0.7, 1.5, 2, 3.3]
NP_OF_TORCH_PAD = {"constant": "constant", "replicate": "edge", "reflect": "reflect", "circular": "wrap"}


def gauss5(x):
    """a user callable: a Gaussian, sigma 0.8, with a support of 5"""
    if isinstance(x, np.ndarray):
        return np.exp(-x ** 2 / (2 * 0.8 ** 2))
    return torch.exp(-x ** 2 / (2 * 0.8 ** 2))


gauss5.support_sz = 5


def make_input(seed, shape, dtype):
    """the seeded rule: values on 0..255 (integers for uint8)"""
    rng = np.random.default_rng(seed)
    if dtype == "uint8":
        return rng.integers(0, 256, size=shape, dtype=np.uint8)
    return rng.uniform(0.0, 255.0, size=shape).astype(dtype)


def cases():
    """[{cls, fw, shape, dtype, kw}]: kw are resize()'s keyword arguments with interp_method by name"""
    out = []

    def add(cls, fws, shape, dtypes=None, **kw):
        for fw in fws:
            for dt in dtypes or (["float64"] if fw == "np" else ["float32"]):
                out.append({"cls": cls, "fw": fw, "shape": list(shape), "dtype": dt, "kw": kw})

    # the five kernels x seven scales, anti-aliasing on and off.  torch resizes the LAST two dims of [1, 12, 10].
    for k in KERNELS:
        for s in SWEEP_SCALES:
            for aa in (True, False):
                # without anti-aliasing a narrow kernel at a small scale never reaches the borders: the pad is negative (a crop),
                # which np.pad refuses ("index can't contain negative values"), so the reference's numpy branch cannot run
                # linear at x1/4, x1/3 and box at x1/4, x1/3, x1/2.  Its torch branch crops (F.pad) and is listed.
                if not (not aa and ((k == "linear" and s < 0.4) or (k == "box" and s < 0.6))):
                    add("sweep/" + k, ("np",), (12, 10), scale_factors=s, interp_method=k, antialiasing=aa)
                add("sweep/" + k, ("torch",), (1, 12, 10), scale_factors=s, interp_method=k, antialiasing=aa)
    # anisotropic pairs, one dim at scale 1
    for sf in ([1 / 1.5, 1 / 2], [2, 0.5], [1, 0.5], [2.5, 1]):
        add("aniso", ("np",), (15, 14, 3), scale_factors=sf)
        add("aniso", ("torch",), (2, 3, 15, 14), scale_factors=sf)
    # out_shape alone, out_shape with scales, scalar scale
    add("shape", ("np",), (15, 14, 3), out_shape=[9, 20])
    add("shape", ("torch",), (2, 3, 15, 14), out_shape=[9, 20])
    add("shape", ("np",), (15, 14, 3), out_shape=[8, 7], scale_factors=[0.5, 0.5])
    add("shape", ("torch",), (2, 3, 15, 14), out_shape=[8, 7], scale_factors=[0.5, 0.5])
    add("shape", ("np",), (15, 14, 3), scale_factors=0.6)
    add("shape", ("torch",), (2, 3, 15, 14), scale_factors=0.6)
    # ndim 1..4 and which dims move by default (numpy: the first, torch: the last)
    add("ndim", ("np",), (17,), scale_factors=[0.5])
    add("ndim", ("np",), (17,), scale_factors=[0.125], interp_method="lanczos3")       # 48 taps on a last-dim pass
    add("ndim", ("np",), (17,), scale_factors=[2.2])
    add("ndim", ("np",), (13, 9), scale_factors=[1.7])
    add("ndim", ("np",), (13, 9, 3), scale_factors=0.5)
    add("ndim", ("np",), (6, 7, 5, 2), scale_factors=[2, 0.5, 1.5])
    add("ndim", ("np",), (6, 7, 5, 2), scale_factors=[0.5, 0.5, 0.5, 0.5])
    # torch tensors of fewer than 3 dims: the reference's fw_pad adds two leading dims for them and never removes them
    # (resize_right.py:398-399), so any padded pass of a 1-D or 2-D torch tensor fails in the reference itself: not listed.
    add("ndim", ("torch",), (4, 13, 9), scale_factors=[1.7])
    add("ndim", ("torch",), (2, 3, 13, 9), scale_factors=0.5)
    add("ndim", ("torch",), (2, 3, 6, 7), scale_factors=[2, 0.5, 1.5])
    add("ndim", ("torch",), (1, 1, 64, 5), scale_factors=[1, 0.125])                   # taps wider than the 5-pixel dim, n_out = 1
    add("ndim", ("np",), (5, 70), scale_factors=[0.125, 1])                             # x1/8 of a 5-pixel dim: 32 taps, n_out = 1
    add("ndim", ("np",), (1, 9), scale_factors=[3, 2])                                  # a 1-pixel dim
    # every pad mode
    for pm in ("constant", "edge", "reflect", "symmetric", "wrap"):
        add("pad", ("np",), (11, 9, 2), scale_factors=[0.4, 2.3], pad_mode=pm)
        add("pad", ("np",), (11, 9, 2), scale_factors=[1.5, 0.5], pad_mode=pm, interp_method="lanczos3")
    for pm in ("constant", "replicate", "reflect", "circular"):
        add("pad", ("torch",), (2, 2, 11, 9), scale_factors=[0.4, 2.3], pad_mode=pm)
    # a support_sz override and a user callable
    add("custom", ("np",), (14, 12), scale_factors=[0.5, 1.6], support_sz=6)
    add("custom", ("torch",), (1, 1, 14, 12), scale_factors=[0.5, 1.6], support_sz=6)
    add("custom", ("np",), (14, 12), scale_factors=[0.5, 1.6], interp_method="gauss5")
    add("custom", ("torch",), (1, 1, 14, 12), scale_factors=[0.5, 1.6], interp_method="gauss5")
    # dtypes
    add("dtype", ("np",), (14, 12, 3), ["uint8", "float32", "float64"], scale_factors=[1 / 3, 1 / 3])
    add("dtype", ("np",), (14, 12, 3), ["uint8", "float32"], scale_factors=[2, 2])
    add("dtype64", ("torch",), (2, 3, 14, 12), ["float64"], scale_factors=[1 / 3, 1 / 3])
    add("dtype64", ("torch",), (2, 3, 14, 12), ["float64"], scale_factors=[2, 1.5], pad_mode="reflect")
    return out


# the torch cases whose input gradient is recorded: indices into the torch float32 / float64 cases, picked by content
def wants_grad(c):
    kw = c["kw"]
    if c["fw"] != "torch":
        return False
    return ((c["cls"] == "sweep/cubic" and kw["scale_factors"] in (0.5, 2) and kw["antialiasing"]) or
            (c["cls"] == "sweep/lanczos3" and kw["scale_factors"] == 0.7 and kw["antialiasing"]) or
            (c["cls"] == "pad" and kw["pad_mode"] in ("reflect", "circular")) or
            (c["cls"] == "dtype64" and kw.get("pad_mode") is None))


def method_of(im, name):
    return gauss5 if name == "gauss5" else getattr(im, name)


def ref_kwargs(im, kw):
    k = dict(kw)
    k["interp_method"] = method_of(im, k.get("interp_method", "cubic"))
    return k


def axis_tables(rr, im, c, fw):
    """left and weights of the LAST resized dim of the case, by the reference's own functions"""
    kw = ref_kwargs(im, c["kw"])
    eps = fw.finfo(fw.float32).eps
    sf, osz, _ = rr.set_scale_and_out_sz(c["shape"], kw.get("out_shape"), kw.get("scale_factors"), False, None, 10, eps, fw)
    dims = [d for d in sorted(range(len(c["shape"])), key=lambda i: sf[i]) if sf[d] != 1.]
    d = dims[-1]
    support = kw.get("support_sz") or kw["interp_method"].support_sz
    grid = rr.get_projected_grid(c["shape"][d], osz[d], sf[d], fw, False, None)
    method, support = rr.apply_antialiasing_if_needed(kw["interp_method"], support, sf[d], kw.get("antialiasing", True))
    fov = rr.get_field_of_view(grid, support, fw, eps, None)
    left = np.asarray(fov[:, 0]).astype(np.int64).copy()
    _, grid, fov = rr.calc_pad_sz(c["shape"][d], osz[d], fov, grid, sf[d], False, fw, None)
    w = rr.get_weights(method, grid, fov)
    return d, left, np.asarray(w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(HERE, "g29_rr.npz"))
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    import resize_right.interp_methods as im
    import resize_right.resize_right as rr

    data = {}
    # interp_methods on a fixed float64 grid (kinks, zeros and the support's ends included)
    x = np.concatenate([np.linspace(-3.5, 3.5, 141), np.array([0.0, 1e-9, -1e-9, 1 / 3, -2 / 3, 2.0, -2.0, 3.0])])
    data["im_x"] = x
    for k in KERNELS:
        data["im_" + k] = np.asarray(getattr(im, k)(x), dtype=np.float64)

    cs = cases()
    gaps = {}
    for i, c in enumerate(cs):
        xin = make_input(1000 + i, c["shape"], c["dtype"])
        kw = ref_kwargs(im, c["kw"])
        if c["fw"] == "np":
            out = rr.resize(xin.copy(), **kw)
            d, left, w = axis_tables(rr, im, c, np)
        else:
            t = torch.from_numpy(xin.copy())
            out = rr.resize(t, **kw).numpy()
            d, left, w = axis_tables(rr, im, c, torch)
            if c["dtype"] == "float32":
                kn = dict(kw)
                kn["pad_mode"] = NP_OF_TORCH_PAD[kw.get("pad_mode", "constant")]
                nsf, nos = kn.get("scale_factors"), kn.get("out_shape")
                nd = len(c["shape"])
                # numpy resizes the first dims by default: spell the torch default out
                if nsf is not None:
                    nsf = list(nsf) if isinstance(nsf, (list, tuple)) else [nsf, nsf]
                    kn["scale_factors"] = [1] * (nd - len(nsf)) + nsf
                if nos is not None:
                    kn["out_shape"] = list(c["shape"][:nd - len(nos)]) + list(nos)
                try:
                    o64 = rr.resize(xin.astype(np.float64), **kn)
                except ValueError:          # a negative pad: the numpy branch cannot run (see cases()); no gap from this case
                    o64 = None
                if o64 is not None:
                    gap = float(np.max(np.abs(out.astype(np.float64) - o64)))
                    data["gap_%d" % i] = np.float64(gap)
                    gaps[c["cls"]] = max(gaps.get(c["cls"], 0.0), gap)
            if wants_grad(c):
                t = torch.from_numpy(xin.copy()).requires_grad_(True)
                y = torch.from_numpy(make_input(5000 + i, out.shape, c["dtype"]) / 255.0).to(t.dtype)
                (rr.resize(t, **kw) * y).sum().backward()
                data["grad_%d" % i] = t.grad.numpy()
                if c["dtype"] == "float32":
                    # the reference's own float32 gradient error: against its float64 autograd on the same input
                    t64 = torch.from_numpy(xin.astype(np.float64)).requires_grad_(True)
                    (rr.resize(t64, **kw) * y.double()).sum().backward()
                    ggap = float(np.max(np.abs(t.grad.numpy().astype(np.float64) - t64.grad.numpy())))
                    data["ggap_%d" % i] = np.float64(ggap)
                    gaps["grad"] = max(gaps.get("grad", 0.0), ggap)
        c["out_dtype"] = str(out.dtype)
        c["table_dim"] = int(d)
        data["out_%d" % i] = out
        data["left_%d" % i] = left
        data["w_%d" % i] = w
    data["cases"] = np.array(json.dumps(cs))
    np.savez_compressed(a.out, **data)
    print("%d cases -> %s (%d bytes)" % (len(cs), a.out, os.path.getsize(a.out)))
    for k in sorted(gaps):
        print("largest float32 gap of class %-16s %.3e" % (k, gaps[k]))


if __name__ == "__main__":
    main()
