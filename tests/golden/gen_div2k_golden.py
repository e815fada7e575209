"""Writes tests/golden/g30_div2k.npz: what the REFERENCE's resample/data.py DIV2K.__getitem__ returns for seeded draws, the
draws themselves, and the defaults of the reference's TrainOptions.  Data only.

    python tests/golden/gen_div2k_golden.py

The DIV2K objects are built without touching the disk (`__new__` plus attributes) over four seeded random uint8 HR images
of unequal sizes (45x57, 39x51, 60x39, 48x48) with LR images of ceil(H / scale) x ceil(W / scale).  Per case, after
random.seed(seed), 24 consecutive __getitem__ results are recorded; the same seed is then replayed with the draws written
out (file, li, lj, hi, hj, chan, fliplr, flipud, k), and tests/patch_ref.py must rebuild every recorded sample from them
before anything is written.

Every HR size is a multiple of 3, so at scales 3 and 1.5 the LR size times the scale is the HR size and every HR window is
inside its image.  At scales 2 and 4 the odd sizes make ceil() round up, and a crop at the far border asks for an HR window
that leaves the image: the reference's slice then returns a label smaller than the patch.  Those samples are recorded as
they are (`lb_<case>_<n>` is stored per sample for that reason) and flagged in `inside_<case>`; the kernel's precondition
is inside == True.
"""
import json
import math
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.modules["cv2"] = types.ModuleType("cv2")
sys.path.insert(0, os.path.dirname(HERE))                      # tests/: patch_ref
sys.path.insert(0, os.path.join(REF, "resample"))
sys.path.insert(0, REF)
import patch_ref  # noqa: E402
import data as ref_data  # noqa: E402
from common.option import TrainOptions  # noqa: E402

HR_SIZES = [(45, 57), (39, 51), (60, 39), (48, 48)]
FILES = ["0001", "0002", "0003", "0004"]
N = 24
CASES = [
    {"scale": 2, "sz": 7, "inC": 1, "nsigma": -1, "seed": 101},
    {"scale": 3, "sz": 6, "inC": 3, "nsigma": -1, "seed": 102},
    {"scale": 4, "sz": 8, "inC": 1, "nsigma": -1, "seed": 103},
    {"scale": 1.5, "sz": 9, "inC": 3, "nsigma": -1, "seed": 104},
    {"scale": 3, "sz": 6, "inC": 1, "nsigma": 5, "seed": 105, "np_seed": 205},
]


def replay(case, lr_ims):
    """the draws of one __getitem__ (data.py:108, 117, 118, 126, 132, 136, 140), written out"""
    key = random.choice(FILES)
    shape = lr_ims[key].shape
    i = random.randint(0, shape[0] - case["sz"])
    j = random.randint(0, shape[1] - case["sz"])
    c = random.choice([0, 1, 2]) if case["inC"] == 1 else 0
    fl = int(random.uniform(0, 1) < 0.5)
    fu = int(random.uniform(0, 1) < 0.5)
    k = random.choice([0, 1, 2, 3])
    s = case["scale"]
    return [FILES.index(key), i, j, int(i * s), int(j * s), c, fl, fu, k]


def main():
    rng = np.random.default_rng(30)
    out = {}
    hr_ims = {f: rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for f, (h, w) in zip(FILES, HR_SIZES)}
    for n, f in enumerate(FILES):
        out["hr_%d" % n] = hr_ims[f]
    for ci, case in enumerate(CASES):
        s, sz, C = case["scale"], case["sz"], case["inC"]
        hsz = int(sz * s)
        lr_ims = {f: rng.integers(0, 256, (math.ceil(h / s), math.ceil(w / s), 3), dtype=np.uint8)
                  for f, (h, w) in zip(FILES, HR_SIZES)}
        for n, f in enumerate(FILES):
            out["lr_%d_%d" % (ci, n)] = lr_ims[f]
        ds = ref_data.DIV2K.__new__(ref_data.DIV2K)
        ds.scale, ds.sz, ds.rigid_aug, ds.inC, ds.nsigma = s, sz, True, C, case["nsigma"]
        ds.file_list, ds.hr_ims, ds.lr_ims = FILES, hr_ims, lr_ims
        random.seed(case["seed"])
        if case["nsigma"] > 0:
            np.random.seed(case["np_seed"])
        got = [ds[0] for _ in range(N)]
        random.seed(case["seed"])
        draws = np.array([replay(case, lr_ims) for _ in range(N)], dtype=np.int64)
        noise = None
        if case["nsigma"] > 0:                                   # the same normal draws, kept: im = patch + noise
            np.random.seed(case["np_seed"])
            noise = np.stack([np.random.normal(0, case["nsigma"] / 255.0, (C, sz, sz)).astype(np.float32) for _ in range(N)])
            out["noise_%d" % ci] = noise
        inside = np.zeros(N, bool)
        for n, (im, lb) in enumerate(got):
            d = draws[n]
            rim, rlb = patch_ref.sample(lr_ims[FILES[d[0]]], hr_ims[FILES[d[0]]], d, sz, hsz, C, None if noise is None else noise[n])
            assert im.dtype == np.float32 and lb.dtype == np.float32
            assert np.array_equal(im.view(np.uint32), rim.view(np.uint32)), (ci, n)
            assert lb.shape == rlb.shape and np.array_equal(lb.view(np.uint32), rlb.view(np.uint32)), (ci, n)
            inside[n] = patch_ref.inside(hr_ims[FILES[d[0]]].shape, d, hsz)
            assert inside[n] == (lb.shape == (C, hsz, hsz))
            out["lb_%d_%d" % (ci, n)] = np.ascontiguousarray(lb)
        out["im_%d" % ci] = np.stack([np.ascontiguousarray(im) for im, _ in got])
        out["draws_%d" % ci] = draws
        out["inside_%d" % ci] = inside
        print("case %d %s: %d of %d samples inside" % (ci, case, int(inside.sum()), N))
    out["cases"] = np.array(json.dumps(CASES))
    out["files"] = np.array(json.dumps(FILES))

    import argparse
    ap = TrainOptions().initialize(argparse.ArgumentParser())
    opts = [[a.dest, a.default] for a in ap._actions if a.dest != "help"]
    out["options"] = np.array(json.dumps(opts))
    path = os.path.join(HERE, "g30_div2k.npz")
    np.savez_compressed(path, **out)
    print("-> %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
