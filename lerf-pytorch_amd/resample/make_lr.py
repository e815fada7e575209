"""Make the low-resolution side of an SR benchmark from its HR images, with the resize that made the shipped
`rrLR_X*` folders (resize_right.resize: cubic, anti-aliased, on the GPU):

    python -m lerf_pytorch_amd.resample.make_lr --testDir D --datasets Set5 --scales 2x2 3x3 1.5x2

writes D/<dataset>/LR_bicubic/rrLR_X{h:.2f}_{w:.2f}/<name>.png from D/<dataset>/HR/<name>.png, the layout
eval_harness and eval_model read.

Integer pairs follow the rule that reproduces the shipped Set5 folders byte for byte: H and W are cut down to multiples
of the scale (`modcrop`, common/utils.py:31-42 of the reference), the crop is resized in float64 with
scale_factors=[1/h, 1/w], and the result is rounded half to even and clipped to uint8.  For NON-INTEGER pairs nothing of
the authors' survives to compare against: the same function runs on the UNCROPPED HR image.  That rule is this project's
choice, not a reproduction.

An existing scale folder is not overwritten unless --force is given.
"""
from __future__ import annotations

import argparse
import os

import numpy as np

from ..resize_right.resize_right import resize_to_uint8


def parse_pair(text):
    """'3x3' / '1.5x2' / '2' -> (h, w) floats"""
    parts = text.lower().split("x")
    if len(parts) == 1:
        parts = parts * 2
    if len(parts) != 2:
        raise argparse.ArgumentTypeError("a scale pair looks like 2x2 or 1.5x2, not %r" % text)
    try:
        h, w = float(parts[0]), float(parts[1])
    except ValueError:
        raise argparse.ArgumentTypeError("a scale pair looks like 2x2 or 1.5x2, not %r" % text)
    if not (h > 0 and w > 0):
        raise argparse.ArgumentTypeError("scales must be positive: %r" % text)
    return h, w


def modcrop(img, sh, sw):
    """cut H and W down to multiples of the (integer) scales"""
    H, W = img.shape[:2]
    return img[:H - H % sh, :W - W % sw]


def make_lr_image(hr, sh, sw):
    """uint8 HR image [H, W(, C)] -> uint8 LR image (a numpy array)"""
    hr = np.asarray(hr)
    if float(sh).is_integer() and float(sw).is_integer():
        hr = modcrop(hr, int(sh), int(sw))
    lr = resize_to_uint8(np.ascontiguousarray(hr).astype(np.float64), scale_factors=[1 / sh, 1 / sw])
    return np.asarray(lr)


def lr_folder(test_dir, dataset, sh, sw):
    return os.path.join(test_dir, dataset, "LR_bicubic", "rrLR_X{:.2f}_{:.2f}".format(sh, sw))


def make_lr(test_dir, datasets, scales, force=False):
    """-> list of folders written"""
    from PIL import Image
    done = []
    for ds in datasets:
        hr_dir = os.path.join(test_dir, ds, "HR")
        files = sorted(f for f in os.listdir(hr_dir) if "png" in f)
        for sh, sw in scales:
            out_dir = lr_folder(test_dir, ds, sh, sw)
            if os.path.exists(out_dir) and not force:
                raise FileExistsError("%s exists; pass --force to overwrite it" % out_dir)
            os.makedirs(out_dir, exist_ok=True)
            for f in files:
                hr = np.array(Image.open(os.path.join(hr_dir, f)))
                Image.fromarray(make_lr_image(hr, sh, sw)).save(os.path.join(out_dir, f))
            done.append(out_dir)
    return done


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--testDir", type=str, default="./data/rrBenchmark")
    ap.add_argument("--datasets", type=str, nargs="+", default=["Set5"])
    ap.add_argument("--scales", type=parse_pair, nargs="+", default=[(2.0, 2.0), (3.0, 3.0), (4.0, 4.0)])
    ap.add_argument("--force", action="store_true", default=False, help="overwrite existing rrLR_X* folders")
    opt = ap.parse_args(argv)
    for d in make_lr(opt.testDir, opt.datasets, opt.scales, opt.force):
        print(d)


if __name__ == "__main__":
    main()
