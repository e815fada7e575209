"""The checker of the DIV2K patch kernel: the reference's per-sample statements (resample/data.py:116-152, 163) in numpy.

A draw is the row the fixture stores: (file, li, lj, hi, hj, chan, fliplr, flipud, k).  `patch` is one side of one sample,
`sample` both; a crop that leaves its image is cut short by the slice, as in the reference."""
import numpy as np


def patch(img, i, j, n, C, chan, fliplr, flipud, k):
    """img uint8 [H, W, 3] -> float32 [C, n, n]"""
    a = img[i:i + n, j:j + n, :]                     # 1. crop
    if C == 1:
        a = a[:, :, chan]                            # 2. the channel
    if fliplr:
        a = np.fliplr(a)                             # 3.
    if flipud:
        a = np.flipud(a)                             # 4.
    a = np.rot90(a, k)                               # 5.
    a = a.astype(np.float32) / 255.0                 # 6. float32 / python float -> float32 division
    return np.expand_dims(a, axis=0) if C == 1 else np.transpose(a, [2, 0, 1])


def sample(lr, hr, draw, sz, hsz, C, noise=None):
    """(im [C, sz, sz], lb [C, hsz, hsz]) float32 of one draw; `noise` float32 [C, sz, sz] is added to im"""
    _, li, lj, hi, hj, chan, fl, fu, k = (int(v) for v in draw)
    im = patch(lr, li, lj, sz, C, chan, fl, fu, k)
    lb = patch(hr, hi, hj, hsz, C, chan, fl, fu, k)
    if noise is not None:
        im = im + noise
    return im, lb


def inside(hr_shape, draw, hsz):
    """whether the HR window of the draw lies inside the HR image (the kernel's precondition)"""
    return int(draw[3]) + hsz <= hr_shape[0] and int(draw[4]) + hsz <= hr_shape[1]
