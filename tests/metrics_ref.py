"""Yardstick of the metric kernels (csrc/lerf_metrics.hip), independent of the package: the float32 terms that the reference's
PSNR (common/utils.py:138-151) and mPSNR (:168-175) square and average, formed with plain numpy exactly as the reference forms
them, and their exact sum by math.fsum.  A device sum is then held against a number that carries no summation error of its own.

Frames made of black/white pixels or of the eight RGB primaries have a float32 Y that does not depend on how the float64 dot
product was evaluated (tests/test_metrics_ref_cpu.py shows the margin), so the device's terms are the same numbers as these and
only the order of the float64 additions differs."""
import math

import numpy as np

from oracle import lerf_oracle as O

Y_BLACK, Y_WHITE = 16.0, 235.0
SQ_BW = 47961.0                # (235 - 16)^2: the one non-zero term a black/white pair can have

PRIMARIES = [(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)]


def y_terms(gt, out, shave):
    """float32 squared Y differences of the shaved window, flattened row by row (PSNR, utils.py:143-149)"""
    a = np.array(O.rgb2y(gt), dtype=np.float32)
    b = np.array(O.rgb2y(out), dtype=np.float32)
    diff = b - a
    if shave > 0:
        diff = diff[shave:-shave, shave:-shave]
    assert diff.dtype == np.float32
    return (diff * diff).ravel()


def masked_terms(sr, hr, mask):
    """float32 (m * (sr - hr) / 255)^2, every step in float32 and left to right (mPSNR, utils.py:170-174); m is 1 where the
    mask is non-zero"""
    m = (np.asarray(mask) != 0).astype(np.float32)
    d = m * (np.asarray(sr).astype(np.float32) - np.asarray(hr).astype(np.float32)) / np.float32(255)
    assert d.dtype == np.float32
    return (d * d).ravel()


def exact_sum(terms):
    """the sum of the terms, correctly rounded to float64"""
    return math.fsum(np.asarray(terms, dtype=np.float64).ravel().tolist())


def psnr_db(sse, n):
    return 20.0 * math.log10(255.0 / math.sqrt(sse / n))


def mpsnr_db(sse, msum, n):
    return -10.0 * math.log10((n / msum) * (sse / n))


def bw_frame(rng, h, w):
    """uint8 [h, w, 3]: every pixel (0,0,0) or (255,255,255)"""
    return np.repeat((rng.integers(0, 2, (h, w, 1)) * 255).astype(np.uint8), 3, axis=2)


def primaries_frame(rng, h, w):
    """uint8 [h, w, 3]: every channel 0 or 255"""
    return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)


def sum_bound(n_terms, exact):
    """|float64 sum in any order - exact| for n non-negative terms that are exact in float64: (n - 1) * 2^-53 relative to first
    order; the bound doubles that"""
    return n_terms * 2.0 ** -52 * exact
