"""CPU anchor of tests/metrics_ref.py: what the exact GPU tests of the metric kernels rest on, shown with the reference
restatement (oracle/lerf_oracle.py) alone.  No GPU, no library call."""
import math
import warnings
from fractions import Fraction

import numpy as np
import pytest

import metrics_ref as MR

T0 = (0.256788235294118, 0.504129411764706, 0.097905882352941)     # common/utils.py:54, as the doubles they are


def _exact_y(rgb):
    return sum(Fraction(c) * v for c, v in zip(T0, rgb)) + 16


def _boundary_distance(y):
    """distance of the rational y to the nearest point where its float32 rounding changes (a midpoint of two neighbours)"""
    f = np.float32(float(y))
    lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
    mids = [(Fraction(float(f)) + Fraction(float(n))) / 2 for n in (lo, hi)]
    assert mids[0] < y < mids[1]
    return min(y - mids[0], mids[1] - y)


def test_primaries_y_is_far_from_a_float32_rounding_boundary(oracle):
    """A float64 evaluation of the Y dot product, in any order and contracted or not, is off by ~1e-13 at most (three products
    and three sums below 256, each within 2^-45).  The exact Y of every primary lies >= 4e-7 from the nearest float32 rounding
    boundary, so its float32 value is one number on every machine.  The smallest margin is black's: 16 is a power of two, the
    float32 spacing below it is 2^-20, half of that is 4.77e-7."""
    dist = {}
    for rgb in MR.PRIMARIES:
        y = _exact_y(rgb)
        dist[rgb] = float(_boundary_distance(y))
        px = np.array([[rgb]], dtype=np.uint8)
        assert np.float32(oracle.rgb2y(px)[0, 0]) == np.float32(float(y))
    assert min(dist.values()) >= 4e-7
    assert min(dist, key=dist.get) == (0, 0, 0) and dist[(0, 0, 0)] == 2.0 ** -21
    assert np.float32(float(_exact_y((0, 0, 0)))) == MR.Y_BLACK
    assert np.float32(float(_exact_y((255, 255, 255)))) == MR.Y_WHITE
    assert (np.float32(MR.Y_WHITE) - np.float32(MR.Y_BLACK)) ** 2 == MR.SQ_BW


def test_frame_makers():
    rng = np.random.default_rng(1)
    bw = MR.bw_frame(rng, 37, 41)
    assert bw.dtype == np.uint8 and bw.shape == (37, 41, 3)
    assert np.all((bw == 0) | (bw == 255)) and np.all(bw[:, :, 0] == bw[:, :, 1]) and np.all(bw[:, :, 0] == bw[:, :, 2])
    assert 0 < int((bw[:, :, 0] == 255).sum()) < 37 * 41
    pr = MR.primaries_frame(rng, 37, 41)
    assert pr.dtype == np.uint8 and np.all((pr == 0) | (pr == 255))
    assert len({tuple(p) for p in pr.reshape(-1, 3)}) == 8
    assert np.array_equal(MR.bw_frame(np.random.default_rng(7), 5, 6), MR.bw_frame(np.random.default_rng(7), 5, 6))


@pytest.mark.parametrize("shape,shave", [((9, 9), 4), ((64, 33), 0), ((1040, 1030), 3)])
def test_black_white_sum_is_an_integer_count(shape, shave):
    """exact_sum(y_terms) of black/white frames is 47 961 x (differing window pixels), whichever frame is called gt.  At
    1040 x 1030 that is below 5.1e10, far below 2^53: a float64 sum of these terms is exact in any order."""
    rng = np.random.default_rng(shape[0])
    a, b = MR.bw_frame(rng, *shape), MR.bw_frame(rng, *shape)
    win = (slice(shave, shape[0] - shave), slice(shave, shape[1] - shave))
    differing = int((a[win][:, :, 0] != b[win][:, :, 0]).sum())
    for gt, out in ((a, b), (b, a)):
        t = MR.y_terms(gt, out, shave)
        assert t.dtype == np.float32 and t.size == (shape[0] - 2 * shave) * (shape[1] - 2 * shave)
        assert set(np.unique(t).tolist()) <= {0.0, MR.SQ_BW}
        s = MR.exact_sum(t)
        assert s == MR.SQ_BW * differing and s == int(s) and s < 2.0 ** 53
        assert float(np.sum(t.astype(np.float64)[::-1])) == s


def test_terms_are_the_reference_terms(oracle):
    """y_terms is the correctly rounded float32 square d * d of the reference's float32 difference.  The reference writes
    np.power(diff, 2); numpy's vectorised float32 power is not correctly rounded on every build (here it is one float32 ulp
    off on a few entries), so that form is held to one ulp and the kernel to d * d.  Masked terms are 0 or 1 for frames in
    {0, 255}."""
    rng = np.random.default_rng(3)
    gt = rng.integers(0, 256, (23, 31, 3), dtype=np.uint8)
    out = rng.integers(0, 256, (23, 31, 3), dtype=np.uint8)
    d = (np.array(oracle.rgb2y(out), dtype=np.float32) - np.array(oracle.rgb2y(gt), dtype=np.float32))[2:-2, 2:-2].ravel()
    t = MR.y_terms(gt, out, 2)
    assert np.array_equal(t, (d.astype(np.float64) ** 2).astype(np.float32))      # the float64 square is exact: one rounding
    assert np.all(np.abs(np.power(d, 2) - t) <= np.spacing(t))
    sr, hr = MR.primaries_frame(rng, 23, 31), MR.primaries_frame(rng, 23, 31)
    mask = rng.integers(0, 2, sr.shape).astype(bool)
    t = MR.masked_terms(sr, hr, mask)
    assert t.dtype == np.float32 and set(np.unique(t).tolist()) <= {0.0, 1.0}
    assert MR.exact_sum(t) == int((mask & (sr != hr)).sum())
    assert np.array_equal(MR.masked_terms(sr, hr, mask.astype(np.uint8) * 255), t)        # non-zero is inside


@pytest.mark.parametrize("shape,shave", [((40, 52), 2), ((64, 33), 4), ((11, 11), 0), ((300, 257), 3)])
def test_oracle_db_agrees_with_the_exact_sums(oracle, shape, shave):
    """the oracle averages in float32 (numpy pairwise); the dB values from the exact sums differ by far less than 1e-4 dB"""
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    gt = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    out = np.clip(gt.astype(int) + rng.integers(-12, 13, gt.shape), 0, 255).astype(np.uint8)
    t = MR.y_terms(gt, out, shave)
    assert abs(oracle.psnr_y(gt, out, shave) - MR.psnr_db(MR.exact_sum(t), t.size)) < 1e-4
    mask = rng.integers(0, 2, gt.shape).astype(bool)
    tm = MR.masked_terms(out, gt, mask)
    assert abs(oracle.mpsnr(out, gt, mask) - MR.mpsnr_db(MR.exact_sum(tm), float(mask.sum()), tm.size)) < 1e-4


@pytest.mark.parametrize("shape", [(11, 11), (27, 43), (64, 33)])
def test_oracle_ssim_of_equal_frames_is_exactly_one(oracle, shape):
    """with equal inputs the numerator and the denominator of every map entry are the same floating-point value"""
    a = np.random.default_rng(shape[1]).integers(0, 256, shape + (3,), dtype=np.uint8)
    assert oracle.ssim_y(a, a.copy()) == 1.0


def test_oracle_degenerate_results(oracle):
    """what the reference gives for empty sums (with numpy warnings): the library returns the same (metrics.psnr_y, mpsnr)"""
    rng = np.random.default_rng(11)
    a = rng.integers(0, 256, (20, 24, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (20, 24, 3), dtype=np.uint8)
    full, empty = np.ones(a.shape, bool), np.zeros(a.shape, bool)
    some = rng.integers(0, 2, a.shape).astype(bool)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        assert oracle.psnr_y(a, a.copy(), 2) == math.inf
        assert oracle.psnr_y(a, a.copy(), 0) == math.inf
        assert math.isnan(oracle.mpsnr(a, b, empty))
        assert math.isnan(oracle.mpsnr(a, a.copy(), empty))
        assert oracle.mpsnr(a, a.copy(), some) == math.inf
        assert oracle.mpsnr(a, a.copy(), full) == math.inf


def test_tables_format_an_infinite_score():
    """one perfect image puts an inf into a column; the tables print it as the reference's '{:.2f}' does"""
    from lerf_pytorch_amd.resample import eval_harness as EH

    class Stub:
        def run_sr_many(self, dataset, scales):
            return {sc: [[math.inf, 1.0], [30.0, 0.9]] for sc in scales}

        def run_warp(self, dataset, mode):
            return [[math.inf], [30.0]] if mode == "isc" else [[math.nan], [30.0]]

    lines = EH.sr_table(Stub(), scales=((2, 2), (3, 3)))
    assert lines[1].split() == ["Set5", "inf/0.9500", "inf/0.9500"]
    lines = EH.warp_table(Stub())
    assert lines[1].split() == ["Set5", "inf", "nan"]
