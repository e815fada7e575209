"""Exact GPU tests of the three metric kernels (csrc/lerf_metrics.hip: y_sse_kernel, ssim_y_kernel, masked_sse_kernel) through
the raw (sum, count) pairs of metrics.y_sse / ssim_y_sum / masked_sse.

The yardstick is tests/metrics_ref.py, anchored by tests/test_metrics_ref_cpu.py:
  * black/white frames: every term of y_sse is 0 or 47 961 and every partial sum is an integer below 2^53, so the device sum
    is exact in any order and one dropped, doubled or misplaced pixel changes it: `==` on both doubles.
  * frames in {0, 255} under a bool mask: every term of masked_sse is 0 or 1.0: `==` again.
  * eight-primaries frames (y_sse) and random uint8 frames (masked_sse): the device's float32 terms are the reference's terms
    bit for bit, only the order of the float64 additions differs.  |device - fsum| <= N * 2^-52 * fsum  (metrics_ref.sum_bound).
    The block sums reach `result` through atomics, whose order changes from run to run: two runs are therefore compared to
    each other with that same bound, not bit for bit.
  * SSIM of equal frames is exactly 1 per map entry (numerator and denominator are the same value), so the sum is the count.

Both SSE kernels cap their grid at 4096 workgroups of 256 threads; shapes above 1 048 576 terms make every thread take more
than one trip of its grid-stride loop."""
import functools
import math

import numpy as np
import pytest

import metrics_ref as MR

pytestmark = pytest.mark.gpu

CAP = 4096 * 256                      # grid_for(): threads of the largest grid of the two SSE kernels


@pytest.fixture(scope="module")
def M():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from lerf_pytorch_amd import metrics
    return metrics


def _pair(t):
    s, n = t.tolist()
    return s, n


def _window(a, shave):
    return a[shave:a.shape[0] - shave, shave:a.shape[1] - shave]


def _pitched(gt, out, pads=((2, 3), (7, 4))):
    """views buf[:, c0:c0 + W] of two wider device buffers with different pitches and non-zero c0.  The surplus columns are
    white beside gt and black beside out: a read of the padding meets a pixel pair that differs."""
    import torch
    views = []
    for a, (c0, c1), fill in ((gt, pads[0], 255), (out, pads[1], 0)):
        H, W = a.shape[:2]
        buf = torch.full((H, c0 + W + c1, 3), fill, dtype=torch.uint8, device="cuda")
        v = buf[:, c0:c0 + W]
        v.copy_(torch.from_numpy(a))
        assert not v.is_contiguous() and v.stride(1) == 3 and v.data_ptr() != buf.data_ptr()
        views.append(v)
    assert views[0].stride(0) != views[1].stride(0)
    return views


# ---------------------------------------------------------------------------------------------------------------------------
# coverage: every window pixel / element exactly once
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame,shave,window", [
    ((9, 9), 4, (1, 1)),
    ((7, 306), 3, (1, 300)),
    ((306, 7), 3, (300, 1)),
    ((259, 261), 2, (255, 257)),
    ((1025, 1027), 0, (1025, 1027)),
    ((1031, 1033), 3, (1025, 1027)),
])
def test_y_sse_counts_every_window_pixel_once(M, frame, shave, window):
    rng = np.random.default_rng(frame[0] * 7 + frame[1])
    gt, out = MR.bw_frame(rng, *frame), MR.bw_frame(rng, *frame)
    wg, wo = _window(gt, shave), _window(out, shave)
    assert wg.shape[:2] == window
    if window == (1025, 1027):
        assert window[0] * window[1] > CAP            # the smallest ragged window above the cap: more than one trip
    differing = int((wg[:, :, 0] != wo[:, :, 0]).sum())
    if window != (1, 1):
        assert 0 < differing < window[0] * window[1]
        assert int((gt[:, :, 0] != out[:, :, 0]).sum()) != differing or shave == 0     # the border differs too
    s, n = _pair(M.y_sse(gt, out, shave))
    assert s == MR.SQ_BW * differing
    assert n == float(window[0] * window[1])


@pytest.mark.parametrize("shape", [(1,), (255,), (256,), (257,), (65537,), (593, 590, 3)])
def test_masked_sse_counts_every_element_once(M, shape):
    n = int(np.prod(shape))
    if len(shape) == 3:
        assert n == 1049610 and n > CAP
    rng = np.random.default_rng(n)
    sr = (rng.integers(0, 2, shape) * 255).astype(np.uint8)
    hr = (rng.integers(0, 2, shape) * 255).astype(np.uint8)
    mask = rng.integers(0, 2, shape).astype(bool)
    if n == 1:
        sr[...], hr[...], mask[...] = 255, 0, True
    s, c = _pair(M.masked_sse(sr, hr, mask))
    assert s == float((mask & (sr != hr)).sum())
    assert c == float(mask.sum())


# ---------------------------------------------------------------------------------------------------------------------------
# position: the shaved window starts and ends where the reference's diff[shave:-shave, shave:-shave] does
# ---------------------------------------------------------------------------------------------------------------------------
_PH, _PW, _PS = 37, 45, 3            # window rows 3..33, columns 3..41: 31 x 39 = 1209 pixels, five workgroups
_INSIDE = [(3, 3), (3, 41), (33, 3), (33, 41), (3, 22), (33, 22), (18, 3), (18, 41)]
_OUTSIDE = [(2, 2), (2, 42), (34, 2), (34, 42), (2, 3), (3, 2), (34, 41), (33, 42), (0, 0), (36, 44)]


@pytest.mark.parametrize("pitched", [False, True])
def test_y_sse_window_position(M, pitched):
    gt = np.zeros((_PH, _PW, 3), np.uint8)
    for pos, want in [(p, MR.SQ_BW) for p in _INSIDE] + [(p, 0.0) for p in _OUTSIDE]:
        out = np.zeros_like(gt)
        out[pos] = 255
        a, b = _pitched(gt, out) if pitched else (gt, out)
        assert _pair(M.y_sse(a, b, _PS)) == (want, 31.0 * 39.0), pos
        assert _pair(M.y_sse(b, a, _PS)) == (want, 31.0 * 39.0), pos


def test_y_sse_pitched_views_above_the_cap(M):
    """pitch arithmetic at rows past the first trip of the grid-stride loop"""
    rng = np.random.default_rng(99)
    gt, out = MR.bw_frame(rng, 1031, 1033), MR.bw_frame(rng, 1031, 1033)
    differing = int((_window(gt, 3)[:, :, 0] != _window(out, 3)[:, :, 0]).sum())
    a, b = _pitched(gt, out)
    assert _pair(M.y_sse(a, b, 3)) == (MR.SQ_BW * differing, 1025.0 * 1027.0)


# ---------------------------------------------------------------------------------------------------------------------------
# values, tight
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _y_case(frame, shave):
    rng = np.random.default_rng(frame[0] + frame[1] + shave)
    gt, out = MR.primaries_frame(rng, *frame), MR.primaries_frame(rng, *frame)
    t = MR.y_terms(gt, out, shave)
    return gt, out, t.size, MR.exact_sum(t)


@functools.lru_cache(maxsize=None)
def _masked_case(shape):
    rng = np.random.default_rng(shape[0] + shape[1])
    sr = rng.integers(0, 256, shape, dtype=np.uint8)
    hr = rng.integers(0, 256, shape, dtype=np.uint8)
    mask = rng.integers(0, 2, shape).astype(bool)
    t = MR.masked_terms(sr, hr, mask)
    return sr, hr, mask, t.size, MR.exact_sum(t)


@pytest.mark.parametrize("frame,shave", [((64, 33), 0), ((64, 33), 4), ((1025, 1027), 0), ((1031, 1033), 3)])
def test_y_sse_values_tight(M, frame, shave):
    gt, out, n, exact = _y_case(frame, shave)
    bound = MR.sum_bound(n, exact)
    s1, n1 = _pair(M.y_sse(gt, out, shave))
    s2, n2 = _pair(M.y_sse(gt, out, shave))
    print("y_sse %s shave %d: N = %d, |device - exact| / bound = %.3g, run to run %.3g"
          % (frame, shave, n, abs(s1 - exact) / bound, abs(s1 - s2) / bound))
    assert n1 == n2 == float(n) and exact > 0
    assert abs(s1 - exact) <= bound and abs(s2 - exact) <= bound
    assert abs(s1 - s2) <= bound                      # atomics: the order differs from run to run, so not bit for bit


@pytest.mark.parametrize("shape", [(64, 33, 3), (593, 590, 3)])
def test_masked_sse_values_tight(M, shape):
    sr, hr, mask, n, exact = _masked_case(shape)
    bound = MR.sum_bound(n, exact)
    s1, c1 = _pair(M.masked_sse(sr, hr, mask))
    s2, c2 = _pair(M.masked_sse(sr, hr, mask))
    print("masked_sse %s: N = %d, |device - exact| / bound = %.3g, run to run %.3g"
          % (shape, n, abs(s1 - exact) / bound, abs(s1 - s2) / bound))
    assert c1 == c2 == float(mask.sum()) and exact > 0
    assert abs(s1 - exact) <= bound and abs(s2 - exact) <= bound
    assert abs(s1 - s2) <= bound                      # atomics: the order differs from run to run, so not bit for bit


# ---------------------------------------------------------------------------------------------------------------------------
# SSIM: 16 x 16 output tiles, 26 x 26 clamped patches
# ---------------------------------------------------------------------------------------------------------------------------
_SEAM = [1, 15, 16, 17, 33]
_SEAMS = [(oh, ow) for oh in _SEAM for ow in _SEAM]


@functools.lru_cache(maxsize=None)
def _ssim_frames(oh, ow):
    rng = np.random.default_rng(oh * 100 + ow)
    gt = rng.integers(0, 256, (oh + 10, ow + 10, 3), dtype=np.uint8)
    out = np.clip(gt.astype(int) + rng.integers(-12, 13, gt.shape), 0, 255).astype(np.uint8)
    return gt, out


@pytest.mark.parametrize("oh,ow", _SEAMS)
def test_ssim_equal_frames_sum_to_the_count(M, oh, ow):
    gt, _ = _ssim_frames(oh, ow)
    assert _pair(M.ssim_y_sum(gt, gt.copy())) == (float(oh * ow), float(oh * ow))
    assert M.ssim_y(gt, gt.copy()) == 1.0


@pytest.mark.parametrize("oh,ow", _SEAMS)
def test_ssim_seams_vs_oracle(M, oracle, oh, ow):
    gt, out = _ssim_frames(oh, ow)
    want = oracle.ssim_y(gt, out)
    s, n = _pair(M.ssim_y_sum(gt, out))
    assert n == float(oh * ow)
    assert abs(s / n - want) < 1e-9
    assert abs(M.ssim_y(gt, out) - want) < 1e-9


@pytest.mark.parametrize("oh,ow", _SEAMS)
def test_ssim_impulse_vs_oracle(M, oracle, oh, ow):
    """out = gt except one pixel, black in gt and white in out (255 levels in every channel; opposite moves of the channels
    would cancel in Y).  A frame corner enters one window only, with the smallest weight of the 11 x 11 Gaussian (1.05e-6),
    and still moves the mean of the largest map here by 1.1e-8, ten times the tolerance: a load that misses the pixel, or a
    clamp that repeats it, shows."""
    base, _ = _ssim_frames(oh, ow)
    H, W = base.shape[:2]
    ran = 0
    for y, x in [(0, 0), (H - 1, W - 1), (H - 1, 0), (15, 16), (16, 15), (25, 26)]:
        if y >= H or x >= W:
            continue
        gt = base.copy()
        gt[y, x] = 0
        out = gt.copy()
        out[y, x] = 255
        want = oracle.ssim_y(gt, out)
        assert 1.0 - want > 1e-8
        assert abs(M.ssim_y(gt, out) - want) < 1e-9, (y, x)
        ran += 1
    assert ran >= 3 and (ran == 6 or min(H, W) < 27)


def test_ssim_pitched_views(M, oracle):
    gt, out = _ssim_frames(33, 17)
    a, b = _pitched(gt, out)
    assert abs(M.ssim_y(a, b) - oracle.ssim_y(gt, out)) < 1e-9
    a, b = _pitched(gt, gt)
    assert _pair(M.ssim_y_sum(a, b)) == (33.0 * 17.0, 33.0 * 17.0)
    dark, imp = gt.copy(), gt.copy()
    dark[42, 26], imp[42, 26] = 0, 255                    # last row, last column: the clamped loads of the edge tiles
    a, b = _pitched(dark, imp)
    assert abs(M.ssim_y(a, b) - oracle.ssim_y(dark, imp)) < 1e-9


# ---------------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------------
def test_metrics_on_a_side_stream(M):
    """CUDA-tensor inputs, launches on a non-default stream.  Frames with exact sums give equal dB values; random ones meet
    the bounds of the tight tests (SSIM: N map entries of magnitude <= 1, so the mean moves by N * 2^-52 at most)."""
    import torch
    rng = np.random.default_rng(21)
    bw_a, bw_b = MR.bw_frame(rng, 70, 90), MR.bw_frame(rng, 70, 90)
    bmask = rng.integers(0, 2, bw_a.shape).astype(bool)
    gt, out, n_y, exact_y = _y_case((64, 33), 4)
    sr, hr, mask, n_m, exact_m = _masked_case((64, 33, 3))
    host = [bw_a, bw_b, bmask, gt, out, sr, hr, mask]

    def run(t):
        A, B, BM, GT, OUT, SR, HR, MASK = t
        return (M.psnr_y(A, B, 3), M.mpsnr(A, B, BM), M.ssim_y(A, B), _pair(M.y_sse(GT, OUT, 4)),
                _pair(M.masked_sse(SR, HR, MASK)))

    dev = [torch.from_numpy(a).cuda() for a in host]
    base = run(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side
        got = run(dev)
    side.synchronize()
    assert math.isfinite(base[0]) and math.isfinite(base[1])
    assert got[0] == base[0] and got[1] == base[1]
    assert abs(got[2] - base[2]) <= 60 * 80 * 2.0 ** -52
    assert got[3][1] == float(n_y) and abs(got[3][0] - exact_y) <= MR.sum_bound(n_y, exact_y)
    assert got[4][1] == float(mask.sum()) and abs(got[4][0] - exact_m) <= MR.sum_bound(n_m, exact_m)
    assert run(host)[:2] == base[:2]                     # numpy inputs take the same path


def test_uint8_mask_reads_non_zero_as_inside(M):
    """the *_mask.png the harness writes holds 0/255; a 1 or a 128 is inside as well"""
    import torch
    rng = np.random.default_rng(8)
    shape = (50, 41, 3)
    sr = (rng.integers(0, 2, shape) * 255).astype(np.uint8)
    hr = (rng.integers(0, 2, shape) * 255).astype(np.uint8)
    mask = rng.integers(0, 2, shape).astype(bool)
    want = (float((mask & (sr != hr)).sum()), float(mask.sum()))
    assert _pair(M.masked_sse(sr, hr, mask)) == want
    assert _pair(M.masked_sse(sr, hr, mask.astype(np.uint8) * 255)) == want
    assert _pair(M.masked_sse(sr, hr, mask.astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8))) == want
    assert _pair(M.masked_sse(sr, hr, torch.from_numpy(mask).cuda())) == want
    assert M.mpsnr(sr, hr, mask.astype(np.uint8) * 255) == M.mpsnr(sr, hr, mask)
    assert "non-zero is inside" in M.mpsnr.__doc__


def test_refusals(M):
    import torch
    ok = torch.zeros((40, 40, 3), dtype=torch.uint8, device="cuda")
    chw = torch.zeros((3, 40, 40), dtype=torch.uint8, device="cuda").permute(1, 2, 0)
    rgba = torch.zeros((40, 40, 4), dtype=torch.uint8, device="cuda")[:, :, :3]
    assert chw.shape == ok.shape and rgba.shape == ok.shape and rgba.stride(1) != 3
    for bad in (chw, rgba, ok.float(), np.zeros((40, 40, 3), np.float32)):
        for fn in (lambda a, b: M.psnr_y(a, b, 2), M.ssim_y, lambda a, b: M.y_sse(a, b, 2), M.ssim_y_sum):
            with pytest.raises(ValueError):
                fn(bad, ok)
            with pytest.raises(ValueError):
                fn(ok, bad)
    with pytest.raises(ValueError):
        M.mpsnr(ok.float(), ok, ok)
    small = np.zeros((10, 40, 3), np.uint8)
    with pytest.raises(ValueError):
        M.ssim_y(small, small)
    with pytest.raises(ValueError):
        M.ssim_y(small.transpose(1, 0, 2), small.transpose(1, 0, 2))
    assert M.ssim_y(np.zeros((11, 40, 3), np.uint8), np.zeros((11, 40, 3), np.uint8)) == 1.0
    with pytest.raises(ValueError):
        M.psnr_y(np.zeros((8, 12, 3), np.uint8), np.ones((8, 12, 3), np.uint8), 4)       # H - 2 * shave == 0
    with pytest.raises(ValueError):
        M.psnr_y(np.zeros((12, 8, 3), np.uint8), np.ones((12, 8, 3), np.uint8), 4)       # W - 2 * shave == 0


# ---------------------------------------------------------------------------------------------------------------------------
# empty sums: what the reference gives (tests/test_metrics_ref_cpu.py::test_oracle_degenerate_results)
# ---------------------------------------------------------------------------------------------------------------------------
def test_psnr_of_equal_windows_is_inf(M):
    rng = np.random.default_rng(31)
    a = rng.integers(0, 256, (20, 24, 3), dtype=np.uint8)
    assert M.psnr_y(a, a.copy(), 2) == math.inf
    assert M.psnr_y(a, a.copy(), 0) == math.inf
    b = a.copy()
    b[:2], b[-2:], b[:, :2], b[:, -2:] = 0, 255, 0, 255          # differs in the shaved border only
    assert M.psnr_y(a, b, 2) == math.inf
    assert math.isfinite(M.psnr_y(a, b, 1))


def test_mpsnr_of_empty_sums(M):
    rng = np.random.default_rng(32)
    a = rng.integers(0, 256, (20, 24, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (20, 24, 3), dtype=np.uint8)
    empty = np.zeros(a.shape, bool)
    some = rng.integers(0, 2, a.shape).astype(bool)
    assert math.isnan(M.mpsnr(a, b, empty))
    assert math.isnan(M.mpsnr(a, a.copy(), empty))
    assert M.mpsnr(a, a.copy(), some) == math.inf
    assert M.mpsnr(a, a.copy(), np.ones(a.shape, bool)) == math.inf
    assert M.mpsnr(np.where(some, a, b), a, some) == math.inf    # differs outside the mask only
    assert math.isfinite(M.mpsnr(a, b, some))
