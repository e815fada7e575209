"""CPU-only: the closed form of exact x2 SR geometry (csrc/lerf_host_geometry.h: x2_left, x2_dis, x2_owned -- what the X2 flavour
of the tile-fused kernels computes instead of reading tables) against the tables of the host geometry entry point,
lerf_sr_axis_tables, bit for bit: first tap, float32 and float64 distances (compared as integers) and the owned output ranges of
every tile, for every axis length 1..200 (both axes of a frame are tables of one axis each: every H and W in 1..200) and the
supports 2 and 4; and the builder's verdict, lerf_sr_geometry_flags, which is what sets LERF_GEO_EXACT_X2."""
import numpy as np
import pytest

from lerf_pytorch_amd import _lib

SIZES = range(1, 201)
TILES = (64, 32, 16)          # tile rows of the three RGB instances; tile columns are 64


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


@pytest.mark.parametrize("S", [2, 4])
def test_closed_form_equals_the_tables_bit_for_bit(S):
    for n in SIZES:
        left, d64, d32, _ = _lib.sr_axis_tables(n, 2 * n, 2.0, S)
        cl, c64, c32 = _lib.sr_x2_tables(2 * n, S)
        assert np.array_equal(left, cl), "first taps, n = %d" % n
        assert np.array_equal(_bits(d64), _bits(c64)), "float64 distances, n = %d" % n
        assert np.array_equal(_bits(d32), _bits(c32)), "float32 distances, n = %d" % n
        # the closed form, spelled out: first tap (i + 1) // 2 - S / 2, distances by the parity of i
        i = np.arange(2 * n)
        assert np.array_equal(cl, (i + 1) // 2 - S // 2)
        k = np.arange(S)
        assert np.array_equal(c64, (S // 2 - k)[None, :] - np.where(i % 2 == 1, 0.75, 0.25)[:, None])


@pytest.mark.parametrize("S", [2, 4])
def test_owned_ranges_equal_the_searches_in_the_tables(S):
    """a tile of T LR pixels from t0 owns the outputs whose first tap lies in [t0 - S/2, t0 + T - S/2), the first and the last
    tile what lies beyond the frame's borders: the table kernels find the bounds with lower-bound searches in `left`"""
    for n in SIZES:
        left = _lib.sr_axis_tables(n, 2 * n, 2.0, S)[0]
        for T in TILES:
            tn = (n + T - 1) // T
            want = np.empty((tn, 2), np.int32)
            for t in range(tn):
                want[t, 0] = 0 if t == 0 else np.searchsorted(left, t * T - S // 2, side="left")
                want[t, 1] = 2 * n if t == tn - 1 else np.searchsorted(left, (t + 1) * T - S // 2, side="left")
            got = _lib.sr_x2_owned(n, T)
            assert np.array_equal(got, want), "n = %d, tile %d" % (n, T)
            assert got[0, 0] == 0 and got[-1, 1] == 2 * n and np.array_equal(got[1:, 0], got[:-1, 1])     # a partition of the outputs


def test_builder_sets_the_promise_for_whole_frame_x2_only():
    def flags(H, W, sh, sw, S, oh=None, ow=None, edit=None):
        oh, ow = _lib.out_size(H, sh) if oh is None else oh, _lib.out_size(W, sw) if ow is None else ow
        lr, r64, r32, _ = _lib.sr_axis_tables(H, oh, sh, S)
        lc, c64, c32, _ = _lib.sr_axis_tables(W, ow, sw, S)
        if edit:
            edit(lr, r64, r32, lc, c64, c32)
        return _lib.sr_geometry_flags((H, W), (oh, ow), (sh, sw), S, lr, r64, r32, lc, c64, c32)

    for S in (2, 4):
        for H, W in ((1, 1), (65, 64), (70, 130), (200, 200)):
            assert flags(H, W, 2.0, 2.0, S) == _lib.GEO_EXACT_X2
        assert flags(70, 130, 2.0, 1.5, S) == 0 and flags(70, 130, 1.5, 2.0, S) == 0 and flags(70, 130, 3.0, 3.0, S) == 0
        assert flags(70, 130, 2.0, 2.0, S, oh=139) == 0                      # out != 2 x in
        assert flags(70, 130, 2.0 + 2 ** -40, 2.0, S, oh=140) == 0           # not exactly 2.0
        # one entry off by one unit in the last place, or one first tap moved: no promise
        assert flags(70, 130, 2.0, 2.0, S, edit=lambda lr, r64, r32, lc, c64, c32: r64.__setitem__((7, 0), np.nextafter(r64[7, 0], 9.0))) == 0
        assert flags(70, 130, 2.0, 2.0, S, edit=lambda lr, r64, r32, lc, c64, c32: c32.__setitem__((9, 1), np.nextafter(c32[9, 1], np.float32(9.0)))) == 0
        assert flags(70, 130, 2.0, 2.0, S, edit=lambda lr, r64, r32, lc, c64, c32: lc.__setitem__(100, lc[100] + 1)) == 0
    assert _lib.GEO_EXACT_X2 == 512 and _lib.GEO_FORCE_TABLES == 1024
