"""GPU: the LeRF-G stage-2 binning of the tile-fused kernels (csrc/lerf_fused_impl.h: counting sort of the hyper-region
positions into three level bins, whole-wave padding, empty-bin skip, the per-bin LUT piece) on crafted level maps.

tests/bin_frames.py supplies identity stage-1 tables (feat == img, so the test image IS the level map stage 2 bins) and
frames whose tiles have a chosen bin census: one bin only, one stray position, an empty middle / first bin, totals on and
next to multiples of 64, bins keyed by wave or striped through every thread, end levels only, frames of a few positions, and
interior tiles.  tests/test_bin_frames_cpu.py pins the census of every frame used here.

Everything is compared exactly with the numpy oracle: the packed stages (with the shipped and with random stage-2 tables,
where any wrong entry read shows) through every EMIT instance, and full SR x2 with the shipped tables through every launch
path of the SR kernels.  LeRF-L (no bins) runs the same frames as a control."""
import numpy as np
import pytest

import bin_frames as bf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


# --------------------------------------------------------------------------- tables, engines and oracle results, once each
_TABLES, _ENGINES, _STAGES, _SR = {}, {}, {}, {}


def _tables(which, luts_g, luts_l):
    """'shipped' / 'random' (LeRF-G), 'l-shipped' / 'l-random' (LeRF-L, oC = 1): identity stage 1 in all of them"""
    if which not in _TABLES:
        base = bf.identity_stage1(luts_l if which.startswith("l-") else luts_g)
        _TABLES[which] = bf.random_stage2(base, 2024) if which.endswith("random") else base
    return _TABLES[which]


def _engine(which, S, luts_g, luts_l):
    import lerf_pytorch_amd as L
    if (which, S) not in _ENGINES:
        luts = L.LutSet.from_arrays(_tables(which, luts_g, luts_l))
        assert luts.struct.fused_pack is not None and luts.oC == (1 if which.startswith("l-") else 3)
        _ENGINES[(which, S)] = L.LerfEngine(luts, support=S)
    return _ENGINES[(which, S)]


def _ref_stages(oracle, frame, which, luts_g, luts_l):
    key = (frame.name, which)
    if key not in _STAGES:
        feat, hq = oracle.lut_stages(frame.img, _tables(which, luts_g, luts_l), 1 if which.startswith("l-") else 3)
        assert np.array_equal(feat, frame.img), "identity stage-1 tables"
        feat.setflags(write=False)
        hq.setflags(write=False)
        _STAGES[key] = (feat, hq)
    return _STAGES[key]


def _ref_sr(oracle, frame, S, luts_g, luts_l):
    """oracle.sr_pipeline(img, shipped tables, 2, 2, S) as its own two steps (test_bin_frames_cpu pins the equality), so the
    stage outputs are computed once per frame: (float64 before rounding, uint8)"""
    key = (frame.name, S)
    if key not in _SR:
        feat, hq = _ref_stages(oracle, frame, "shipped", luts_g, luts_l)
        f64 = oracle.resize_u8(feat, hq, 2, 2, S, 10, "gauss")
        _SR[key] = (f64, oracle.to_u8(f64))
    return _SR[key]


# --------------------------------------------------------------------------- comparisons
def _check_stages(torch, ops, packed, oC, refs, what):
    """packed [N, H, W, C] against a list of N (feat, hq) oracle pairs"""
    feat, hq = ops.unpack_stages(packed, oC)
    feat, hq = feat.cpu().numpy(), hq.cpu().numpy()
    for i, (rf, rh) in enumerate(refs):
        assert np.array_equal(feat[i], rf), "%s, frame %d: feat differs at %d positions" % (what, i, int((feat[i] != rf).sum()))
        if not np.array_equal(hq[i], rh):
            bad = np.argwhere((hq[i] != rh).any(-1))
            vals = rf[tuple(bad.T)]
            raise AssertionError("%s, frame %d: hq differs at %d positions, first (y, x, ch) = %s, bins of the centre values %s" %
                                 (what, i, len(bad), bad[0].tolist(), np.bincount(bf.bins_of(vals), minlength=3).tolist()))


def _check_sr(got, ref, what, hq_ok=None):
    f64, u8 = ref
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.shape == u8.shape, what
    if not np.array_equal(got, u8):
        bad = np.argwhere(got != u8)
        first = [(tuple(b.tolist()), int(got[tuple(b)]), int(u8[tuple(b)]), float(f64[tuple(b)])) for b in bad[:5]]
        stage = {None: "", True: " -- hq equals the oracle: a stage-3 finding", False: " -- hq differs as well: stage 2"}[hq_ok]
        raise AssertionError("%s: %d bytes differ%s; (index, got, oracle, oracle float64 before rounding): %s" % (what, len(bad), stage, first))


def _hq_ok(torch, ops, eng, x, ref_stages):
    f, h = ops.unpack_stages(ops.stages_packed(x, eng.luts), eng.luts.oC)
    return bool(np.array_equal(f.cpu().numpy(), ref_stages[0]) and np.array_equal(h.cpu().numpy(), ref_stages[1]))


def _sr_every_path(torch, oracle, luts_g, luts_l, frame, S, tile_rows=True):
    """full SR x2 of one frame through every launch path == the oracle, byte for byte"""
    from lerf_pytorch_amd import _lib, ops
    eng = _engine("shipped", S, luts_g, luts_l)
    img = frame.img
    H, W, C = img.shape
    x = torch.from_numpy(img).cuda()
    geo = eng.sr_geometry((H, W), 2)
    variants = [("default", geo)]
    if tile_rows:
        variants += [("rows64", geo.with_flags(_lib.GEO_TILE_ROWS_64)), ("rows32", geo.with_flags(_lib.GEO_TILE_ROWS_32)),
                     ("rows16", geo.with_flags(_lib.GEO_TILE_ROWS_16)),
                     ("rows64-general", geo.with_flags(_lib.GEO_TILE_ROWS_64 | _lib.GEO_FORCE_GENERAL))]
    ref = _ref_sr(oracle, frame, S, luts_g, luts_l)
    hq_ok = None
    for name, g in variants:
        assert ops.sr_fused_supported(C, eng.luts, g, eng.kind, eng.max_sigma), "%s must take the tile-fused kernels" % name
        for ws in (None, False):
            got = ops.sr_fused_u8(x, eng.luts, g, eng.kind, eng.max_sigma, workspace=ws)
            if hq_ok is None and not np.array_equal(got.cpu().numpy(), ref[1]):
                hq_ok = _hq_ok(torch, ops, eng, x, _ref_stages(oracle, frame, "shipped", luts_g, luts_l))
            _check_sr(got, ref, "%s S=%d %s %s" % (frame.name, S, name, "two launches" if ws is None else "single launch"), hq_ok)
    _check_sr(eng.sr(img, 2, fused=False), ref, "%s S=%d direct kernels" % (frame.name, S))


# --------------------------------------------------------------------------- packed stages: every EMIT instance
BATCHES = [(192, 64), (48, 32), (12, 16)]          # frames in the batch -> tile rows tile_rows_for picks (192 / 96 / fewer tiles)


def _batch(torch, frames, N):
    """N frames: the distinct ones repeated in turn, so different recipes sit next to each other"""
    order = [i % len(frames) for i in range(N)]
    return torch.from_numpy(np.stack([frames[i].img for i in order])).cuda(), order


@pytest.mark.parametrize("which", ["shipped", "random", "l-shipped", "l-random"])
@pytest.mark.parametrize("N,TH", BATCHES)
def test_packed_stages_of_every_emit_instance(torch, oracle, luts_g, luts_l, N, TH, which):
    from lerf_pytorch_amd import ops
    frames = bf.single_tile_frames(3, TH)
    if N < len(frames):                                     # the 16-row batch: the first 12 frames hold every recipe (4 tiles each)
        frames = frames[:N]
        assert {t[3][0] for f in frames for t in f.painted} == {r[0] for r in bf.RECIPES}
    eng = _engine(which, 2, luts_g, luts_l)
    x, order = _batch(torch, frames, N)
    assert tuple(x.shape) == (N, 64, 64, 3)
    refs = [_ref_stages(oracle, frames[i], which, luts_g, luts_l) for i in order]
    _check_stages(torch, ops, ops.stages_packed(x, eng.luts), eng.luts.oC, refs, "%d x 64 x 64 x 3 (%d-row tiles), %s" % (N, TH, which))


# --------------------------------------------------------------------------- full SR: single-tile and tiny frames, C = 3
@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("i", range(len(bf.RECIPES)), ids=[bf.recipe_name(r) for r in bf.RECIPES])
def test_full_sr_single_tile_frames(torch, oracle, luts_g, luts_l, i, S):
    _sr_every_path(torch, oracle, luts_g, luts_l, bf.single_tile_frames(3, 64)[i], S)


@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("C", [3, 1, 4])
def test_tiny_frames_stages_sr_and_one_ragged_launch(torch, oracle, luts_g, luts_l, C, S):
    from lerf_pytorch_amd import ops
    frames = bf.tiny_frames(C) if C == 3 else bf.tiny_frames(C)[:3]
    eng = _engine("shipped", S, luts_g, luts_l)
    for which in ("shipped", "random", "l-shipped"):
        e2 = _engine(which, 2, luts_g, luts_l)
        for f in frames:
            x = torch.from_numpy(f.img).cuda()
            _check_stages(torch, ops, ops.stages_packed(x, e2.luts).unsqueeze(0), e2.luts.oC,
                          [_ref_stages(oracle, f, which, luts_g, luts_l)], "%s, %s" % (f.name, which))
    for f in frames:
        _sr_every_path(torch, oracle, luts_g, luts_l, f, S, tile_rows=(C == 3))
    xs = [torch.from_numpy(f.img).cuda() for f in frames]
    geos = [eng.sr_geometry(f.img.shape[:2], 2) for f in frames]
    for f, g in zip(frames, geos):
        assert ops.sr_fused_supported(C, eng.luts, g, eng.kind, eng.max_sigma)
    outs = ops.sr_fused_ragged_u8(xs, eng.luts, geos, eng.kind, eng.max_sigma)
    for f, o in zip(frames, outs):
        _check_sr(o, _ref_sr(oracle, f, S, luts_g, luts_l), "%s S=%d ragged launch" % (f.name, S))


# --------------------------------------------------------------------------- interior tiles
def _interior(C, S):
    return bf.interior_frames(C, S)


@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("i", range(len(bf.INTERIOR_RECIPES[3])), ids=[bf.recipe_name(r) for r in bf.INTERIOR_RECIPES[3]])
def test_interior_tile_full_sr(torch, oracle, luts_g, luts_l, i, S):
    _sr_every_path(torch, oracle, luts_g, luts_l, _interior(3, S)[i], S)


@pytest.mark.parametrize("S,which", [(2, "shipped"), (2, "random"), (2, "l-shipped"), (4, "shipped"), (4, "random")])
@pytest.mark.parametrize("i", range(len(bf.INTERIOR_RECIPES[3])), ids=[bf.recipe_name(r) for r in bf.INTERIOR_RECIPES[3]])
def test_interior_tile_packed_stages(torch, oracle, luts_g, luts_l, i, S, which):
    """(the EMIT kernels' regions have no ring: the frames painted for S = 4 are further level maps to them)"""
    from lerf_pytorch_amd import ops
    f = _interior(3, S)[i]
    eng = _engine(which, 2, luts_g, luts_l)
    x = torch.from_numpy(f.img).cuda()
    _check_stages(torch, ops, ops.stages_packed(x, eng.luts).unsqueeze(0), eng.luts.oC, [_ref_stages(oracle, f, which, luts_g, luts_l)],
                  "%s, %s" % (f.name, which))


# --------------------------------------------------------------------------- C = 1 and C = 4: the general kernels
@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("C", [1, 4])
def test_general_channel_counts(torch, oracle, luts_g, luts_l, C, S):
    """only(1), pair(0, 2) and whole-wave totals on 64 x TW single-tile frames (TW = 192 / 48), and an interior tile with an
    empty middle bin: packed stages (shipped, random, LeRF-L) and full SR"""
    from lerf_pytorch_amd import ops
    frames = list(bf.general_single_tile_frames(C))
    if S == 2:
        frames += bf.interior_frames(C, 2)
    for which in ("shipped", "random", "l-shipped"):
        eng = _engine(which, 2, luts_g, luts_l)
        for f in frames:
            x = torch.from_numpy(f.img).cuda()
            _check_stages(torch, ops, ops.stages_packed(x, eng.luts).unsqueeze(0), eng.luts.oC,
                          [_ref_stages(oracle, f, which, luts_g, luts_l)], "%s, %s" % (f.name, which))
    for f in frames:
        _sr_every_path(torch, oracle, luts_g, luts_l, f, S, tile_rows=False)


# --------------------------------------------------------------------------- the tile-fused warp
def test_fused_warp_of_interior_bins_equals_packed_path(torch, oracle, luts_g, luts_l):
    """one bin only (199 chunks) and an empty middle bin in the interior tile: the warp kernel's stage 2 gives the bytes of the
    packed-map path (whose packed stages the tests above pin to the oracle)"""
    from lerf_pytorch_amd import ops
    eng = _engine("shipped", 2, luts_g, luts_l)
    fr = bf.interior_frames(3, 2)
    frames = [bf.frame_by_recipe(fr, bf.only(2)), bf.frame_by_recipe(fr, bf.pair(0, 2))]
    x = torch.from_numpy(np.stack([f.img for f in frames])).cuda()
    M = np.array([[2.05, 0.12, 15.0], [-0.08, 1.95, 40.0], [1.5e-5, -1.0e-5, 1.0]])
    geo = ops.WarpGeometry((192, 192), M, (384, 384), 2)
    assert ops.warp_fused_supported(x, eng.luts, geo, eng.kind, eng.max_sigma)
    packed = ops.stages_packed(x, eng.luts)
    _check_stages(torch, ops, packed, 3, [_ref_stages(oracle, f, "shipped", luts_g, luts_l) for f in frames], "warp batch")
    want = ops.warp_packed(packed, geo, eng.kind, eng.max_sigma, out="u8")
    got = ops.warp_fused_u8(x, eng.luts, geo, eng.kind, eng.max_sigma)
    assert got.shape == want.shape and torch.equal(got, want), "%d bytes differ" % int((got != want).sum())
