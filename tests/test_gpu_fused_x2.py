"""GPU: the exact-x2 flavour of the tile-fused SR kernels (csrc/lerf_fused_impl.h, GeoX2; LERF_GEO_EXACT_X2), which takes the
stage-3 geometry -- owned ranges, first taps, float32 and float64 distances, row / column groups, pair codes -- from the closed
form instead of the caller's tables.  It serves the 2 x 2 support (LeRF-G and LeRF-L) on the 64-row tile instance.

Every launch is compared byte for byte (0 mismatches) with the C port of the oracle and, where the flavour is taken, with the
same launch forced onto the table path (LERF_GEO_FORCE_TABLES).  Frames (uniform noise, RGB) are the smallest that reach every
tile class:
  200 x 200  a 4 x 4 grid of 64-row tiles: four interior tiles, every edge and corner class, a partial last row / column of 8;
  70 x 130   a 6-row last tile row, a 2-column last tile column, no interior tile;
  65 x 64    the last tile row owns a single LR row.
Per frame: two launches (workspace) and one; a batch of 3; output rows padded to a 16-byte pitch; the tie queue at its default
capacity, at 4 entries (overflow) and switched off (every tie resolved inside the task loop), so that each of the three tie paths
takes its float64 distances from the closed form.

That the X2 kernels RUN where they should is observed, not assumed (test_x2_kernels_do_not_read_the_distance_tables): with the
float32 distance tables on the device overwritten, a launch that carries the promise still gives the oracle's bytes -- the
closed form never reads them -- while the same launch forced onto the tables does not.

The 4 x 4 support and the 32- / 16-row instances carry the promise too but run the table path (DESIGN.md, appendix "exact-x2
geometry"); their cases pin the bytes of a flagged launch against the oracle, and the overwritten-tables launch shows that
they do read the tables.

Dispatch: the bit is the host geometry builder's verdict and is set for whole-frame x2 only; slices drop it.  A caller who sets
it on a launch whose sizes are not out = 2 x in, or on a region of interest, gets the TABLE path (documented in lerf_hip.h) --
shown here by correct bytes from launches on which the closed form would be wrong.

The library has no entry point called lerf_sr_fused_many: frames in one call are the batch (above) and the ragged launch
(LerfEngine.sr_many -> lerf_sr_fused_ragged_u8), which runs the general kernels and therefore the table path; two x2 items go
through it here all the same."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAMES64 = [(200, 200), (70, 130), (65, 64)]
CASES = [(h, w, 64) for h, w in FRAMES64] + [(h, w, r) for r in (32, 16) for h, w in FRAMES64[:2]]
MODELS = {"g2": ("lerf-g", 2), "g4": ("lerf-g", 4), "l2": ("lerf-l", 2)}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


_ENG, _IMG, _REF = {}, {}, {}


def _engine(model):
    import lerf_pytorch_amd as L
    if model not in _ENG:
        name, S = MODELS[model]
        _ENG[model] = L.LerfEngine.shipped(name, support=S)
    return _ENG[model]


def _frames(H, W):
    """three noise frames of one size (the first is the single-frame input)"""
    if (H, W) not in _IMG:
        a = np.random.default_rng(1000 * H + W).integers(0, 256, (3, H, W, 3), dtype=np.uint8)
        a.setflags(write=False)
        _IMG[(H, W)] = a
    return _IMG[(H, W)]


def _ref(model, H, W, luts_g, luts_l, sh=2, sw=2):
    """the C port of the oracle on the three frames, once per (model, size, scale)"""
    from oracle import c_oracle
    key = (model, H, W, sh, sw)
    if key not in _REF:
        name, S = MODELS[model]
        lin = name == "lerf-l"
        r = np.stack([c_oracle.sr_u8(f, luts_l if lin else luts_g, sh, sw, S=S, linear=lin) for f in _frames(H, W)])
        r.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def _rows(rows):
    from lerf_pytorch_amd import _lib
    return {64: _lib.GEO_TILE_ROWS_64, 32: _lib.GEO_TILE_ROWS_32, 16: _lib.GEO_TILE_ROWS_16}[rows]


def _run(torch, eng, geo, frames, workspace=None, out=None):
    from lerf_pytorch_amd import ops
    x = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    o = ops.sr_fused_u8(x, eng.luts, geo, eng.kind, eng.max_sigma, out=out, workspace=workspace)
    return o.cpu().numpy()


def _takes_x2(model, rows):
    """the launches the library serves with the X2 kernels: 2 x 2 support, 64-row tiles"""
    return MODELS[model][1] == 2 and rows == 64


def _same(got, ref, what):
    n = int((got != ref).sum())
    assert got.shape == ref.shape and n == 0, "%s: %d of %d bytes differ" % (what, n, ref.size)


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("H,W,rows", CASES)
def test_x2_flavour_equals_oracle_and_table_path(torch, luts_g, luts_l, model, H, W, rows):
    from lerf_pytorch_amd import _lib
    eng = _engine(model)
    frames, ref = _frames(H, W), _ref(model, H, W, luts_g, luts_l)
    geo = eng.sr_geometry((H, W), 2).with_flags(_rows(rows))
    assert geo.struct.flags & _lib.GEO_EXACT_X2, "the host geometry builder sets the promise for whole-frame x2"
    tab = geo.with_flags(_lib.GEO_FORCE_TABLES)
    what = "%s %dx%d rows%d" % (model, H, W, rows)
    both = _takes_x2(model, rows)              # (elsewhere the flagged launch IS the table path: one comparison, with the oracle)
    for form, ws in (("two launches", None), ("single launch", False)):
        x2 = _run(torch, eng, geo, frames[0], workspace=ws)
        _same(x2, ref[0], "%s, %s, flagged launch vs oracle" % (what, form))
        if both:
            _same(_run(torch, eng, tab, frames[0], workspace=ws), x2, "%s, %s, tables vs X2" % (what, form))
    # a batch of 3
    x2 = _run(torch, eng, geo, frames)
    _same(x2, ref, what + ", batch of 3, flagged launch vs oracle")
    if both:
        _same(_run(torch, eng, tab, frames), x2, what + ", batch of 3, tables vs X2")
    # the tie queue: 4 entries (overflow: the rest is resolved inside the loop) and none at all
    for cap in (4, 0):
        g = geo.with_tie_queue_cap(cap)
        assert g.struct.tie_queue_cap == (-1 if cap == 0 else cap) and g.struct.flags & _lib.GEO_EXACT_X2
        x2 = _run(torch, eng, g, frames)
        _same(x2, ref, "%s, tie_queue_cap %d, flagged launch vs oracle" % (what, g.struct.tie_queue_cap))
        if both:
            t = tab.with_tie_queue_cap(cap)
            assert t.struct.flags & _lib.GEO_FORCE_TABLES
            _same(_run(torch, eng, t, frames), x2, "%s, tie_queue_cap %d, tables vs X2" % (what, g.struct.tie_queue_cap))
    # output rows at a pitch padded to 16 bytes (and one chunk more, so that the rows do not abut)
    oH, oW = 2 * H, 2 * W
    pitch = (oW * 3 + 15) // 16 * 16 + 16
    for g, name in ((geo, "flagged launch"), (tab, "tables")):
        buf = torch.full((oH * pitch,), 0xA5, dtype=torch.uint8, device="cuda")
        out = torch.as_strided(buf, (1, oH, oW, 3), (oH * pitch, pitch, 3, 1))
        _run(torch, eng, g, frames[:1], out=out)
        b = buf.cpu().numpy().reshape(oH, pitch)
        _same(b[:, :oW * 3].reshape(oH, oW, 3), ref[0], "%s, out_row_pitch %d, %s vs oracle" % (what, pitch, name))
        assert (b[:, oW * 3:] == 0xA5).all(), "%s, out_row_pitch %d, %s: bytes written into the row padding" % (what, pitch, name)


@pytest.mark.parametrize("rows", [64, 32, 16])
@pytest.mark.parametrize("model", list(MODELS))
def test_x2_kernels_do_not_read_the_distance_tables(torch, luts_g, luts_l, model, rows):
    """Which kernels run, observed: the float32 distance tables on the device are overwritten with 0.5 (first taps and float64
    tables intact, so every path stays inside its tile and the tie guard stays armed).  Where the X2 kernels serve the launch
    the bytes are still the oracle's, both launch forms; forced onto the tables -- and where the library keeps the table path
    (4 x 4 support, 32- / 16-row tiles) -- the same launch must NOT give them."""
    from lerf_pytorch_amd import _lib
    eng = _engine(model)
    H, W = 200, 200
    frames, ref = _frames(H, W), _ref(model, H, W, luts_g, luts_l)
    geo = eng.sr_geometry((H, W), 2).with_flags(_rows(rows))
    bad = geo.with_flags(0)                                        # a copy with tables of its own
    bad.host = dict(geo.host)
    bad.host["dis_r32"] = np.full_like(geo.host["dis_r32"], 0.5)
    bad.host["dis_c32"] = np.full_like(geo.host["dis_c32"], 0.5)
    bad._upload()
    assert bad.struct.flags & _lib.GEO_EXACT_X2 and bad.struct.dis_r != geo.struct.dis_r
    what = "%s rows%d, float32 distance tables overwritten" % (model, rows)
    for form, ws in (("two launches", None), ("single launch", False)):
        got = _run(torch, eng, bad, frames[0], workspace=ws)
        if _takes_x2(model, rows):
            _same(got, ref[0], "%s, %s: the X2 kernels read no table" % (what, form))
        else:
            assert (got != ref[0]).any(), "%s, %s: this launch runs the table path" % (what, form)
        forced = _run(torch, eng, bad.with_flags(_lib.GEO_FORCE_TABLES), frames[0], workspace=ws)
        assert (forced != ref[0]).any(), "%s, %s: LERF_GEO_FORCE_TABLES reads the tables" % (what, form)


@pytest.mark.parametrize("model", list(MODELS))
def test_ragged_launch_of_two_x2_items(torch, luts_g, luts_l, model):
    """two x2 frames of different sizes in one ragged launch (general kernels: the table path, whatever the items' flags say)"""
    eng = _engine(model)
    sizes = [(200, 200), (70, 130)]
    outs = eng.sr_many([_frames(h, w)[0] for h, w in sizes], [2, 2])
    for (h, w), o in zip(sizes, outs):
        _same(o, _ref(model, h, w, luts_g, luts_l)[0], "%s ragged item %dx%d vs oracle" % (model, h, w))


@pytest.mark.parametrize("model", list(MODELS))
def test_other_scales_and_slices_take_the_table_path(torch, luts_g, luts_l, model):
    from lerf_pytorch_amd import _lib, ops
    eng = _engine(model)
    H, W = 70, 130
    frames = _frames(H, W)
    # scale (2.0, 1.5): no promise from the builder; a caller who sets the bit all the same runs the table path (the sizes are
    # not out = 2 x in) -- the closed form would give other bytes
    geo = eng.sr_geometry((H, W), (2.0, 1.5))
    assert not geo.struct.flags & _lib.GEO_EXACT_X2
    ref = _ref(model, H, W, luts_g, luts_l, 2.0, 1.5)
    for g in (geo, geo.with_flags(_lib.GEO_EXACT_X2)):
        _same(_run(torch, eng, g.with_flags(_lib.GEO_TILE_ROWS_64), frames[0]), ref[0], "%s scale (2.0, 1.5), flags %#x" % (model, g.struct.flags))
    geo = eng.sr_geometry((H, W), (1.5, 2.0))
    assert not geo.struct.flags & _lib.GEO_EXACT_X2
    # a row slice / a block of the x2 tables drops the promise; with the bit forced back on, the launch still runs the table path
    # (a strip's sizes are not out = 2 x in; a block's launch has a region of interest)
    full = eng.sr_geometry((H, W), 2)
    ref = _ref(model, H, W, luts_g, luts_l)[0]
    R3 = eng.support // 2
    left = full.host["left_r"]
    lr0, lr1 = 17, 53                                            # owned LR rows of the strip
    o0, o1 = int(np.searchsorted(left, lr0 - R3)), int(np.searchsorted(left, lr1 - R3))
    y0, y1 = lr0 - 8, lr1 + 8                                     # ... held with a halo that covers the reach of all three stages
    strip = full.row_slice(y0, y1 - y0, o0, o1)
    assert full.struct.flags & _lib.GEO_EXACT_X2 and not strip.struct.flags & _lib.GEO_EXACT_X2
    for g in (strip, strip.with_flags(_lib.GEO_EXACT_X2)):
        got = _run(torch, eng, g.with_flags(_lib.GEO_TILE_ROWS_64), frames[0][y0:y1])
        _same(got, ref[o0:o1], "%s row slice, flags %#x" % (model, g.struct.flags))
    leftc = full.host["left_c"]
    lc0, lc1 = 24, 100
    p0, p1 = int(np.searchsorted(leftc, lc0 - R3)), int(np.searchsorted(leftc, lc1 - R3))
    x0, x1 = lc0 - 8, lc1 + 8
    block = full.block_slice(y0, y1 - y0, o0, o1, x0, x1 - x0, p0, p1, roi=(lr0 - y0, lc0 - x0, lr1 - lr0, lc1 - lc0))
    assert not block.struct.flags & _lib.GEO_EXACT_X2 and block.struct.roi_h == lr1 - lr0
    for g in (block, block.with_flags(_lib.GEO_EXACT_X2)):
        got = _run(torch, eng, g.with_flags(_lib.GEO_TILE_ROWS_64), frames[0][y0:y1, x0:x1])
        _same(got, ref[o0:o1, p0:p1], "%s block with a region of interest, flags %#x" % (model, g.struct.flags))
    assert ops.sr_fused_supported(3, eng.luts, full, eng.kind, eng.max_sigma)
