"""GPU: the lean stage-2 set-up of the exact-x2 LeRF-G kernel (csrc/lerf_fused_impl.h, stage2_gauss<.., LEAN>: interior tiles bin
their positions by one running address, write the lists' 0xFFFF only into the padding tail of each bin, do not read the chunks
behind the last bin, and take the row of a slot's address by a multiply and a shift).

All cases: LeRF-G, S = 2, RGB, scale exactly 2.0, 64-row tiles, both launch forms (two launches with a workspace, and
LERF_GEO_SINGLE_LAUNCH).  Every launch is compared byte for byte (0 mismatches) with the C port of the oracle
(oracle/c_oracle.sr_u8) and with the same launch under LERF_GEO_FORCE_TABLES, which runs the table-geometry kernel: the
generic set-up on every tile.

  136 x 136 -> 272 x 272: the smallest frame with an interior tile (a 3 x 3 grid, tile (1, 1): its feat and input regions end at
  rows / columns 131 and 134).  The interior tile's region is painted by every entry of bin_frames.INTERIOR_RECIPES[3] through
  the identity stage-1 tables (feat == img): one bin only (199 chunks: a tail of 61 in the LAST used chunk, chunks 199..207
  unwritten), a stray position in the last wave (a bin of one position: a tail of 63), an empty first or middle bin, totals on
  and next to multiples of 64 (bins of whole chunks, no tail / tails of 63 and 1).
  The same frame size with the shipped and with random stage-2 tables on uniform noise and on a constant frame (one bin, the
  other two empty).
  200 x 136: edge and interior tiles together ((1, 1) and (2, 1) are interior; the last tile row holds 8 rows, the last tile column
  8 columns): the edge tiles of the same kernel keep the generic set-up.
  A batch of two frames, only(2) beside noise: a census must not leak from one tile into the next."""
import numpy as np
import pytest

import bin_frames as bf

pytestmark = pytest.mark.gpu

INST = bf.Inst(64, 3, 1)
H0 = W0 = 136
RECIPES = bf.INTERIOR_RECIPES[3]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


_TABLES, _ENGINES, _FRAMES, _REF = {}, {}, {}, {}


def _tables(which, luts_g):
    """'identity' (identity stage 1, shipped stage 2), 'shipped', 'random' (shipped stage 1, seeded stage 2)"""
    if which not in _TABLES:
        _TABLES[which] = {"identity": lambda: bf.identity_stage1(luts_g), "shipped": lambda: luts_g,
                          "random": lambda: bf.random_stage2(luts_g, 2025)}[which]()
    return _TABLES[which]


def _engine(which, luts_g):
    import lerf_pytorch_amd as L
    if which not in _ENGINES:
        _ENGINES[which] = L.LerfEngine(L.LutSet.from_arrays(_tables(which, luts_g)), support=2)
    return _ENGINES[which]


def _noise(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _frame(name):
    """the test frames, once each, read-only"""
    if name not in _FRAMES:
        if name.startswith("recipe"):
            i = int(name[6:])
            img = _noise(H0, W0, 700 + i)
            rc, n = bf.paint(img, INST, 1, 1, RECIPES[i], 710 + i)
            assert n == 65 * 65 * 3, "the interior tile looks up its whole region but the last row and column"
            want = bf.expected_counts(rc, n)
            assert want is None or bf.census(img, 64, 3, 1, 1, 1) == want, "the recipe's census"
        elif name == "noise":
            img = _noise(H0, W0, 801)
        elif name == "constant":
            img = np.full((H0, W0, 3), 128, np.uint8)
        elif name == "mixed":
            img = _noise(200, 136, 802)
        else:
            raise KeyError(name)
        img.setflags(write=False)
        _FRAMES[name] = img
    return _FRAMES[name]


def _ref(name, which, luts_g):
    from oracle import c_oracle
    if (name, which) not in _REF:
        r = c_oracle.sr_u8(_frame(name), _tables(which, luts_g), 2, 2, S=2, linear=False)
        r.setflags(write=False)
        _REF[(name, which)] = r
    return _REF[(name, which)]


def _same(got, ref, what):
    n = int((got != ref).sum())
    assert got.shape == ref.shape and n == 0, "%s: %d of %d bytes differ" % (what, n, ref.size)


def _check(torch, luts_g, names, which):
    """the frames `names` (one size) as one launch: flagged launch == oracle == table path, both launch forms"""
    from lerf_pytorch_amd import _lib, ops
    eng = _engine(which, luts_g)
    frames = np.stack([_frame(n) for n in names])
    ref = np.stack([_ref(n, which, luts_g) for n in names])
    H, W = frames.shape[1:3]
    geo = eng.sr_geometry((H, W), 2).with_flags(_lib.GEO_TILE_ROWS_64)
    assert geo.struct.flags & _lib.GEO_EXACT_X2, "whole-frame x2: the exact-x2 kernel serves the launch"
    x = torch.from_numpy(frames).cuda()
    what = "%s, %s tables" % ("+".join(names), which)
    for form, g, ws in (("two launches", geo, None), ("single launch", geo.with_flags(_lib.GEO_SINGLE_LAUNCH), None)):
        assert ops.sr_fused_supported(3, eng.luts, g, eng.kind, eng.max_sigma)
        got = ops.sr_fused_u8(x, eng.luts, g, eng.kind, eng.max_sigma, workspace=ws).cpu().numpy()
        tab = ops.sr_fused_u8(x, eng.luts, g.with_flags(_lib.GEO_FORCE_TABLES), eng.kind, eng.max_sigma, workspace=ws).cpu().numpy()
        _same(got, ref, "%s, %s: lean set-up vs the C port" % (what, form))
        _same(tab, ref, "%s, %s: table path vs the C port" % (what, form))
        _same(got, tab, "%s, %s: lean set-up vs table path" % (what, form))


@pytest.mark.parametrize("i", range(len(RECIPES)), ids=[bf.recipe_name(r) for r in RECIPES])
def test_interior_tile_with_a_crafted_census(torch, luts_g, i):
    _check(torch, luts_g, ["recipe%d" % i], "identity")


@pytest.mark.parametrize("which", ["shipped", "random"])
@pytest.mark.parametrize("name", ["noise", "constant"])
def test_shipped_and_random_stage2_tables(torch, luts_g, name, which):
    _check(torch, luts_g, [name], which)


def test_edge_and_interior_tiles_together(torch, luts_g):
    assert _frame("mixed").shape == (200, 136, 3)
    _check(torch, luts_g, ["mixed"], "shipped")


def test_batch_of_two_frames(torch, luts_g):
    i = [r[0] for r in RECIPES].index("only")
    assert RECIPES[i] == bf.only(2)
    _check(torch, luts_g, ["recipe%d" % i, "noise"], "identity")
