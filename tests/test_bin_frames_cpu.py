"""CPU checks of tests/bin_frames.py: the identity stage-1 tables really give feat == img, every crafted frame has the bin
census its recipe promises for the kernel instance it is meant for, and the full SR output with the SHIPPED stage-2 tables
shows every lost stage-2 position (which is why the GPU test compares full SR with the shipped tables and keeps the random
ones for the exact hq comparison)."""
import numpy as np
import pytest

import bin_frames as bf


@pytest.fixture(scope="module")
def ident_g(luts_g):
    return bf.identity_stage1(luts_g)


def test_identity_tables_return_the_image(oracle, ident_g, luts_g, luts_l):
    rng = np.random.default_rng(0)
    noise = rng.integers(0, 256, (37, 41, 3), dtype=np.uint8)
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)
    for img in (noise, ramp):
        assert np.array_equal(oracle.stage1_feat(img, ident_g), img)
    assert np.array_equal(oracle.stage1_feat(noise, bf.identity_stage1(luts_l)), noise)
    for k in ident_g:                                            # only stage 1 moved
        assert (k.startswith("s1_")) != (ident_g[k] is luts_g[k])
    for f in bf.all_frames():
        assert np.array_equal(oracle.stage1_feat(f.img, ident_g), f.img), f.name


def test_random_stage2_tables_are_seeded_and_leave_stage1(luts_g, luts_l):
    for base in (luts_g, luts_l):
        a, b, c = bf.random_stage2(base, 1), bf.random_stage2(base, 1), bf.random_stage2(base, 2)
        for k in base:
            if k.startswith("s2_"):
                assert a[k].dtype == np.int8 and a[k].shape == np.asarray(base[k]).shape
                assert np.array_equal(a[k], b[k]) and not np.array_equal(a[k], c[k])
                assert a[k].min() == -128 and a[k].max() == 127
            else:
                assert a[k] is base[k]


def test_region_restatement_sizes():
    """the instances' region sizes as csrc/lerf_fused_impl.h's Dims states them (NH, positions per thread, looked-up total)"""
    for (TH, C, HR), (NH, KH) in {(64, 3, 1): (13068, 13), (64, 3, 2): (13872, 14), (64, 3, 0): (12288, 12), (32, 3, 0): (6144, 6),
                                  (16, 3, 0): (3072, 3), (64, 1, 1): (66 * 194, 13), (64, 4, 2): (68 * 52 * 4, 14)}.items():
        inst = bf.Inst(TH, C, HR)
        assert (inst.NH, inst.KH) == (NH, KH)
        assert inst.KH <= 15 and inst.KH * bf.NT >= inst.NH
    # an interior tile lists the region without its last row and column; an EMIT tile lists all of it
    r = bf.region(bf.Inst(64, 3, 1), 192, 192, 1, 1)
    assert int(r.listed.sum()) == 65 * 65 * 3 and r.gy[0] == 63 and r.gx[0] == 63
    assert int(bf.region(bf.Inst(64, 3, 0), 64, 64, 0, 0).listed.sum()) == 12288 == 192 * 64
    # the corner tile of a frame: only the in-frame pixels, the ring outside is not looked up
    r = bf.region(bf.Inst(64, 3, 1), 70, 70, 1, 1)
    assert int(r.listed.sum()) == 7 * 7 * 3 and r.gy[r.listed].min() == 63 and r.gy[r.listed].max() == 69


def _check_tile(f, inst, ty, tx, rc, n):
    c = bf.census(f.img, inst.TH, inst.C, inst.HR, ty, tx)
    assert c[3] == n and sum(c[:3]) == n, f.name
    want = bf.expected_counts(rc, n)
    if want is not None:
        assert c == want, (f.name, rc, c, want)
    r = bf.region(inst, f.img.shape[0], f.img.shape[1], ty, tx)
    vals = f.img[r.gy[r.listed], r.gx[r.listed], r.ch[r.listed]].astype(int)
    kind = rc[0]
    if kind == "only":
        assert [c[b] for b in range(3) if b != rc[1]] == [0, 0]
    elif kind == "stray":
        p = np.flatnonzero(r.listed)
        at = np.flatnonzero(bf.bins_of(vals) == rc[2])
        assert len(at) == 1
        w = r.wave[p]
        assert at[0] == {"first": 0, "last": n - 1, "last_wave": np.flatnonzero(w == w.max())[0]}[rc[3]]
    elif kind == "pair":
        third = ({0, 1, 2} - set(rc[1:])).pop()
        assert c[third] == 0 and (n < 64 or min(c[rc[1]], c[rc[2]]) > 0.4 * n)
    elif kind == "waves":
        if rc[3:] == (0, 0):
            assert c[0] % 64 == 0 and c[1] % 64 == 0 and c[0] > 0 and c[1] > 0
        else:
            assert c[0] % 64 == 1 and c[1] % 64 == 63
    elif kind == "by_wave":
        wc = bf.wave_census(f.img, inst, ty, tx)
        own = wc.sum(1) > 0
        assert own.sum() >= 3 and ((wc[own] == 0).sum(1) == 2).all()      # every owning wave feeds ONE bin
        assert min(c[:3]) > 0
    elif kind == "striped":
        if n >= 3:
            assert max(c[:3]) - min(c[:3]) <= 1
        if n >= 1024 * 3:                                                 # every thread that owns three positions holds all bins
            p = np.flatnonzero(r.listed)
            th = p // inst.KH
            for t in (0, th.max() // 2):
                assert set(bf.bins_of(vals[th == t])) == {0, 1, 2}
    elif kind == "edges":
        assert set(vals >> 4) == {0, 5, 6, 10, 11, 15} and set(vals & 15) == {0, 15}
    # both end levels of every populated bin with room for them; 0 in bin 0 and 255 in bin 2
    for b in range(3):
        if c[b] >= 2:
            lv = set(vals[bf.bins_of(vals) == b] >> 4)
            assert bf.BIN_LO[b] in lv and bf.BIN_LO[b + 1] - 1 in lv, (f.name, b)
    if c[0] >= 1:
        assert (vals == 0).any()
    if c[2] >= 1:
        assert (vals == 255).any()


def test_census_of_every_frame(capsys):
    frames = bf.all_frames()
    assert len({f.name for f in frames}) == len(frames)
    for f in frames:
        for inst, ty, tx, rc, n in f.painted:
            assert inst.C == f.C
            _check_tile(f, inst, ty, tx, rc, n)
    with capsys.disabled():
        print("\n" + "\n".join(bf.census_table(frames)))


def test_single_tile_frames_hold_one_tile_per_instance():
    for th, ntile, nh in ((64, 1, 12288), (32, 2, 6144), (16, 4, 3072)):
        fr = bf.single_tile_frames(3, th)
        assert len(fr) == len(bf.RECIPES) >= 12
        for f in fr:
            assert f.img.shape == (64, 64, 3) and len(f.painted) == ntile
            assert all(n == nh and nh % 64 == 0 for _, _, _, _, n in f.painted)      # whole waves: only(b) is a whole-wave total
    # the 64-row frames are single-tile frames of the SR kernels as well: same census with a ring of 1 or 2
    for f in bf.single_tile_frames(3, 64):
        for hr in (1, 2):
            assert bf.census(f.img, 64, 3, hr, 0, 0) == bf.census(f.img, 64, 3, 0, 0, 0)
    for C in (1, 4):
        for f in bf.general_single_tile_frames(C):
            assert f.img.shape == (64, 192 // C, C)
            for hr in (1, 2):
                assert bf.census(f.img, 64, C, hr, 0, 0) == bf.census(f.img, 64, C, 0, 0, 0)


def test_tiny_frames_and_slivers():
    for C in (1, 3, 4):
        TW = 192 // C
        one, wave2, four, wide, tall = bf.tiny_frames(C)
        assert one.img.shape == (1, 1, C) and bf.census(one.img, 64, C, 1, 0, 0)[3] == C
        assert wave2.img.shape == (1, 66 // C, C)
        if C == 3:
            assert bf.census(wave2.img, 64, 3, 1, 0, 0)[3] == 66                 # one wave plus two
        assert four.img.shape == (65, TW + 1, C)
        for hr in (0, 1, 2):
            # four tiles; the corner lists less than a wave, all of it in bin 2 ...
            c = bf.census(four.img, 64, C, hr, 1, 1)
            assert 1 <= c[3] <= 63 and c[:3] == (0, 0, c[3])
            assert c[3] == (hr + 1) ** 2 * C
            # ... its edge neighbours list a sliver of 64 rows / TW columns (more than a wave for every C)
            assert bf.census(four.img, 64, C, hr, 0, 1)[3] == (64 + (hr == 2)) * (hr + 1) * C
            assert bf.census(four.img, 64, C, hr, 1, 0)[3] == (hr + 1) * (TW + (hr == 2)) * C
            # the frames whose slivers stay below one wave (C = 3: 21 / 42 / 63 positions)
            if 7 * (hr + 1) * C <= 63:
                assert bf.census(wide.img, 64, C, hr, 0, 1)[3] == 7 * (hr + 1) * C
                assert bf.census(tall.img, 64, C, hr, 1, 0)[3] == 7 * (hr + 1) * C
    for hr in (0, 1, 2):
        assert 1 <= bf.census(bf.tiny_frames(3)[3].img, 64, 3, hr, 0, 1)[3] <= 63
        assert 1 <= bf.census(bf.tiny_frames(3)[4].img, 64, 3, hr, 1, 0)[3] <= 63


def test_interior_frames():
    for C in (3, 1, 4):
        for S in ((2, 4) if C == 3 else (2,)):
            inst = bf.Inst(64, C, S // 2)
            for f in bf.interior_frames(C, S):
                H, W = f.img.shape[:2]
                assert (H, W) == (192, 3 * inst.TW)
                # interior for the single-launch kernel too: input region = tile + S/2 + 3 + 3 on every side
                m = S // 2 + 6
                assert 64 - m >= 0 and 128 + m <= H and inst.TW - m >= 0 and 2 * inst.TW + m <= W
                (_, ty, tx, rc, n), = f.painted
                assert (ty, tx) == (1, 1) and n == (inst.HY - 1) * (inst.HX - 1) * C
    # only(2), C = 3, S = 2: 199 chunks of one bin
    f = bf.frame_by_recipe(bf.interior_frames(3, 2), bf.only(2))
    assert -(-f.painted[0][4] // 64) == 199


def test_sr_pipeline_is_stages_then_resize(oracle, luts_g):
    """the GPU test caches oracle.lut_stages per (frame, tables) and finishes with resize_u8 + to_u8: sr_pipeline's own body"""
    img = bf.single_tile_frames(3, 16)[0].img[:20, :24]
    for S in (2, 4):
        feat, hq = oracle.lut_stages(img, luts_g, 3)
        assert np.array_equal(oracle.to_u8(oracle.resize_u8(feat, hq, 2, 2, S, 10, "gauss")), oracle.sr_pipeline(img, luts_g, 2, 2, S=S))


@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("recipe", [bf.only(0), bf.only(2), bf.STRIPED], ids=["bin0", "bin2", "allbins"])
def test_full_sr_shows_every_lost_position_with_shipped_stage2(oracle, ident_g, recipe, S):
    """A position the binning loses keeps hq = 127 (a zero sum).  With the shipped stage-2 tables every one of 49 sampled
    positions changes output bytes inside its own footprint.  The samples are 9 pixels apart, further than any footprint
    reaches (S / 2 + 1 pixels), so they are perturbed together and judged one by one."""
    f = bf.frame_by_recipe(bf.single_tile_frames(3, 64), recipe)
    feat, hq = oracle.lut_stages(f.img, ident_g, 3)
    ref = oracle.to_u8(oracle.resize_u8(feat, hq, 2, 2, S, 10, "gauss"))
    lost = hq.copy()
    pts = [(y, x, (i + j) % 3) for i, y in enumerate(range(4, 64, 9)) for j, x in enumerate(range(4, 64, 9))]
    assert len(pts) == 49
    for y, x, c in pts:
        lost[y, x, c, :] = 127
    out = oracle.to_u8(oracle.resize_u8(feat, lost, 2, 2, S, 10, "gauss"))
    diff = out != ref
    seen = 0
    reach = S // 2 + 1
    for y, x, c in pts:
        win = diff[max(2 * (y - reach), 0):2 * (y + reach + 1), max(2 * (x - reach), 0):2 * (x + reach + 1), c]
        seen += bool(win.any())
    # nothing changes outside the footprints, or in another channel
    mask = np.zeros_like(diff)
    for y, x, c in pts:
        mask[max(2 * (y - reach), 0):2 * (y + reach + 1), max(2 * (x - reach), 0):2 * (x + reach + 1), c] = True
    assert not (diff & ~mask).any()
    assert seen == 49, "%d of 49 lost positions show" % seen


@pytest.mark.parametrize("recipe", [bf.only(0), bf.only(2), bf.STRIPED], ids=["bin0", "bin2", "allbins"])
def test_exact_hq_shows_every_walk_in_the_wrong_piece_with_random_stage2(oracle, luts_g, recipe):
    """A mis-binned position walks the piece of another bin: it reads the entries of level - bin_lo(own) + bin_lo(other).
    With the random stage-2 tables hq at every one of 49 sampled positions changes when its centre is moved that way (the
    samples are 9 pixels apart, further than any pattern reaches, so no sample is another one's neighbour)."""
    tables = bf.random_stage2(bf.identity_stage1(luts_g), 2024)
    f = bf.frame_by_recipe(bf.single_tile_frames(3, 64), recipe)
    pts = [(y, x, (i + j) % 3) for i, y in enumerate(range(4, 64, 9)) for j, x in enumerate(range(4, 64, 9))]
    moved = f.img.copy()
    for y, x, c in pts:
        v = int(f.img[y, x, c])
        b = int(bf.bins_of(v))
        other = (b + 1 + (y + x) % 2) % 3
        level = min((v >> 4) - bf.BIN_LO[b] + bf.BIN_LO[other], 15)
        moved[y, x, c] = level * 16 + (v & 15)                    # (offset 5 of bin 0 is the sixth of a piece's seven levels)
        assert level != v >> 4
    h0, h1 = oracle.stage2_hyper(f.img, tables, 3), oracle.stage2_hyper(moved, tables, 3)
    seen = sum(bool((h0[y, x, c] != h1[y, x, c]).any()) for y, x, c in pts)
    assert seen == 49, "%d of 49 wrong-piece walks show" % seen
