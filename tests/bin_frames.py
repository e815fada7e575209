"""Crafted level maps for the LeRF-G stage-2 binning of the tile-fused kernels (csrc/lerf_fused_impl.h, sr_fused_kernel).

Numpy only.  Three parts:

* identity stage-1 tables: LUT[a, b, c, d] = 4 * a makes every stage-1 pass return 16 * 4 * a-interpolated = 4 * pixel, the
  twelve passes sum to 48 * pixel, so feat == img exactly and the test image IS the level map stage 2 bins;
* a restatement of which positions of a tile's hyper region the kernel looks up, who owns them (thread-major lists:
  thread = p // KH, wave = thread // 64) and the bin census of a tile;
* recipes that assign a bin to every looked-up position of one region, and the frames built from them.

The bin of a position is that of the top-axis level (value >> 4) of its centre value: levels 0..5, 6..10, 11..15.
"""
import functools
from collections import namedtuple

import numpy as np

BIN_LO = (0, 6, 11, 16)
NT = 1024                      # threads per workgroup
LEVELS = 17


# --------------------------------------------------------------------------- tables
def identity_stage1(arrays):
    """copy of a LUT dict whose stage-1 tables are LUT[a, b, c, d] = 4 * a (a = the pixel at offset (0, 0), the top axis of
    every mode and rotation): stage 1 then returns its input"""
    out = dict(arrays)
    ident = (4 * (np.arange(LEVELS ** 4) // LEVELS ** 3)).astype(np.int8).reshape(-1, 1)
    for k in arrays:
        if k.startswith("s1_"):
            assert np.asarray(arrays[k]).size == ident.size
            out[k] = ident.copy()
    return out


def random_stage2(arrays, seed):
    """copy of a LUT dict whose stage-2 tables are seeded uniform int8: every entry distinctive"""
    out = dict(arrays)
    rng = np.random.default_rng(seed)
    for k in sorted(arrays):
        if k.startswith("s2_"):
            out[k] = rng.integers(-128, 128, np.asarray(arrays[k]).shape, dtype=np.int8)
    return out


# --------------------------------------------------------------------------- region restatement
class Inst(namedtuple("Inst", "TH C HR")):
    """one kernel instance: tile rows, channels, ring of the hyper region (S // 2 for the SR kernels, 0 for EMIT)"""
    __slots__ = ()
    TW = property(lambda s: 192 // s.C)
    HY = property(lambda s: s.TH + 2 * s.HR)
    HX = property(lambda s: s.TW + 2 * s.HR)
    HP = property(lambda s: s.HX * s.C)
    NH = property(lambda s: s.HY * s.HP)
    KH = property(lambda s: -(-s.NH // NT))


Region = namedtuple("Region", "gy gx ch listed wave")


def region(inst, H, W, ty, tx):
    """per position p of tile (ty, tx)'s hyper region: frame coordinates, channel, looked up or not, owner wave"""
    p = np.arange(inst.NH)
    ry, r3 = p // inst.HP, p % inst.HP
    rx, ch = r3 // inst.C, r3 % inst.C
    gy, gx = ty * inst.TH - inst.HR + ry, tx * inst.TW - inst.HR + rx
    listed = (gy >= 0) & (gy < H) & (gx >= 0) & (gx < W)
    if inst.HR > 0:
        listed &= (ry != inst.HY - 1) & (rx != inst.HX - 1)
    return Region(gy, gx, ch, listed, (p // inst.KH) // 64)


def bins_of(values, bin_lo=BIN_LO):
    return np.digitize(np.asarray(values).astype(np.int32) >> 4, bin_lo[1:-1])


def census(img, TH, C, HR, ty, tx, bin_lo=BIN_LO):
    """(count of bin 0, bin 1, bin 2, looked-up total) of tile (ty, tx)"""
    img = np.asarray(img)
    assert img.shape[2] == C
    r = region(Inst(TH, C, HR), img.shape[0], img.shape[1], ty, tx)
    b = bins_of(img[r.gy[r.listed], r.gx[r.listed], r.ch[r.listed]], bin_lo)
    n = np.bincount(b, minlength=3)
    return int(n[0]), int(n[1]), int(n[2]), int(r.listed.sum())


def wave_census(img, inst, ty, tx):
    """[16, 3] counts per owner wave and bin"""
    img = np.asarray(img)
    r = region(inst, img.shape[0], img.shape[1], ty, tx)
    b = bins_of(img[r.gy[r.listed], r.gx[r.listed], r.ch[r.listed]])
    out = np.zeros((NT // 64, 3), np.int64)
    np.add.at(out, (r.wave[r.listed], b), 1)
    return out


def tiles_of(inst, H, W):
    return [(ty, tx) for ty in range(-(-H // inst.TH)) for tx in range(-(-W // inst.TW))]


# --------------------------------------------------------------------------- recipes
def only(b): return ("only", b)
def stray(b, b2, where): return ("stray", b, b2, where)          # where: first | last | last_wave
def pair(b, b2): return ("pair", b, b2)
def waves(k, m, d0, d1): return ("waves", k, m, d0, d1)          # k = m = None: sized from the region (n // 192, n // 256)
BY_WAVE, STRIPED, EDGES = ("by_wave",), ("striped",), ("edges",)


def resolve(recipe, n):
    if recipe[0] == "waves" and recipe[1] is None:
        return waves(max(n // 192, 1), max(n // 256, 1), recipe[3], recipe[4])
    return recipe


def assign(recipe, p, wave, rng):
    """bin of every looked-up position (p, wave: their position indices and owner waves, in position order)"""
    n = len(p)
    kind = recipe[0]
    if kind == "only":
        return np.full(n, recipe[1])
    if kind == "stray":
        b = np.full(n, recipe[1])
        at = {"first": 0, "last": n - 1, "last_wave": int(np.flatnonzero(wave == wave.max())[0])}[recipe[3]]
        b[at] = recipe[2]
        return b
    if kind == "pair":
        b = np.where(rng.random(n) < 0.5, recipe[1], recipe[2])
        if n >= 2:
            b[rng.permutation(n)[:2]] = recipe[1:3]
        return b
    if kind == "waves":
        n0, n1 = 64 * recipe[1] + recipe[3], 64 * recipe[2] + recipe[4]
        assert n0 + n1 <= n, "region too small for this recipe"
        b = np.full(n, 2)
        perm = rng.permutation(n)
        b[perm[:n0]] = 0
        b[perm[n0:n0 + n1]] = 1
        return b
    if kind == "by_wave":
        return wave % 3
    if kind == "striped":
        return p % 3
    if kind == "edges":
        return rng.integers(0, 3, n)
    raise ValueError(recipe)


def expected_counts(recipe, n):
    """the census a recipe promises for a region of n looked-up positions (None where it promises a property instead)"""
    kind = recipe[0]
    c = [0, 0, 0]
    if kind == "only":
        c[recipe[1]] = n
    elif kind == "stray":
        c[recipe[1]], c[recipe[2]] = n - 1, 1
    elif kind == "waves":
        c = [64 * recipe[1] + recipe[3], 64 * recipe[2] + recipe[4]]
        c.append(n - c[0] - c[1])
    else:
        return None
    return tuple(c) + (n,)


def draw(bins, rng, edges=False):
    """values inside the bins: level uniform over the bin's range, LSB uniform over 0..15 (edges: end levels, LSB 0 / 15).
    Forced where the bin has the positions for it, in this order: bin 0 value 0 then its top level, bin 1 both end levels,
    bin 2 value 255 then its bottom level -- a bin of ONE position (a stray) takes the first of them."""
    v = np.zeros(len(bins), np.uint8)
    for b in range(3):
        idx = np.flatnonzero(bins == b)
        m = len(idx)
        if m == 0:
            continue
        lo, hi = BIN_LO[b], BIN_LO[b + 1] - 1
        if edges:
            lev, lsb = rng.choice([lo, hi], m), rng.choice([0, 15], m)
        else:
            lev, lsb = rng.integers(lo, hi + 1, m), rng.integers(0, 16, m)
        forced = {0: [(lo, 0), (hi, 15)], 1: [(lo, 0), (hi, 15)], 2: [(hi, 15), (lo, 0)]}[b]
        slots = rng.permutation(m)[:len(forced)]
        for s, (fl, fs) in zip(slots, forced):
            lev[s] = fl
            if edges or (fl, fs) in ((0, 0), (15, 15)):
                lsb[s] = fs
        v[idx] = lev * 16 + lsb
    return v


def paint(img, inst, ty, tx, recipe, seed):
    """paint tile (ty, tx)'s looked-up positions by a recipe; returns (resolved recipe, looked-up total)"""
    H, W = img.shape[:2]
    r = region(inst, H, W, ty, tx)
    p = np.flatnonzero(r.listed)
    recipe = resolve(recipe, len(p))
    rng = np.random.default_rng(seed)
    b = assign(recipe, p, r.wave[p], rng)
    img[r.gy[p], r.gx[p], r.ch[p]] = draw(b, rng, edges=recipe[0] == "edges")
    return recipe, len(p)


# --------------------------------------------------------------------------- frames
class Frame:
    """img: uint8 [H, W, C]; painted: [(inst, ty, tx, recipe, n)] -- the tiles whose census is fixed by construction"""

    def __init__(self, name, img, painted):
        self.name, self.img, self.painted = name, img, painted
        self.C = img.shape[2]

    def __repr__(self):
        return self.name


def _noise(H, W, C, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, C), dtype=np.uint8)


def recipe_name(recipe):
    return "-".join(str(x) for x in recipe if x is not None)


RECIPES = [only(0), only(1), only(2), stray(0, 2, "first"), stray(2, 0, "last"), stray(1, 0, "last_wave"),
           pair(0, 2), pair(1, 2), pair(0, 1), waves(None, None, 0, 0), waves(None, None, 1, 63), BY_WAVE, STRIPED, EDGES]


def tiled_frame(name, inst, H, W, recipes, seed, paint_inst=None):
    """every tile of an H x W frame painted by its recipe (tiles in row-major order).  The regions of a ring-less (EMIT)
    instance and those of a single-tile frame do not overlap, so each tile's census is the recipe's by construction."""
    img = _noise(H, W, inst.C, seed)
    painted = []
    for i, (ty, tx) in enumerate(tiles_of(inst, H, W)):
        rc, n = paint(img, paint_inst or inst, ty, tx, recipes[i % len(recipes)], seed * 131 + i)
        painted.append((paint_inst or inst, ty, tx, rc, n))
    return Frame(name, img, painted)


@functools.lru_cache(maxsize=None)
def single_tile_frames(C, TH=64):
    """64 x TW frames.  TH = 64: one tile per frame, one recipe each -- the census is the frame's content for the EMIT kernels
    and for the SR kernels of any support (the ring lies outside the frame).  TH = 32 / 16: the same frame size cut into two /
    four ring-less EMIT tiles, each painted by a different recipe."""
    inst = Inst(TH, C, 0)
    per = 64 // TH
    step = {1: [0], 2: [0, 5], 4: [0, 3, 7, 10]}[per]
    frames = []
    for i, rc in enumerate(RECIPES):
        rcs = [RECIPES[(i + s) % len(RECIPES)] for s in step]
        frames.append(tiled_frame("c%d_h%d_%s" % (C, TH, recipe_name(rc)), inst, 64, inst.TW, rcs, 1000 * TH + 10 * i + C))
    return tuple(frames)


def frame_by_recipe(frames, recipe):
    """the frame whose first painted tile follows `recipe` (None matches any parameter)"""
    for f in frames:
        got = f.painted[0][3]
        if got[0] == recipe[0] and all(a == b for a, b in zip(recipe[1:], got[1:]) if a is not None):
            return f
    raise KeyError(recipe)


@functools.lru_cache(maxsize=None)
def tiny_frames(C):
    """frames of a few positions: 1 x 1; one wave plus two (C = 3: 1 x 22); the four-tile frame (TH + 1) x (TW + 1) whose
    corner tile lists fewer than 64 positions (its 64-row / TW-column edge tiles list a whole sliver: 64 x C and more); and two
    frames whose sliver tiles all stay below one wave, 7 x (TW + 1) and (TH + 1) x 7"""
    e, TW = Inst(64, C, 0), 192 // C
    fr = [tiled_frame("c%d_1x1" % C, e, 1, 1, [STRIPED], 7 + C),
          tiled_frame("c%d_1x%d" % (C, 66 // C), e, 1, 66 // C, [STRIPED], 8 + C)]
    img = _noise(65, TW + 1, C, 9 + C)
    big = Inst(64, C, 2)                                           # the widest ring paints the corner for S = 2 and S = 4
    rc, n = paint(img, big, 1, 1, only(2), 10 + C)
    fr.append(Frame("c%d_65x%d" % (C, TW + 1), img, [(big, 1, 1, rc, n)]))     # (a narrower ring lists a subset: still bin 2 only)
    fr.append(Frame("c%d_7x%d" % (C, TW + 1), _noise(7, TW + 1, C, 11 + C), []))
    fr.append(Frame("c%d_65x7" % C, _noise(65, 7, C, 12 + C), []))
    return tuple(fr)


SLIVERS = {"7x": (0, 1), "65x7": (1, 0)}                            # tiny frame -> its tile of fewer than 64 positions


INTERIOR_RECIPES = {3: [only(2), waves(None, None, 1, 63), waves(None, None, 0, 0), stray(0, 2, "last_wave"), pair(0, 2)],
                    1: [pair(0, 2)], 4: [pair(0, 2)]}


@functools.lru_cache(maxsize=None)
def interior_frames(C, S):
    """3 x 3 tiles of 64 x TW: the centre tile is interior (region, halos and the input region inside the frame).  Its REGION
    (tile + ring of S // 2, reaching into the neighbours' pixels) is painted by a recipe, the remainder is noise."""
    inst = Inst(64, C, S // 2)
    out = []
    for i, rc in enumerate(INTERIOR_RECIPES[C]):
        img = _noise(192, 3 * inst.TW, C, 50 + 10 * i + C + S)
        rc2, n = paint(img, inst, 1, 1, rc, 60 + 10 * i + C + S)
        out.append(Frame("c%d_s%d_3x3_%s" % (C, S, recipe_name(rc)), img, [(inst, 1, 1, rc2, n)]))
    return tuple(out)


def general_single_tile_frames(C):
    """the single-tile frames of the general C = 1 / C = 4 kernels"""
    fr = single_tile_frames(C)
    return tuple(frame_by_recipe(fr, rc) for rc in (only(1), pair(0, 2), waves(None, None, 0, 0)))


def all_frames():
    """every frame the GPU tests use"""
    out = []
    for th in (64, 32, 16):
        out += single_tile_frames(3, th)
    out += tiny_frames(3)
    for S in (2, 4):
        out += interior_frames(3, S)
    for C in (1, 4):
        out += general_single_tile_frames(C) + tiny_frames(C)[:3] + interior_frames(C, 2)
    return out


def census_table(frames):
    """lines 'frame  instance  tile  recipe  n0 n1 n2 total' of the painted tiles"""
    lines = []
    for f in frames:
        for inst, ty, tx, rc, n in f.painted:
            c = census(f.img, inst.TH, inst.C, inst.HR, ty, tx)
            lines.append("%-28s TH=%-2d C=%d HR=%d tile(%d,%d) %-22s %5d %5d %5d  total %5d" %
                         (f.name, inst.TH, inst.C, inst.HR, ty, tx, recipe_name(rc), c[0], c[1], c[2], c[3]))
    return lines
