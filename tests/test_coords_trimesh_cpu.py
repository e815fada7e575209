"""CPU-only: the triangle-mesh rasteriser's host twin (lerf_coords_trimesh_host: tri_setup / tri_pixel / tri_attr of
csrc/lerf_coords_models.h in a plain loop over faces and their pixel boxes with a plain min), coords.from_triangles and
coords.grid_faces on numpy arrays.

  1. the five entry points are declared, listed and exported; the ABI version stays 7;
  2. out, keys and depth_out equal the independent restatement (tests/coords_trimesh_ref.py) BY INTEGER PATTERN: a fan wider than the
     frame, one face over the whole frame, overlapping faces with depth ties, runs of skipped faces, every face skipped, F = 1, every
     orient and max_span, a texture seam through attr_faces; tiles at an origin in a strided out, every dtype mix;
  3. on invert_raster's own triangulation (grid_faces) from_triangles IS invert_raster, bit for bit, on every case of raster_cases();
  4. watertightness on a shared-edge mesh;
  5. perspective-correct interpolation against from_homography;
  6. a batch, shared faces, tiles of a larger frame, operands unmodified;
  7. every refused argument, on a sentinel-filled arena;
  8. the size rule.
"""
import functools
import os
import re

import numpy as np
import pytest

import coords_ref as R
import coords_trimesh_ref as TR
from conftest import REPO
from test_coords_raster_cpu import raster_cases

from lerf_pytorch_amd import _lib, coords

EINVAL, EUNSUPPORTED = -1, -2
NO_KEY = np.uint64(2 ** 64 - 1)
F32, F64 = _lib.LERF_F32, _lib.LERF_F64
NAMES = ("lerf_coords_trimesh_workspace_bytes", "lerf_coords_trimesh", "lerf_coords_trimesh_host", "lerf_coords_trimesh_batched",
         "lerf_coords_trimesh_batched_host")
HOMOGRAPHY = np.array([[1.9, 0.12, 5.0], [-0.08, 2.1, 3.0], [2.5e-3, -1.5e-3, 1.0]])


# ---------------------------------------------------------------------------------------------- the meshes
def fan_mesh(radius=200.0):
    """7 triangles around a centre vertex, far wider than either frame: every box is clipped on all four sides"""
    ang = 2.0 * np.pi * (np.arange(7) + 0.3) / 7.0
    pos = np.concatenate([[[14.3, 18.6]], np.stack([14.3 + radius * np.sin(ang), 18.6 + radius * np.cos(ang)], axis=-1)])
    attr = 0.37 * pos[:, ::-1] + np.array([3.0, -2.0])
    faces = np.array([[0, 1 + k, 1 + (k + 1) % 7] for k in range(7)], np.int32)
    return pos, attr, faces


def random_mesh():
    """20 overlapping faces on 12 vertices with depth: faces 7 and 11 repeat faces 2 and 3 (equal depth everywhere: the lower face
    wins), vertices 9 .. 11 lie far outside, so the faces made of them alone draw nothing"""
    rng = np.random.default_rng(11)
    pos = rng.uniform(-8.0, 45.0, (12, 2))
    pos[9:] = rng.uniform(-90.0, -40.0, (3, 2))
    attr = rng.uniform(0.0, 100.0, (12, 2))
    faces = rng.integers(0, 9, (20, 3)).astype(np.int32)
    for f in range(20):                                                  # three different vertices a face
        while len(set(faces[f])) < 3:
            faces[f] = rng.integers(0, 9, 3)
    faces[7], faces[11] = faces[2], faces[3]
    faces[15], faces[19] = (9, 10, 11), (11, 10, 9)
    depth = rng.choice(np.array([1.0, 1.5, 2.0], np.float32), 12)
    return pos, attr, faces, depth


def skipped_mesh():
    """drawn faces with runs of skipped ones before, between and after them; every kind of skip"""
    good = np.array([[2.5, 3.5], [30.0, 6.0], [8.0, 33.0], [27.0, 30.0], [5.0, 20.0], [5.0, 24.0], [5.0, 30.0]])      # 4, 5, 6 collinear
    bad = np.array([[np.nan, 4.0], [3.0, np.inf], [-np.inf, 2.0], [1e300, 1e300], [-1e300, 1e300]])      # two of them in a face: area2 is not finite
    extra = np.array([[12.0, 12.0], [20.0, 14.0], [15.0, 22.0], [22.0, 25.0]])      # 12: NaN depth; 13, 14, 15: w 0, negative, inf
    pos = np.concatenate([good, bad, extra])
    V = len(pos)
    attr = np.stack([np.arange(V) * 1.25, 50.0 - np.arange(V) * 0.5], axis=-1)
    depth = np.linspace(1.0, 2.0, V).astype(np.float32)
    depth[12] = np.nan
    w = np.linspace(0.75, 1.5, V).astype(np.float32)
    w[13], w[14], w[15] = 0.0, -1.0, np.inf
    skipped = [[0, 1, 7], [8, 1, 2], [0, 9, 2], [10, 11, 2], [11, 1, 10], [0, 0, 1], [1, 2, 2], [-1, 1, 2], [0, V, 2], [0, 1, 2 ** 31 - 1],
               [4, 5, 6], [0, 1, 12], [0, 13, 2], [14, 1, 2], [0, 1, 15], [-2 ** 31, 1, 2]]
    faces = np.array(skipped[:6] + [[0, 1, 2]] + skipped[6:11] + [[3, 2, 1]] + skipped[11:], np.int32)
    return pos, attr, faces, depth, w, np.array(skipped, np.int32)


def seam_mesh():
    """a welded quad whose two faces carry their own texture coordinates: attr_faces differs from faces"""
    pos = np.array([[2.0, 3.0], [4.0, 30.0], [25.0, 2.0], [26.0, 33.0]])
    attr = np.array([[0.0, 0.0], [0.0, 10.0], [10.0, 0.0], [50.0, 60.0], [50.0, 50.0], [60.0, 60.0]])
    return pos, attr, np.array([[0, 1, 2], [2, 1, 3]], np.int32), np.array([[0, 1, 2], [3, 4, 5]], np.int32)


def trimesh_cases():
    """name -> (pos, attr, faces, out_hw, keywords): what the host twin, the restatement and the kernel agree on"""
    cases = {}
    small, wide = (29, 37), (64, 150)
    pos, attr, faces = fan_mesh()
    cases["fan_small"] = (pos, attr, faces, small, {})
    cases["fan_wide"] = (pos.astype(np.float32), attr, faces, wide, {"out_dtype": np.float32})
    cases["fan_tile"] = (pos, attr.astype(np.float32), faces, (5, 67), {"origin": (3, 7), "out_dtype": np.float64})
    cases["fan_pixel"] = (pos.astype(np.float32), attr.astype(np.float32), faces, (1, 1), {"origin": (3, 7), "out_dtype": np.float32})
    cases["whole"] = (np.array([[-10.0, -10.0], [-10.0, 400.0], [200.0, -10.0]]), np.array([[0.0, 0.0], [0.0, 1.0], [1.0, 0.0]]),
                      np.array([[0, 1, 2]], np.int32), wide, {})
    pos, attr, faces, depth = random_mesh()
    cases["random_depth"] = (pos, attr, faces, small, {"depth": depth})
    cases["random_depth_f32"] = (pos.astype(np.float32), attr.astype(np.float32), faces, small, {"depth": depth, "out_dtype": np.float32})
    cases["random_plain"] = (pos, attr, faces, small, {})
    pos, attr, faces, depth, w, skipped = skipped_mesh()
    cases["skipped"] = (pos, attr, faces, small, {"depth": depth, "w": w})
    cases["skipped_tile"] = (pos, attr, faces, (5, 67), {"depth": depth, "w": w, "origin": (3, 7)})
    cases["all_skipped"] = (pos, attr, skipped, small, {"depth": depth, "w": w})
    cases["one_face"] = (pos, attr, faces[6:7], small, {"w": w})
    # faces one pixel and a dozen pixels wide, then five of the fan's faces (both orientations, some 200 wide, with gaps between them),
    # then a face 400 pixels wide that covers the columns from 20 on: every orient and max_span
    pos, attr, faces = fan_mesh()
    faces[1::2] = faces[1::2][:, ::-1]
    tiny = np.array([[4.8, 4.9], [5.3, 4.7], [5.1, 5.4], [10.2, 20.1], [21.7, 22.3], [12.4, 31.6], [20.2, 3.1], [9.6, 5.5], [18.4, 14.9],
                     [-10.0, 20.0], [-10.0, 420.0], [200.0, 20.0]])
    more = np.array([[8, 9, 10], [10, 9, 8], [11, 12, 13], [14, 15, 16], [16, 15, 14]], np.int32)
    pos, attr = np.concatenate([pos, tiny]), np.concatenate([attr, 2.0 * tiny + 1.0])
    faces = np.concatenate([more, faces[[1, 2, 4, 5, 6]], np.array([[17, 18, 19]], np.int32)])
    for orient in (-1, 0, 1):
        for span in (0, 1, 16, 300):
            cases["orient%d_span%d" % (orient, span)] = (pos, attr, faces, small, {"orient": orient, "max_span": span})
    cases["span300_wide"] = (pos, attr, faces, wide, {"max_span": 300})
    pos, attr, faces, afaces = seam_mesh()
    cases["seam"] = (pos, attr, faces, small, {"attr_faces": afaces})
    return cases


CASES = trimesh_cases()


@functools.lru_cache(maxsize=None)
def restated(name):
    """(out, keys, depth_out) of a case by the restatement: computed once, shared, left unchanged"""
    pos, attr, faces, hw, kw = CASES[name]
    res = TR.trimesh(pos, attr, faces, hw, **kw)
    for a in res:
        a.setflags(write=False)
    return res


def run_case(one, name, wrap=lambda a: a):
    """the case through `one` (coords_trimesh_host or ops.coords_trimesh): tiles are written in place into a larger strided map"""
    pos, attr, faces, hw, kw = CASES[name]
    kw = dict(kw)
    dt = kw.pop("out_dtype", np.float64)
    origin = kw.get("origin", (0, 0))
    full = wrap(np.full((origin[0] + hw[0] + 2, origin[1] + hw[1] + 3, 2), -7.0, dt))
    view = full[origin[0]:origin[0] + hw[0], origin[1]:origin[1] + hw[1]]
    args = {k: (v if isinstance(v, (int, tuple)) else wrap(v)) for k, v in kw.items()}
    res = one(wrap(pos), wrap(attr), wrap(faces), hw, out=view, return_keys=True, return_depth="depth" in kw, **args)
    return full, view, res


def check_case(name, full, view, res, to_numpy=np.asarray):
    pos, attr, faces, hw, kw = CASES[name]
    ref_out, ref_keys, ref_depth = restated(name)
    full, out, keys = to_numpy(full), to_numpy(res[0]), to_numpy(res[1]).view(np.uint64)
    assert R.same_bits(out, ref_out), name
    assert np.array_equal(keys, ref_keys), name
    if "depth" in kw:
        assert R.same_bits(to_numpy(res[2]), ref_depth), name
    origin = kw.get("origin", (0, 0))
    rest = np.ones(full.shape[:2], bool)
    rest[origin[0]:origin[0] + hw[0], origin[1]:origin[1] + hw[1]] = False
    assert (full[rest] == -7.0).all(), name                              # nothing beside the tile is written
    return out, keys


def grid_call(F, hw, depth, span, orient, one=None, wrap=lambda a: a):
    """from_triangles on invert_raster's own triangulation of the map F"""
    fH, fW = F.shape[:2]
    ii, jj = np.meshgrid(np.arange(fH, dtype=np.float64), np.arange(fW, dtype=np.float64), indexing="ij")
    one = _lib.coords_trimesh_host if one is None else one
    return one(wrap(np.ascontiguousarray(F.reshape(-1, 2))), wrap(np.stack([ii, jj], axis=-1).reshape(-1, 2)), wrap(coords.grid_faces(fH, fW)), hw,
               depth=None if depth is None else wrap(np.ascontiguousarray(depth.reshape(-1))), max_span=span, orient=orient, return_keys=True)


# ---------------------------------------------------------------------------------------------- 1. exports
def test_exports_and_abi_version():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "lerf_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lerf_[a-z0-9_]+)\s*\(", src))
    for n in NAMES:
        assert n in declared and n in _lib.EXPORTS and hasattr(_lib.lib(), n), n
    assert _lib.lib().lerf_abi_version() == 7


# ---------------------------------------------------------------------------------------------- 2. the restatement
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_twin_equals_the_restatement(name):
    out, keys = check_case(name, *run_case(_lib.coords_trimesh_host, name))
    holes = keys == NO_KEY
    assert np.array_equal(np.isnan(out[..., 0]), holes) and np.array_equal(np.isnan(out[..., 1]), holes)


def test_what_the_cases_exercise():
    """the properties the cases were built for, read off the restatement"""
    _, keys, _ = restated("fan_small")
    assert not (keys == NO_KEY).any() and len(np.unique(keys & np.uint64(0xffffffff))) == 7
    _, keys, _ = restated("whole")
    assert not (keys == NO_KEY).any()
    _, keys, _ = restated("random_depth")
    faces = set(int(k) & 0xffffffff for k in keys[keys != NO_KEY])
    assert faces and not faces & {7, 11, 15, 19} and (keys == NO_KEY).any()          # the repeated faces lose their ties; two faces lie outside
    _, plain, _ = restated("random_plain")
    assert (plain != keys).any()
    out, keys, _ = restated("skipped")
    assert set(int(k) & 0xffffffff for k in keys[keys != NO_KEY]) == {6, 12}
    out, keys, zo = restated("all_skipped")
    assert (keys == NO_KEY).all() and np.isnan(out).all() and np.isnan(zo).all()
    kept = {(o, s): set(int(k) & 0xffffffff for k in restated("orient%d_span%d" % (o, s))[1].ravel()) - {0xffffffff} for o in (-1, 0, 1)
            for s in (0, 1, 16, 300)}
    assert kept[0, 1] and kept[0, 1] < kept[0, 16] < kept[0, 300] < kept[0, 0] and kept[0, 0] - kept[0, 300] == {10}
    assert kept[1, 0] and kept[-1, 0] and not kept[1, 0] & kept[-1, 0] and kept[1, 0] | kept[-1, 0] >= kept[0, 0]
    out, keys, _ = restated("seam")
    low = keys & np.uint64(0xffffffff)
    assert out[low == 0].max() <= 10.0 and out[(low == 1) & (keys != NO_KEY)].min() >= 50.0


# ---------------------------------------------------------------------------------------------- 3. against invert_raster
@pytest.mark.parametrize("case", raster_cases(), ids=lambda c: c[0])
def test_grid_faces_give_invert_raster(case):
    name, F, hw, depth, span, orient = case
    G, K = _lib.coords_invert_raster_host(np.ascontiguousarray(F), hw, depth=depth, max_span=span, orient=orient, return_keys=True)
    out, keys = grid_call(F, hw, depth, span, orient)
    assert R.same_bits(out, G) and np.array_equal(keys, K)
    fH, fW = F.shape[:2]
    ii, jj = np.meshgrid(np.arange(fH, dtype=np.float64), np.arange(fW, dtype=np.float64), indexing="ij")
    got = coords.from_triangles(F.reshape(-1, 2), np.stack([ii, jj], axis=-1).reshape(-1, 2), coords.grid_faces(fH, fW), hw,
                                depth=None if depth is None else depth.reshape(-1), max_span=span, orient=orient, return_faces=True)
    assert R.same_bits(got[0], G)
    assert np.array_equal(got[1], np.where(K == NO_KEY, np.int64(-1), (K & np.uint64(0xffffffff)).astype(np.int64)))


def test_grid_faces():
    f = coords.grid_faces(3, 4)
    assert f.dtype == np.int32 and f.shape == (12, 3)
    assert f[:2].tolist() == [[0, 1, 4], [5, 4, 1]] and f[-1].tolist() == [11, 10, 7]
    for bad in ((1, 4), (3, 1)):
        with pytest.raises(ValueError):
            coords.grid_faces(*bad)


# ---------------------------------------------------------------------------------------------- 4. watertightness
def test_shared_edges_leave_no_hole():
    ident = coords.from_flow(np.zeros((13, 17, 2)))
    out, keys = grid_call(1.5 * ident, (19, 25), None, 0, 0)
    assert not (keys == NO_KEY).any() and not np.isnan(out).any()
    rot = ident @ np.array([[0.75, -1.25], [1.25, 0.75]]).T + np.array([20.0, 0.0])
    out, keys = grid_call(rot, (30, 28), None, 0, 0)
    assert int((keys != NO_KEY).sum()) == 416


# ---------------------------------------------------------------------------------------------- 5. perspective
def test_perspective_correct_interpolation_matches_the_homography():
    src = np.array([[0.0, 0.0], [0.0, 31.0], [23.0, 0.0], [23.0, 31.0]])          # (row, col) corners of a 24 x 32 source
    X = HOMOGRAPHY @ np.stack([src[:, 1], src[:, 0], np.ones(4)])                  # x = col, y = row
    pos = np.stack([X[1] / X[2], X[0] / X[2]], axis=-1)
    faces = np.array([[0, 1, 2], [3, 2, 1]], np.int32)
    got, face = coords.from_triangles(pos, src, faces, (70, 90), w=X[2], return_faces=True)
    ref = coords.from_homography(HOMOGRAPHY, (70, 90))
    covered = face >= 0
    err = np.abs(got - ref)[covered] / np.maximum(np.abs(ref[covered]), 1.0)
    print("perspective: %d covered pixels, max error %.3g of the bound 1e-9" % (covered.sum(), err.max()))
    assert covered.sum() > 2000 and err.max() <= 1e-9
    affine = coords.from_triangles(pos, src, faces, (70, 90))
    off = np.abs(affine - ref)[covered].max()
    print("the same call without w: off by up to %.3g px" % off)
    assert off > 0.1


# ---------------------------------------------------------------------------------------------- 6. operand handling
def test_a_batch_equals_its_single_calls():
    pos, attr, faces, depth = random_mesh()
    rng = np.random.default_rng(5)
    P = np.stack([pos, pos + rng.uniform(-2.0, 2.0, pos.shape), pos[::-1]])
    A = np.stack([attr, attr * 0.5, attr + 1.0]).astype(np.float32)
    D = np.stack([depth, depth[::-1], depth])
    Fs = np.stack([faces, faces[::-1], np.roll(faces, 3, axis=0)])
    singles = [_lib.coords_trimesh_host(P[s], A[s], Fs[s], (29, 37), depth=D[s], return_keys=True, return_depth=True) for s in range(3)]
    before = [a.copy() for a in (P, A, D, Fs)]
    batch = _lib.coords_trimesh_host(P, A, Fs, (29, 37), depth=D, return_keys=True, return_depth=True)
    assert batch[0].shape == (3, 29, 37, 2) and batch[0].dtype == np.float32
    for s in range(3):
        assert all(R.same_bits(batch[k][s], singles[s][k]) if k != 1 else np.array_equal(batch[k][s], singles[s][k]) for k in range(3))
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip((P, A, D, Fs), before))          # operands unmodified
    # shared faces (a set stride of 0) against the same faces per set
    shared = _lib.coords_trimesh_host(P, A, faces, (29, 37), depth=D, return_keys=True)
    per_set = _lib.coords_trimesh_host(P, A, np.stack([faces] * 3), (29, 37), depth=D, return_keys=True)
    assert R.same_bits(shared[0], per_set[0]) and np.array_equal(shared[1], per_set[1])
    # the public function: a batch in, a batch out
    got = coords.from_triangles(P, A, faces.astype(np.int64), (29, 37), depth=D, return_depth=True, return_faces=True)
    assert R.same_bits(got[0], per_set[0]) and got[1].shape == (3, 29, 37) and got[2].dtype == np.int64


def test_tiles_of_a_larger_frame_equal_the_whole():
    pos, attr, faces, depth = random_mesh()
    whole = _lib.coords_trimesh_host(pos, attr, faces, (29, 37), depth=depth, return_keys=True, return_depth=True)
    for origin, hw in (((0, 0), (4, 16)), ((3, 7), (5, 27)), ((27, 30), (2, 7)), ((11, 19), (1, 1))):
        tile = _lib.coords_trimesh_host(pos, attr, faces, hw, depth=depth, origin=origin, return_keys=True, return_depth=True)
        for k in range(3):
            assert np.array_equal(R.bits(tile[k]) if k != 1 else tile[k],
                                  (R.bits(whole[k]) if k != 1 else whole[k])[origin[0]:origin[0] + hw[0], origin[1]:origin[1] + hw[1]])


# ---------------------------------------------------------------------------------------------- 7. refusals
def _ptr(a):
    return a.ctypes.data


def test_every_refused_argument_leaves_the_arena_untouched():
    lib = _lib.lib()
    V, F, oH, oW = 5, 3, 6, 8
    need = lib.lerf_coords_trimesh_workspace_bytes(F, 1)
    assert need == 4 * (F + 1) and lib.lerf_coords_trimesh_workspace_bytes(F, 2) == 8 * (F + 1)
    assert lib.lerf_coords_trimesh_workspace_bytes(0, 1) == 0 and lib.lerf_coords_trimesh_workspace_bytes(F, 0) == 0
    pos = np.array([[0.5, 0.5], [0.5, 7.0], [5.0, 0.5], [5.0, 7.0], [2.0, 3.0]])
    attr = pos * 2.0
    faces = np.array([[0, 1, 2], [3, 2, 1], [0, 4, 1]], np.int32)
    depth, w = np.ones(V, np.float32), np.ones(V, np.float32)
    out, keys, zo = np.full((oH, oW, 2), -7.0), np.full((oH, oW), 5, np.uint64), np.full((oH, oW), -7.0, np.float32)
    ws = np.full(2 * need + 8, 0x55, np.uint8)
    big = np.full((12, 8, 2), -7.0)
    arena = (pos, attr, faces, depth, w)
    before = [a.copy() for a in arena]

    def tri(P=pos, pdt=F64, V=V, A=attr, adt=F64, Va=V, Fc=faces, AF=None, F=F, D=depth, Wv=w, wdt=F32, o=out, dt=F64, so=16, oH=oH, oW=oW, i0=0, j0=0,
            span=0, orient=0, K=keys, Z=None, S=ws, sb=None, poff=0, aoff=0, foff=0, off=0, koff=0, soff=0, host=True, batch=None):
        p = lambda a, o=0: None if a is None else _ptr(a) + o
        sb = lib.lerf_coords_trimesh_workspace_bytes(F, batch[0] if batch else 1) if sb is None else sb
        args = (p(P, poff), pdt, V, p(A, aoff), adt, Va, p(Fc, foff), p(AF), F, p(D), p(Wv), wdt, p(o, off), dt, so, oH, oW, i0, j0, span, orient,
                p(K, koff), p(Z), p(S, soff), sb)
        if batch is not None:
            name, args = "lerf_coords_trimesh_batched", args + batch
        else:
            name = "lerf_coords_trimesh"
        return getattr(lib, name + "_host")(*args) if host else getattr(lib, name)(*args, None)

    assert tri() == 0 and tri(D=None, Wv=None) == 0 and tri(Z=zo) == 0 and tri(AF=faces) == 0
    assert not (out == -7.0).all()
    out[:], keys[:], zo[:], ws[:] = -7.0, 5, -7.0, 0x55
    two = (2, 0, 0, 0, 0, 0, 0)                                          # two sets that share every input
    for host in (True, False):                                            # the device entry point refuses before it touches the GPU
        calls = [tri(P=None, host=host), tri(A=None, host=host), tri(Fc=None, host=host), tri(o=None, host=host), tri(K=None, host=host),
                 tri(S=None, host=host), tri(pdt=0, host=host), tri(adt=9, host=host), tri(dt=9, host=host), tri(wdt=9, host=host), tri(wdt=0, host=host),
                 tri(V=0, host=host), tri(Va=0, host=host), tri(F=0, host=host), tri(V=-1, host=host), tri(F=-3, host=host),
                 tri(oH=0, host=host), tri(oW=0, host=host), tri(oH=-1, host=host), tri(so=15, host=host), tri(so=14, host=host),
                 tri(span=-1, host=host), tri(span=65537, host=host), tri(orient=2, host=host), tri(orient=-2, host=host),
                 tri(D=None, Z=zo, host=host),                                                     # depth_out without depth
                 tri(sb=need - 1, host=host), tri(soff=1, host=host), tri(sb=0, host=host),        # a short or misaligned workspace
                 tri(i0=-1, host=host), tri(j0=-1, host=host), tri(i0=2 ** 31 - 3, host=host),
                 tri(poff=8, host=host), tri(aoff=4, host=host), tri(foff=2, host=host), tri(off=8, host=host), tri(koff=4, host=host),
                 tri(o=pos, oH=1, oW=5, so=10, host=host), tri(o=attr, oH=1, oW=5, so=10, host=host),   # out IS an input
                 tri(K=pos, oH=1, oW=5, host=host), tri(K=out, host=host), tri(Z=out, dt=F64, host=host),
                 tri(S=out, host=host), tri(S=keys, host=host), tri(S=pos, sb=80, host=host), tri(S=faces, sb=36, host=host),
                 tri(Z=depth, oH=1, oW=5, host=host), tri(o=big, K=big, koff=8 * 16 * 3, oH=6, so=16, host=host),
                 tri(batch=two + (0, 48, 0), host=host), tri(batch=two + (96, 0, 0), host=host),   # an output shared between sets
                 tri(batch=two + (96, 48, 0), Z=zo, host=host), tri(batch=two + (95, 48, 0), host=host),
                 tri(batch=(0, 0, 0, 0, 0, 0, 0, 0, 0, 0), host=host), tri(batch=(2, 1, 0, 0, 0, 0, 0, 96, 48, 0), host=host)]
        assert calls == [EINVAL] * len(calls), (host, calls)
    assert (out == -7.0).all() and (keys == 5).all() and (zo == -7.0).all() and (ws == 0x55).all() and (big == -7.0).all()
    assert all(np.array_equal(a, b) for a, b in zip(arena, before))
    # through the Python layer
    with pytest.raises(ValueError, match="lerf_coords_trimesh_host"):
        _lib.coords_trimesh_host(pos, attr, faces, (6, 8), max_span=-1)
    with pytest.raises(ValueError, match="lerf_coords_trimesh_host"):
        _lib.coords_trimesh_host(pos, attr, faces, (6, 8), orient=3)
    with pytest.raises(ValueError, match="faces"):
        _lib.coords_trimesh_host(pos, attr, faces.astype(np.int64), (6, 8))
    with pytest.raises(ValueError, match="depth"):
        _lib.coords_trimesh_host(pos, attr, faces, (6, 8), depth=np.ones(V))
    with pytest.raises(ValueError, match="depth"):
        _lib.coords_trimesh_host(pos, attr, faces, (6, 8), return_depth=True)
    with pytest.raises(ValueError, match="keys"):
        _lib.coords_trimesh_host(pos, attr, faces, (6, 8), keys=np.zeros((6, 8), np.int64))
    with pytest.raises(ValueError, match="attr_faces"):
        _lib.coords_trimesh_host(pos, attr, faces, (6, 8), attr_faces=faces[:2])
    with pytest.raises(ValueError):
        _lib.coords_trimesh_host(pos[:, :1], attr, faces, (6, 8))


def test_from_triangles_refuses_mixed_operands_and_autograd():
    import torch
    pos, attr, faces, depth = random_mesh()

    class Dev:                                                        # stands for a device tensor: from_triangles looks at is_cuda
        is_cuda, requires_grad = True, False
    with pytest.raises(ValueError, match="mixed"):
        coords.from_triangles(pos, attr, faces, (8, 8), depth=Dev())
    for k in range(2):
        ops = [torch.from_numpy(pos), torch.from_numpy(attr)]
        ops[k].requires_grad_(True)
        with pytest.raises(ValueError, match="autograd"):
            coords.from_triangles(ops[0], ops[1], faces, (8, 8))
        with torch.no_grad():
            assert R.same_bits(coords.from_triangles(ops[0], ops[1], faces, (8, 8)), coords.from_triangles(pos, attr, faces, (8, 8)))
    with pytest.raises(ValueError, match="autograd"):
        coords.from_triangles(pos, attr, faces, (8, 8), w=torch.ones(12, requires_grad=True))
    for bad in (lambda: coords.from_triangles(pos, attr, faces, (0, 8)), lambda: coords.from_triangles(pos, attr, faces.astype(np.float64), (8, 8)),
                lambda: coords.from_triangles(pos, attr, faces, (8, 8), return_depth=True),
                lambda: coords.from_triangles(pos, attr, faces, (8, 8), dtype=np.int32)):
        with pytest.raises(ValueError):
            bad()
    # an int64 index beyond int32 must not wrap into the mesh
    far = faces.astype(np.int64)
    far[0, 0] += 2 ** 32
    got = coords.from_triangles(pos, attr, far, (29, 37), return_faces=True)
    ref = coords.from_triangles(pos, attr, np.concatenate([[[-1, 0, 1]], faces[1:]]), (29, 37), return_faces=True)
    assert R.same_bits(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and not (got[1] == 0).any()


# ---------------------------------------------------------------------------------------------- 8. the size rule
def test_the_size_rule_is_judged_before_the_pointers():
    lib = _lib.lib()

    def rule(F, n_sets, oH, oW, span, host=True):
        args = (None, F64, 3, None, F64, 3, None, None, F, None, None, F32, None, F64, 2 * oW, oH, oW, 0, 0, span, 0, None, None, None, 0)
        if n_sets > 1:
            args, name = args + (n_sets,) + (0,) * 9, "lerf_coords_trimesh_batched"
        else:
            name = "lerf_coords_trimesh"
        return getattr(lib, name + "_host")(*args) if host else getattr(lib, name)(*args, None)

    tiles = 540 * 240                                                    # the 4 x 16 tiles of 2160 x 3840
    most = (2 ** 32 - 1) // tiles
    assert 33000 < most < 33200
    for host in (True, False):
        assert rule(most, 1, 2160, 3840, 0, host) == EINVAL                # within the rule: the null pointers are what is refused
        assert rule(most + 1, 1, 2160, 3840, 0, host) == EUNSUPPORTED
        assert rule(most // 2 + 1, 2, 2160, 3840, 0, host) == EUNSUPPORTED
        # max_span 16: a box touches at most 5 x 2 tiles
        assert rule((2 ** 32 - 1) // 10, 1, 2160, 3840, 16, host) == EINVAL and rule((2 ** 32 - 1) // 10 + 1, 1, 2160, 3840, 16, host) == EUNSUPPORTED
        assert rule(2 ** 31 - 1, 1, 4, 16, 0, host) == EINVAL               # one tile a face
        assert rule(2 ** 31 - 1, 2, 4, 16, 0, host) == EUNSUPPORTED         # 2^32 slots of the scan
    assert _lib.trimesh_max_items(most + 1, 1, (2160, 3840), 0) > 2 ** 32 - 1 >= _lib.trimesh_max_items(most, 1, (2160, 3840), 0)
    assert _lib.trimesh_max_items(7, 2, (2160, 3840), 16) == 7 * 2 * 10 and _lib.trimesh_max_items(7, 1, (3, 9), 300) == 7
    with pytest.raises(_lib.LerfError, match="max_span"):
        _lib.coords_trimesh_host(np.zeros((3, 2)), np.zeros((3, 2)), np.zeros((most + 1, 3), np.int32), (2160, 3840))
