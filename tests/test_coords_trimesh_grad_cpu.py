"""CPU-only: the host twin of the triangle mesh's adjoint (lerf_coords_trimesh_bwd_host, DESIGN 4.22: tri_attr_bwd / tri_bwd_thread /
tri_face_terms of csrc/lerf_coords_models.h -- a 256-slot array per face, the fixed tree, the sorted per-vertex lists).

  1. the five entry points are declared, listed and exported; the ABI version stays 7;
  2. the three gradients against the independent restatement (tests/coords_trimesh_grad_ref.py: torch float64 autograd on the winning
     faces) within the family's bound 1e-9 * max(max |ref|, 1) per gradient tensor: one face whose clipped box has exactly 1, 3, 4, 5
     and 24 item tiles and one face over the whole 64 x 150 frame (160), the fan, the overlapping faces with depth ties, a texture
     seam, a repeated attribute index, the perspective mesh with w as float32 and float64, a tile at origin (3, 7);
  3. the cap: max_adders 7 passes on the fan, 6 poisons the centre alone; skipped faces leave their vertices' pre-fill bit for bit;
  4. NaN in every hole of grad_out, accumulation, every NULL combination, a batch against its single calls, operands unmodified;
  5. every refusal on a sentinel-filled arena; the size rule without pointers.
"""
import math
import os
import re

import numpy as np
import pytest

import coords_ref as R
import coords_trimesh_grad_ref as GR
from conftest import REPO
from test_coords_trimesh_cpu import HOMOGRAPHY, fan_mesh, random_mesh, seam_mesh, skipped_mesh

from lerf_pytorch_amd import _lib

EINVAL, EUNSUPPORTED = -1, -2
NO_KEY = np.uint64(2 ** 64 - 1)
F32, F64 = _lib.LERF_F32, _lib.LERF_F64
NAMES = ("lerf_coords_trimesh_bwd_workspace_bytes", "lerf_coords_trimesh_bwd", "lerf_coords_trimesh_bwd_host", "lerf_coords_trimesh_bwd_batched",
         "lerf_coords_trimesh_bwd_batched_host")


# ---------------------------------------------------------------------------------------------- the cases
def one_face(tiles):
    """one large face whose clipped box in a 32 x 48 frame has exactly `tiles` item tiles of 4 x 16 pixels"""
    pos = {1: [[0.2, 0.3], [3.6, 2.0], [0.5, 14.8]], 3: [[0.2, 0.5], [3.8, 20.0], [0.4, 46.5]], 4: [[0.5, 0.5], [15.5, 3.0], [6.0, 14.5]],
           5: [[0.5, 0.5], [19.5, 3.0], [8.0, 14.5]], 24: [[1.0, 2.0], [30.0, 10.0], [5.0, 45.0]]}[tiles]
    return np.array(pos), np.array([[3.0, 40.0], [55.0, 8.0], [21.0, 77.0]]), np.array([[0, 1, 2]], np.int32)


def perspective_mesh():
    """the homography-corner mesh of the forward's perspective test: two faces, w the homogeneous coordinate"""
    src = np.array([[0.0, 0.0], [0.0, 31.0], [23.0, 0.0], [23.0, 31.0]])
    X = HOMOGRAPHY @ np.stack([src[:, 1], src[:, 0], np.ones(4)])
    return np.stack([X[1] / X[2], X[0] / X[2]], axis=-1), src, np.array([[0, 1, 2], [3, 2, 1]], np.int32), X[2]


def grad_cases():
    """name -> (pos, attr, faces, out_hw, keywords of the forward): shared with the GPU test"""
    cases = {}
    for n in (1, 3, 4, 5, 24):
        cases["tiles%d" % n] = one_face(n) + ((32, 48), {})
    cases["whole"] = (np.array([[-10.0, -10.0], [-10.0, 400.0], [200.0, -10.0]]), np.array([[0.0, 0.0], [0.0, 1.0], [1.0, 0.0]]),
                      np.array([[0, 1, 2]], np.int32), (64, 150), {})
    cases["whole_w"] = cases["whole"][:4] + ({"w": np.array([0.5, 2.0, 1.25])},)
    pos, attr, faces = fan_mesh()
    cases["fan"] = (pos, attr, faces, (29, 37), {})
    cases["fan_tile"] = (pos, attr.astype(np.float32), faces, (5, 67), {"origin": (3, 7)})
    pos, attr, faces, depth = random_mesh()
    cases["random_depth"] = (pos, attr, faces, (29, 37), {"depth": depth})
    cases["random_f32"] = (pos.astype(np.float32), attr.astype(np.float32), faces, (29, 37), {"depth": depth})
    pos, attr, faces, afaces = seam_mesh()
    cases["seam"] = (pos, attr, faces, (29, 37), {"attr_faces": afaces})
    cases["repeat"] = (pos, attr, faces, (29, 37), {"attr_faces": np.array([[0, 1, 2], [3, 3, 5]], np.int32)})
    pos, attr, faces, w = perspective_mesh()
    cases["perspective_f64"] = (pos, attr, faces, (70, 90), {"w": w})
    cases["perspective_f32"] = (pos, attr, faces, (70, 90), {"w": w.astype(np.float32)})
    return cases


CASES = grad_cases()


def item_tiles(tri, hw, origin=(0, 0)):
    """the 4 x 16 item tiles of a face's clipped box, by the forward's rule"""
    n = 1
    for axis, tile in ((0, 4), (1, 16)):
        lo = max(math.ceil(tri[:, axis].min()), origin[axis])
        hi = min(math.floor(tri[:, axis].max()), origin[axis] + hw[axis] - 1)
        n *= (hi - origin[axis]) // tile - (lo - origin[axis]) // tile + 1
    return n


def area2(tri):
    return (tri[1, 1] - tri[0, 1]) * (tri[2, 0] - tri[0, 0]) - (tri[1, 0] - tri[0, 0]) * (tri[2, 1] - tri[0, 1])


def face_plane(keys):
    keys = np.asarray(keys).view(np.uint64)
    return np.where(keys == NO_KEY, np.int64(-1), (keys & np.uint64(0xffffffff)).astype(np.int64))


def upstream(keys, seed=3):
    """a random upstream gradient with NaN in EVERY hole"""
    keys = np.asarray(keys).view(np.uint64)
    g = np.random.default_rng(seed).standard_normal(keys.shape + (2,))
    g[keys == NO_KEY] = np.nan
    return g


def forward(name):
    pos, attr, faces, hw, kw = CASES[name]
    out, keys = _lib.coords_trimesh_host(pos, attr, faces, hw, return_keys=True, **kw)
    return keys


def backward(name, keys, g, **extra):
    pos, attr, faces, hw, kw = CASES[name]
    need = extra.pop("need", (True, True, "w" in kw))
    return _lib.coords_trimesh_bwd_host(pos, attr, faces, hw, keys, g, need=need, **kw, **extra)


def reference(name, keys, g):
    pos, attr, faces, hw, kw = CASES[name]
    return GR.gradients(face_plane(keys), pos, attr, faces, g, attr_faces=kw.get("attr_faces"), w=kw.get("w"), origin=kw.get("origin", (0, 0)))


def check_against_reference(name, got, ref):
    for what, a, b in zip(("attr", "pos", "w"), got, ref):
        if b is None:
            assert a is None
            continue
        err, bound = GR.within(a, b)
        print("%s %s: max error %.3g, bound %.3g" % (name, what, err, bound))
        assert np.isfinite(a).all() and err <= bound, (name, what, err, bound)


# ---------------------------------------------------------------------------------------------- 1. exports
def test_exports_and_abi_version():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "lerf_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lerf_[a-z0-9_]+)\s*\(", src))
    for n in NAMES:
        assert n in declared and n in _lib.EXPORTS and hasattr(_lib.lib(), n), n
    assert _lib.lib().lerf_abi_version() == 7


# ---------------------------------------------------------------------------------------------- 2. the restatement
def test_the_one_face_cases_have_the_stated_item_tiles():
    for n in (1, 3, 4, 5, 24):
        pos, _, _, hw, _ = CASES["tiles%d" % n]
        assert item_tiles(pos, hw) == n and abs(area2(pos)) >= 1.0
    assert item_tiles(CASES["whole"][0], (64, 150)) == 160
    pos, _, _, hw, _ = CASES["tiles24"]
    assert (math.floor(pos[:, 1].max()) // 16) - (math.ceil(pos[:, 1].min()) // 16) + 1 == 3          # ntc > 1


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_twin_within_the_bound_of_the_restatement(name):
    keys = forward(name)
    assert (keys != NO_KEY).any()
    g = upstream(keys)                                                   # NaN in every hole: it must reach nothing
    got = backward(name, keys, g)
    check_against_reference(name, got, reference(name, keys, g))
    again = backward(name, keys, g)
    assert all(a is None and b is None or R.same_bits(a, b) for a, b in zip(got, again))


def test_only_winners_contribute():
    keys = forward("random_depth")
    won = set(int(k) & 0xffffffff for k in keys[keys != NO_KEY])
    assert won and not won & {7, 11, 15, 19}
    pos, attr, faces, hw, kw = CASES["random_depth"]
    ga, gp, _ = backward("random_depth", keys, upstream(keys))
    losers = sorted(set(range(12)) - set(int(v) for f in won for v in faces[f]))
    assert losers and (ga[losers] == 0.0).all() and (gp[losers] == 0.0).all()


# ---------------------------------------------------------------------------------------------- 3. the cap and the skipped faces
def test_max_adders_poisons_the_centre_of_the_fan_alone():
    keys = forward("fan")
    g = upstream(keys)
    ga7, gp7, _, most = backward("fan", keys, g, max_adders=7, return_most=True)
    assert most == 7 and np.isfinite(ga7).all() and np.isfinite(gp7).all()
    ga6, gp6, _, most = backward("fan", keys, g, max_adders=6, return_most=True)
    assert most == 7
    assert np.isnan(ga6[0]).all() and np.isnan(gp6[0]).all()
    assert R.same_bits(ga6[1:], ga7[1:]) and R.same_bits(gp6[1:], gp7[1:])


def _prefill(shape, seed):
    v = np.random.default_rng(seed).standard_normal(shape)
    v.reshape(-1)[::3] = -0.0
    return v


def test_skipped_faces_leave_their_vertices_untouched():
    pos, attr, faces, depth, w, skipped = skipped_mesh()
    V = len(pos)
    for fc, drawn in ((faces, [0, 1, 2, 3]), (skipped, [])):
        out, keys = _lib.coords_trimesh_host(pos, attr, fc, (29, 37), depth=depth, w=w, return_keys=True)
        pre = [_prefill((V, 2), 1), _prefill((V, 2), 2), _prefill((V,), 3)]
        got = _lib.coords_trimesh_bwd_host(pos, attr, fc, (29, 37), keys, upstream(keys), depth=depth, w=w, need=(True, True, True),
                                           grad_attr=pre[0].copy(), grad_pos=pre[1].copy(), grad_w=pre[2].copy(), return_most=True)
        rest = sorted(set(range(V)) - set(drawn))
        for a, b in zip(got[:3], pre):
            assert R.same_bits(a[rest], b[rest])
            assert not drawn or (np.isfinite(a[drawn]).all() and not R.same_bits(a[drawn], b[drawn]))
        assert got[3] == (2 if drawn else 0)                             # vertices 1 and 2 lie on both drawn faces


# ---------------------------------------------------------------------------------------------- 4. operand handling
def test_accumulation_into_prefilled_gradients():
    keys = forward("perspective_f64")
    g = upstream(keys)
    ref = reference("perspective_f64", keys, g)
    pre = [_prefill((4, 2), 4), _prefill((4, 2), 5), _prefill((4,), 6)]
    got = backward("perspective_f64", keys, g, grad_attr=pre[0].copy(), grad_pos=pre[1].copy(), grad_w=pre[2].copy())
    check_against_reference("prefilled", got, [p + r for p, r in zip(pre, ref)])


def test_every_null_combination_of_the_outputs():
    keys = forward("perspective_f32")
    g = upstream(keys)
    full = backward("perspective_f32", keys, g)
    for mask in range(1, 8):
        need = (bool(mask & 1), bool(mask & 2), bool(mask & 4))
        got = backward("perspective_f32", keys, g, need=need)
        for k in range(3):
            assert (got[k] is None) if not need[k] else R.same_bits(got[k], full[k]), (mask, k)
    with pytest.raises(ValueError, match="at least one"):
        backward("perspective_f32", keys, g, need=(False, False, False))
    with pytest.raises(ValueError, match="needs w"):
        backward("fan", forward("fan"), upstream(forward("fan")), need=(True, False, True))


def test_a_batch_equals_its_single_calls_and_leaves_the_operands():
    pos, attr, faces, depth = random_mesh()
    rng = np.random.default_rng(5)
    P = np.stack([pos, pos + rng.uniform(-2.0, 2.0, pos.shape), pos[::-1]])
    A = np.stack([attr, attr * 0.5, attr + 1.0]).astype(np.float32)
    Wv = rng.uniform(0.5, 2.0, (3, 12))
    for Fs in (faces, np.stack([faces, faces[::-1], np.roll(faces, 3, axis=0)])):
        per = lambda s: Fs if Fs.ndim == 2 else Fs[s]
        out, K = _lib.coords_trimesh_host(P, A, Fs, (29, 37), w=Wv, return_keys=True)
        G = np.stack([upstream(K[s], seed=s) for s in range(3)])
        arena = (P, A, Wv, Fs, K, G)
        before = [a.copy() for a in arena]
        batch = _lib.coords_trimesh_bwd_host(P, A, Fs, (29, 37), K, G, w=Wv, need=(True, True, True), return_most=True)
        assert batch[0].shape == (3, 12, 2) and batch[1].shape == (3, 12, 2) and batch[2].shape == (3, 12)
        most = 0
        for s in range(3):
            single = _lib.coords_trimesh_bwd_host(P[s], A[s], per(s), (29, 37), K[s], G[s], w=Wv[s], need=(True, True, True), return_most=True)
            assert all(R.same_bits(batch[k][s], single[k]) for k in range(3)), s
            most = max(most, single[3])
        assert batch[3] == most
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(arena, before))          # operands unmodified
    # an operand the batch shares gets one gradient per set
    out, K = _lib.coords_trimesh_host(P, A[0], faces, (29, 37), return_keys=True)
    shared = _lib.coords_trimesh_bwd_host(P, A[0], faces, (29, 37), K, G, need=(True, True, False))
    for s in range(3):
        single = _lib.coords_trimesh_bwd_host(P[s], A[0], faces, (29, 37), K[s], G[s], need=(True, True, False))
        assert R.same_bits(shared[0][s], single[0]) and R.same_bits(shared[1][s], single[1])
    assert shared[0].shape == (3, 12, 2)


# ---------------------------------------------------------------------------------------------- 5. refusals and the size rule
def _ptr(a, off=0):
    return None if a is None else a.ctypes.data + off


def test_every_refused_argument_leaves_the_arena_untouched():
    lib = _lib.lib()
    V, F, oH, oW = 5, 3, 6, 8
    need = lib.lerf_coords_trimesh_bwd_workspace_bytes(F, V, V, 1)
    assert need == 16 + 8 * 15 * F + 4 * (V + 3 * F)
    assert lib.lerf_coords_trimesh_bwd_workspace_bytes(F, V, 9, 2) == 16 + 2 * (8 * 15 * F + 4 * (9 + 3 * F))
    for bad in ((0, V, V, 1), (F, 0, V, 1), (F, V, 0, 1), (F, V, V, 0), (2 ** 24, V, V, 1)):
        assert lib.lerf_coords_trimesh_bwd_workspace_bytes(*bad) == 0
    pos = np.array([[0.5, 0.5], [0.5, 7.0], [5.0, 0.5], [5.0, 7.0], [2.0, 3.0]])
    attr = pos * 2.0
    faces = np.array([[0, 1, 2], [3, 2, 1], [0, 4, 1]], np.int32)
    depth, w = np.ones(V, np.float32), np.ones(V, np.float32)
    out, keys = _lib.coords_trimesh_host(pos, attr, faces, (oH, oW), depth=depth, w=w, return_keys=True)
    gout = np.ones((oH, oW, 2))
    ga, gp, gw = np.full((V, 2), -7.0), np.full((V, 2), -7.0), np.full(V, -7.0)
    ws = np.full(2 * need + 16, 0x55, np.uint8)
    arena = (pos, attr, faces, depth, w, keys, gout)
    before = [a.copy() for a in arena]

    def bwd(P=pos, pdt=F64, V=V, A=attr, adt=F64, Va=V, Fc=faces, AF=None, F=F, D=depth, Wv=w, wdt=F32, oH=oH, oW=oW, i0=0, j0=0, span=0, orient=0,
            K=keys, G=gout, GA=ga, GP=gp, GW=gw, S=ws, sb=None, cap=16, poff=0, koff=0, goff=0, gaoff=0, soff=0, host=True, batch=None):
        sb = lib.lerf_coords_trimesh_bwd_workspace_bytes(F, V, Va, batch[0] if batch else 1) if sb is None else sb
        args = (_ptr(P, poff), pdt, V, _ptr(A), adt, Va, _ptr(Fc), _ptr(AF), F, _ptr(D), _ptr(Wv), wdt, oH, oW, i0, j0, span, orient, _ptr(K, koff),
                _ptr(G, goff), _ptr(GA, gaoff), _ptr(GP), _ptr(GW), _ptr(S, soff), sb, cap)
        name = "lerf_coords_trimesh_bwd" + ("_batched" if batch is not None else "")
        args = args + (batch or ())
        return getattr(lib, name + "_host")(*args) if host else getattr(lib, name)(*args, None)

    assert bwd() == 0 and not (ga == -7.0).all() and not (gp == -7.0).all() and not (gw == -7.0).all()
    ga[:], gp[:], gw[:], ws[:] = -7.0, -7.0, -7.0, 0x55
    two = (2, 0, 0, 0, 0, 0, 0)                                          # two sets that share every mesh operand
    for host in (True, False):                                            # the device entry point refuses before it touches the GPU
        calls = [bwd(P=None, host=host), bwd(A=None, host=host), bwd(Fc=None, host=host), bwd(K=None, host=host), bwd(G=None, host=host),
                 bwd(S=None, host=host), bwd(GA=None, GP=None, GW=None, host=host), bwd(Wv=None, host=host),      # grad_w without w
                 bwd(pdt=0, host=host), bwd(adt=9, host=host), bwd(wdt=9, host=host), bwd(V=0, host=host), bwd(Va=0, host=host), bwd(F=0, host=host),
                 bwd(F=-3, host=host), bwd(oH=0, host=host), bwd(oW=-1, host=host), bwd(span=-1, host=host), bwd(span=65537, host=host),
                 bwd(orient=2, host=host), bwd(orient=-2, host=host), bwd(i0=-1, host=host), bwd(j0=-1, host=host), bwd(i0=2 ** 31 - 3, host=host),
                 bwd(cap=0, host=host), bwd(cap=-1, host=host),
                 bwd(sb=need - 1, host=host), bwd(sb=0, host=host), bwd(soff=4, host=host), bwd(soff=1, host=host),      # short, misaligned
                 bwd(poff=8, host=host), bwd(koff=4, host=host), bwd(goff=8, host=host), bwd(gaoff=8, host=host),
                 bwd(GA=attr, host=host), bwd(GP=pos, host=host), bwd(GA=pos, host=host), bwd(GP=gout, oH=1, oW=5, host=host),      # a gradient IS an input
                 bwd(GW=keys, oH=1, oW=5, host=host), bwd(GA=gp, host=host), bwd(S=gp, sb=80, host=host), bwd(S=keys, host=host),
                 bwd(S=gout, host=host), bwd(S=pos, sb=80, host=host), bwd(S=faces, sb=36, host=host),
                 bwd(batch=two + (48, 96, 0, 10, 5), host=host), bwd(batch=two + (48, 96, 10, 0, 5), host=host),      # a gradient shared between sets
                 bwd(batch=two + (48, 96, 10, 10, 0), host=host), bwd(batch=two + (0, 96, 10, 10, 5), host=host),
                 bwd(batch=two + (48, 95, 10, 10, 5), host=host), bwd(batch=(0,) + (0,) * 11, host=host)]
        assert calls == [EINVAL] * len(calls), (host, calls)
    assert (ga == -7.0).all() and (gp == -7.0).all() and (gw == -7.0).all() and (ws == 0x55).all()
    assert all(np.array_equal(a, b) for a, b in zip(arena, before))
    # through the Python layer
    for kw, match in (({"max_span": -1}, "max_span"), ({"orient": 3}, "orient"), ({"max_adders": 0}, "max_adders"),
                      ({"grad_pos": np.zeros((V, 2), np.float32)}, "grad_pos"), ({"attr_faces": faces[:2]}, "attr_faces")):
        with pytest.raises(ValueError, match=match):
            _lib.coords_trimesh_bwd_host(pos, attr, faces, (oH, oW), keys, gout, **kw)
    with pytest.raises(ValueError, match="keys"):
        _lib.coords_trimesh_bwd_host(pos, attr, faces, (oH, oW), keys.astype(np.int64), gout)
    with pytest.raises(ValueError, match="grad_out"):
        _lib.coords_trimesh_bwd_host(pos, attr, faces, (oH, oW), keys, gout[:-1])


def test_the_size_rule_is_judged_before_the_pointers():
    lib = _lib.lib()

    def rule(F, n_sets, oH, oW, span, host=True):
        args = (None, F64, 3, None, F64, 3, None, None, F, None, None, F32, oH, oW, 0, 0, span, 0, None, None, None, None, None, None, 0, 16)
        if n_sets > 1:
            args, name = args + (n_sets,) + (0,) * 11, "lerf_coords_trimesh_bwd_batched"
        else:
            name = "lerf_coords_trimesh_bwd"
        return getattr(lib, name + "_host")(*args) if host else getattr(lib, name)(*args, None)

    most = (2 ** 32 - 1) // (540 * 240)                                  # the forward's rule at 2160 x 3840
    for host in (True, False):
        assert rule(most, 1, 2160, 3840, 0, host) == EINVAL                # within the rule: the null pointers are what is refused
        assert rule(most + 1, 1, 2160, 3840, 0, host) == EUNSUPPORTED
        assert rule(most // 2 + 1, 2, 2160, 3840, 0, host) == EUNSUPPORTED
        assert rule(2 ** 24 - 1, 1, 4, 16, 0, host) == EINVAL               # one workgroup a face
        assert rule(2 ** 24, 1, 4, 16, 0, host) == EUNSUPPORTED
    with pytest.raises(_lib.LerfError, match="size rule"):
        _lib.coords_trimesh_bwd_host(np.zeros((3, 2)), np.zeros((3, 2)), np.zeros((most + 1, 3), np.int32), (2160, 3840),
                                     np.zeros((2160, 3840), np.uint64), None)
