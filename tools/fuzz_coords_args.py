#!/usr/bin/env python3
"""Differential fuzz of the ARGUMENT CHECKS of the coordinate-map entry points (csrc/lerf_coords.hip): what a call returns, and what
it writes, for argument tuples on and around every line the contract draws (include/lerf_hip.h, "a refused call launches and
writes nothing").  Run it once per build of the library, in a process of its own, with the same seed; the two outputs must be equal
byte for byte:

    fuzz_coords_args.py --lib A/liblerf_hip.so --out a.jsonl && fuzz_coords_args.py --lib B/liblerf_hip.so --out b.jsonl && cmp a.jsonl b.jsonl

For every host twin that takes maps (build, mesh, compose, invert, invert_raster, compose_bwd, invert_bwd, build_bwd, reproject,
reproject_bwd, trimesh, trimesh_bwd, splat, splat_bwd, the batched forms and the _ordered forms of the three scatters) it draws a VALID
call on tiny shapes (h, w <= 6, V, Va <= 6, F <= 4, C <= 2) and replaces zero to two of its arguments by a value the contract tells
apart: dtype codes in and out of range, dimensions and counts -1 .. 6, row strides odd / short / exact / padded / negative, set strides
-span / 0 / odd / span - 2 / span / padded, n_sets -1 .. 3 and 65536, null and misaligned pointers, a pointer moved onto another
operand's bytes, the scalar limits (max_span, max_adders, with_norm, ...).  Workspace sizes are the library's own *_workspace_bytes.
All operands live in ONE arena (page-aligned, so alignment is the same in every process), each in a slot of its own, the first and the
last a margin away from the arena's ends: what a broken check lets through still lands inside.  The arena is reset before every call,
then the planes an accepted call needs are prepared (parameter blocks, face indices, keys that name faces); one record per case goes
to --out: entry point, arguments (pointers as arena offsets), return code, digest of the arena afterwards.

Every pointer carries its operand's name and whether the call WRITES it, marked from the text of include/lerf_hip.h: what
tests/test_coords_overlap_cpu.py moves onto what (full_call: one valid call with every optional operand present).

The device-only entry points (mesh_bwd, mesh_bwd_batched, build_dev, build_bwd, and the device forms of reproject and reproject_bwd) get the same cases with HOST pointers, which a
refused call never reads; they run only where there is no device (lerf_device_count() <= 0), where a call that passes the checks
fails at its launch and touches nothing either.

The summary (stdout) counts the return codes per entry point and says whether the generator is balanced: every entry point at least
a quarter accepted (the device-only group excepted) and a quarter refused, every batched one each of 0, -1, -2.

tests/test_coords_batch_cpu.py draws from the same generator (single_and_batched)."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

F32, F64 = 1, 2
# bytes: the arena's two margins, one operand's slot (3 padded sets of a 6 x 6 float64 map: 2352; the ordered workspace of 3 sets of
# 36 entries and 36 targets: 2176; the mesh adjoint's of 3 sets of 6 faces: 2464); SLOTS: the mesh adjoint has twelve pointer operands
MARGIN, SLOT, SLOTS = 8192, 4096, 12
N_PARAMS = {0: 9, 1: 8, 2: 21, 16: 17, 17: 13}
REPROJECT_PARAMS = 12
CHAINED = ("mesh", "compose", "invert", "invert_raster", "compose_bwd", "invert_bwd")
N_SET_STRIDES = {"mesh": 2, "compose": 3, "invert": 3, "invert_raster": 4, "compose_bwd": 5, "invert_bwd": 4}


class Arena:
    """one page-aligned buffer for every operand of a call; float32 values in [0.5, 5), which are finite float64 read in pairs"""

    def __init__(self, slots=SLOTS):
        size = 2 * MARGIN + slots * SLOT
        raw = np.zeros(size + 4096, np.uint8)
        skip = -raw.ctypes.data % 4096
        self.buf = raw[skip:skip + size]
        self.base = self.buf.ctypes.data
        self.fresh = np.random.default_rng(7).uniform(0.5, 5.0, size // 4).astype(np.float32).view(np.uint8)
        self.reset()

    def reset(self):
        np.copyto(self.buf, self.fresh)

    def digest(self):
        return hashlib.blake2b(self.buf, digest_size=8).hexdigest()

    def put(self, off, values):
        """a prepared plane at offset `off` (a parameter block, indices, keys): what an accepted call needs to find there"""
        self.buf[off:off + values.nbytes] = values.view(np.uint8)


class Arg:
    def __init__(self, kind, v, **meta):
        self.kind, self.v, self.meta = kind, v, meta


class Call:
    """a valid call under construction: the arguments in the C order, each with the kind its mutations are drawn by"""

    def __init__(self, rng, batched, full=False):
        """full: the call of tests/test_coords_overlap_cpu.py -- every optional operand present, nothing shared or in place, n_sets = 2
        for a batch and 1 otherwise (also where the entry point always takes n_sets)"""
        self.rng, self.batched, self.full, self.args, self.slots, self.span, self.tail, self.planes, self.given = rng, batched, full, [], 0, {}, [], [], {}
        self.n = (2 if full else int(rng.integers(1, 4))) if batched else 1

    def own_n(self):
        """n_sets of an entry point that always takes it"""
        self.n = (2 if self.batched else 1) if self.full else int(self.rng.integers(1, 4))
        self.add("nsets", self.n)

    def add(self, kind, v, **meta):
        self.args.append(Arg(kind, v, **meta))

    def coin(self, p=0.5):
        return bool(self.rng.random() < p)

    def rare(self, p):
        """a coin for what the full call leaves out: a null optional operand, a shared one, the in-place form"""
        return self.coin(p) and not self.full

    def ptr(self, name, null=False, same_as=None, writes=False):
        """writes: the header says the call writes through this pointer (an output, a gradient, keys, a workspace)"""
        off = MARGIN + self.slots * SLOT
        self.slots += 1
        null = null and not self.full
        self.given[name] = not null
        self.add("ptr", None if null else off if same_as is None else same_as, name=name, writes=writes)
        return off

    def ws(self, need):
        """workspace, workspace_bytes"""
        self.ptr("ws", writes=True)
        self.add("ws_bytes", need, need=need)

    def params(self, off, n_params):
        """a usable parameter block at `off`, for three sets: near-identity numbers, so that every model stays finite"""
        self.planes.append((off, np.tile(np.linspace(0.9, 1.1, n_params), 3)))

    def indices(self, off, count, below):
        """an index plane at `off` (every set, the padding between sets included): `count` int32 below `below`"""
        self.planes.append((off, ((np.arange(count, dtype=np.int64) * 7 + 1) % below).astype(np.int32)))

    def dims(self, *hw):
        for d in hw:
            self.add("dim", d)

    def map(self, name, h, w, with_dims=False, null=False, like=None, writes=False):
        """pointer, dtype, row stride [, h, w] of a strided map; like = (offset, dtype, stride): the same operand once more (in place)"""
        dt, rs = (like[1], like[2]) if like else (int(self.rng.choice([F32, F64])), 2 * w + 4 * int(self.coin()))
        off = self.ptr(name, null, like[0] if like else None, writes)
        self.add("dtype", dt)
        self.add("rstride", rs, w=w)
        if with_dims:
            self.dims(h, w)
        self.span[name] = (h - 1) * rs + 2 * w
        return off, dt, rs

    def dense(self, name, h, w, null=False, writes=False):
        off = self.ptr(name, null, writes=writes)
        self.span[name] = 2 * h * w
        return off

    def plane(self, name, h, w, null=False, writes=False):
        off = self.ptr(name, null, writes=writes)
        self.span[name] = h * w
        return off

    def sets(self, *names, share=(), same=None):
        """n_sets and one set stride per operand, behind everything else; same = (name, of): the set stride of `of` once more"""
        if not self.batched:
            return
        self.add("nsets", self.n)
        drawn = {}
        for name in names:
            s = self.span[name]
            v = 0 if name in share and self.rare(0.3) else s + 6 * int(self.coin())
            if same and name == same[0]:
                v = drawn[same[1]]
            drawn[name] = v
            self.add("sstride", v, span=s)


_LIBRARY = None


def library():
    """the library under test: the workspace sizes are its own"""
    global _LIBRARY
    if _LIBRARY is None:
        from lerf_pytorch_amd import _lib
        _LIBRARY = _lib.lib()
    return _LIBRARY


def _hw(rng, lo=1):
    return int(rng.integers(lo, 7)), int(rng.integers(lo, 7))


def _tile(c, oH, oW):
    i0, j0 = (3, 7) if c.coin() else (0, 0)
    c.dims(oH, oW)
    c.add("origin", i0)
    c.add("origin", j0)
    return i0, j0


def mesh(c):
    (gh, gw), (oH, oW) = _hw(c.rng, 2), _hw(c.rng)
    c.ptr("ctrl")
    c.add("dtype", int(c.rng.choice([F32, F64])))
    c.dims(gh, gw)
    c.span["ctrl"] = 2 * gh * gw
    c.add("interp", int(c.coin()))
    i0, j0 = (3, 7) if c.coin() else (0, 0)
    c.add("full", i0 + oH + 2, need=i0 + oH)
    c.add("full", j0 + oW + 2, need=j0 + oW)
    c.map("out", oH, oW, writes=True)
    c.dims(oH, oW)
    c.add("origin", i0)
    c.add("origin", j0)
    c.sets("ctrl", "out")


def compose(c):
    (aH, aW), (oH, oW) = _hw(c.rng), _hw(c.rng)
    c.map("a", aH, aW, True)
    b = c.map("b", oH, oW)
    in_place = c.rare(0.2)
    c.map("out", oH, oW, like=b if in_place else None, writes=True)
    c.dims(oH, oW)
    c.sets("a", "b", "out", share=("a",), same=("out", "b") if in_place else None)


def invert(c):
    (fH, fW), (oH, oW) = _hw(c.rng, 2), _hw(c.rng)
    c.map("f", fH, fW, True)
    c.map("init", oH, oW, null=c.coin(0.4))
    c.map("out", oH, oW, writes=True)
    _tile(c, oH, oW)
    c.add("max_iter", int(c.rng.choice([1, 3, 16])))
    c.add("tol", float(c.rng.choice([0.0, 1e-9])))
    c.sets("f", "init", "out", share=("f", "init"))


def invert_raster(c):
    (fH, fW), (oH, oW) = _hw(c.rng, 2), _hw(c.rng)
    c.map("f", fH, fW, True)
    c.plane("depth", fH, fW, null=c.coin(0.4))
    c.map("out", oH, oW, writes=True)
    _tile(c, oH, oW)
    c.add("max_span", int(c.rng.choice([1, 16, 64])))
    c.add("orient", int(c.rng.integers(-1, 2)))
    c.plane("keys", oH, oW, writes=True)
    c.sets("f", "depth", "out", "keys", share=("f", "depth"))


def _ordered_tail(c, n_entries, n_targets):
    """what an _ordered entry point takes behind its sibling's arguments: workspace, workspace_bytes, max_adders"""
    c.ws(int(library().lerf_scatter_ordered_workspace_bytes(n_entries, n_targets, c.n)))
    c.add("max_adders", int(c.rng.choice([1, 4, 64])))


def compose_bwd(c, ordered=False):
    (aH, aW), (oH, oW) = _hw(c.rng, 2), _hw(c.rng)
    c.map("a", aH, aW, True)
    c.map("b", oH, oW)
    c.dense("gout", oH, oW)
    c.dims(oH, oW)
    skip = int(c.rng.integers(0, 4))                    # 0, 3: both gradients; 1: no grad_a; 2: no grad_b
    c.dense("ga", aH, aW, null=skip == 1, writes=True)
    c.dense("gb", oH, oW, null=skip == 2, writes=True)
    if c.batched:
        # one grad_a for all sets goes with one outer map for all sets (the ordered form: never, a target has one owner)
        c.add("nsets", c.n)
        shared = c.rare(0.3) and not ordered
        for name in ("a", "b", "gout", "ga", "gb"):
            s = c.span[name]
            c.add("sstride", 0 if shared and name in ("a", "ga") else s + 6 * int(c.coin()), span=s)
    if ordered:
        _ordered_tail(c, oH * oW, aH * aW)


def invert_bwd(c, ordered=False):
    (fH, fW), (oH, oW) = _hw(c.rng, 2), _hw(c.rng)
    c.map("f", fH, fW, True)
    c.map("g", oH, oW)
    c.dense("gout", oH, oW)
    c.dims(oH, oW)
    c.dense("gf", fH, fW, writes=True)
    c.sets("f", "g", "gout", "gf", share=("f",))
    if ordered:
        _ordered_tail(c, oH * oW, fH * fW)


def _mesh_head(c):
    """pos .. w_dtype of the triangle mesh and its adjoint -> (V, Va, F); faces and attr_faces hold indices inside the mesh"""
    V, Va, F = int(c.rng.integers(1, 7)), int(c.rng.integers(1, 7)), int(c.rng.integers(1, 5))
    for name, n in (("pos", V), ("attr", Va)):
        c.ptr(name)
        c.add("dtype", int(c.rng.choice([F32, F64])))
        c.add("count", n)
        c.span[name] = 2 * n
    c.indices(c.plane("faces", F, 3), 3 * (3 * F + 6), V)
    c.indices(c.plane("afaces", F, 3, null=c.coin(0.4)), 3 * (3 * F + 6), Va)
    c.add("count", F)
    c.plane("depth", V, 1, null=c.coin(0.3))
    c.plane("w", V, 1, null=c.coin(0.4))
    c.add("dtype", int(c.rng.choice([F32, F64])))
    return V, Va, F


MESH_SETS = ("pos", "attr", "faces", "afaces", "depth", "w")


def trimesh(c):
    V, Va, F = _mesh_head(c)
    oH, oW = _hw(c.rng)
    c.map("out", oH, oW, writes=True)
    _tile(c, oH, oW)
    c.add("tri_span", int(c.rng.choice([0, 16, 65536])))
    c.add("orient", int(c.rng.integers(-1, 2)))
    c.plane("keys", oH, oW, writes=True)
    c.plane("dout", oH, oW, null=c.coin(0.4) or not c.given["depth"], writes=True)          # depth_out goes with depth
    c.ws(int(library().lerf_coords_trimesh_workspace_bytes(F, c.n)))
    c.sets(*MESH_SETS, "out", "keys", "dout", share=MESH_SETS)


def trimesh_bwd(c):
    V, Va, F = _mesh_head(c)
    oH, oW = _hw(c.rng)
    _tile(c, oH, oW)
    c.add("tri_span", int(c.rng.choice([0, 16, 65536])))
    c.add("orient", int(c.rng.integers(-1, 2)))
    keys = c.plane("keys", oH, oW)
    k = np.arange(3 * (oH * oW + 6), dtype=np.uint64) % np.uint64(F + 1)                    # the faces in turn, then a hole
    c.planes.append((keys, np.where(k == F, np.uint64(0xffffffffffffffff), k)))
    c.dense("gout", oH, oW)
    skip = int(c.rng.integers(0, 4))                    # 1, 2: one gradient left out; grad_w goes with w
    c.dense("gattr", Va, 1, null=skip == 1, writes=True)
    c.dense("gpos", V, 1, null=skip == 2, writes=True)
    c.plane("gw", V, 1, null=c.coin(0.3) or not c.given["w"], writes=True)
    c.ws(int(library().lerf_coords_trimesh_bwd_workspace_bytes(F, V, Va, c.n)))
    c.add("max_adders", int(c.rng.choice([1, 4, 64])))
    c.sets(*MESH_SETS, "keys", "gout", "gattr", "gpos", "gw", share=MESH_SETS)


def _splat_head(c):
    """x .. m_set_stride of the splat and its adjoint -> (C, H, W, oH, oW); every form takes n_sets, as its last argument"""
    c.n = (2 if c.batched else 1) if c.full else int(c.rng.integers(1, 4))
    C, (H, W), (oH, oW) = int(c.rng.integers(1, 3)), _hw(c.rng), _hw(c.rng)
    c.ptr("x")
    c.add("dtype", int(c.rng.choice([F32, F64])))
    c.add("planes", C)
    c.dims(H, W)
    c.add("sstride", C * H * W + 6 * int(c.coin()), span=C * H * W)
    rs = 2 * W + 4 * int(c.coin())
    c.ptr("f")
    c.add("dtype", int(c.rng.choice([F32, F64])))
    c.add("rstride", rs, w=W)
    span = (H - 1) * rs + 2 * W
    c.add("sstride", 0 if c.rare(0.3) else span + 6 * int(c.coin()), span=span)
    c.ptr("m", null=c.coin(0.4))
    c.add("sstride", H * W + 6 * int(c.coin()), span=H * W)
    return C, H, W, oH, oW


def splat(c, ordered=False):
    C, H, W, oH, oW = _splat_head(c)
    c.ptr("acc", writes=True)
    norm = int(c.coin())
    c.add("with_norm", norm)
    c.dims(oH, oW)
    c.add("sstride", (C + norm) * oH * oW + 6 * int(c.coin()), span=(C + norm) * oH * oW)
    c.add("nsets", c.n)
    if ordered:
        _ordered_tail(c, H * W, oH * oW)


def splat_bwd(c):
    C, H, W, oH, oW = _splat_head(c)
    c.ptr("g")
    norm = int(c.coin())
    c.add("with_norm", norm)
    c.dims(oH, oW)
    c.add("sstride", (C + norm) * oH * oW + 6 * int(c.coin()), span=(C + norm) * oH * oW)
    skip = int(c.rng.integers(0, 5))                    # 1, 2, 3: one gradient left out
    for k, (name, span) in enumerate((("gx", C * H * W), ("gm", H * W), ("gf", 2 * H * W))):
        c.ptr(name, null=skip == k + 1, writes=True)
        c.add("sstride", span + 6 * int(c.coin()), span=span)
    c.add("nsets", c.n)


def _model(c):
    model = int(c.rng.choice(list(N_PARAMS)))
    c.add("model", model)
    c.params(c.ptr("params"), N_PARAMS[model])
    return model


def build(c):
    model = _model(c)
    c.add("n_params", N_PARAMS[model])
    oH, oW = _hw(c.rng)
    c.map("out", oH, oW, writes=True)
    _tile(c, oH, oW)


def build_dev(c):
    model = _model(c)
    c.own_n()
    c.add("n_params", N_PARAMS[model])
    oH, oW = _hw(c.rng)
    c.ptr("out", writes=True)
    c.add("dtype", int(c.rng.choice([F32, F64])))
    rs = 2 * oW + 4 * int(c.coin())
    span = (oH - 1) * rs + 2 * oW
    c.add("sstride", span + 6 * int(c.coin()), span=span)
    c.add("rstride", rs, w=oW)
    _tile(c, oH, oW)
    c.tail = [None]


def build_bwd(c, device=False):
    model = _model(c)
    c.own_n()
    c.add("n_params", N_PARAMS[model])
    oH, oW = _hw(c.rng)
    c.ptr("gmap")
    _tile(c, oH, oW)
    c.ptr("gparams", writes=True)
    if device:
        c.ws(c.n * N_PARAMS[model] * 8)                 # one block of 64 x 64 covers a tile of 6 x 6
        c.tail = [None]


def mesh_bwd(c):
    (oH, oW), (gh, gw) = _hw(c.rng), _hw(c.rng, 2)
    c.dense("g", oH, oW)
    c.dims(oH, oW)
    c.add("interp", int(c.coin()))
    c.dims(gh, gw)
    c.dense("gc", gh, gw, writes=True)
    c.ws(c.n * gh * oW * 16)
    c.sets("g", "gc")
    c.tail = [None]


def _reproject_head(c):
    """kind, params, n_sets, depth, its dtype and set stride (0: one plane for every set) -> (oH, oW)"""
    c.add("depth_kind", int(c.coin()))
    c.params(c.ptr("params"), REPROJECT_PARAMS)
    c.own_n()
    oH, oW = _hw(c.rng)
    c.ptr("depth")
    c.add("dtype", int(c.rng.choice([F32, F64])))
    c.add("sstride", 0 if c.rare(0.3) else oH * oW + 6 * int(c.coin()), span=oH * oW)
    return oH, oW


def reproject(c, device=False):
    oH, oW = _reproject_head(c)
    c.ptr("out", writes=True)
    c.add("dtype", int(c.rng.choice([F32, F64])))
    rs = 2 * oW + 4 * int(c.coin())
    span = (oH - 1) * rs + 2 * oW
    c.add("sstride", span + 6 * int(c.coin()), span=span)
    c.add("rstride", rs, w=oW)
    c.ptr("zo", null=c.coin(0.3), writes=True)          # depth_out
    c.add("sstride", oH * oW + 6 * int(c.coin()), span=oH * oW)
    _tile(c, oH, oW)
    if device:
        c.tail = [None]


def reproject_bwd(c, device=False):
    oH, oW = _reproject_head(c)
    c.ptr("gmap")
    c.ptr("gzo", null=c.coin(0.3))                      # grad_depth_out
    _tile(c, oH, oW)
    skip = int(c.rng.integers(0, 4))                    # 0, 3: both gradients; 1: no grad_depth; 2: no grad_params
    c.ptr("gdepth", null=skip == 1, writes=True)
    c.ptr("gparams", null=skip == 2, writes=True)
    if device:
        c.ws(c.n * REPROJECT_PARAMS * 8)                # one block of 64 x 64 covers a tile of 6 x 6
        c.tail = [None]


# entry point -> (the call's builder, batched)
HOST = {"lerf_coords_build_host": (build, False), "lerf_coords_build_bwd_host": (build_bwd, False),
        "lerf_coords_reproject_host": (reproject, False), "lerf_coords_reproject_bwd_host": (reproject_bwd, False)}
for _op in CHAINED + ("trimesh", "trimesh_bwd"):
    HOST["lerf_coords_%s_host" % _op] = (globals()[_op], False)
    HOST["lerf_coords_%s_batched_host" % _op] = (globals()[_op], True)
for _op in (compose_bwd, invert_bwd):
    HOST["lerf_coords_%s_ordered_host" % _op.__name__] = (lambda c, op=_op: op(c, True), False)
    HOST["lerf_coords_%s_batched_ordered_host" % _op.__name__] = (lambda c, op=_op: op(c, True), True)
HOST.update({"lerf_splat_host": (splat, False), "lerf_splat_bwd_host": (splat_bwd, False),
             "lerf_splat_ordered_host": (lambda c: splat(c, True), False)})
# the entry points that always take n_sets: the generator draws it whatever `batched` says, and a full call follows `batched`
OWN_NSETS = ("lerf_coords_build_bwd_host", "lerf_coords_reproject_host", "lerf_coords_reproject_bwd_host", "lerf_splat_host",
             "lerf_splat_bwd_host", "lerf_splat_ordered_host")
DEVICE_ONLY = {"lerf_coords_mesh_bwd": (mesh_bwd, False), "lerf_coords_mesh_bwd_batched": (mesh_bwd, True),
               "lerf_coords_build_dev": (build_dev, False), "lerf_coords_build_bwd": (lambda c: build_bwd(c, True), False),
               "lerf_coords_reproject": (lambda c: reproject(c, True), False), "lerf_coords_reproject_bwd": (lambda c: reproject_bwd(c, True), False)}


def _values(arg, call, i):
    """the values the contract tells apart for argument i of the call"""
    k, m = arg.kind, arg.meta
    if k == "ptr":
        out = [None]
        if arg.v is not None:
            out += [arg.v + 1, arg.v + 4, arg.v + 8]
        others = [a.v for n, a in enumerate(call.args) if a.kind == "ptr" and n != i and a.v is not None]
        return out + [o + d for o in others for d in (-720, -64, -16, 0, 16, 48, 208, 720)]
    if k == "dtype":
        return [-1, 0, F32, F64, 3, 4]
    if k == "dim":
        return [-1, 0, 1, 2, 3, 4, 5, 6]
    if k == "rstride":
        w = m["w"]
        return [2 * w + 1, 2 * w - 2, 2 * w, 2 * w + 4, -2 * w]
    if k == "sstride":
        s = m["span"]
        return [-s, 0, s + 1, s - 2, s, s + 6]
    if k == "nsets":
        return [-1, 0, 1, 2, 3, 65536]
    if k in ("full", "ws_bytes"):
        return [max(m["need"] - 8, 0) if k == "ws_bytes" else m["need"] - 1, 0, m["need"], m["need"] + 64]
    return {"max_iter": [0, 1, 64, 65], "tol": [-1.0, float("nan"), float("inf"), 0.0, 1e-9], "max_span": [0, 1, 64, 65],
            "orient": [-2, -1, 0, 1, 2], "interp": [-1, 0, 1, 2], "depth_kind": [-1, 0, 1, 2], "origin": [-1, 0, 3, 7], "model": [-1, 0, 1, 2, 3, 16, 17, 18],
            "n_params": [-1, 0, 8, 9, 10, 13, 17, 21], "count": [-1, 0, 1, 2, 4, 6], "planes": [-1, 0, 1, 2], "with_norm": [-1, 0, 1, 2],
            "max_adders": [-1, 0, 1, 4], "tri_span": [-1, 0, 1, 16, 65536, 65537]}[k]


def draw(builder, batched, rng):
    """one case: a valid call with zero to two arguments replaced.  Returns (arguments: ("p", offset or None) for a pointer, the plain
    value otherwise; the tail the device forms take (a null stream); the planes to prepare in the arena, (offset, values) each)"""
    c = Call(rng, batched)
    builder(c)
    n_mut = int(rng.choice([0, 1, 2], p=[0.2, 0.45, 0.35]))
    for i in rng.choice(len(c.args), n_mut, replace=False):
        vals = _values(c.args[i], c, int(i))
        c.args[i].v = vals[int(rng.integers(len(vals)))]
    args = [("p", a.v) if a.kind == "ptr" else a.v for a in c.args]
    return args, c.tail, c.planes


def full_call(builder, batched):
    """the valid call tests/test_coords_overlap_cpu.py moves pointers in: every optional operand present, n_sets = 2 for `batched`"""
    c = Call(np.random.default_rng(0), batched, full=True)
    builder(c)
    return c


def run_case(fn, arena, args, tail=(), planes=()):
    """reset the arena, prepare the planes, make the call, return (return code, digest of the arena afterwards)"""
    arena.reset()
    for off, values in planes:
        arena.put(off, values)
    real = [(None if a[1] is None else arena.base + a[1]) if isinstance(a, tuple) else a for a in args]
    rc = fn(*real, *tail)
    return rc, arena.digest()


def single_and_batched(op, n_cases, seed):
    """for the chained operation `op`: n_cases argument lists of the single-map host twin, and the same call as the batched twin takes
    it (n_sets = 1, every set stride 0)"""
    rng = np.random.default_rng([seed, CHAINED.index(op)])
    for _ in range(n_cases):
        args, _, _ = draw(globals()[op], False, rng)
        yield args, args + [1] + [0] * N_SET_STRIDES[op]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", help="another build of liblerf_hip.so (default: the product library)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cases", type=int, default=10000, help="per entry point")
    ap.add_argument("--out", required=True, help="one JSON record per case")
    a = ap.parse_args()
    from lerf_pytorch_amd import _lib
    if a.lib:
        _lib.use_library(a.lib)
    L = _lib.lib()
    entries = dict(HOST)
    if L.lerf_device_count() <= 0:                      # 0, or LERF_ENODEVICE where there is no driver either
        entries.update(DEVICE_ONLY)
    else:
        print("a device is present: the device-only entry points are left out")
    arena = Arena()
    balanced = True
    with open(a.out, "w") as out:
        for k, (name, (builder, batched)) in enumerate(sorted(entries.items())):
            rng = np.random.default_rng([a.seed, k])
            fn, counts = getattr(L, name), {}
            for _ in range(a.cases):
                args, tail, planes = draw(builder, batched, rng)
                rc, digest = run_case(fn, arena, args, tail, planes)
                counts[rc] = counts.get(rc, 0) + 1
                out.write(json.dumps({"e": name, "a": args, "rc": rc, "d": digest}) + "\n")
            ok = counts.get(-1, 0) + counts.get(-2, 0) >= a.cases / 4
            if name in HOST:
                ok = ok and counts.get(0, 0) >= a.cases / 4 and (not batched or all(counts.get(c, 0) > 0 for c in (0, -1, -2)))
            balanced = balanced and ok
            print("%-42s %s%s" % (name, "  ".join("%d: %d" % (c, counts[c]) for c in sorted(counts, reverse=True)), "" if ok else "   UNBALANCED"))
    print("generator balanced" if balanced else "generator NOT balanced: do not trust this run")
    return 0 if balanced else 1


if __name__ == "__main__":
    sys.exit(main())
