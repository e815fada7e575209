#!/usr/bin/env python3
"""Differential fuzz of the ARGUMENT CHECKS of the coordinate-map entry points (csrc/lerf_coords.hip): what a call returns, and what
it writes, for argument tuples on and around every line the contract draws (include/lerf_hip.h, "a refused call launches and
writes nothing").  Run it once per build of the library, in a process of its own, with the same seed; the two outputs must be equal
byte for byte:

    fuzz_coords_args.py --lib A/liblerf_hip.so --out a.jsonl && fuzz_coords_args.py --lib B/liblerf_hip.so --out b.jsonl && cmp a.jsonl b.jsonl

For every host twin that takes maps (build, mesh, compose, invert, invert_raster, compose_bwd, invert_bwd, build_bwd, reproject,
reproject_bwd and the six batched forms) it draws a VALID call on tiny shapes (h, w <= 6) and replaces zero to two of its arguments by a value the contract tells
apart: dtype codes in and out of range, dimensions -1 .. 6, row strides odd / short / exact / padded / negative, set strides
-span / 0 / odd / span - 2 / span / padded, n_sets -1 .. 3 and 65536, null and misaligned pointers, a pointer moved onto another
operand's bytes, the scalar limits.  All operands live in ONE arena (page-aligned, so alignment is the same in every process), each
in a slot of its own, the first and the last a margin away from the arena's ends: what a broken check lets through still lands inside.
The arena is reset before every call; one record per case goes to --out: entry point, arguments (pointers as arena offsets), return
code, digest of the arena afterwards.

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
MARGIN, SLOT = 8192, 4096               # bytes: the arena's two margins, one operand's slot (3 padded sets of a 6 x 6 float64 map: 2304)
N_PARAMS = {0: 9, 1: 8, 2: 21, 16: 17, 17: 13}
REPROJECT_PARAMS = 12
CHAINED = ("mesh", "compose", "invert", "invert_raster", "compose_bwd", "invert_bwd")
N_SET_STRIDES = {"mesh": 2, "compose": 3, "invert": 3, "invert_raster": 4, "compose_bwd": 5, "invert_bwd": 4}


class Arena:
    """one page-aligned buffer for every operand of a call; float32 values in [0.5, 5), which are finite float64 read in pairs"""

    def __init__(self, slots=8):
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

    def set_params(self, off, n_params, n_sets):
        """a usable parameter block at offset `off`: near-identity numbers, so that every model stays finite"""
        p = np.tile(np.linspace(0.9, 1.1, n_params), n_sets)
        self.buf[off:off + p.nbytes] = p.view(np.uint8)


class Arg:
    def __init__(self, kind, v, **meta):
        self.kind, self.v, self.meta = kind, v, meta


class Call:
    """a valid call under construction: the arguments in the C order, each with the kind its mutations are drawn by"""

    def __init__(self, rng, batched):
        self.rng, self.batched, self.args, self.slots, self.span, self.tail = rng, batched, [], 0, {}, []
        self.n = int(rng.integers(1, 4)) if batched else 1

    def add(self, kind, v, **meta):
        self.args.append(Arg(kind, v, **meta))

    def coin(self, p=0.5):
        return bool(self.rng.random() < p)

    def ptr(self, null=False, same_as=None):
        off = MARGIN + self.slots * SLOT
        self.slots += 1
        self.add("ptr", None if null else off if same_as is None else same_as)
        return off

    def dims(self, *hw):
        for d in hw:
            self.add("dim", d)

    def map(self, name, h, w, with_dims=False, null=False, like=None):
        """pointer, dtype, row stride [, h, w] of a strided map; like = (offset, dtype, stride): the same operand once more (in place)"""
        dt, rs = (like[1], like[2]) if like else (int(self.rng.choice([F32, F64])), 2 * w + 4 * int(self.coin()))
        off = self.ptr(null, like[0] if like else None)
        self.add("dtype", dt)
        self.add("rstride", rs, w=w)
        if with_dims:
            self.dims(h, w)
        self.span[name] = (h - 1) * rs + 2 * w
        return off, dt, rs

    def dense(self, name, h, w, null=False):
        self.ptr(null)
        self.span[name] = 2 * h * w

    def plane(self, name, h, w, null=False):
        self.ptr(null)
        self.span[name] = h * w

    def sets(self, *names, share=(), same=None):
        """n_sets and one set stride per operand, behind everything else; same = (name, of): the set stride of `of` once more"""
        if not self.batched:
            return
        self.add("nsets", self.n)
        drawn = {}
        for name in names:
            s = self.span[name]
            v = 0 if name in share and self.coin(0.3) else s + 6 * int(self.coin())
            if same and name == same[0]:
                v = drawn[same[1]]
            drawn[name] = v
            self.add("sstride", v, span=s)


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
    c.ptr()
    c.add("dtype", int(c.rng.choice([F32, F64])))
    c.dims(gh, gw)
    c.span["ctrl"] = 2 * gh * gw
    c.add("interp", int(c.coin()))
    i0, j0 = (3, 7) if c.coin() else (0, 0)
    c.add("full", i0 + oH + 2, need=i0 + oH)
    c.add("full", j0 + oW + 2, need=j0 + oW)
    c.map("out", oH, oW)
    c.dims(oH, oW)
    c.add("origin", i0)
    c.add("origin", j0)
    c.sets("ctrl", "out")


def compose(c):
    (aH, aW), (oH, oW) = _hw(c.rng), _hw(c.rng)
    c.map("a", aH, aW, True)
    b = c.map("b", oH, oW)
    in_place = c.coin(0.2)
    c.map("out", oH, oW, like=b if in_place else None)
    c.dims(oH, oW)
    c.sets("a", "b", "out", share=("a",), same=("out", "b") if in_place else None)


def invert(c):
    (fH, fW), (oH, oW) = _hw(c.rng, 2), _hw(c.rng)
    c.map("f", fH, fW, True)
    c.map("init", oH, oW, null=c.coin(0.4))
    c.map("out", oH, oW)
    _tile(c, oH, oW)
    c.add("max_iter", int(c.rng.choice([1, 3, 16])))
    c.add("tol", float(c.rng.choice([0.0, 1e-9])))
    c.sets("f", "init", "out", share=("f", "init"))


def invert_raster(c):
    (fH, fW), (oH, oW) = _hw(c.rng, 2), _hw(c.rng)
    c.map("f", fH, fW, True)
    c.plane("depth", fH, fW, null=c.coin(0.4))
    c.map("out", oH, oW)
    _tile(c, oH, oW)
    c.add("max_span", int(c.rng.choice([1, 16, 64])))
    c.add("orient", int(c.rng.integers(-1, 2)))
    c.plane("keys", oH, oW)
    c.sets("f", "depth", "out", "keys", share=("f", "depth"))


def compose_bwd(c):
    (aH, aW), (oH, oW) = _hw(c.rng, 2), _hw(c.rng)
    c.map("a", aH, aW, True)
    c.map("b", oH, oW)
    c.dense("gout", oH, oW)
    c.dims(oH, oW)
    skip = int(c.rng.integers(0, 4))                    # 0, 3: both gradients; 1: no grad_a; 2: no grad_b
    c.dense("ga", aH, aW, null=skip == 1)
    c.dense("gb", oH, oW, null=skip == 2)
    if not c.batched:
        return
    # one grad_a for all sets goes with one outer map for all sets
    c.add("nsets", c.n)
    shared = c.coin(0.3)
    for name in ("a", "b", "gout", "ga", "gb"):
        s = c.span[name]
        c.add("sstride", 0 if shared and name in ("a", "ga") else s + 6 * int(c.coin()), span=s)


def invert_bwd(c):
    (fH, fW), (oH, oW) = _hw(c.rng, 2), _hw(c.rng)
    c.map("f", fH, fW, True)
    c.map("g", oH, oW)
    c.dense("gout", oH, oW)
    c.dims(oH, oW)
    c.dense("gf", fH, fW)
    c.sets("f", "g", "gout", "gf", share=("f",))


def _model(c):
    model = int(c.rng.choice(list(N_PARAMS)))
    c.add("model", model)
    c.params = (c.ptr(), N_PARAMS[model])
    return model


def build(c):
    model = _model(c)
    c.add("n_params", N_PARAMS[model])
    oH, oW = _hw(c.rng)
    c.map("out", oH, oW)
    _tile(c, oH, oW)


def build_dev(c):
    model = _model(c)
    c.n = int(c.rng.integers(1, 4))
    c.add("nsets", c.n)
    c.add("n_params", N_PARAMS[model])
    oH, oW = _hw(c.rng)
    off = c.ptr()
    c.add("dtype", int(c.rng.choice([F32, F64])))
    rs = 2 * oW + 4 * int(c.coin())
    span = (oH - 1) * rs + 2 * oW
    c.add("sstride", span + 6 * int(c.coin()), span=span)
    c.add("rstride", rs, w=oW)
    _tile(c, oH, oW)
    c.tail = [None]


def build_bwd(c, device=False):
    model = _model(c)
    c.n = int(c.rng.integers(1, 4))
    c.add("nsets", c.n)
    c.add("n_params", N_PARAMS[model])
    oH, oW = _hw(c.rng)
    c.ptr()
    _tile(c, oH, oW)
    c.ptr()
    if device:
        need = c.n * N_PARAMS[model] * 8                # one block of 64 x 64 covers a tile of 6 x 6
        c.ptr()
        c.add("ws_bytes", need, need=need)
        c.tail = [None]


def mesh_bwd(c):
    (oH, oW), (gh, gw) = _hw(c.rng), _hw(c.rng, 2)
    c.dense("g", oH, oW)
    c.dims(oH, oW)
    c.add("interp", int(c.coin()))
    c.dims(gh, gw)
    c.dense("gc", gh, gw)
    c.ptr()
    need = c.n * gh * oW * 16
    c.add("ws_bytes", need, need=need)
    c.sets("g", "gc")
    c.tail = [None]


def _reproject_head(c):
    """kind, params, n_sets, depth, its dtype and set stride (0: one plane for every set) -> (oH, oW)"""
    c.add("depth_kind", int(c.coin()))
    c.params = (c.ptr(), REPROJECT_PARAMS)
    c.n = int(c.rng.integers(1, 4))
    c.add("nsets", c.n)
    oH, oW = _hw(c.rng)
    c.ptr()
    c.add("dtype", int(c.rng.choice([F32, F64])))
    c.add("sstride", 0 if c.coin(0.3) else oH * oW + 6 * int(c.coin()), span=oH * oW)
    return oH, oW


def reproject(c, device=False):
    oH, oW = _reproject_head(c)
    c.ptr()
    c.add("dtype", int(c.rng.choice([F32, F64])))
    rs = 2 * oW + 4 * int(c.coin())
    span = (oH - 1) * rs + 2 * oW
    c.add("sstride", span + 6 * int(c.coin()), span=span)
    c.add("rstride", rs, w=oW)
    c.ptr(null=c.coin(0.3))                             # depth_out
    c.add("sstride", oH * oW + 6 * int(c.coin()), span=oH * oW)
    _tile(c, oH, oW)
    if device:
        c.tail = [None]


def reproject_bwd(c, device=False):
    oH, oW = _reproject_head(c)
    c.ptr()                                             # grad_map
    c.ptr(null=c.coin(0.3))                             # grad_depth_out
    _tile(c, oH, oW)
    skip = int(c.rng.integers(0, 4))                    # 0, 3: both gradients; 1: no grad_depth; 2: no grad_params
    c.ptr(null=skip == 1)
    c.ptr(null=skip == 2)
    if device:
        need = c.n * REPROJECT_PARAMS * 8               # one block of 64 x 64 covers a tile of 6 x 6
        c.ptr()
        c.add("ws_bytes", need, need=need)
        c.tail = [None]


# entry point -> (the call's builder, batched)
HOST = {"lerf_coords_build_host": (build, False), "lerf_coords_build_bwd_host": (build_bwd, False),
        "lerf_coords_reproject_host": (reproject, False), "lerf_coords_reproject_bwd_host": (reproject_bwd, False)}
for _op in CHAINED:
    HOST["lerf_coords_%s_host" % _op] = (globals()[_op], False)
    HOST["lerf_coords_%s_batched_host" % _op] = (globals()[_op], True)
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
        return [m["need"] - 8 if k == "ws_bytes" else m["need"] - 1, 0, m["need"], m["need"] + 64]
    return {"max_iter": [0, 1, 64, 65], "tol": [-1.0, float("nan"), float("inf"), 0.0, 1e-9], "max_span": [0, 1, 64, 65],
            "orient": [-2, -1, 0, 1, 2], "interp": [-1, 0, 1, 2], "depth_kind": [-1, 0, 1, 2], "origin": [-1, 0, 3, 7], "model": [-1, 0, 1, 2, 3, 16, 17, 18],
            "n_params": [-1, 0, 8, 9, 10, 13, 17, 21]}[k]


def draw(builder, batched, rng):
    """one case: a valid call with zero to two arguments replaced.  Returns (arguments: ("p", offset or None) for a pointer, the plain
    value otherwise; the tail the device forms take (a null stream); (offset, model, n_sets) of the parameter block to prepare, or None)"""
    c = Call(rng, batched)
    builder(c)
    params = getattr(c, "params", None)
    n_mut = int(rng.choice([0, 1, 2], p=[0.2, 0.45, 0.35]))
    for i in rng.choice(len(c.args), n_mut, replace=False):
        vals = _values(c.args[i], c, int(i))
        c.args[i].v = vals[int(rng.integers(len(vals)))]
    args = [("p", a.v) if a.kind == "ptr" else a.v for a in c.args]
    return args, c.tail, (params[0], params[1], 3) if params else None


def run_case(fn, arena, args, tail=(), params=None):
    """reset the arena, make the call, return (return code, digest of the arena afterwards)"""
    arena.reset()
    if params:
        arena.set_params(*params)
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
                args, tail, params = draw(builder, batched, rng)
                rc, digest = run_case(fn, arena, args, tail, params)
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
