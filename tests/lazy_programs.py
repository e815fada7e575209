"""Seeded straight-line programs over the deferred sum / expression layer of lerf_pytorch_amd.lazy (a helper for
test_lazy_programs_cpu.py and test_gpu_lazy_fuzz.py, not a test).

A program is a list of statements in the vocabulary a caller of the unchanged call sites could write around
`FourSimplexInterpFaster`: start a sum, accumulate passes into it, derive values from it (`pred / k`, `np.clip`, `np.round`,
views, copies), finish them (`.astype`), consume them (`/ 255.0`, a stage-2 pass, reductions) and mutate what they were made
from.  `generate(seed)` builds one, `render` prints it as the numpy statements it stands for, `execute` runs it on
`(interp, pads, luts, dev)` and returns every value it names that is still alive, in naming order, and `analyse` reports which
kinds of statements and which interleavings it holds.  The expectation of a program is numpy itself: the same `execute` on plain
ndarrays.

The generator places two interleavings on purpose, because hand-written scenarios miss them:
  derive -> mutate -> read: a value is derived from a sum that is still pending, the sum is accumulated into again, and only
      then is the derived value read (numpy computed it at the derivation; a deferred layer must not see the later pass);
  a round / clip pair with NON-integer clip bounds whose float32 result feeds `/ 255.0` or a stage-2 pass (the result is not
      a uint8 image, whatever its last two steps look like).

One statement is left out on purpose: `v = np.asarray(pred[i])` / `np.asarray(pred.transpose(...))` followed by a write to
`pred`.  In numpy the result is still a view of `pred` and sees the write; the host array a device view hands to `np.asarray`
cannot alias device memory.  That is a limit of every DeviceArray, not of the deferred sums, so the generator
finishes views with `.astype` instead."""
import numpy as np

KINDS = ("start", "accumulate", "derive", "finish", "consume", "mutate")
ARITH = ("div", "mul", "add", "radd", "rmul", "clip", "round")
DERIVE_OPS = ARITH + ("index", "transpose", "copy")
STARTS = ("int0", "float0", "zeros", "pass")
ACC_FORMS = ("iadd", "add", "radd")
FINISHES = ("f32", "f64", "asarray", "none")
CONSUMES = ("div255", "pass2", "sum0", "max")
MUTATIONS = ("iadd", "imul", "fill", "img", "del")
MODES = "sctdy"
S1_KEYS = ("s1_sr0", "s1_cr0", "s1_tr0")
S2_KEYS = ("s2_sr0", "s2_sr1", "s2_cr0", "s2_cr1", "s2_tr0", "s2_tr1")
INTERVAL = 4
INT16_PASSES = 16                    # 16 * (127 << 4) = 32 512 <= 32 767 < 17 * (127 << 4): the in-place int16 sum ends here
CONSTS = (2.0, 3.0, 12.0, 0.5, 255.0, 127.0, 1.5, -1.0, 8.0, 0.1, 0.0, 1, 3, 12, 0, 127)
BOUNDS = ((0, 255), (0.0, 255.0), (0.5, 254.5), (-0.0, 255), (10, 200), (-3.5, 3.5), (0, 1), (0.25, 100.75))
FRACTIONAL_BOUNDS = ((0.5, 254.5), (0.25, 100.75), (1.5, 200.5), (0.5, 255))
SEEDS = tuple(range(12))             # the fixed list of both tests; tests/test_lazy_programs_cpu.py holds its conditions


# ------------------------------------------------------------------------------------------------------------- generation
def _pass_spec(rng, img, oC):
    key = S1_KEYS[int(rng.integers(3))] if oC == 1 else S2_KEYS[int(rng.integers(6))]      # a table holds oC bytes per entry
    return (img, key, MODES[int(rng.integers(5))], int(rng.integers(4)), oC)


def _step(rng, op=None):
    op = op or ARITH[int(rng.integers(len(ARITH)))]
    if op == "clip":
        return ("clip",) + BOUNDS[int(rng.integers(len(BOUNDS)))]
    if op == "round":
        return ("round",)
    k = CONSTS[int(rng.integers(len(CONSTS)))]
    if op == "div" and k == 0 and rng.random() < 0.8:
        k = 3                                        # x / 0 (inf, NaN) stays in, but rare
    return (op, k)


def _chain(rng):
    n = int(rng.choice([1, 1, 2, 2, 3, 3, 4, 5, 8, 9]))          # 8 is the longest fused program, the 9th step must fall back
    return [_step(rng) for _ in range(n)]


def _image_chain(rng, fractional):
    """pred / k + b, then a round / clip pair inside [0, 255]: what may be the image of a pass (finite, in the pixel range)"""
    k, b = [(3, 0), (12, 127), (8, 127), (2, 0.5), (3.0, 0.5)][int(rng.integers(5))]
    head = [("div", k)] + ([("add", b)] if rng.random() < 0.7 else [])
    lo, hi = FRACTIONAL_BOUNDS[int(rng.integers(len(FRACTIONAL_BOUNDS)))] if fractional else [(0, 255), (0.0, 255.0), (10, 200)][int(rng.integers(3))]
    pair = [("round",), ("clip", lo, hi)] if (fractional or rng.random() < 0.5) else [("clip", lo, hi), ("round",)]
    if fractional and rng.random() < 0.3:
        pair = [("clip", lo, hi), ("round",), ("clip", lo, hi)]          # clip, round, clip: the last two steps still look like a stage
    return head + pair


class _Gen(object):
    def __init__(self, seed):
        self.rng = np.random.default_rng([seed, 0x1E2F])
        self.prog = []
        self.n = {"img": 0, "v": 0, "w": 0}
        self.derived = []            # live derived names of this section: (name, is_image_chain)
        self.views = seed
        self.views_of_pred = set()

    def name(self, kind):
        self.n[kind] += 1
        return "%s%d" % (kind, self.n[kind])

    def image(self):
        nm = self.name("img")
        self.prog.append(("img", nm, int(self.rng.integers(1, 1000))))
        return nm

    def accumulate(self, img, oC, count, forms=ACC_FORMS):
        for _ in range(count):
            self.prog.append(("accumulate", forms[int(self.rng.integers(len(forms)))], _pass_spec(self.rng, img, oC)))

    def derive(self, src="pred", chain=None, image=False):
        v = self.name("v")
        self.prog.append(("derive", v, src, chain if chain is not None else _chain(self.rng)))
        self.derived.append((v, image))
        return v

    def view(self, op=None):
        op = op or ("index", "transpose", "copy")[int(self.rng.integers(3))]
        st = (op, int(self.rng.integers(3))) if op == "index" else ((op, (1, 2, 0)) if op == "transpose" else (op,))
        v = self.derive(chain=[st])
        if op != "copy":
            self.views_of_pred.add(v)
        return v

    def finish(self, v, how=None):
        how = how or FINISHES[int(self.rng.integers(4))]
        if how == "asarray" and v in self.views_of_pred:
            how = "f64"                                  # see the module docstring: np.asarray of a VIEW is left out
        if how != "none":
            self.prog.append(("finish", v, how))

    def consume(self, v, image, oC, how=None):
        rng = self.rng
        if how is None:
            how = "pass2" if (image and oC == 1 and rng.random() < 0.5) else CONSUMES[int(rng.integers(4))]
        if how == "pass2" and not (image and oC == 1):
            how = "div255"
        spec = _pass_spec(rng, None, 3) if how == "pass2" else None
        self.prog.append(("consume", self.name("w"), v, how, spec))

    def mutate(self, img, oC, how=None):
        rng = self.rng
        how = how or MUTATIONS[int(rng.integers(len(MUTATIONS)))]
        if how == "del":
            if not self.derived:
                how = "imul"
            else:
                v, _ = self.derived.pop(int(rng.integers(len(self.derived))))
                self.prog.append(("mutate", "del", v, None))
                return
        if how == "iadd":
            self.prog.append(("accumulate", "iadd", _pass_spec(rng, img, oC)))
            self.prog.append(("mutate", "iadd", "pred", None))          # a marker: the accumulate above is the mutation
        else:
            self.prog.append(("mutate", how, img if how == "img" else "pred", None))

    def section(self, template):
        rng = self.rng
        self.derived = []
        oC = 1 if rng.random() < 0.65 else 3
        img = self.image()
        pending = template in ("interleave", "fractional", "overflow")
        start = STARTS[int(rng.integers(2))] if pending else STARTS[int(rng.integers(4))]
        self.prog.append(("start", start, _pass_spec(rng, img, oC) if start == "pass" else None, oC))
        if template == "overflow":
            self.accumulate(img, oC, int(rng.integers(15, 17)), forms=("iadd",))       # up to the int16 bound ...
            self.derive()
            self.accumulate(img, oC, 1, forms=("iadd",))                               # ... and across it, with a reader pending
        else:
            self.accumulate(img, oC, int(rng.integers(1, 5)), forms=("iadd",) if pending else ACC_FORMS)
        if template == "interleave":
            for _ in range(int(rng.integers(1, 4))):
                self.derive()
            if rng.random() < 0.5:                                       # one level deeper: an expression of an expression
                self.derive(src=self.derived[0][0], chain=[_step(rng) for _ in range(int(rng.integers(1, 3)))])
            self.accumulate(img, oC, int(rng.integers(1, 3)), forms=("iadd",))
            self.prog.append(("mutate", "iadd", "pred", None))
        if template == "fractional":
            v = self.derive(chain=_image_chain(rng, True), image=True)
            self.finish(v, "f32" if rng.random() < 0.8 else "f64")
            self.consume(v, True, oC, "pass2" if (oC == 1 and rng.random() < 0.5) else "div255")
            if rng.random() < 0.5:
                self.consume(v, True, oC)
        for j in range(2):                                               # two views or copies: they ask for the sum's values
            self.views += 1
            self.view(("index", "transpose", "copy")[self.views % 3])
        for _ in range(int(rng.integers(2, 5))):                         # the free part: derive, finish, mutate, consume in any order
            if rng.random() < 0.2:
                self.view()
            elif rng.random() < 0.25:
                self.derive(chain=_image_chain(rng, rng.random() < 0.3), image=True)
            else:
                self.derive()
        order = list(self.derived)
        rng.shuffle(order)
        mutated = False
        for v, image in order:
            if not mutated and rng.random() < 0.5:
                self.mutate(img, oC)
                mutated = True
            if not any(v == d[0] for d in self.derived):                 # deleted by the mutation
                continue
            self.finish(v)
            if rng.random() < 0.6:
                self.consume(v, image, oC)
        if not mutated:
            self.mutate(img, oC)


def generate(seed):
    """the program of a seed: two or three sections, each one sum with what is derived from it"""
    g = _Gen(seed)
    r = g.rng.random()
    first = "interleave" if r < 0.62 else ("fractional" if r < 0.78 else ("overflow" if r < 0.84 else "free"))
    templates = [first] + [("interleave", "fractional", "overflow", "free", "free", "free", "free", "free")[int(g.rng.integers(8))]
                           for _ in range(int(g.rng.integers(1, 3)))]
    for t in templates:
        g.section(t)
    return g.prog


# -------------------------------------------------------------------------------------------------------------- rendering
def _pass_text(spec, img=None):
    im, key, mode, r, oC = spec
    return "F(%s, %r, mode=%r, r=%d, oC=%d)" % (img or im, key, mode, r, oC)


def _chain_text(src, chain):
    t = src
    for st in chain:
        op = st[0]
        if op == "div":
            t = "(%s / %r)" % (t, st[1])
        elif op == "mul":
            t = "(%s * %r)" % (t, st[1])
        elif op == "add":
            t = "(%s + %r)" % (t, st[1])
        elif op == "radd":
            t = "(%r + %s)" % (st[1], t)
        elif op == "rmul":
            t = "(%r * %s)" % (st[1], t)
        elif op == "clip":
            t = "np.clip(%s, %r, %r)" % (t, st[1], st[2])
        elif op == "round":
            t = "np.round(%s)" % t
        elif op == "index":
            t = "%s[%d]" % (t, st[1])
        elif op == "transpose":
            t = "%s.transpose(%r)" % (t, st[1])
        else:
            t = "%s.copy()" % t
    return t


def render(prog):
    """the program as the numpy statements it stands for (F = one LUT pass: rot90, edge pad, transpose, FourSimplexInterpFaster)"""
    out = []
    for st in prog:
        k = st[0]
        if k == "img":
            out.append("%s = dev(image(%d))" % (st[1], st[2]))
        elif k == "start":
            rhs = {"int0": "0", "float0": "0.0", "zeros": "np.zeros(shape)"}.get(st[1]) or _pass_text(st[2])
            out.append("pred = %s" % rhs)
        elif k == "accumulate":
            f = _pass_text(st[2])
            out.append({"iadd": "pred += %s", "add": "pred = pred + %s", "radd": "pred = %s + pred"}[st[1]] % f)
        elif k == "derive":
            out.append("%s = %s" % (st[1], _chain_text(st[2], st[3])))
        elif k == "finish":
            out.append({"f32": "{0} = {0}.astype(np.float32)", "f64": "{0} = {0}.astype(np.float64)", "asarray": "{0} = np.asarray({0})"}[st[2]].format(st[1]))
        elif k == "consume":
            rhs = {"div255": "%s / 255.0" % st[2], "sum0": "%s.sum(axis=0)" % st[2], "max": "%s.max()" % st[2]}.get(st[3]) \
                or _pass_text(st[4], "%s.transpose((1, 2, 0))" % st[2])
            out.append("%s = %s" % (st[1], rhs))
        elif st[1] == "iadd":
            out.append("# (the pass above mutates the sum after values were derived from it)")
        else:
            out.append({"imul": "pred *= 0.5", "fill": "pred[...] = 7", "img": "%s[:, :, 0] = 7.0" % st[2], "del": "del %s" % st[2]}[st[1]])
    return "\n".join(out)


# -------------------------------------------------------------------------------------------------------------- execution
def image(seed, hw):
    return np.random.default_rng(seed).integers(0, 256, (hw[0], hw[1], 3)).astype(np.float32)


def lut_pass(interp, pads, luts, img, key, mode, r, oC):
    """one pass as the call sites make it (resample/eval_lut_sr.py:549-555): rotate, edge-pad, CHW, interpolate, rotate back"""
    p = pads[mode]
    rot = np.rot90(img, r)
    h, w, _ = rot.shape
    chw = np.pad(rot, ((0, p), (0, p), (0, 0)), mode="edge").transpose((2, 0, 1))
    return interp(luts[key], chw, h, w, INTERVAL, 4 - r, upscale=1, mode=mode, oC=oC)


def _apply(x, chain):
    for st in chain:
        op = st[0]
        if op == "div":
            x = x / st[1]
        elif op == "mul":
            x = x * st[1]
        elif op == "add":
            x = x + st[1]
        elif op == "radd":
            x = st[1] + x
        elif op == "rmul":
            x = st[1] * x
        elif op == "clip":
            x = np.clip(x, st[1], st[2])
        elif op == "round":
            x = np.round(x)
        elif op == "index":
            x = x[st[1]]
        elif op == "transpose":
            x = x.transpose(st[1])
        else:
            x = x.copy()
    return x


def execute(prog, interp, pads, luts, dev, hw):
    """run the program; -> [(name, value)] of every name still alive, in the order the names first appeared"""
    env, order = {}, []

    def bind(name, value):
        if name not in order:
            order.append(name)
        env[name] = value

    def F(spec, img=None):
        im, key, mode, r, oC = spec
        return lut_pass(interp, pads, luts, env[im] if img is None else img, key, mode, r, oC)

    with np.errstate(all="ignore"):
        for st in prog:
            k = st[0]
            if k == "img":
                bind(st[1], dev(image(st[2], hw)))
            elif k == "start":
                how, spec, oC = st[1], st[2], st[3]
                bind("pred", 0 if how == "int0" else (0.0 if how == "float0" else (np.zeros((3 * oC, hw[0], hw[1])) if how == "zeros" else F(spec))))
            elif k == "accumulate":
                pred = env["pred"]
                if st[1] == "iadd":
                    pred += F(st[2])
                elif st[1] == "add":
                    pred = pred + F(st[2])
                else:
                    pred = F(st[2]) + pred
                env["pred"] = pred
                del pred
            elif k == "derive":
                bind(st[1], _apply(env[st[2]], st[3]))
            elif k == "finish":
                v = env[st[1]]
                env[st[1]] = v.astype(np.float32) if st[2] == "f32" else (v.astype(np.float64) if st[2] == "f64" else np.asarray(v))
                del v
            elif k == "consume":
                v = env[st[2]]
                if st[3] == "div255":
                    w = v / 255.0
                elif st[3] == "sum0":
                    w = v.sum(axis=0)
                elif st[3] == "max":
                    w = v.max()
                else:
                    w = F(st[4], v.transpose((1, 2, 0)))
                bind(st[1], w)
                del v, w
            elif st[1] == "imul":
                pred = env["pred"]
                pred *= 0.5
                env["pred"] = pred
                del pred
            elif st[1] == "fill":
                env["pred"][...] = 7
            elif st[1] == "img":
                env[st[2]][:, :, 0] = 7.0
            elif st[1] == "del":
                del env[st[2]]
    return [(nm, env[nm]) for nm in order if nm in env]


def stub_interp(weight, img_in, h, w, interval, rot, upscale=4, mode="s", oC=1):
    """a stand-in for FourSimplexInterpFaster in plain numpy: deterministic multiples of 1 / 2^interval inside the value range of a
    pass (|value| <= 127), float64 [C * oC, h', w'] turned back by `rot` quarter turns -- the generator's CPU test needs no library"""
    x = np.round(np.clip(np.asarray(img_in, dtype=np.float64)[:, :h, :w], 0, 255))
    salt = sum(ord(c) for c in str(weight) + mode) + 31 * rot
    planes = [((x[c] * (7 + 2 * j) + np.roll(x[c], 1, axis=1) * 3 + salt * (c + 1)) % 4065 - 2032) / float(1 << interval)
              for c in range(x.shape[0]) for j in range(oC)]
    return np.rot90(np.stack(planes), rot, [1, 2]).copy()


STUB_PADS = {"s": 1, "d": 2, "y": 2, "c": 3, "t": 3}
STUB_LUTS = {k: k for k in S1_KEYS + S2_KEYS}


# --------------------------------------------------------------------------------------------------------------- analysis
def _fractional_pair(chain):
    """the chain ends in a round / clip pair (either order) whose clip bounds are not both integers"""
    if len(chain) < 2 or sorted(st[0] for st in chain[-2:]) != ["clip", "round"]:
        return False
    clip = [st for st in chain[-2:] if st[0] == "clip"][0]
    return float(clip[1]) != np.floor(clip[1]) or float(clip[2]) != np.floor(clip[2])


def analyse(prog):
    """-> {"kinds": {kind: count}, "ops": {derive operator: count}, "interleaved": bool, "fractional_feed": bool, ...}.
    `interleaved`: some value was derived by arithmetic from a sum that a deferred layer can still hold pending (started from 0 /
    0.0, accumulated by `+=` only, at most 16 passes, nothing has asked for its values), the sum was accumulated into again, and
    the derived value had not been read before that.  It is a property of the statements alone, computed without the generator."""
    kinds = dict.fromkeys(KINDS, 0)
    ops = dict.fromkeys(DERIVE_OPS, 0)
    detail = {"start": dict.fromkeys(STARTS, 0), "accumulate": dict.fromkeys(ACC_FORMS, 0), "finish": dict.fromkeys(FINISHES, 0),
              "consume": dict.fromkeys(CONSUMES, 0), "mutate": dict.fromkeys(MUTATIONS, 0)}
    pending, passes, max_passes = False, 0, 0
    unread, chains = set(), {}
    interleaved = fractional_feed = crossed = False
    finished = set()
    for st in prog:
        k = st[0]
        if k == "img":
            continue
        kinds[k] += 1
        if k == "start":
            detail[k][st[1]] += 1
            pending, passes, unread = st[1] in ("int0", "float0"), 1 if st[1] == "pass" else 0, set()
        elif k == "accumulate":
            detail[k][st[1]] += 1
            passes += 1
            max_passes = max(max_passes, passes)
            pending = pending and st[1] == "iadd" and passes <= INT16_PASSES
            if passes > INT16_PASSES and unread:
                crossed = True
            if pending and passes > 1 and unread:
                interleaved = True
        elif k == "derive":
            for op in st[3]:
                ops[op[0]] += 1
            arithmetic = all(op[0] in ARITH for op in st[3])
            chains[st[1]] = (chains.get(st[2], []) if st[2] != "pred" else []) + list(st[3])
            if st[2] == "pred":
                if arithmetic and pending and passes >= 1:
                    unread.add(st[1])
                elif not arithmetic:
                    pending = False                      # a view or a copy asks for the sum's values
            elif st[2] in unread and arithmetic:
                unread.add(st[1])
        elif k == "finish":
            detail[k][st[2]] += 1
            unread.discard(st[1])
            finished.add(st[1])
        elif k == "consume":
            detail[k][st[3]] += 1
            unread.discard(st[2])
            if st[3] in ("div255", "pass2") and _fractional_pair(chains.get(st[2], [])):
                fractional_feed = True
        else:
            detail[k][st[1]] += 1
            if st[1] == "del":
                unread.discard(st[2])
            elif st[1] in ("imul", "fill"):
                pending = False
    for v in chains:
        if v not in finished:
            detail["finish"]["none"] += 1
    kinds["finish"] += detail["finish"]["none"]
    return {"kinds": kinds, "ops": ops, "detail": detail, "interleaved": interleaved, "fractional_feed": fractional_feed,
            "max_passes": max_passes, "crossed_int16_bound_with_reader": crossed}
