"""GPU: lerf_numer_epilogue_f32 (numer_epilogue_kernel, csrc/lerf_lut_interp.hip) against numpy, bit for bit.

The kernel turns int16 numerators (value = numerator / 2^interval) into float32 through a program of up to 8 float64 steps.
Its contract is numpy's own result of the same statements on the float64 array, so the reference here is exactly that: one
numpy call per step on the host in float64, then `.astype(np.float32)`.  The comparison is on the BIT PATTERNS (the sign of
zero counts; `np.array_equal` cannot see it), with one allowance: where both sides are NaN any payload passes.  The C ABI is
called directly through ctypes, on every int16 value, every interval, on pointers of every alignment the three code paths of
the kernel distinguish (8-byte `uint2` loads, 16-byte `float4` stores, the scalar tail), and on every argument it must refuse."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIV, MUL, ADD, CLIP, ROUND = 0, 1, 2, 3, 4          # LERF_EPI_* of include/lerf_hip.h
NAMES = {DIV: "div", MUL: "mul", ADD: "add", CLIP: "clip", ROUND: "round"}
LERF_OK, LERF_EINVAL = 0, -1
ALL_I16 = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16)
SENTINEL = np.float32(-1234.5)


def reference(acc, interval, prog):
    """the program executed by numpy: float64 statements in the caller's order, one rounding to float32 at the end"""
    with np.errstate(all="ignore"):
        x = acc.astype(np.float64) / float(1 << interval)
        for st in prog:
            if st[0] == DIV:
                x = x / st[1]
            elif st[0] == MUL:
                x = x * st[1]
            elif st[0] == ADD:
                x = x + st[1]
            elif st[0] == CLIP:
                x = np.clip(x, st[1], st[2])
            else:
                x = np.round(x)
        return x.astype(np.float32)


def show(prog):
    return "[" + ", ".join("%s(%s)" % (NAMES.get(st[0], st[0]), ", ".join(repr(float(v)) for v in st[1:])) for st in prog) + "]"


def same_bits(got, want):
    """boolean array: equal bit patterns, or NaN on both sides"""
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))


def assert_bits(got, want, acc, interval, prog, what=""):
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    ok = same_bits(got, want)
    if not ok.all():
        k = int(np.flatnonzero(~ok)[0])
        pytest.fail("%s program %s interval %d: %d of %d differ; first at index %d, numerator %d: got %r (0x%08x), numpy %r (0x%08x)"
                    % (what, show(prog), interval, int((~ok).sum()), ok.size, k, int(acc[k]), float(got[k]),
                       int(got.view(np.uint32)[k]), float(want[k]), int(want.view(np.uint32)[k])))


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    L = __import__("lerf_pytorch_amd")._lib
    return torch, L, L.lib()


def make_ops(L, prog):
    ops = (L.EpiOp * max(len(prog), 1))()
    for k, st in enumerate(prog):
        ops[k].op = int(st[0])
        ops[k].a = float(st[1]) if len(st) > 1 else 0.0
        ops[k].b = float(st[2]) if len(st) > 2 else 0.0
    return ops


def call(dev, acc_t, n, interval, prog, out_t, n_ops=None, ops_null=False):
    """the C ABI as it is: pointers, counts, the current stream; returns the status"""
    torch, L, lib = dev
    ops = make_ops(L, prog)
    rc = lib.lerf_numer_epilogue_f32(C.c_void_p(acc_t.data_ptr() if acc_t is not None else None), C.c_int64(n), int(interval),
                                     None if ops_null else C.cast(ops, C.c_void_p), len(prog) if n_ops is None else int(n_ops),
                                     C.c_void_p(out_t.data_ptr() if out_t is not None else None), L.current_stream())
    torch.cuda.synchronize()
    return rc


def run(dev, acc, interval, prog):
    torch = dev[0]
    a = torch.from_numpy(acc).cuda()
    out = torch.full((acc.size,), float(SENTINEL), dtype=torch.float32, device="cuda")
    assert call(dev, a, acc.size, interval, prog, out) == LERF_OK
    return out.cpu().numpy()


EXHAUSTIVE = {
    "empty": [],
    "div_3": [(DIV, 3.0)],
    "mul_3": [(MUL, 3.0)],
    "add_127": [(ADD, 127.0)],
    "clip_0_255": [(CLIP, 0.0, 255.0)],
    "round": [(ROUND,)],
    "stage1_clip_round": [(DIV, 3.0), (ADD, 0.0), (CLIP, 0.0, 255.0), (ROUND,)],
    "stage1_round_clip": [(DIV, 3.0), (ADD, 0.0), (ROUND,), (CLIP, 0.0, 255.0)],
    "stage2_clip_round": [(DIV, 12.0), (ADD, 127.0), (CLIP, 0.0, 255.0), (ROUND,)],
    "stage2_round_clip": [(DIV, 12.0), (ADD, 127.0), (ROUND,), (CLIP, 0.0, 255.0)],
    "div_round_clip_no_add": [(DIV, 3.0), (ROUND,), (CLIP, 0.0, 255.0)],          # round(-0.3) = -0.0 reaches the clip
    "eight_steps": [(DIV, 3.0), (MUL, 1.5), (ADD, -7.25), (CLIP, -100.0, 300.0), (ROUND,), (MUL, 0.1), (ADD, 0.5), (ROUND,)],
    "div_0_clip_round": [(DIV, 0.0), (CLIP, 0.0, 255.0), (ROUND,)],               # 0 / 0 = NaN, the rest +-inf
    "div_neg0_round_clip": [(DIV, -0.0), (ROUND,), (CLIP, 0.0, 255.0)],
    "clip_lower_neg0": [(MUL, 0.0), (CLIP, -0.0, 255.0)],                         # +-0.0 against a -0.0 bound
    "clip_upper_neg0": [(MUL, 0.0), (CLIP, -1.0, -0.0)],
    "ties_div3_mul3_add_half_round": [(DIV, 3.0), (MUL, 3.0), (ADD, 0.5), (ROUND,)],
    "ties_div12_add_half_round": [(DIV, 12.0), (ADD, 0.5), (ROUND,)],
    "round_clip_fractional_bounds": [(DIV, 3.0), (ROUND,), (CLIP, 0.5, 254.5)],
    "clip_bounds_crossed": [(CLIP, 5.0, 1.0)],                                    # numpy: min(max(x, 5), 1) = 1 everywhere
    "clip_nan_bound": [(CLIP, float("nan"), 255.0)],                              # numpy: NaN everywhere
    "overflow_to_inf": [(MUL, 1e300), (MUL, 1e300), (CLIP, -1e300, 1e300)],
    "float32_overflow_and_subnormals": [(MUL, 1e36), (ROUND,), (MUL, 1e-80)],
}


@pytest.mark.parametrize("name", list(EXHAUSTIVE))
def test_every_int16_numerator_at_every_interval(dev, name):
    prog = EXHAUSTIVE[name]
    for interval in range(1, 8):
        assert_bits(run(dev, ALL_I16, interval, prog), reference(ALL_I16, interval, prog), ALL_I16, interval, prog, name)


# ---- seeded random programs: lengths uniform in 0..8, operands from a pool of the hazards plus random doubles
SEED = 20261016
N_RANDOM = 200
POOL = [0.0, -0.0, 0.5, 1.0, 3.0, 12.0, 127.0, 255.0, 254.5, 1e-300, 1e300, -1.0]


def random_programs(seed=SEED, count=N_RANDOM):
    rng = np.random.default_rng(seed)

    def operand():
        if rng.random() < 0.65:
            return POOL[int(rng.integers(len(POOL)))]
        return float(rng.standard_normal() * 10.0 ** int(rng.integers(-3, 5)))
    progs = []
    for _ in range(count):
        prog = []
        for _ in range(int(rng.integers(0, 9))):
            op = int(rng.integers(0, 5))
            prog.append((op, operand(), operand()) if op == CLIP else ((op,) if op == ROUND else (op, operand())))
        progs.append((prog, int(rng.integers(1, 8))))
    return progs


RANDOM = random_programs()


def test_random_programs_are_what_the_file_says():
    assert len(RANDOM) >= 200 and random_programs() == RANDOM
    lengths = {len(p) for p, _ in RANDOM}
    assert lengths == set(range(9)), lengths
    assert {q for _, q in RANDOM} == set(range(1, 8))


@pytest.mark.parametrize("first", range(0, N_RANDOM, 25))
def test_random_programs(dev, first):
    for k in range(first, min(first + 25, N_RANDOM)):
        prog, interval = RANDOM[k]
        assert_bits(run(dev, ALL_I16, interval, prog), reference(ALL_I16, interval, prog), ALL_I16, interval, prog, "random #%d" % k)


# ---- shapes and alignment: acc and out at 0..3 elements from a 256-byte-aligned allocation, sentinels around out
SIZES = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 65537]
GUARD = 8
STAGE2 = EXHAUSTIVE["stage2_clip_round"]


@pytest.mark.parametrize("n", SIZES)
def test_every_alignment_of_acc_and_out(dev, n):
    torch = dev[0]
    rng = np.random.default_rng(n)
    for ao in range(4):
        for oo in range(4):
            acc = rng.integers(-32768, 32768, n).astype(np.int16)
            abuf = torch.zeros(n + 8, dtype=torch.int16, device="cuda")
            obuf = torch.full((n + 2 * GUARD + 4,), float(SENTINEL), dtype=torch.float32, device="cuda")
            assert abuf.data_ptr() % 256 == 0 and obuf.data_ptr() % 256 == 0
            a = abuf[ao:ao + n]
            a.copy_(torch.from_numpy(acc))
            lo = GUARD + oo                                    # GUARD * 4 bytes keeps the 16-byte phase: out is `oo` floats off
            o = obuf[lo:lo + n]
            assert a.data_ptr() == abuf.data_ptr() + 2 * ao and o.data_ptr() == obuf.data_ptr() + 4 * lo
            assert call(dev, a, n, 4, STAGE2, o) == LERF_OK
            whole = obuf.cpu().numpy()
            what = "n=%d acc+%d out+%d" % (n, ao, oo)
            assert_bits(whole[lo:lo + n], reference(acc, 4, STAGE2), acc, 4, STAGE2, what)
            assert (whole[:lo].view(np.uint32) == SENTINEL.view(np.uint32)).all(), what + ": wrote before out"
            assert (whole[lo + n:].view(np.uint32) == SENTINEL.view(np.uint32)).all(), what + ": wrote past out + n"


# ---- contract: what the entry point refuses, it refuses without touching out
def test_bad_arguments_are_refused_and_out_is_untouched(dev):
    torch = dev[0]
    n = 1024
    acc = torch.from_numpy(ALL_I16[:n].copy()).cuda()
    good = [(DIV, 3.0), (ROUND,)]
    cases = {
        "n_ops -1": dict(prog=good, n_ops=-1),
        "n_ops 9": dict(prog=good * 5, n_ops=9),
        "interval 0": dict(prog=good, interval=0),
        "interval 8": dict(prog=good, interval=8),
        "op code -1": dict(prog=[(DIV, 3.0), (-1, 1.0)]),
        "op code 5": dict(prog=[(5, 1.0), (ROUND,)]),
        "n 0": dict(prog=good, n=0),
        "acc NULL": dict(prog=good, acc=None),
        "out NULL": dict(prog=good, out=None),
        "ops NULL with n_ops > 0": dict(prog=good, ops_null=True),
    }
    for what, kw in cases.items():
        out = torch.full((n,), float(SENTINEL), dtype=torch.float32, device="cuda")
        rc = call(dev, kw.get("acc", acc), kw.get("n", n), kw.get("interval", 4), kw["prog"], kw.get("out", out),
                  n_ops=kw.get("n_ops"), ops_null=kw.get("ops_null", False))
        assert rc == LERF_EINVAL, (what, rc)
        assert (out.cpu().numpy().view(np.uint32) == SENTINEL.view(np.uint32)).all(), what + ": out was written"
    out = torch.full((n,), float(SENTINEL), dtype=torch.float32, device="cuda")
    assert call(dev, acc, n, 4, [], out, ops_null=True) == LERF_OK             # no steps: ops may be NULL
    assert_bits(out.cpu().numpy(), reference(ALL_I16[:n], 4, []), ALL_I16[:n], 4, [], "NULL ops, 0 steps")


def test_two_runs_are_bitwise_equal(dev):
    prog = EXHAUSTIVE["eight_steps"]
    a, b = run(dev, ALL_I16, 4, prog), run(dev, ALL_I16, 4, prog)
    assert (a.view(np.uint32) == b.view(np.uint32)).all()
