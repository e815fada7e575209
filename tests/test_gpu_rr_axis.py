"""GPU: lerf_rr_axis (csrc/lerf_rr.hip) called directly through ctypes with crafted tables, on every launch path, against
tests/rr_axis_ref.py.

Every comparison is on bit patterns: include/lerf_hip.h promises products and sums rounded separately, in tap order, in the
accumulator type, and axis_ref / csr_ref do exactly that, so there is no tolerance to choose.  (The one exception is the
autograd check at the end, which compares with a dense float64 matrix product to the project's float64 bound, 1e-9.)

Every output buffer is filled with NaN (uint8: 0xA5) before the call and sits between two guard bands of 64 elements: an
output no thread wrote shows as a surviving NaN, a write outside the output as a changed guard element.

Which path a case takes (wide / narrow, LDS window / global memory) is not visible in the numbers; tests/test_rr_axis_cpu.py
proves from the kernel's own constants that rr_axis_ref.CASES reaches each one."""
import ctypes as C

import numpy as np
import pytest
import torch

import rr_axis_ref as A
from rr_axis_ref import CASES, F32, F64, I16, U8

import lerf_pytorch_amd as L                                                  # noqa: F401
from lerf_pytorch_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
EINVAL, EUNSUPPORTED = -1, -2
F64_TOL = 1e-9                                                                # the F64_TOL of tests/test_gpu_rr.py
ACCS = pytest.mark.parametrize("acc", [F32, F64], ids=["f32", "f64"])

# the fill of an output buffer, as bits: quiet NaNs; 0xA5 bytes
FILL = {U8: (torch.uint8, torch.uint8, 0xA5), F32: (torch.int32, torch.float32, 0x7FC00000), F64: (torch.int64, torch.float64, 0x7FF8000000000000)}
BITS = {1: np.uint8, 4: np.uint32, 8: np.uint64}


def bits(a):
    return np.ascontiguousarray(a).view(BITS[a.dtype.itemsize])


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


class Guarded(object):
    """a filled device buffer of n elements between two guard bands"""

    def __init__(self, n, code):
        raw, dt, pattern = FILL[code]
        self.n, self.pattern = n, pattern
        self.buf = torch.full((n + 2 * GUARD,), pattern, dtype=raw, device=DEV).view(dt)
        self.ptr = self.buf.data_ptr() + GUARD * self.buf.element_size()

    def host(self, what):
        """the n elements, after checking that both guard bands still hold the fill"""
        h = self.buf.cpu().numpy()
        b = bits(h)
        for name, band in (("below", b[:GUARD]), ("above", b[GUARD + self.n:])):
            assert np.all(band == self.pattern), "%s: %d guard elements %s the output were overwritten" % (what, int((band != self.pattern).sum()), name)
        return h[GUARD:GUARD + self.n]

    def assert_untouched(self, what):
        assert np.all(bits(self.host(what)) == self.pattern), "%s: a refused call wrote to its output" % what


def rr_axis(x, in_code, outer, inner, n_in, n_out, taps, pad, acc, out_code, left=None, w=None, row_ptr=None, idx=None, what="", rc=0,
            raw_in=None):
    """one lerf_rr_axis call on device copies of the host arrays -> the output [outer][n_out][inner] on the host (rc == 0), after the
    guard check; `x` a host array or a device tensor; raw_in: a device address used as is"""
    xt = x if isinstance(x, torch.Tensor) or x is None else dev(x)
    tabs = [dev(np.asarray(t, dtype=np.int32)) if t is not None else None for t in (left, row_ptr, idx)]
    wt = dev(np.asarray(w, dtype=A.NP_OF[acc])) if w is not None and acc in A.NP_OF and acc != U8 else dev(w)
    ax = _lib.RrAxis(n_in, n_out, taps, ptr(tabs[0]), ptr(tabs[1]), ptr(tabs[2]), ptr(wt), pad)
    out = Guarded(outer * n_out * inner, out_code)
    got = _lib.lib().lerf_rr_axis(raw_in if raw_in is not None else ptr(xt), in_code, outer, inner, C.byref(ax), acc, out.ptr, out_code,
                                  _lib.current_stream())
    torch.cuda.synchronize()
    assert got == rc, "%s: lerf_rr_axis returned %d, expected %d" % (what, got, rc)
    if rc != 0:
        out.assert_untouched(what)
        return None
    return out.host(what).reshape(outer, n_out, inner)


def assert_bit_equal(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    if got.dtype.kind == "f":
        unwritten = np.isnan(got)
        assert not unwritten.any(), "%s: %d of %d outputs still hold the NaN fill, first at %s" % (
            what, int(unwritten.sum()), got.size, tuple(int(v) for v in np.argwhere(unwritten)[0]))
    bad = bits(got) != bits(want)
    if bad.any():
        at = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d outputs differ in bits, first at %s: got %r, want %r" % (what, int(bad.sum()), got.size, at, got[at], want[at]))


def run_case(c, acc):
    in_code = acc                                                    # float input of the accumulator's type
    x, w = A.case_data(c, in_code, acc)
    want = A.axis_ref(x, c.left, w, c.n_in, c.pad, A.NP_OF[acc])
    got = rr_axis(x, in_code, c.outer, c.inner, c.n_in, c.n_out, c.taps, c.pad, acc, acc, left=c.left, w=w, what=c.name)
    assert_bit_equal(got, want, c.name)


# ---------------------------------------------------------------------------------------------------------- crafted forward tables
@ACCS
@pytest.mark.parametrize("name", [c.name for c in CASES if not c.group.startswith("pad-")])
def test_crafted_table(name, acc):
    """window limit (4096 / 4097, inner 1 and 3), narrow lane mappings, wide tails, unordered left[]"""
    (c,) = [c for c in CASES if c.name == name]
    run_case(c, acc)


@ACCS
@pytest.mark.parametrize("pad", range(5), ids=A.PAD_NAMES)
@pytest.mark.parametrize("place", ["staged", "unstaged", "wide"])
def test_pad_rule_far_outside(place, pad, acc):
    """n_in 1, 2, 3, 5 with left from -40 upward: many bounces of reflect / symmetric, several turns of wrap"""
    cases = [c for c in CASES if c.group == "pad-" + place and c.pad == pad]
    assert len(cases) == 12
    for c in cases:
        run_case(c, acc)


# ---------------------------------------------------------------------------------------------------------- grid strides
def _stride_case(kind):
    if kind == "wide-outer":                  # gridDim.z = 65535 < outer
        return A.Case(kind, "stride", 65600, 2, 2, 64, 2, np.array([-1, 1], np.int32), 2, 9001)
    if kind == "wide-n_out":                  # gridDim.y = 65535 < n_out
        return A.Case(kind, "stride", 1, 9, 65600, 64, 3, ((np.arange(65600) * 5) % 11 - 2).astype(np.int32), 3, 9002)
    # narrow, gridDim.y = 65535 < outer: workgroups 0 .. 4464 take a second slice and stage their window again
    return A.Case(kind, "stride", 70000, 5, 4, 3, 3, np.array([-1, 0, 2, 3], np.int32), 4, 9003)


@ACCS
@pytest.mark.parametrize("kind", ["wide-outer", "wide-n_out", "narrow-outer"])
def test_grid_stride_loops(kind, acc):
    c = _stride_case(kind)
    p = A.paths(c.n_out, c.inner, c.left, c.taps)
    assert p == ("wide" if kind.startswith("wide") else ["lds"])
    assert max(c.outer, c.n_out) > 65535
    x, w = A.case_data(c, acc, acc)
    want = A.axis_ref(x, c.left, w, c.n_in, c.pad, A.NP_OF[acc])
    xt = dev(x)
    got = rr_axis(xt, acc, c.outer, c.inner, c.n_in, c.n_out, c.taps, c.pad, acc, acc, left=c.left, w=w, what=kind)
    assert_bit_equal(got, want, kind)
    if kind == "narrow-outer":                # the window is reused across slices: a second run gives the same bits
        again = rr_axis(xt, acc, c.outer, c.inner, c.n_in, c.n_out, c.taps, c.pad, acc, acc, left=c.left, w=w, what=kind + " (again)")
        assert_bit_equal(again, got, kind + ": second run against the first")


@ACCS
@pytest.mark.parametrize("kind", ["wide-outer", "narrow-outer"])
def test_grid_stride_loops_csr(kind, acc):
    c = _stride_case(kind)
    rng = np.random.default_rng(c.seed)
    w = A.make_values(rng, (c.n_out, c.taps)).astype(A.NP_OF[acc])
    g = A.make_values(rng, (c.outer, c.n_out, c.inner)).astype(A.NP_OF[acc])
    row_ptr, idx, wt = A.adjoint_csr(c.left, w, c.n_in, c.pad)
    want = A.csr_ref(g, row_ptr, idx, wt, A.NP_OF[acc])
    got = rr_axis(g, acc, c.outer, c.inner, c.n_out, c.n_in, 0, 0, acc, acc, row_ptr=row_ptr, idx=idx, w=wt, what=kind + " csr")
    assert_bit_equal(got, want, kind + " csr")


# ---------------------------------------------------------------------------------------------------------- types
def _type_table(inner):
    return A.Case("types-%d" % inner, "types", 2, 11, 9, inner, 4, (np.arange(9) - 2).astype(np.int32), 3, 9100 + inner)


@pytest.mark.parametrize("inner", [3, 70])
@ACCS
@pytest.mark.parametrize("in_code", [U8, F32, F64], ids=["u8", "f32", "f64"])
def test_input_types(in_code, acc, inner):
    """every input type into every accumulator; float64 into a float32 accumulator rounds to nearest first"""
    c = _type_table(inner)
    x, w = A.case_data(c, in_code, acc)
    if in_code == F64 and acc == F32:
        assert np.any(x.astype(np.float32).astype(np.float64) != x)
    want = A.axis_ref(x, c.left, w, c.n_in, c.pad, A.NP_OF[acc])
    got = rr_axis(x, in_code, c.outer, c.inner, c.n_in, c.n_out, c.taps, c.pad, acc, acc, left=c.left, w=w, what=c.name)
    assert_bit_equal(got, want, c.name)


@pytest.mark.parametrize("inner", [3, 70])
@pytest.mark.parametrize("in_code", [U8, F32, F64], ids=["u8", "f32", "f64"])
def test_uint8_epilogue_input_types(in_code, inner):
    c = _type_table(inner)
    rng = np.random.default_rng([c.seed, in_code])
    shape = (c.outer, c.n_in, c.inner)
    w = np.exp2(rng.uniform(-4.0, 0.0, (c.n_out, c.taps))) * rng.choice([-1.0, 1.0, 1.0], (c.n_out, c.taps))      # sums inside and either side of 0 .. 255
    if in_code == U8:
        x = rng.integers(0, 256, shape, dtype=np.uint8)
    else:
        x = (np.exp2(rng.uniform(-10.0, 10.0, shape)) * rng.choice([-1.0, 1.0, 1.0, 1.0], shape)).astype(A.NP_OF[in_code])
    want = A.axis_ref(x, c.left, w, c.n_in, c.pad, np.float64, out_u8=True)
    assert 0.2 < np.mean((want > 0) & (want < 255)) and (want == 0).any() and (want == 255).any()      # the clip and its inside
    got = rr_axis(x, in_code, c.outer, c.inner, c.n_in, c.n_out, c.taps, c.pad, F64, U8, left=c.left, w=w, what=c.name)
    assert_bit_equal(got, want, c.name + " uint8")


def _tie_values(dtype):
    ties = np.arange(-1, 256, dtype=np.float64) + 0.5
    v = [ties, np.array([0.0, -0.0, 255.4999, 255.5, 300.0, -7.0])]
    t = ties.astype(dtype)
    assert np.array_equal(t.astype(np.float64), ties)
    v += [np.nextafter(t, dtype(-np.inf)).astype(np.float64), np.nextafter(t, dtype(np.inf)).astype(np.float64)]
    return np.concatenate(v).astype(dtype)


@pytest.mark.parametrize("inner", [1, 64])
@pytest.mark.parametrize("in_code", [F64, F32], ids=["f64", "f32"])
def test_uint8_epilogue_rounds_half_to_even(in_code, inner):
    """an identity table (taps = 1, w = 1, left[j] = j): every k + 0.5, one ulp either side, the clip's ends"""
    v = _tie_values(A.NP_OF[in_code])
    n = len(v)
    x = np.broadcast_to(v[None, :, None], (1, n, inner)).copy()
    want = np.round(np.clip(x.astype(np.float64), 0, 255)).astype(np.uint8)
    assert want[0, 1, 0] == 0 and want[0, 2, 0] == 2 and want[0, 3, 0] == 2 and want[0, 4, 0] == 4           # 0.5, 1.5, 2.5, 3.5
    got = rr_axis(x, in_code, 1, inner, n, n, 1, 1, F64, U8, left=np.arange(n), w=np.ones((n, 1)), what="ties")
    assert_bit_equal(got, want, "ties")


# ---------------------------------------------------------------------------------------------------------- refusals on device buffers
def _refusal(what, rc, **kw):
    a = dict(inp=True, axis=True, w=True, left=True, row_ptr=True, idx=True, outer=2, inner=3, n_in=4, n_out=5, taps=2, pad_mode=1,
             in_dtype=F64, acc_dtype=F64, out_dtype=F64, out=True)
    assert set(kw) <= set(a), kw
    a.update(kw)
    scratch = torch.zeros(4096, dtype=torch.float64, device=DEV)
    p = scratch.data_ptr()
    ax = _lib.RrAxis(a["n_in"], a["n_out"], a["taps"], p if a["left"] else None, p if a["row_ptr"] else None, p if a["idx"] else None,
                     p if a["w"] else None, a["pad_mode"])
    out = Guarded(256, a["out_dtype"] if a["out_dtype"] in FILL else F64)
    got = _lib.lib().lerf_rr_axis(p if a["inp"] else None, a["in_dtype"], a["outer"], a["inner"], C.byref(ax) if a["axis"] else None,
                                  a["acc_dtype"], out.ptr if a["out"] else None, a["out_dtype"], _lib.current_stream())
    torch.cuda.synchronize()
    assert got == rc, (what, kw, got)
    out.assert_untouched(what)
    assert not bool(scratch.any())


def test_refused_type_combinations_leave_the_output_untouched():
    for in_dtype in (U8, F32, F64):
        _refusal("uint8 out, float32 accumulator", EUNSUPPORTED, in_dtype=in_dtype, acc_dtype=F32, out_dtype=U8)
        _refusal("float32 out, float64 accumulator", EUNSUPPORTED, in_dtype=in_dtype, acc_dtype=F64, out_dtype=F32)
        _refusal("float64 out, float32 accumulator", EUNSUPPORTED, in_dtype=in_dtype, acc_dtype=F32, out_dtype=F64)
    for inner in (3, 64):
        for taps in (2, 0):
            _refusal("int16 in", EINVAL, in_dtype=I16, inner=inner, taps=taps)
            _refusal("int16 in, uint8 out", EINVAL, in_dtype=I16, out_dtype=U8, inner=inner, taps=taps)
            _refusal("uint8 accumulator", EINVAL, acc_dtype=U8, inner=inner, taps=taps)
            _refusal("int16 accumulator", EINVAL, acc_dtype=I16, inner=inner, taps=taps)


def test_argument_checks_on_device_buffers():
    import test_rr_axis_cpu as T                   # the same table, this time with every pointer on the device
    for code, cases in T.HOST_REFUSALS.items():
        for case in cases:
            kw = {k: (v if v is not None else False) for k, v in case.items()}
            _refusal("argument check", code, **kw)
    _refusal("null out", EINVAL, out=False)


# ---------------------------------------------------------------------------------------------------------- CSR
CSR_TABLES = {"bounces": (7, 40, 7, -20, 1), "two-workgroups": (300, 130, 9, -5, 2)}      # n_in, n_out, taps, offset, stride


@pytest.mark.parametrize("inner", [1, 3, 64])
@ACCS
@pytest.mark.parametrize("pad", range(5), ids=A.PAD_NAMES)
def test_csr_from_the_adjoint_table(pad, acc, inner):
    for name, (n_in, n_out, taps, offset, stride) in CSR_TABLES.items():
        rng = np.random.default_rng([pad, acc, inner, n_in])
        left = (np.arange(n_out) * stride + offset).astype(np.int32)
        w = A.make_values(rng, (n_out, taps)).astype(A.NP_OF[acc])
        g = A.make_values(rng, (2, n_out, inner)).astype(A.NP_OF[acc])
        row_ptr, idx, wt = A.adjoint_csr(left, w, n_in, pad)
        if len(idx) == 0:
            idx, wt = np.zeros(1, np.int32), np.zeros(1, wt.dtype)
        want = A.csr_ref(g, row_ptr, idx, wt, A.NP_OF[acc])
        got = rr_axis(g, acc, 2, inner, n_out, n_in, 0, 0, acc, acc, row_ptr=row_ptr, idx=idx, w=wt, what="csr " + name)
        assert_bit_equal(got, want, "csr " + name)


@pytest.mark.parametrize("inner", [3, 64])
@ACCS
def test_csr_empty_rows_and_no_entries(acc, inner):
    rng = np.random.default_rng([acc, inner])
    counts = np.array([0, 2, 1, 3, 0, 0, 1, 2, 0])                      # empty first, middle (two in a row) and last rows
    row_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    n_src = 6
    idx = rng.integers(0, n_src, row_ptr[-1]).astype(np.int32)
    w = A.make_values(rng, (int(row_ptr[-1]),), zeros=0.0).astype(A.NP_OF[acc])
    x = A.make_values(rng, (3, n_src, inner), zeros=0.0).astype(A.NP_OF[acc])
    want = A.csr_ref(x, row_ptr, idx, w, A.NP_OF[acc])
    got = rr_axis(x, acc, 3, inner, n_src, len(counts), 0, 0, acc, acc, row_ptr=row_ptr, idx=idx, w=w, what="csr empty rows")
    assert_bit_equal(got, want, "csr empty rows")
    assert not bits(got[:, counts == 0, :]).any() and bits(got[:, counts > 0, :]).all()          # exactly +0, and only there
    # nnz = 0: one-element dummies behind idx and w
    none = rr_axis(x, acc, 3, inner, n_src, 9, 0, 0, acc, acc, row_ptr=np.zeros(10, np.int32), idx=np.zeros(1, np.int32),
                   w=np.full(1, 7.0), what="csr nnz = 0")
    assert none.shape == (3, 9, inner) and not bits(none).any()


# ---------------------------------------------------------------------------------------------------------- 64-bit offsets
def test_offsets_past_2_31():
    """one flat uint8 buffer of 2^31 + 2^20 bytes, zero except where the tables read"""
    total = (1 << 31) + (1 << 20)
    buf = torch.zeros(total, dtype=torch.uint8, device=DEV)
    v1 = v2 = None
    try:
        gen = torch.Generator(device=DEV)
        gen.manual_seed(31)
        # view 2, narrow: [32769][65536][1], taps read columns 65530 .. 65535 of every slice; the last slice starts at 2^31
        v2 = buf[:32769 * 65536].view(32769, 65536)
        v2[:, 65530:] = torch.randint(0, 256, (32769, 6), dtype=torch.uint8, device=DEV, generator=gen)
        # view 1, wide: [1][2049][2^20], taps read rows 2047 and 2048; row 2048 starts at 2^31
        v1 = buf.view(2049, 1 << 20)
        v1[2047:] = torch.randint(0, 256, (2, 1 << 20), dtype=torch.uint8, device=DEV, generator=gen)
        for acc in (F64, F32):
            rng = np.random.default_rng(acc)
            w1 = A.make_values(rng, (1, 2), zeros=0.0).astype(A.NP_OF[acc])
            got = rr_axis(None, U8, 1, 1 << 20, 2049, 1, 2, 1, acc, acc, left=[2047], w=w1, what="wide past 2^31", raw_in=buf.data_ptr())
            rows = v1[2047:].cpu().numpy()[None]                                      # [1][2][2^20]
            assert rows[0, 1].any()
            assert_bit_equal(got, A.axis_ref(rows, [0], w1, 2, 1, A.NP_OF[acc]), "wide past 2^31")
            w2 = A.make_values(rng, (2, 2), zeros=0.0).astype(A.NP_OF[acc])
            left = np.array([65530, 65534], np.int32)
            assert A.paths(2, 1, left, 2) == ["lds"]
            got = rr_axis(None, U8, 32769, 1, 65536, 2, 2, 1, acc, acc, left=left, w=w2, what="narrow past 2^31", raw_in=buf.data_ptr())
            cols = v2[:, 65530:].cpu().numpy()[:, :, None]                            # [32769][6][1]
            assert cols[32768].any()
            assert_bit_equal(got, A.axis_ref(cols, left - 65530, w2, 6, 1, A.NP_OF[acc]), "narrow past 2^31")
    finally:
        del buf, v1, v2
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------- through the Python wrapper
def test_resize_to_uint8_of_uint8_and_float32_images():
    from lerf_pytorch_amd.resize_right.resize_right import resize, resize_to_uint8
    rng = np.random.default_rng(12)
    for shape, sf in (((33, 47, 3), [1 / 3, 1 / 3]), ((20, 31), [0.5, 2]), ((9, 70, 3), [1, 0.5])):
        for x in (rng.integers(0, 256, shape, dtype=np.uint8), rng.uniform(-40, 300, shape).astype(np.float32)):
            f = np.asarray(resize(x, scale_factors=sf))
            u = np.asarray(resize_to_uint8(x, scale_factors=sf))
            assert f.dtype == np.float64 and u.dtype == np.uint8
            assert np.array_equal(u, np.round(np.clip(f, 0, 255)).astype(np.uint8)), (shape, sf, x.dtype)


@pytest.mark.parametrize("method", ["cubic", "linear"])
def test_backward_of_an_unfiltered_downscale_leaves_unread_pixels_zero(method):
    """antialiasing=False at x0.25 / x0.3: the taps skip source pixels, so the adjoint table has empty rows"""
    from lerf_pytorch_amd.resize_right import interp_methods as IM
    from lerf_pytorch_amd.resize_right import resize_right as R
    fn = getattr(IM, method)
    rng = np.random.default_rng(13)
    x = torch.from_numpy(rng.normal(size=(3, 37, 41))).to(DEV).requires_grad_(True)
    out = R.resize(x, scale_factors=[0.25, 0.3], interp_method=fn, antialiasing=False)
    assert tuple(out.shape) == (3, 10, 13) and out.dtype == torch.float64
    g = rng.normal(size=(3, 10, 13))
    (gx,) = torch.autograd.grad(out, x, torch.from_numpy(g).to(DEV))
    gx = gx.cpu().numpy()
    mats = []
    for n_in, n_out, s in ((37, 10, 0.25), (41, 13, 0.3)):
        tab = R.axis_table(n_in, n_out, s, fn, fn.support_sz, False, 0, False)
        mats.append(A.dense_matrix(tab.left, tab.w.astype(np.float64), n_in, 0))
    want = np.einsum("js,bjk,kt->bst", mats[0], g, mats[1])
    assert float(np.max(np.abs(gx - want))) <= F64_TOL
    unread_r, unread_c = ~mats[0].any(0), ~mats[1].any(0)
    assert unread_r.any() and unread_c.any()
    assert not bits(gx[:, unread_r, :]).any() and not bits(gx[:, :, unread_c]).any()              # exactly +0
    assert np.all(gx[:, ~unread_r][:, :, ~unread_c] != 0)
