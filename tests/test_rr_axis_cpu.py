"""CPU-only: the reference of tests/test_gpu_rr_axis.py is tied to the mathematical operation, its launch-path rule to the
kernel source, its case list to the paths it claims to reach; and the argument checks of lerf_rr_axis that return before any
HIP call are pinned on host memory.

Bounds.  axis_ref adds `taps` rounded products one after the other: by the standard bound for recursive summation its
error is below taps * u' * sum_k |w_k x_k| with u' = 2 u the spacing of the accumulator type (2^-52 float64, 2^-23
float32; u the unit roundoff).  The dense matrix folds at most `taps` weights into one entry in float64, which stays
inside the same bound, and the product with it is evaluated in extended precision (or with math.fsum)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import REPO

import rr_axis_ref as A
from rr_axis_ref import CASES, F32, F64

from lerf_pytorch_amd import _lib

EINVAL, EUNSUPPORTED = -1, -2
SPACING = {F32: 2.0 ** -23, F64: 2.0 ** -52}


def exact_apply(m, x):
    """m [r][c] float64 applied along axis 1 of x [outer][c][inner], without float64 rounding of the sums"""
    if np.finfo(np.longdouble).nmant >= 63:
        return np.einsum("jc,oci->oji", m.astype(np.longdouble), x.astype(np.longdouble))
    out = np.zeros((x.shape[0], m.shape[0], x.shape[2]), np.float64)
    for o in range(x.shape[0]):
        for j in range(m.shape[0]):
            nz = np.nonzero(m[j])[0]
            for i in range(x.shape[2]):
                out[o, j, i] = math.fsum((m[j, nz] * x[o, nz, i]).tolist())
    return out


def _small(case):
    return case.n_out * case.n_in * case.inner * case.outer <= 1 << 21


DENSE_CASES = [c for c in CASES if _small(c)] + [c for c in CASES if c.group == "window"]


def test_dense_cases_cover_every_group():
    assert {c.group for c in DENSE_CASES} == {c.group for c in CASES}
    assert len(CASES) == len({c.name for c in CASES}) == len({c.seed for c in CASES})


@pytest.mark.parametrize("acc", [F64, F32], ids=["f64", "f32"])
def test_axis_ref_against_the_dense_matrix(acc):
    worst = 0.0
    for c in DENSE_CASES:
        if c.group == "window" and acc == F32 and c.inner == 3:
            continue                                             # the float64 run covers the table; keep the CPU suite quick
        x, w = A.case_data(c, F64 if acc == F64 else F32, acc)
        got = A.axis_ref(x, c.left, w, c.n_in, c.pad, A.NP_OF[acc])
        assert got.dtype == A.NP_OF[acc] and got.shape == (c.outer, c.n_out, c.inner)
        m = A.dense_matrix(c.left, w, c.n_in, c.pad)
        want = exact_apply(m, x.astype(np.float64))
        mag = exact_apply(A.dense_matrix(c.left, np.abs(w), c.n_in, c.pad), np.abs(x.astype(np.float64)))
        bound = c.taps * SPACING[acc] * mag
        err = np.abs(got.astype(np.longdouble) - want)
        assert np.all(err <= bound), (c.name, float(np.max(err - bound)))
        nz = np.asarray(mag > 0)
        if nz.any():
            worst = max(worst, float(np.max(err[nz] / bound[nz])))
        # no sum of this case consists of -0.0 products only: a +0 start and no start then give the same bits
        assert not np.any(np.signbit(got) & (got == 0)), c.name
    print("axis_ref / dense: worst error is %.3f of its bound" % worst)
    assert worst > 0.0                                           # the bound was exercised, not vacuous


def test_source_rows_are_numpy_pad_and_agree_with_the_adjoint_table():
    """np.pad's index rule, and through lerf_rr_adjoint_csr the project's own (host::source_tap), agree on every tap of the pad cases"""
    for c in CASES:
        if c.group != "pad-staged":
            continue
        src = A.source_rows(c.left, c.taps, c.n_in, c.pad)
        assert src.min() >= (-1 if c.pad == 0 else 0) and src.max() < c.n_in
        w = np.arange(1, c.n_out * c.taps + 1, dtype=np.float64).reshape(c.n_out, c.taps)      # weight = 1 + flat tap number
        row_ptr, idx, wt = A.adjoint_csr(c.left, w, c.n_in, c.pad)
        flat = wt.astype(np.int64) - 1
        for s in range(c.n_in):
            taps_of_s = flat[row_ptr[s]:row_ptr[s + 1]]
            assert np.array_equal(taps_of_s, np.nonzero(src.reshape(-1) == s)[0]), (c.name, s)
            assert np.array_equal(idx[row_ptr[s]:row_ptr[s + 1]], taps_of_s // c.taps)


@pytest.mark.parametrize("pad", range(5), ids=A.PAD_NAMES)
@pytest.mark.parametrize("acc", [F64, F32], ids=["f64", "f32"])
def test_csr_ref_on_the_adjoint_table_is_the_transposed_matrix(pad, acc):
    rng = np.random.default_rng(40 + pad)
    for n_in, n_out, taps, inner in ((5, 30, 7, 3), (23, 9, 4, 1), (2, 12, 32, 2), (40, 6, 3, 4)):
        left = (np.arange(n_out) * 2 - 9 - 4 * n_in * (n_in < 6)).astype(np.int32)
        w = A.make_values(rng, (n_out, taps)).astype(A.NP_OF[acc])
        g = A.make_values(rng, (2, n_out, inner)).astype(A.NP_OF[acc])
        row_ptr, idx, wt = A.adjoint_csr(left, w, n_in, pad)
        assert row_ptr[0] == 0 and row_ptr[-1] == len(idx) == len(wt) and np.all(np.diff(row_ptr) >= 0)
        got = A.csr_ref(g, row_ptr, idx, wt, A.NP_OF[acc])
        assert got.shape == (2, n_in, inner) and got.dtype == A.NP_OF[acc]
        g64 = g.astype(np.float64)
        want = exact_apply(A.dense_matrix(left, w, n_in, pad).T, g64)
        mag = exact_apply(A.dense_matrix(left, np.abs(w), n_in, pad).T, np.abs(g64))
        rows = int(np.max(np.diff(row_ptr)))
        err = np.abs(got.astype(np.longdouble) - want)
        assert np.all(err <= max(rows, 1) * SPACING[acc] * mag), (pad, n_in, n_out, taps)


def test_constants_are_the_kernel_sources():
    src = open(os.path.join(REPO, "lerf-pytorch_amd", "csrc", "lerf_rr.hip")).read()
    for name in ("kThreads", "kVec", "kWin"):
        found = re.findall(r"^constexpr int %s = (\d+);" % name, src, flags=re.M)
        assert len(found) == 1, name
        assert int(found[0]) == getattr(A, name), name
    assert "inner >= 64" in src and "kThreads / (int)inner" in src          # the wide / narrow split and jt of paths()


def test_case_list_reaches_every_path():
    seen = set()
    for c in CASES:
        p = A.paths(c.n_out, c.inner, c.left, c.taps)
        if p == "wide":
            seen.add("wide")
            assert c.inner >= 64
            if A.wide_x_blocks(c.inner) > 1 and c.inner % (A.kThreads * A.kVec) == 1:
                seen.add("wide: an x-block with one live lane")
            continue
        kinds = set(p)
        seen.add({("lds",): "narrow all-lds", ("global",): "narrow all-global"}.get(tuple(sorted(kinds)), "narrow mixed"))
        for _, _, sp in A.workgroup_spans(c.n_out, c.inner, c.left, c.taps):
            if sp * c.inner == A.kWin:
                seen.add("sp * inner == kWin")
            if A.kWin < sp * c.inner < A.kWin + c.inner + 1:
                seen.add("kWin < sp * inner < kWin + inner + 1")
            if sp <= 0:
                seen.add("sp <= 0")
        if 256 % c.inner and c.n_out % (A.kThreads // c.inner):
            seen.add("narrow: idle tail lanes and a partial last workgroup")
    want = {"wide", "wide: an x-block with one live lane", "narrow all-lds", "narrow all-global", "narrow mixed", "sp * inner == kWin",
            "kWin < sp * inner < kWin + inner + 1", "sp <= 0", "narrow: idle tail lanes and a partial last workgroup"}
    assert seen == want, want - seen


def test_case_list_is_what_the_gpu_tests_announce():
    by = {c.name: c for c in CASES}
    assert A.paths(600, 1, by["window-1x4096"].left, 271) == ["lds"] * 3
    assert A.paths(600, 1, by["window-1x4097"].left, 272) == ["global", "global", "lds"]
    assert A.paths(200, 3, by["window-3x1365"].left, 21) == ["lds"] * 3
    assert A.paths(200, 3, by["window-3x1366"].left, 22) == ["global", "global", "lds"]
    for c in CASES:
        p = A.paths(c.n_out, c.inner, c.left, c.taps)
        if c.group == "pad-staged" or c.group == "lanes":
            assert p == ["lds"] * len(p), c.name
        elif c.group == "pad-unstaged":
            assert p == ["global"], c.name
        elif c.group in ("pad-wide", "wide"):
            assert p == "wide", c.name
        if c.group.startswith("pad-"):
            assert c.left.min() == -40 and c.left.min() < -7 * c.n_in and c.left.max() > 7 * c.n_in    # many bounces, both sides
        else:
            src = A.source_rows(c.left, c.taps, c.n_in, 0)
            assert (src[c.left.argmin()] < 0).any() and (src[c.left.argmax()] < 0).any(), c.name       # taps in both pads
    desc = by["order-descending-1"]
    assert np.all(np.diff(desc.left) < 0)
    assert sorted(by["order-permuted-3"].left.tolist()) == sorted(by["order-descending-3"].left.tolist())
    for inner in (1, 3):
        c = by["order-outliers-%d" % inner]
        for j0, j1, _ in A.workgroup_spans(c.n_out, inner, c.left, c.taps):
            assert c.left[j0 + 1:j1].min() < c.left[j0] and c.left[j0 + 1:j1].max() > c.left[j1]


# ---------------------------------------------------------------------------------------------------------- refusals on host memory
_BUF = np.zeros(4096, np.float64)                  # every pointer is HOST memory: a call that got past its checks would launch on it
_PTR = _BUF.ctypes.data
_NULL = None


def refused(ptr=_PTR, **kw):
    """lerf_rr_axis with valid arguments (pointers: `ptr`) except for the overrides"""
    a = dict(inp=ptr, out=ptr, axis=True, w=ptr, left=ptr, row_ptr=ptr, idx=ptr, outer=2, inner=3, n_in=4, n_out=5, taps=2, pad_mode=1,
             in_dtype=F64, acc_dtype=F64, out_dtype=F64)
    assert set(kw) <= set(a), kw
    a.update(kw)
    ax = _lib.RrAxis(a["n_in"], a["n_out"], a["taps"], a["left"], a["row_ptr"], a["idx"], a["w"], a["pad_mode"])
    return _lib.lib().lerf_rr_axis(a["inp"], a["in_dtype"], a["outer"], a["inner"], C.byref(ax) if a["axis"] else None, a["acc_dtype"],
                                   a["out"], a["out_dtype"], None)


HOST_REFUSALS = {
    EINVAL: (dict(inp=_NULL), dict(out=_NULL), dict(axis=False), dict(w=_NULL),
             dict(outer=0), dict(outer=-1), dict(inner=0), dict(inner=-3), dict(n_in=0), dict(n_in=-1), dict(n_out=0), dict(n_out=-2),
             dict(taps=-1), dict(taps=2, left=_NULL), dict(taps=0, row_ptr=_NULL), dict(taps=0, idx=_NULL),
             dict(pad_mode=-1), dict(pad_mode=5), dict(taps=0, pad_mode=5),
             # two at once: the argument checks come before the table-size check
             dict(n_out=1 << 20, taps=1 << 12, inp=_NULL), dict(n_out=1 << 20, taps=1 << 12, pad_mode=5)),
    EUNSUPPORTED: (dict(n_out=1 << 20, taps=1 << 11), dict(n_out=(1 << 31) - 1, taps=2), dict(n_out=1 << 16, taps=1 << 15),
                   dict(n_out=3, taps=(1 << 30))),
}


@pytest.mark.parametrize("code", sorted(HOST_REFUSALS), ids=["EUNSUPPORTED", "EINVAL"])
def test_rr_axis_refuses_before_any_launch(code):
    for case in HOST_REFUSALS[code]:
        assert refused(**case) == code, case
    assert not _BUF.any()


def test_the_largest_table_passes_the_size_check():
    """the table-size check from both sides, as far as host memory allows (a call that passed every check would launch):
    2^31 - 1 entries with a bad pad mode are still LERF_EINVAL, 2^31 entries with valid arguments are LERF_EUNSUPPORTED"""
    assert refused(n_out=(1 << 31) - 1, taps=1, pad_mode=5) == EINVAL
    assert refused(n_out=1 << 30, taps=2) == EUNSUPPORTED
