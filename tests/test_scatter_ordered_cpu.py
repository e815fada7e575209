"""CPU-only: the ORDERED scatter through its host twins -- lerf_splat_ordered_host, lerf_coords_compose_bwd_ordered_host,
lerf_coords_invert_bwd_ordered_host and the scan lerf_scan_exclusive_u32_host.  The ordered twins run the device's four passes serially
(count, scan, fill in DESCENDING entry order, sort and sum), so the sort, the duplicate skip and the cap run here.  Their reference is
the plain host twin of the same operation, and every comparison is made on the raw bits: the order of the sum is defined, so there is
no tolerance to choose.

  1. the exports, the ABI version, the workspace formula;
  2. the scan against numpy.cumsum at its block seams;
  3. the splat forward, every operand variant, special entries, a pre-filled accumulator -- after showing that the test has power;
  4. the adjoints of compose and invert: clamped taps, NaN entries, a pre-filled gradient, each half alone, a batch, both dtypes;
  5. the cap: NaN in exactly the element over it, the header's count, LerfError from the wrapper;
  6. every refusal leaves a sentinel-filled arena untouched, the workspace included.

The cases the GPU suite runs against the plain host twins are built here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import splat_ref as SR
from conftest import REPO
from test_splat_cpu import as_batch, make_case, same_bits

from lerf_pytorch_amd import _lib, coords

EINVAL, EUNSUPPORTED = -1, -2
F32, F64 = _lib.LERF_F32, _lib.LERF_F64
f32, f64 = np.float32, np.float64
NAMES = ("lerf_scatter_ordered_workspace_bytes", "lerf_splat_ordered", "lerf_splat_ordered_host", "lerf_coords_compose_bwd_ordered",
         "lerf_coords_compose_bwd_ordered_host", "lerf_coords_compose_bwd_batched_ordered", "lerf_coords_compose_bwd_batched_ordered_host",
         "lerf_coords_invert_bwd_ordered", "lerf_coords_invert_bwd_ordered_host", "lerf_coords_invert_bwd_batched_ordered",
         "lerf_coords_invert_bwd_batched_ordered_host", "lerf_scan_exclusive_u32", "lerf_scan_exclusive_u32_host",
         "lerf_scan_exclusive_u32_block", "lerf_scan_exclusive_u32_workspace_bytes")
CAP = 4096                     # the cap of every case that is not about the cap: the wrappers' default

# test_splat_cpu's case tuples (source hw, output hw, C, B, per-sample map, T, map dtype, norm plane, weight) at the issue's three
# geometries: a frame larger than the source, 9 100 source pixels into an 8 x 8 patch (contention: segments of several hundred ids,
# far beyond the insertion sort), a single pixel
PATCH = ((70, 130), (8, 8))
SPLAT_CASES = [
    ((23, 31), (29, 37), 1, 0, False, f32, f32, False, False),
    ((23, 31), (29, 37), 3, 3, False, f64, f64, True, True),
    ((23, 31), (29, 37), 3, 3, True, f32, f64, True, False),
    ((23, 31), (29, 37), 1, 3, True, f64, f32, False, True),
    PATCH + (3, 0, False, f32, f32, True, True),
    PATCH + (1, 3, True, f64, f32, False, True),
    PATCH + (3, 3, False, f32, f64, True, False),
    ((1, 1), (1, 1), 1, 0, False, f32, f32, True, False),
    ((1, 1), (1, 1), 3, 3, True, f64, f64, True, True),
]
SPLAT_IDS = ["%dx%d-%dx%d-C%d-B%d%s-%s-%s%s%s" % (c[0] + c[1] + (c[2], c[3], "m" if c[4] else "", c[5].__name__[5:], c[6].__name__[5:],
                                                                "-norm" if c[7] else "", "-w" if c[8] else "")) for c in SPLAT_CASES]
POWER_CASE = SPLAT_CASES[4]


def prefilled(shape, T, seed=9):
    return np.random.default_rng(seed).standard_normal(shape).astype(T)


# ---------------------------------------------------------------------------------------------- the adjoint cases (shared with the GPU suite)
A_HW, B_HW = (7, 9), (11, 13)


def positions(a_hw, hw, seed, spill=2.5):
    """[h, w, 2] float64 positions over an a_hw map and `spill` beyond it on every side (those clamp onto the border cells), with NaN
    entries, integers (one tap), the far corner and +-1e300 on a stride-7 walk"""
    rng = np.random.default_rng(seed)
    P = np.stack([rng.uniform(-spill, a_hw[0] - 1 + spill, hw), rng.uniform(-spill, a_hw[1] - 1 + spill, hw)], -1)
    sp = [(np.nan, 2.0), (3.0, np.nan), (2.0, 3.0), (a_hw[0] - 1.0, a_hw[1] - 1.0), (0.0, 0.0), (-1e300, 1e300), (a_hw[0] + 5.0, -4.0), (1.5, 4.0),
          (-0.0, 8.0), (np.nan, np.nan)]
    flat = P.reshape(-1, 2)
    n = min(len(sp), flat.shape[0] // 7)
    flat[0:7 * n:7] = sp[:n]
    return P


def adjoint_case(B, dt_outer, dt_inner, seed=0):
    """(outer [.., 7, 9, 2], inner [.., 11, 13, 2], upstream [.., 11, 13, 2] float64): B = 0 is the single form.  The outer map is smooth with
    a distinct Jacobian in every cell (the invert adjoint solves with it); NaN sits in one corner of set 0"""
    rng = np.random.default_rng(50 + seed)
    lead = (B,) if B else ()
    i, j = np.meshgrid(np.arange(A_HW[0], dtype=f64), np.arange(A_HW[1], dtype=f64), indexing="ij")
    outs = []
    for s in range(max(B, 1)):
        A = np.stack([1.1 * i + 0.2 * np.sin(0.9 * j + s) + 0.05 * i * j, 0.9 * j + 0.3 * np.cos(0.7 * i + s) - 0.03 * i * j], -1)
        A += 0.01 * rng.standard_normal(A.shape)
        outs.append(A)
    outs[0][4, 6] = np.nan
    outer = (np.stack(outs) if B else outs[0]).astype(dt_outer)
    with np.errstate(over="ignore"):                                # +-1e300 is +-inf in float32
        inner = (np.stack([positions(A_HW, B_HW, 70 + seed + s) for s in range(B)]) if B else positions(A_HW, B_HW, 70 + seed)).astype(dt_inner)
    g = rng.standard_normal(lead + B_HW + (2,))
    return outer, inner, g


ADJ_CASES = [(0, f64, f64), (0, f32, f64), (0, f64, f32), (3, f64, f64), (3, f32, f32)]
ADJ_IDS = ["B%d-%s-%s" % (b, a.__name__, c.__name__) for b, a, c in ADJ_CASES]


# ---------------------------------------------------------------------------------------------- 1. exports, the workspace
def test_exports_and_abi_version():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "lerf_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lerf_[a-z0-9_]+)\s*\(", src))
    for n in NAMES:
        assert n in declared and n in _lib.EXPORTS and hasattr(_lib.lib(), n), n
    assert _lib.lib().lerf_abi_version() == 7
    assert re.search(r"#define\s+LERF_ORDERED_MAX_COUNT_OFFSET\s+4\b", src) and _lib.ORDERED_MAX_COUNT_OFFSET == 4


def formula(n_entries, n_targets, n_sets):
    """the documented layout: uint32 words -- header [4], cursor [sets][targets], list [sets][4 entries], partials [sets][P(targets)]"""
    B, n, P = _lib.scan_block(), n_targets, 0
    while n > B:
        n = (n + B - 1) // B
        P += n
    return 4 * (4 + n_sets * (n_targets + 4 * n_entries + P))


def test_workspace_bytes_follow_the_documented_formula():
    B = _lib.scan_block()
    assert B >= 64 and B & (B - 1) == 0
    for ne, nt, ns in [(1, 1, 1), (9100, 64, 3), (143, 63, 1), (5, B, 2), (5, B + 1, 2), (7, B * B, 1), (7, B * B + 1, 3), (2 ** 30 - 1, 2 ** 32 - 1, 2),
                       (1920 * 1080, 1920 * 1080, 8)]:
        assert _lib.ordered_workspace_bytes(ne, nt, ns) == formula(ne, nt, ns) == _lib.ordered_workspace_formula(ne, nt, ns), (ne, nt, ns)
    for ne, nt, ns in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 65536), (2 ** 30, 1, 1), (1, 2 ** 32, 1), (-1, 1, 1)]:
        assert _lib.ordered_workspace_bytes(ne, nt, ns) == 0, (ne, nt, ns)


# ---------------------------------------------------------------------------------------------- 2. the scan
def scan_lengths():
    B = _lib.scan_block()
    return [1, B - 1, B, B + 1, B * B + 1]


def scan_input(n, seed=0):
    """counts like the scatter's (mostly 0 .. 8) with a few large ones; from B + 1 elements on they sum past 2^16"""
    rng = np.random.default_rng(seed + n)
    v = rng.integers(0, 9, n).astype(np.uint32)
    v[rng.integers(0, n, max(1, n // 97))] = 70000
    return v


def scan_ref(v):
    return (np.cumsum(v.astype(np.uint64)) - v).astype(np.uint64) & 0xffffffff


@pytest.mark.parametrize("k", range(5))
def test_scan_against_cumsum(k):
    n = scan_lengths()[k]
    v = scan_input(n)
    assert n == 1 or int(v.astype(np.uint64).sum()) > 2 ** 16
    got = _lib.scan_exclusive_u32_host(v.copy())
    assert got.dtype == np.uint32 and np.array_equal(got.astype(np.uint64), scan_ref(v))


def test_scan_wraps_modulo_2_32_and_refuses():
    v = np.full(5, 0xc0000000, np.uint32)
    assert np.array_equal(_lib.scan_exclusive_u32_host(v.copy()).astype(np.uint64), scan_ref(v))
    L = _lib.lib()
    a = np.zeros(4, np.uint32)
    assert L.lerf_scan_exclusive_u32_host(None, 4) == EINVAL and L.lerf_scan_exclusive_u32_host(a.ctypes.data, 0) == EINVAL
    assert L.lerf_scan_exclusive_u32_host(a.ctypes.data + 2, 1) == EINVAL and L.lerf_scan_exclusive_u32_host(a.ctypes.data, 2 ** 32) == EINVAL
    B = _lib.scan_block()
    assert L.lerf_scan_exclusive_u32_workspace_bytes(B) == 0 and L.lerf_scan_exclusive_u32_workspace_bytes(B + 1) == 8
    assert L.lerf_scan_exclusive_u32_workspace_bytes(B * B + 1) == 4 * (B + 1 + 2)
    with pytest.raises(ValueError):
        _lib.scan_exclusive_u32_host(np.zeros(4, np.int32))


# ---------------------------------------------------------------------------------------------- 3. the splat forward
def test_the_bit_comparison_has_power_and_the_cap_is_clear():
    """on the contention case (9 100 float32 source pixels into 8 x 8): summing one element's terms in REVERSED order changes its bits, so
    equal bits do show the order; and the longest segment is below the cap the cases use"""
    X, F, M = make_case(POWER_CASE)
    assert X.dtype == f32 and POWER_CASE[:2] == ((70, 130), (8, 8))
    _, n, _ = SR.splat(*as_batch(X, F, M), (8, 8), True)
    most = int(n.max())
    print("largest n[q] = %d, cap %d" % (most, CAP))
    assert 16 < most < CAP
    finite, on, inside, w, q, _, _ = SR._taps(F, 8, 8)
    k, target = 0, int(np.argmax(n[0, 0]))
    wm = w * M.astype(f64)[..., None]
    term = (wm * X[k].astype(f64)[..., None]).astype(f32).reshape(-1)
    mine = term[on.reshape(-1) & (q.reshape(-1) == target)]
    assert mine.size == most
    fwd = rev = f32(0.0)
    for v in mine:
        fwd = f32(fwd + v)
    for v in mine[::-1]:
        rev = f32(rev + v)
    assert fwd.tobytes() == _lib.splat_host(X, F, (8, 8), M, True)[k].reshape(-1)[target].tobytes()
    assert fwd.tobytes() != rev.tobytes()


@pytest.mark.parametrize("case", SPLAT_CASES, ids=SPLAT_IDS)
def test_splat_ordered_host_is_the_host_twin_bit_for_bit(case):
    X, F, M = make_case(case)
    ohw, norm = case[1], case[7]
    keep = [a.copy() for a in (X, F)]
    ref = _lib.splat_host(X, F, ohw, M, norm)
    got = _lib.splat_ordered_host(X, F, ohw, M, norm, max_adders=CAP)
    assert same_bits(got, ref) and np.isfinite(ref).all() and np.any(ref != 0)
    assert same_bits(X, keep[0]) and same_bits(F, keep[1])
    # a pre-filled accumulator: the running value starts from what the caller left
    base = prefilled(ref.shape, ref.dtype)
    ref2 = _lib.splat_host(X, F, ohw, M, norm, acc=base.copy())
    got2 = _lib.splat_ordered_host(X, F, ohw, M, norm, acc=base.copy(), max_adders=CAP)
    assert same_bits(got2, ref2) and not same_bits(ref2, ref)


def test_coords_splat_accepts_the_flag_on_numpy():
    X, F, M = make_case(SPLAT_CASES[1])
    a = coords.splat(X, F, (29, 37), M, mode="linear")
    b = coords.splat(X, F, (29, 37), M, mode="linear", deterministic=True, max_adders=3)
    assert same_bits(a, b)


# ---------------------------------------------------------------------------------------------- 4. the adjoints
@pytest.mark.parametrize("case", ADJ_CASES, ids=ADJ_IDS)
def test_compose_bwd_ordered_host_is_the_host_twin_bit_for_bit(case):
    outer, inner, g = adjoint_case(*case)
    base_a, base_b = prefilled(outer.shape, f64, 11), prefilled(inner.shape, f64, 12)
    for need in ((True, True), (True, False), (False, True)):
        ra, rb = _lib.coords_compose_bwd_host(outer, inner, g, base_a.copy() if need[0] else None, base_b.copy() if need[1] else None, need)
        ga, gb = _lib.coords_compose_bwd_ordered_host(outer, inner, g, base_a.copy() if need[0] else None, base_b.copy() if need[1] else None,
                                                       need, max_adders=CAP)
        for got, ref, base in ((ga, ra, base_a), (gb, rb, base_b)):
            assert (got is None) == (ref is None)
            if ref is not None:
                assert same_bits(got, ref) and not same_bits(ref, base)
    # entries outside the outer map were there: their taps clamp onto the border cells
    r, c = inner[..., 0].astype(f64), inner[..., 1].astype(f64)
    assert np.any(r < 0) and np.any(r > A_HW[0] - 1) and np.any(c < 0) and np.any(c > A_HW[1] - 1) and np.isnan(r).any()


@pytest.mark.parametrize("case", ADJ_CASES, ids=ADJ_IDS)
def test_invert_bwd_ordered_host_is_the_host_twin_bit_for_bit(case):
    fmap, inverse, g = adjoint_case(*case)
    base = prefilled(fmap.shape, f64, 13)
    ref = _lib.coords_invert_bwd_host(fmap, inverse, g, base.copy())
    got = _lib.coords_invert_bwd_ordered_host(fmap, inverse, g, base.copy(), max_adders=CAP)
    assert same_bits(got, ref) and not same_bits(ref, base)
    changed = (ref != base) | (np.isnan(ref) != np.isnan(base))
    assert changed.mean() > 0.5                      # the solve went through for most cells (the NaN corner's four are skipped)


def test_a_shared_outer_map_in_a_batch_sums_its_sets_in_order():
    outer, inner, g = adjoint_case(3, f64, f64)
    shared = np.ascontiguousarray(outer[1])
    base = prefilled(shared.shape, f64, 14)
    ga, gb = _lib.coords_compose_bwd_ordered_host(shared, inner, g, base.copy(), None, (True, True), max_adders=CAP)
    want = base.copy()
    for s in range(3):
        want += _lib.coords_compose_bwd_host(shared, inner[s], g[s], None, None, (True, False))[0]
    assert same_bits(ga, want)
    assert same_bits(gb, _lib.coords_compose_bwd_host(shared, inner, g, None, None, (False, True))[1])


# ---------------------------------------------------------------------------------------------- 5. the cap
def cap_case(T=f32):
    """3 x 4 source pixels: nine land on output pixel (2, 3) exactly (one tap each), three at fractional positions elsewhere"""
    X = np.random.default_rng(5).standard_normal((2, 3, 4)).astype(T)
    F = np.empty((3, 4, 2), f64)
    F[...] = (2.0, 3.0)
    F[0, 0], F[1, 2], F[2, 3] = (0.25, 0.5), (3.5, 1.25), (1.75, 4.5)
    return X, F


def raw_splat_ordered_host(X, F, acc, norm, ws, max_adders):
    Cn, H, W = X.shape
    oH, oW = acc.shape[-2:]
    return _lib.lib().lerf_splat_ordered_host(X.ctypes.data, _lib.LERF_F32 if X.dtype == f32 else F64, Cn, H, W, 0, F.ctypes.data, F64, 2 * W, 0, None,
                                              0, acc.ctypes.data, int(norm), oH, oW, 0, 1, ws.ctypes.data, ws.nbytes, max_adders)


@pytest.mark.parametrize("T", [f32, f64])
def test_the_cap_poisons_exactly_the_element_over_it(T):
    X, F = cap_case(T)
    ohw = (5, 6)
    ref = _lib.splat_host(X, F, ohw, None, True)
    ws = np.full(_lib.ordered_workspace_bytes(12, 30, 1), 0xa5, np.uint8)
    for cap, over in ((4, True), (8, True), (9, False)):
        acc = np.zeros((3,) + ohw, T)
        assert raw_splat_ordered_host(X, F, acc, True, ws, cap) == 0
        header = ws[:16].view(np.uint32)
        assert header[1] == 9 and header[0] == 0 and header[2] == 0 and header[3] == 0
        mask = np.zeros(acc.shape, bool)
        mask[:, 2, 3] = over
        assert np.isnan(acc[mask]).all() and mask.sum() == (3 if over else 0)
        assert np.array_equal(acc[~mask].view(np.uint32 if T == f32 else np.uint64), ref[~mask].view(np.uint32 if T == f32 else np.uint64))
    with pytest.raises(_lib.LerfError, match=r"9 .*max_adders = 4"):
        _lib.splat_ordered_host(X, F, ohw, None, True, max_adders=4)
    assert same_bits(_lib.splat_ordered_host(X, F, ohw, None, True, max_adders=9), ref)
    with pytest.raises(ValueError, match="max_adders"):
        _lib.splat_ordered_host(X, F, ohw, None, True, max_adders=0)


def test_the_cap_on_the_adjoints():
    outer, _, _ = adjoint_case(0, f64, f64)
    inner = np.empty((3, 4, 2))
    inner[...] = (2.0, 3.0)
    inner[0, 0], inner[1, 2], inner[2, 3] = (0.25, 0.5), (3.5, 1.25), (5.75, 7.5)
    g = np.random.default_rng(6).standard_normal((3, 4, 2))
    ra, _ = _lib.coords_compose_bwd_host(outer, inner, g, None, None, (True, False))
    rf = _lib.coords_invert_bwd_host(outer, inner, g)
    for name, ref, extra in (("lerf_coords_compose_bwd_ordered_host", ra, (None,)), ("lerf_coords_invert_bwd_ordered_host", rf, ())):
        ws = np.full(_lib.ordered_workspace_bytes(12, 63, 1), 0x5a, np.uint8)
        grad = np.zeros(outer.shape)
        rc = getattr(_lib.lib(), name)(outer.ctypes.data, F64, 2 * A_HW[1], A_HW[0], A_HW[1], inner.ctypes.data, F64, 8, g.ctypes.data, 3, 4,
                                       grad.ctypes.data, *extra, ws.ctypes.data, ws.nbytes, 4)
        assert rc == 0 and ws[:16].view(np.uint32)[1] == 9
        mask = np.zeros(grad.shape, bool)
        mask[2, 3] = True
        assert np.isnan(grad[mask]).all() and np.array_equal(grad[~mask].view(np.uint64), ref[~mask].view(np.uint64))
    with pytest.raises(_lib.LerfError, match="max_adders"):
        _lib.coords_compose_bwd_ordered_host(outer, inner, g, None, None, (True, False), max_adders=8)
    with pytest.raises(_lib.LerfError, match="max_adders"):
        _lib.coords_invert_bwd_ordered_host(outer, inner, g, max_adders=8)


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_every_refusal_leaves_the_arena_untouched():
    L = _lib.lib()
    Cn, H, W, oH, oW, B = 2, 3, 4, 5, 6, 2
    n, on = H * W, oH * oW
    arena = np.full(8192, -7.0)
    base = arena.ctypes.data
    assert base % 16 == 0
    X, F, M, ACC, WS = (base + 8 * k for k in (0, 256, 512, 768, 2048))
    need = _lib.ordered_workspace_bytes(n, on, B)
    assert 0 < need <= 8 * 2048

    def fwd(x=X, f=F, fset=2 * n, m=M, acc=ACC, aset=(Cn + 1) * on, n_sets=B, h=H, w=W, oh=oH, ow=oW, ws=WS, wsb=need, cap=16):
        return L.lerf_splat_ordered_host(x, F64, Cn, h, w, Cn * n, f, F64, 2 * w, fset, m, n, acc, 1, oh, ow, aset, n_sets, ws, wsb, cap)

    for kw in [dict(ws=None), dict(ws=WS + 2), dict(wsb=need - 1), dict(wsb=0), dict(cap=0), dict(cap=-3), dict(ws=X), dict(ws=F), dict(ws=M), dict(ws=ACC),
               dict(ws=F - need + 8), dict(ws=ACC + 8 * (B * (Cn + 1) * on) - 4), dict(aset=0), dict(acc=None), dict(x=None), dict(n_sets=0),
               dict(oh=0), dict(acc=X)]:
        assert fwd(**kw) == EINVAL, kw
    # sizes the 32-bit ids cannot hold are judged before the pointers: nothing is read, nothing is written
    for kw in [dict(h=32768, w=32768), dict(oh=65536, ow=65536), dict(h=2 ** 15, w=2 ** 15, x=None)]:
        assert fwd(**kw) == EUNSUPPORTED, kw
    assert fwd(n_sets=65536) == EINVAL             # the splat's rule for n_sets beyond the grid

    # the adjoints: outer / f [B][4][5][2], inner / inverse and grad_out [B][3][4][2], grad_a [B][4][5][2], grad_b [B][3][4][2]
    aH, aW = 4, 5
    A, Bm, G, GA, GB = (base + 8 * k for k in (0, 256, 512, 768, 1024))
    na, nb = 2 * aH * aW, 2 * H * W
    need2 = _lib.ordered_workspace_bytes(H * W, aH * aW, B)

    def cbwd(a=A, aset=na, b=Bm, g=G, ga=GA, gb=GB, gaset=na, n_sets=B, ah=aH, aw=aW, oh=H, ow=W, ws=WS, wsb=need2, cap=16):
        return L.lerf_coords_compose_bwd_batched_ordered_host(a, F64, 2 * aw, ah, aw, b, F64, 2 * ow, g, oh, ow, ga, gb, n_sets, aset, nb, nb, gaset, nb,
                                                              ws, wsb, cap)

    def ibwd(f=A, b=Bm, g=G, gf=GA, gfset=na, n_sets=B, fh=aH, fw=aW, oh=H, ow=W, ws=WS, wsb=need2, cap=16):
        return L.lerf_coords_invert_bwd_batched_ordered_host(f, F64, 2 * fw, fh, fw, b, F64, 2 * ow, g, oh, ow, gf, n_sets, na, nb, nb, gfset, ws, wsb, cap)

    for kw in [dict(ws=None), dict(ws=WS + 2), dict(wsb=need2 - 1), dict(cap=0), dict(ws=A), dict(ws=Bm), dict(ws=G), dict(ws=GA), dict(ws=GB),
               dict(ws=GB + 8 * B * nb - 4), dict(gaset=0), dict(gaset=0, aset=0), dict(ga=None, gb=None), dict(a=None), dict(ah=1)]:
        assert cbwd(**kw) == EINVAL, kw
    for kw in [dict(ws=None), dict(ws=WS + 2), dict(wsb=need2 - 1), dict(cap=0), dict(ws=A), dict(ws=Bm), dict(ws=G), dict(ws=GA), dict(ws=GA + 8 * B * na - 4),
               dict(gfset=0), dict(gf=None), dict(fh=1)]:
        assert ibwd(**kw) == EINVAL, kw
    for fn in (cbwd, ibwd):
        assert fn(oh=32768, ow=32768) == EUNSUPPORTED and fn(**({"ah": 65536, "aw": 65536} if fn is cbwd else {"fh": 65536, "fw": 65536})) == EUNSUPPORTED
        assert fn(n_sets=65536) == EUNSUPPORTED
    assert (arena == -7.0).all()

    # the same arena takes the good calls, and they stay inside their operands and the workspace's stated bytes
    arena[:768] = 0.5
    arena[256:256 + 2 * B * n] = 1.25              # the splat's map: positions inside the 5 x 6 frame
    arena[768:2048] = 0.0
    assert fwd() == 0 and fwd(fset=0) == 0 and fwd(m=None) == 0 and fwd(n_sets=1, aset=0) == 0
    assert (arena[768 + B * (Cn + 1) * on:2048] == 0.0).all() and (arena[2048 + (need + 7) // 8:] == -7.0).all()
    arena[768:2048] = 0.0
    assert cbwd() == 0 and cbwd(gb=None) == 0 and cbwd(ga=None) == 0 and cbwd(aset=0) == 0 and ibwd() == 0 and ibwd(n_sets=1, gfset=0) == 0
    assert (arena[768 + B * aH * aW * 2:1024] == 0.0).all() and (arena[1024 + B * H * W * 2:2048] == 0.0).all()
    assert (arena[2048 + (max(need, need2) + 7) // 8:] == -7.0).all()
