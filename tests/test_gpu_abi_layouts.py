"""The C ABI's strided operand contract (include/lerf_hip.h): every entry point that takes lerf_plane_t / lerf_mplane_t
descriptors, driven through ctypes with hand-built descriptors -- padded rows, column strides, interleaved results, negative
strides, reversed channel planes, transposed planes, odd element offsets -- against the oracle.

Every result plane lives in a guard-banded buffer: one flat allocation filled with a sentinel bit pattern, the descriptor's
origin placed so that the lattice it names sits between two guard bands at least as long as the lattice's whole extent.
After the call the buffer comes back whole and two things are checked: (a) the elements on the lattice equal the expected
result, (b) every other element -- the gaps between strided elements and both guard bands -- still holds the sentinel, byte
for byte.  A kernel that writes one stride off lands in the test's own allocation, and the test says so.

Tolerances are those of tests/test_gpu_parity.py: integer results and uint8 bytes exact (uint8 stage-3 results of the
fixed kernels: exact except within 1e-3 of a rounding tie, there <= 1), float64 results <= 1e-9, float32 results
<= 5e-4 where the kernel's arithmetic is float64 and <= 2.55e-2 where it is float32 (lerf_warp_packed)."""
import ctypes as C
import functools

import numpy as np
import pytest

gpu = pytest.mark.gpu

LERF_EUNSUPPORTED = -2
ACC, LDS, DIRECT, TILE64, TILE32, LUT_PLANAR = 1, 2, 4, 8, 16, 32      # LERF_INTERP_*
LUT_PLANE_BYTES = 83584
F32_TOL = 2.55e-2
F32_OBSERVED = 5e-4

SENTINEL = {
    np.dtype(np.uint8): bytes([0xA5]),
    np.dtype(np.int16): bytes([0xA5, 0x5A]),
    np.dtype(np.float32): np.array([0x7FC5A5A5], "<u4").tobytes(),               # a quiet NaN with a payload
    np.dtype(np.float64): np.array([0x7FF8A5A5A5A5A5A5], "<u8").tobytes(),
}
LERF_DTYPE = {np.dtype(np.uint8): 0, np.dtype(np.float32): 1, np.dtype(np.float64): 2, np.dtype(np.int16): 3}


# ----------------------------------------------------------------------------------------------------- the guard-band helper
def lattice(base, shape, strides):
    """element indices of the lattice a descriptor names: base + sum_d i_d * strides[d], shaped like `shape`"""
    idx = np.full(shape, base, dtype=np.int64)
    for d, (n, s) in enumerate(zip(shape, strides)):
        ax = [1] * len(shape)
        ax[d] = n
        idx += (np.arange(n, dtype=np.int64) * s).reshape(ax)
    return idx


def extent(shape, strides):
    """(lowest, highest) element offset of the lattice relative to its origin"""
    lo = sum(min(0, (n - 1) * s) for n, s in zip(shape, strides))
    hi = sum(max(0, (n - 1) * s) for n, s in zip(shape, strides))
    return lo, hi


def guarded_layout(shape, strides, shift=0):
    """(size, base) of a flat buffer for the lattice: its origin at element `base`, a guard band of at least the lattice's
    whole extent below its lowest and above its highest element; `shift` moves the origin (odd element offsets)"""
    lo, hi = extent(shape, strides)
    span = hi - lo + 1
    base = span + shift - lo
    return base + hi + 1 + span, base


def sentinel_fill(dtype, size):
    dt = np.dtype(dtype)
    return np.frombuffer(SENTINEL[dt] * size, dtype=dt).copy()


def exact(got, want):
    if got.dtype.kind == "f":
        return (got == want) | (np.isnan(got) & np.isnan(want))
    return got == want


def within(tol):
    def cmp(got, want):
        return (np.abs(got.astype(np.float64) - want) <= tol) | (np.isnan(got) & np.isnan(want))
    return cmp


def bytes_of(ref):
    """uint8 outputs of a float64 oracle result: to_u8(nan_to_num(ref)) exactly, or <= 1 off within 1e-3 of a rounding tie"""
    ref = np.nan_to_num(ref, nan=0.0)
    want = np.clip(np.round(ref), 0, 255)
    near_tie = np.abs(ref - np.floor(ref) - 0.5) < 1e-3

    def cmp(got, _want):
        d = np.abs(got.astype(np.int64) - want)
        return (d == 0) | (near_tie & (d <= 1))
    return want.astype(np.uint8), cmp


def guard_problems(buf, base, shape, strides, want, equal=exact):
    """What is wrong with the flat buffer `buf` after a call that should have written `want` onto the lattice (base, shape,
    strides) and nothing else; want = None: the call should have written nothing.  Returns a list of findings (empty = right)."""
    idx = lattice(base, shape, strides)
    if np.unique(idx).size != idx.size:
        raise ValueError("the descriptor names some element twice")
    found = []
    other = np.ones(buf.size, dtype=bool)
    if want is not None:
        got = buf[idx]
        bad = ~equal(got, np.asarray(want))
        if bad.any():
            first = tuple(int(v[0]) for v in np.nonzero(bad))
            found.append("%d of %d lattice elements differ from the expected result (first at %s: got %r, want %r)"
                         % (int(bad.sum()), bad.size, first, got[first], np.asarray(want)[first]))
        other[idx.ravel()] = False
    sent = np.frombuffer(SENTINEL[buf.dtype], dtype=np.uint8)
    raw = buf.view(np.uint8).reshape(buf.size, buf.dtype.itemsize)
    stray = np.nonzero(other & (raw != sent).any(axis=1))[0]
    if stray.size:
        lo, hi = extent(shape, strides)
        e = int(stray[0]) - base
        found.append("%d elements the descriptor does not name were written (first at offset %+d from the origin, %s)"
                     % (stray.size, e, "between lattice elements" if lo <= e <= hi else "in a guard band"))
    return found


class Guarded:
    """A device buffer laid out by guarded_layout for one lattice (shape, strides in elements), sentinel-filled; `pre` fills
    the lattice first (accumulate calls)."""

    def __init__(self, torch, dtype, shape, strides, shift=0, pre=None):
        self.dtype, self.shape, self.strides = np.dtype(dtype), tuple(shape), tuple(strides)
        size, self.base = guarded_layout(self.shape, self.strides, shift)
        host = sentinel_fill(self.dtype, size)
        if pre is not None:
            host[lattice(self.base, self.shape, self.strides)] = pre
        self.t = torch.from_numpy(host.view(np.uint8)).cuda()
        self.ptr = self.t.data_ptr() + self.base * self.dtype.itemsize

    def plane(self, sy, sx, sc):
        from lerf_pytorch_amd import _lib
        return _lib.Plane(self.ptr, LERF_DTYPE[self.dtype], int(sy), int(sx), int(sc))

    def problems(self, want, equal=exact):
        buf = self.t.cpu().numpy().view(self.dtype)                 # .cpu() waits for the stream
        return guard_problems(buf, self.base, self.shape, self.strides, want, equal)

    def expect(self, want, equal=exact, what=""):
        """assert (a) and (b) of the module docstring; the failure names every finding"""
        found = self.problems(want, equal)
        assert not found, "%s strides %s: %s" % (what, self.strides, "; ".join(found))


def strided_copy(arr, flip=(), pad=None):
    """The memory image of the logical array `arr` in which the axes in `flip` run backwards and axis pad[0] has pad[1]
    extra elements of stride.  Returns (flat array, element offset of arr[0, ..., 0], element strides of the logical axes)."""
    mem = np.flip(arr, axis=tuple(flip)) if flip else arr
    strides = [int(np.prod(mem.shape[d + 1:])) for d in range(mem.ndim)]
    if pad is not None:
        ax, extra = pad
        inner = strides[ax]
        big = np.zeros(mem.shape[:ax + 1] + (inner + extra,), dtype=mem.dtype)
        big[..., :inner] = mem.reshape(mem.shape[:ax + 1] + (inner,))
        for d in range(ax + 1):
            strides[d] = int(np.prod(big.shape[d + 1:]))
        flat = big.ravel()
    else:
        flat = np.ascontiguousarray(mem).ravel()
    origin = 0
    for d in flip:
        origin += (arr.shape[d] - 1) * strides[d]
        strides[d] = -strides[d]
    return flat, origin, strides


def strided_input(torch, arr, flip=(), pad=None):
    """strided_copy on the device: (tensor to keep alive, address of arr[0, ..., 0], element strides)"""
    flat, origin, strides = strided_copy(arr, flip, pad)
    t = torch.from_numpy(flat).cuda()
    return t, t.data_ptr() + origin * flat.itemsize, strides


def out_layouts(P, h, w):
    """(strides (sc, sy, sx), origin shift) of P result planes of h x w positions, by name"""
    return {
        "contiguous": ((h * w, w, 1), 0),
        "padded_rows": ((h * (w + 7), w + 7, 1), 0),
        "col_stride2": ((2 * h * w, 2 * w, 2), 0),
        "hwc": ((1, w * P, P), 0),                                  # interleaved, sc = 1
        "hwc_pitched": ((2, w * (2 * P + 1) + 5, 2 * P + 1), 0),    # interleaved with gaps, sc = 2
        "flip_x": ((h * w, w, -1), 0),
        "flip_y": ((h * w, -w, 1), 0),
        "rev_planes": ((-h * w, w, 1), 0),
        "transposed": ((w * (h + 3), 1, h + 3), 0),
        "transposed_flip": ((w * (h + 3), -1, -(h + 3)), 0),
        "odd_offset": ((h * w, w, 1), 1),
    }


LAYOUTS = list(out_layouts(3, 5, 7))


def pairable(strides):
    """the LDS kernel stores a lane's two positions as one pair: it covers planes contiguous along x or y"""
    _, sy, sx = strides
    return abs(sy) == 1 or abs(sx) == 1


# ------------------------------------------------------------------------------------------------ the helper is tested too
def test_guard_checker_reports_stray_writes():
    shape, strides = (3, 5, 7), (1, 7 * 3 + 4, -3)
    size, base = guarded_layout(shape, strides)
    lo, hi = extent(shape, strides)
    assert base + lo >= hi - lo + 1 and size - 1 - (base + hi) >= hi - lo + 1        # a whole extent of guard on each side
    rng = np.random.default_rng(0)
    for dtype in (np.uint8, np.int16, np.float32, np.float64):
        want = rng.integers(0, 100, shape).astype(dtype)
        buf = sentinel_fill(dtype, size)
        idx = lattice(base, shape, strides)
        assert guard_problems(buf, base, shape, strides, None) == []
        buf[idx] = want
        assert guard_problems(buf, base, shape, strides, want) == []
        assert len(guard_problems(buf, base, shape, strides, None)) == 1              # written although nothing was due

        def hit(where, value):
            b = buf.copy()
            b[where] = value
            return guard_problems(b, base, shape, strides, want)

        named = set(idx.ravel().tolist())
        gap = next(e for e in range(base + lo, base + hi) if e not in named)          # between two lattice elements
        for where, kind in ((gap, "between"), (0, "guard"), (size - 1, "guard"), (base + hi + 1, "guard"),
                            (base + lo - 1, "guard")):
            p = hit(where, 7)
            assert len(p) == 1 and kind in p[0], (dtype, where, p)
        p = hit(tuple(idx[2, 4, 6].reshape(1)), 101)                                  # a wrong value on the lattice
        assert len(p) == 1 and "lattice elements differ" in p[0]
        if np.dtype(dtype).kind == "f":
            p = hit(gap, np.nan)                                                     # a NaN of another payload is a write
            assert len(p) == 1 and "between" in p[0]
            w2 = want.copy()
            w2[1, 2, 3] = np.nan
            b = buf.copy()
            b[idx[1, 2, 3]] = np.nan
            assert guard_problems(b, base, shape, strides, w2) == []                # NaN expected and found
    # shift: an odd origin still keeps the guard
    size2, base2 = guarded_layout((2, 3), (3, 1), shift=1)
    assert base2 == 7 and size2 == base2 + 5 + 1 + 6


def test_strided_copy_addresses_the_logical_array():
    arr = np.random.default_rng(1).integers(0, 255, (3, 4, 5)).astype(np.uint8)
    for flip, pad in (((), None), ((2,), None), ((1,), (1, 3)), ((0, 2), (0, 2)), ((0, 1, 2), (1, 7))):
        flat, origin, strides = strided_copy(arr, flip, pad)
        assert np.array_equal(flat[lattice(origin, arr.shape, strides)], arr), (flip, pad)
        for d in range(3):
            assert (strides[d] < 0) == (d in flip)
        if pad is not None:
            assert abs(strides[pad[0]]) == int(np.prod(arr.shape[pad[0] + 1:])) + pad[1]


# ------------------------------------------------------------------------------------------------------------- GPU fixtures
@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


@pytest.fixture(scope="module")
def lib(torch):
    from lerf_pytorch_amd import _lib
    return _lib


def _stream():
    from lerf_pytorch_amd import _lib
    return _lib.current_stream()


# ----------------------------------------------------------------------------------------------------------- lerf_lut_interp
# (C, oC, (h, w), mode, rotation): odd and even sizes, partial LDS tiles (128 along the lane axis, 32 / 16 across)
INTERP_COMBOS = [(1, 1, (37, 133), "c", 1), (3, 3, (34, 130), "t", 2), (4, 1, (34, 133), "s", 3),
                 (4, 3, (37, 130), "y", 0), (3, 1, (37, 133), "d", 1), (1, 3, (34, 130), "c", 0)]
INTERP_FLAGS = {"auto": 0, "lds": LDS, "direct": DIRECT, "acc": ACC, "acc_lds": ACC | LDS, "acc_direct": ACC | DIRECT,
                "lds_tile64": LDS | TILE64, "lds_tile32": LDS | TILE32, "lds_planar": LDS | LUT_PLANAR}
OUT_NP = {"i16": np.int16, "f32": np.float32, "f64": np.float64}


@functools.lru_cache(maxsize=None)
def _interp_case(C_, oC, h, w, mode, rot, interval=4, seed=0):
    """(image [C, h+3, w+3] uint8, LUT int8 [L^4, oC], numerators int64 [C*oC, h, w]) from the oracle"""
    from oracle import lerf_oracle as O
    import os
    rng = np.random.default_rng(seed + 7919 * C_ + 31 * oC + h * 1000 + w)
    img = rng.integers(0, 256, (C_, h + 3, w + 3), dtype=np.uint8)
    if interval == 4:
        arrays = O.load_luts(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                          "lerf-pytorch_amd", "assets", "models", "lerf-g"))
        lut = np.ascontiguousarray(arrays["s2_cr1" if oC == 3 else "s1_tr0"].reshape(-1, oC).astype(np.int8))
    else:
        L = 2 ** (8 - interval) + 1
        lut = rng.integers(-128, 128, (L ** 4, oC), dtype=np.int64).astype(np.int8)
    num = O.lut_interp_numer(lut, img.transpose(1, 2, 0), mode, rot, interval)[:h, :w]          # [h, w, C, oC]
    return img, lut, np.ascontiguousarray(num.transpose(2, 3, 0, 1).reshape(C_ * oC, h, w)).astype(np.int64)


def _values(num, out_dt, interval=4):
    return num.astype(np.int16) if out_dt == "i16" else (num / float(2 ** interval)).astype(OUT_NP[out_dt])


def _interp(lib, torch, img_desc, img_hw, C_, h, w, mode, rot, lut_t, oC, interval, out_plane, flags, ex=True):
    dy, dx = lib.mode_offsets(mode, rot)
    L = lib.lib()
    if not ex:
        return L.lerf_lut_interp(C.byref(img_desc), img_hw[0], img_hw[1], C_, h, w, dy.ctypes.data, dx.ctypes.data,
                                 lut_t.data_ptr(), oC, interval, C.byref(out_plane), _stream())
    return L.lerf_lut_interp_ex(C.byref(img_desc), img_hw[0], img_hw[1], C_, h, w, dy.ctypes.data, dx.ctypes.data,
                                lut_t.data_ptr(), oC, interval, C.byref(out_plane), flags, _stream())


def _lut_device(torch, lut, planar):
    if not planar:
        return torch.from_numpy(lut).cuda()
    planes = np.zeros((lut.shape[1], LUT_PLANE_BYTES), dtype=np.int8)
    planes[:, :lut.shape[0]] = lut.T
    return torch.from_numpy(planes).cuda()


@gpu
@pytest.mark.parametrize("flags", list(INTERP_FLAGS))
@pytest.mark.parametrize("out_dt", list(OUT_NP))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_lut_interp_out_layouts(torch, lib, layout, out_dt, flags):
    """every output layout x out dtype x flag set: the lattice holds the oracle's result (plus the pre-filled values for
    the accumulate form), nothing else is touched; the LDS kernel, when insisted on, refuses planes that are contiguous
    along neither axis and then writes nothing"""
    fl = INTERP_FLAGS[flags]
    for C_, oC, (h, w), mode, rot in INTERP_COMBOS:
        img, lut, num = _interp_case(C_, oC, h, w, mode, rot)
        P = C_ * oC
        strides, shift = out_layouts(P, h, w)[layout]
        want = _values(num, out_dt)
        rng = np.random.default_rng(h + w + P)
        pre = None
        if fl & ACC:
            pre = _values(rng.integers(-900, 900, num.shape), out_dt)
            want = (pre.astype(np.float64) + want).astype(OUT_NP[out_dt])
        out = Guarded(torch, OUT_NP[out_dt], (P, h, w), strides, shift, pre)
        x = torch.from_numpy(img).cuda()
        src = lib.Plane(x.data_ptr(), 0, img.shape[2], 1, img.shape[1] * img.shape[2])
        lut_t = _lut_device(torch, lut, fl & LUT_PLANAR)
        rc = _interp(lib, torch, src, img.shape[1:], C_, h, w, mode, rot, lut_t, oC, 4, out.plane(strides[1], strides[2], strides[0]),
                     fl, ex=fl != 0)
        tag = (C_, oC, h, w, mode, rot)
        if (fl & LDS) and not pairable(strides):
            assert rc == LERF_EUNSUPPORTED, tag
            out.expect(pre, what=repr(tag))                      # refused: the planes keep what they held
            continue
        assert rc == 0, (tag, rc)
        out.expect(want, what=repr(tag))


@gpu
@pytest.mark.parametrize("layout", ["hwc", "hwc_pitched", "col_stride2", "contiguous", "transposed_flip", "flip_y"])
@pytest.mark.parametrize("acc", [False, True])
def test_lut_interp_default_path_large(torch, lib, layout, acc):
    """>= 65 536 positions and no flags: the launch the library sends to the LDS kernel when the output plane allows it.
    Interleaved results (|sx| != 1 and |sy| != 1) must come out of the direct kernel, right and in place."""
    C_, oC, h, w = 3, 3, 130, 260
    img, lut, num = _interp_case(C_, oC, h, w, "c", 1)
    P = C_ * oC
    strides, shift = out_layouts(P, h, w)[layout]
    want = _values(num, "f32")
    pre = None
    if acc:
        pre = _values(np.random.default_rng(5).integers(-900, 900, num.shape), "f32")
        want = pre + want
    out = Guarded(torch, np.float32, (P, h, w), strides, shift, pre)
    x = torch.from_numpy(img).cuda()
    src = lib.Plane(x.data_ptr(), 0, img.shape[2], 1, img.shape[1] * img.shape[2])
    rc = _interp(lib, torch, src, img.shape[1:], C_, h, w, "c", 1, torch.from_numpy(lut).cuda(), oC, 4,
                 out.plane(strides[1], strides[2], strides[0]), ACC if acc else 0)
    assert rc == 0
    out.expect(want)


INPUT_LAYOUTS = {                         # (axes of the [C, H, W] image reversed in memory, (axis, extra pitch), HWC order)
    "flip_x": ((2,), None, False),
    "flip_y": ((1,), None, False),
    "rev_planes": ((0,), None, False),
    "padded_rows": ((), (1, 5), False),
    "hwc_flip_x": ((2,), None, True),
    "hwc_padded": ((), (0, 9), True),
}


@gpu
@pytest.mark.parametrize("in_dt", ["u8", "f32"])
@pytest.mark.parametrize("layout", list(INPUT_LAYOUTS))
def test_lut_interp_input_strides(torch, lib, layout, in_dt):
    """negative and padded image strides: the direct kernel honours them; the LDS kernel refuses negative ones
    (LERF_EUNSUPPORTED when insisted on, the direct kernel serves the call otherwise) and takes padded ones"""
    flip, pad, hwc = INPUT_LAYOUTS[layout]
    for C_, oC, (h, w), mode, rot in INTERP_COMBOS[:4]:
        img, lut, num = _interp_case(C_, oC, h, w, mode, rot)
        arr = img.transpose(1, 2, 0) if hwc else img                          # logical [H, W, C] or [C, H, W]
        arr = arr.astype(np.float32) if in_dt == "f32" else arr
        fl_ax = tuple({0: 2, 1: 0, 2: 1}[d] for d in flip) if hwc else flip    # the layout's axes in the memory order
        t, origin, st = strided_input(torch, arr, fl_ax, pad)
        sy, sx, sc = (st[0], st[1], st[2]) if hwc else (st[1], st[2], st[0])
        src = lib.Plane(origin, 0 if in_dt == "u8" else 1, sy, sx, sc)
        lut_t = torch.from_numpy(lut).cuda()
        negative = min(sy, sx, sc) < 0
        for flags in (0, DIRECT, LDS):
            out = Guarded(torch, np.int16, (C_ * oC, h, w), (h * w, w, 1))
            rc = _interp(lib, torch, src, img.shape[1:], C_, h, w, mode, rot, lut_t, oC, 4, out.plane(w, 1, h * w), flags)
            if flags == LDS and negative:
                assert rc == LERF_EUNSUPPORTED
                out.expect(None)
                continue
            assert rc == 0, (flags, rc)
            out.expect(num.astype(np.int16), what=repr((C_, oC, flags)))


@gpu
def test_lut_interp_lds_offset_limits(torch, lib):
    """the LDS kernel forms image offsets in 32 bits: row strides from 1 << 23 and operands whose last element lies at
    2^31 - 16 or beyond go to the direct kernel.  Just below and just above each limit, all kernels agree with the oracle."""
    C_, oC, h, w, mode, rot = 1, 3, 9, 37, "t", 1
    img, lut, num = _interp_case(C_, oC, h, w, mode, rot)
    want = num.astype(np.int16)
    lut_t = torch.from_numpy(lut).cuda()
    H, W = img.shape[1:]

    def run(ptr, sy, sx, sc, Cn, flags):
        out = Guarded(torch, np.int16, (Cn * oC, h, w), (h * w, w, 1))
        rc = _interp(lib, torch, lib.Plane(ptr, 0, sy, sx, sc), (H, W), Cn, h, w, mode, rot, lut_t, oC, 4, out.plane(w, 1, h * w), flags)
        return rc, out

    def check(ptr, sy, sx, sc, Cn, lds_ok, wanted):
        for flags in (LDS, 0, DIRECT):
            rc, out = run(ptr, sy, sx, sc, Cn, flags)
            if flags == LDS and not lds_ok:
                assert rc == LERF_EUNSUPPORTED, (sy, sc)
                out.expect(None, what=repr((sy, sc)))
                continue
            assert rc == 0, (sy, sc, flags, rc)
            out.expect(wanted, what=repr((sy, sc, flags)))

    # the row stride: 1 << 23 - 1 is the LDS kernel's, 1 << 23 is not
    for sy, lds_ok in (((1 << 23) - 1, True), (1 << 23, False)):
        buf = torch.zeros((H - 1) * sy + W + 64, dtype=torch.uint8, device="cuda")
        torch.as_strided(buf, (H, W), (sy, 1)).copy_(torch.from_numpy(img[0]).cuda())
        check(buf.data_ptr(), sy, 1, 0, 1, lds_ok, want)
        del buf
        torch.cuda.empty_cache()
    # the operand's extent: two planes, the second ending at element 2^31 - 17 (LDS) or 2^31 - 16 (direct)
    img2 = np.concatenate([img, img[:, ::-1, ::-1].copy()], axis=0)
    num2 = _interp_num_planes(img2, lut, mode, rot, h, w)
    buf = torch.zeros((1 << 31) + 4096, dtype=torch.uint8, device="cuda")
    tail = (H - 1) * W + (W - 1)
    for last, lds_ok in (((1 << 31) - 17, True), ((1 << 31) - 16, False)):
        sc = last - tail
        buf.zero_()
        torch.as_strided(buf, (2, H, W), (sc, W, 1)).copy_(torch.from_numpy(img2).cuda())
        check(buf.data_ptr(), W, 1, sc, 2, lds_ok, num2.astype(np.int16))
    del buf
    torch.cuda.empty_cache()


def _interp_num_planes(img, lut, mode, rot, h, w, interval=4):
    from oracle import lerf_oracle as O
    num = O.lut_interp_numer(lut, img.transpose(1, 2, 0), mode, rot, interval)[:h, :w]
    return num.transpose(2, 3, 0, 1).reshape(-1, h, w).astype(np.int64)


@gpu
@pytest.mark.parametrize("interval", [3, 5, 6])
@pytest.mark.parametrize("layout", ["hwc", "flip_x", "transposed_flip", "rev_planes"])
def test_lut_interp_other_intervals(torch, lib, interval, layout):
    """intervals other than the shipped 4 (the direct kernel for any interval) through the same strided planes"""
    for C_, oC, (h, w), mode, rot in INTERP_COMBOS[:3]:
        img, lut, num = _interp_case(C_, oC, h, w, mode, rot, interval=interval, seed=interval)
        P = C_ * oC
        strides, shift = out_layouts(P, h, w)[layout]
        lut_t = torch.from_numpy(lut).cuda()
        x = torch.from_numpy(img).cuda()
        src = lib.Plane(x.data_ptr(), 0, img.shape[2], 1, img.shape[1] * img.shape[2])
        for out_dt, flags in (("i16", 0), ("f64", DIRECT), ("f32", ACC)):
            pre = None
            want = _values(num, out_dt, interval)
            if flags & ACC:
                pre = np.full(num.shape, 0.5, np.float32)
                want = pre + want
            out = Guarded(torch, OUT_NP[out_dt], (P, h, w), strides, shift, pre)
            rc = _interp(lib, torch, src, img.shape[1:], C_, h, w, mode, rot, lut_t, oC, interval,
                         out.plane(strides[1], strides[2], strides[0]), flags)
            assert rc == 0
            out.expect(want, what=repr((C_, oC, out_dt)))
        out = Guarded(torch, np.int16, (P, h, w), strides, shift)
        rc = _interp(lib, torch, src, img.shape[1:], C_, h, w, mode, rot, lut_t, oC, interval,
                     out.plane(strides[1], strides[2], strides[0]), LDS)
        assert rc == LERF_EUNSUPPORTED
        out.expect(None)              # the LDS kernel is interval 4 only


# -------------------------------------------------------------------------------------------------------- lerf_lut_stages_u8
@pytest.fixture(scope="module")
def lutsets(torch):
    import lerf_pytorch_amd as L
    return {3: L.LutSet.shipped("lerf-g"), 1: L.LutSet.shipped("lerf-l")}


FEAT_LAYOUTS = {                                     # (H, W, C) lattice strides (sy, sx, sc) of feat
    "planar": lambda H, W, C_: (W, 1, H * W),
    "planar_padded": lambda H, W, C_: (W + 5, 1, H * (W + 5) + 3),
    "hwc_padded": lambda H, W, C_: (W * C_ + 7, C_, 1),
    "hwc_pixel_pitch": lambda H, W, C_: (W * (C_ + 2) + 1, C_ + 2, 1),
}


@gpu
@pytest.mark.parametrize("feat_layout", list(FEAT_LAYOUTS))
@pytest.mark.parametrize("oC", [3, 1])
def test_lut_stages_strided_planes(torch, lib, oracle, luts_g, luts_l, lutsets, feat_layout, oC):
    """stage 1 writes feat through its strides and stage 2 reads it back through them; hyper goes through a padded row and
    pixel pitch with the documented contiguous oC; hyper = NULL writes feat alone"""
    luts = luts_g if oC == 3 else luts_l
    for H, W, C_ in ((23, 37, 3), (16, 21, 1), (9, 30, 4)):
        img = np.random.default_rng(H * W + C_).integers(0, 256, (H, W, C_), dtype=np.uint8)
        of, oh = oracle.lut_stages(img, luts, oC)
        x = torch.from_numpy(img).cuda()
        src = lib.Plane(x.data_ptr(), 0, W * C_, C_, 1)
        fsy, fsx, fsc = FEAT_LAYOUTS[feat_layout](H, W, C_)
        hsx = C_ * oC + 2
        hsy = W * hsx + 11
        for with_hyper in (True, False):
            feat = Guarded(torch, np.uint8, (H, W, C_), (fsy, fsx, fsc))
            hyp = Guarded(torch, np.uint8, (H, W, C_, oC), (hsy, hsx, oC, 1))
            pf = feat.plane(fsy, fsx, fsc)
            ph = hyp.plane(hsy, hsx, oC)
            rc = lib.lib().lerf_lut_stages_u8(C.byref(src), H, W, C_, lutsets[oC].ref(), C.byref(pf),
                                              C.byref(ph) if with_hyper else None, _stream())
            assert rc == 0
            feat.expect(of, what=repr((H, W, C_)))
            hyp.expect(oh if with_hyper else None, what=repr((H, W, C_, with_hyper)))


# --------------------------------------------------------------------------------------------------------------- lerf_resize
def _hwck_hyper(lib, t, origin, st, nh, dtype):
    """three hyper planes over one [H][W][C][oC] tensor (hyper[k] = channel k of oC; fixed kernels: NULL)"""
    arr = (lib.Plane * 3)()
    item = np.dtype(np.uint8 if dtype == 0 else np.float32).itemsize
    for k in range(3):
        arr[k] = lib.Plane(origin + (k if k < nh else 0) * st[3] * item, dtype, st[0], st[1], st[2])
    return arr


def _sr_geo(shape_hw, scale, S, dis_scale=1.0):
    from lerf_pytorch_amd import ops
    return ops.SrGeometry(shape_hw, list(scale), None, S, dis_scale=dis_scale)


RESIZE_CASES = {
    # name: (kind, S given to the oracle, S of the tables, dis_scale, scale, input dtype, out dtype, flipped input axes)
    "cells_gauss_u8": ("gauss", 2, 2, 1.0, (2, 2), "u8", "u8", ()),
    "cells_linear_u8": ("linear", 2, 2, 1.0, (3, 2), "u8", "u8", ()),
    "generic_gauss_flipped_u8": ("gauss", 2, 2, 1.0, (2, 3), "u8", "u8", (1,)),
    "generic_down_f32": ("gauss", 2, 4, 0.5, (0.5, 0.5), "u8", "f32", (0,)),
    "generic_down_f64": ("gauss", 2, 4, 0.5, (0.5, 0.5), "u8", "f64", (1,)),
    "planar_f32_to_f64": ("gauss", 2, 2, 1.0, (1.5, 2), "f32", "f64", (1,)),
    "planar_f32_linear_to_f32": ("linear", 2, 2, 1.0, (2, 2), "f32", "f32", ()),
    "cubic_f64": ("cubic", 4, 4, 1.0, (2, 2), "u8", "f64", (1,)),
    "lanczos3_u8": ("lanczos3", 6, 6, 1.0, (2, 1.5), "u8", "u8", (0,)),
}


@functools.lru_cache(maxsize=None)
def _resize_ref(name):
    from oracle import lerf_oracle as O
    kind, S_or, S, dis_scale, (sh, sw), in_dt, out_dt, flip = RESIZE_CASES[name]
    rng = np.random.default_rng(len(name))
    H, W, C_ = (24, 30, 3) if in_dt == "u8" else (17, 23, 2)
    ms = 10.0 if kind == "gauss" else 1.0
    nh = {"gauss": 3, "linear": 1}.get(kind, 0)
    feat = rng.integers(0, 256, (H, W, C_), dtype=np.uint8)
    hq = rng.integers(0, 256, (H, W, C_, max(nh, 1)), dtype=np.uint8)
    fchw = np.ascontiguousarray(feat.transpose(2, 0, 1)).astype(np.float32)
    hp = [np.ascontiguousarray((hq[..., k].astype(np.float32) / np.float32(255)).transpose(2, 0, 1)) for k in range(nh)]
    hp += [None] * (3 - nh)
    ref = O.resize_params_f32(fchw, hp[0], hp[1], hp[2], sh, sw, S_or, ms, kind)               # [C, oH, oW]
    return feat, hq, ref, ms, nh


@gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", list(RESIZE_CASES))
def test_resize_out_layouts(torch, lib, case, layout):
    """lerf_resize on its kernel families (the uint8 cell kernel, the generic one on uint8 / float32 operands, the fixed
    kernels) through strided / flipped inputs and every output layout"""
    kind, S_or, S, dis_scale, scale, in_dt, out_dt, flip = RESIZE_CASES[case]
    feat, hq, ref, ms, nh = _resize_ref(case)
    H, W, C_ = feat.shape
    geo = _sr_geo((H, W), scale, S, dis_scale)
    oH, oW = geo.out_hw
    assert ref.shape == (C_, oH, oW)
    strides, shift = out_layouts(C_, oH, oW)[layout]
    if in_dt == "u8":
        tf, of_, fs = strided_input(torch, feat, flip)                                          # [H, W, C]
        pf = lib.Plane(of_, 0, fs[0], fs[1], fs[2])
        th, oh_, hs = strided_input(torch, hq, flip)                                            # [H, W, C, oC]
        ph = _hwck_hyper(lib, th, oh_, hs, nh, 0) if nh else None
    else:                                                                                      # planar float32 maps
        fchw = np.ascontiguousarray(feat.transpose(2, 0, 1)).astype(np.float32)
        pflip = tuple(d + 1 for d in flip)
        tf, of_, fs = strided_input(torch, fchw, pflip)                                         # [C, H, W]
        pf = lib.Plane(of_, 1, fs[1], fs[2], fs[0])
        maps = np.stack([(hq[..., k].astype(np.float32) / np.float32(255)).transpose(2, 0, 1) for k in range(nh)])
        th, oh_, hs = strided_input(torch, maps, tuple(d + 1 for d in pflip))                    # [k, C, H, W]
        ph = (lib.Plane * 3)()
        for k in range(3):
            ph[k] = lib.Plane(oh_ + (k if k < nh else 0) * hs[0] * 4, 1, hs[2], hs[3], hs[1])
    dt = {"u8": np.uint8, "f32": np.float32, "f64": np.float64}[out_dt]
    if out_dt == "u8":
        want, cmp = bytes_of(ref)
        if kind in ("gauss", "linear"):
            cmp = exact                                                       # the tie guard makes these the oracle's bytes
    else:
        want, cmp = ref, within(1e-9 if out_dt == "f64" else F32_OBSERVED)
    out = Guarded(torch, dt, (C_, oH, oW), strides, shift)
    rc = lib.lib().lerf_resize(C.byref(pf), ph, H, W, C_, geo.ref(), lib.KINDS[kind], ms,
                               C.byref(out.plane(strides[1], strides[2], strides[0])), _stream())
    assert rc == 0
    out.expect(want, cmp)


# ----------------------------------------------------------------------------------------------------------------- lerf_warp
WARP_CASES = {
    # name: (kind, S, out dtype, matrix key, output size); linear and cubic at 344 x 228 have pixels whose weights all vanish
    "gauss_u8": ("gauss", 2, "u8", "isc", (60, 70)),
    "gauss_f64": ("gauss", 2, "f64", "osc", (97, 41)),
    "linear_f32": ("linear", 2, "f32", "isc", (344, 228)),
    "linear_u8": ("linear", 2, "u8", "osc", (344, 228)),
    "nearest_mask_f32": ("nearest", 1, "f32", "isc", (120, 120)),
    "cubic_f64": ("cubic", 4, "f64", "isc", (344, 228)),
}
WARP_OUT = (60, 70)


@functools.lru_cache(maxsize=None)
def _warp_inputs(seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (52, 52, 3), dtype=np.uint8), rng.integers(0, 256, (52, 52, 3, 3), dtype=np.uint8)


@gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", list(WARP_CASES))
def test_warp_out_layouts(torch, lib, oracle, golden, case, layout):
    """lerf_warp through flipped inputs and every output layout; NaN where the weights vanish (float outputs) and 0 in
    uint8 outputs, like the oracle; the nearest warp of a white frame gives the harness's validity mask"""
    from lerf_pytorch_amd import ops
    kind, S, out_dt, mkey, out_hw = WARP_CASES[case]
    M = golden("g4_warp.npz")["%s/matrix" % mkey]
    feat, hq = _warp_inputs(3)
    nh = {"gauss": 3, "linear": 1}.get(kind, 0)
    ms = 10.0 if kind == "gauss" else 1.0
    if kind == "nearest":
        feat = np.zeros_like(feat)
        feat[4:48, 4:48] = 255
    fchw = feat.transpose(2, 0, 1).astype(np.float32)
    hp = [(hq[..., k].astype(np.float32) / np.float32(255)).transpose(2, 0, 1) for k in range(nh)] + [None] * (3 - nh)
    ref = oracle.warp_params_f32(fchw, hp[0], hp[1], hp[2], M, out_hw, S, ms, kind)             # [C, oH, oW]
    geo = ops.WarpGeometry((52, 52), M, out_hw, S)
    tf, of_, fs = strided_input(torch, feat, (1,))                                              # columns reversed in memory
    pf = lib.Plane(of_, 0, fs[0], fs[1], fs[2])
    th, oh_, hs = strided_input(torch, hq[..., :max(nh, 1)].copy(), (0,))                       # rows reversed in memory
    ph = _hwck_hyper(lib, th, oh_, hs, nh, 0) if nh else None
    strides, shift = out_layouts(3, *out_hw)[layout]
    dt = {"u8": np.uint8, "f32": np.float32, "f64": np.float64}[out_dt]
    if out_dt == "u8":
        want, cmp = bytes_of(ref)
    elif kind == "nearest":
        want, cmp = ref, exact
    else:
        want, cmp = ref, within(1e-9 if out_dt == "f64" else F32_OBSERVED)
    out = Guarded(torch, dt, (3,) + out_hw, strides, shift)
    rc = lib.lib().lerf_warp(C.byref(pf), ph, 52, 52, 3, geo.ref(), lib.KINDS[kind], ms,
                             C.byref(out.plane(strides[1], strides[2], strides[0])), _stream())
    assert rc == 0
    out.expect(want, cmp)
    if kind in ("linear", "cubic"):
        assert np.isnan(ref).any() and not np.isnan(ref).all()              # both kinds of pixels are in the case
    if kind == "nearest":
        got = out.t.cpu().numpy().view(dt)[lattice(out.base, out.shape, out.strides)]
        assert np.array_equal((got == 255).transpose(1, 2, 0), oracle.warp_mask((52, 52), M, out_hw))


@gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("out_dt", ["u8", "f32"])
def test_warp_packed_out_layouts(torch, lib, oracle, golden, luts_g, lutsets, out_dt, layout):
    """lerf_warp_packed: two frames in one launch, each result plane through the layout, frames a padded out_sn apart"""
    from lerf_pytorch_amd import ops
    M = golden("g4_warp.npz")["isc/matrix"]
    imgs = np.random.default_rng(11).integers(0, 256, (2, 52, 52, 3), dtype=np.uint8)
    packed = ops.stages_packed(torch.from_numpy(imgs).cuda(), lutsets[3])
    geo = ops.WarpGeometry((52, 52), M, WARP_OUT, 2)
    refs = []
    for n in range(2):
        f, h = oracle.lut_stages(imgs[n], luts_g, 3)
        refs.append(oracle.warp_u8(f, h, M, WARP_OUT, 2, 10.0, "gauss").transpose(2, 0, 1))
    ref = np.stack(refs)                                                       # [n, C, oH, oW]
    strides, shift = out_layouts(3, *WARP_OUT)[layout]
    lo, hi = extent((3,) + WARP_OUT, strides)
    out_sn = hi - lo + 1 + 13
    dt = np.uint8 if out_dt == "u8" else np.float32
    want, cmp = bytes_of(ref) if out_dt == "u8" else (ref, within(F32_TOL))
    out = Guarded(torch, dt, (2, 3) + WARP_OUT, (out_sn,) + strides, shift)
    p = out.plane(strides[1], strides[2], strides[0])
    rc = lib.lib().lerf_warp_packed(packed.data_ptr(), packed.stride(0), 2, 52, 52, 3, geo.ref(), lib.KINDS["gauss"], 10.0,
                                    C.byref(p), out_sn, _stream())
    assert rc == 0
    out.expect(want, cmp)
