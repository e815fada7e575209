"""Reference, launch-path rule and crafted-table cases of one resize_right axis pass (lerf_rr_axis, csrc/lerf_rr.hip).

axis_ref / csr_ref do what include/lerf_hip.h promises, in plain numpy: the accumulator starts at +0 and takes one product
per tap (per CSR entry), in order, every product and every sum rounded on its own in the accumulator type.  Comparing a
kernel with them needs no tolerance.  The source index of a padded tap comes from np.pad of an index vector, not from a
restatement of the kernel's pad rule.  dense_matrix is the same operation as a float64 matrix, for the high-precision
cross-checks of tests/test_rr_axis_cpu.py.

paths() restates which kernel, and for the narrow kernel which source path (LDS window or global memory) each workgroup
takes; tests/test_rr_axis_cpu.py pins its three constants to the kernel source and proves that CASES reaches every path.

Data rules (make_values): weights are random, signed, not normalised; inputs and weights are zero or of magnitude
2^-10 .. 2^10, so no product is subnormal or infinite in float32."""
import collections

import numpy as np

kThreads = 256          # lanes per workgroup
kVec = 4                # wide kernel: elements per lane
kWin = 4096             # narrow kernel: LDS window, in accumulator elements

PAD_NAMES = ("constant", "edge", "reflect", "symmetric", "wrap")       # index = LERF_PAD_*
U8, F32, F64, I16 = 0, 1, 2, 3                                          # LERF_U8 ...
NP_OF = {U8: np.uint8, F32: np.float32, F64: np.float64}


# ---------------------------------------------------------------------------------------------------------- the reference
def source_rows(left, taps, n_in, pad_mode):
    """int64 [n_out][taps]: the source index of every tap under np.pad's rule `pad_mode`; -1 for a tap in a constant pad"""
    left = np.asarray(left, dtype=np.int64)
    lo = max(0, -int(left.min()))
    hi = max(0, int(left.max()) + taps - n_in)
    base = np.arange(n_in, dtype=np.int64)
    if PAD_NAMES[pad_mode] == "constant":
        padded = np.pad(base, (lo, hi), mode="constant", constant_values=-1)
    else:
        padded = np.pad(base, (lo, hi), mode=PAD_NAMES[pad_mode])
    return padded[left[:, None] + np.arange(taps)[None, :] + lo]


def axis_ref(x, left, w, n_in, pad_mode, acc, out_u8=False):
    """x [outer][n_in][inner] (any of the three input types), left [n_out], w [n_out][taps] -> [outer][n_out][inner] in `acc`
    dtype, or uint8 by np.round(np.clip()) with out_u8"""
    acc = np.dtype(acc)
    x = np.asarray(x)
    w = np.asarray(w, dtype=acc)
    assert x.ndim == 3 and x.shape[1] == n_in and w.ndim == 2 and w.shape[0] == len(left)
    xa = x.astype(acc)
    src = source_rows(left, w.shape[1], n_in, pad_mode)
    out = np.zeros((x.shape[0], len(left), x.shape[2]), acc)
    for k in range(w.shape[1]):
        s = src[:, k]
        xk = xa[:, np.maximum(s, 0), :]
        xk[:, s < 0, :] = 0                                       # a constant-pad tap contributes w * 0
        prod = w[:, k][None, :, None] * xk
        out = out + prod
    assert out.dtype == acc
    if out_u8:
        return np.round(np.clip(out, 0, 255)).astype(np.uint8)
    return out


def csr_ref(x, row_ptr, idx, w, acc, out_u8=False):
    """the CSR form: out[o][j][i] = sum over e in [row_ptr[j], row_ptr[j + 1]) of w[e] * x[o][idx[e]][i], in entry order"""
    acc = np.dtype(acc)
    x = np.asarray(x)
    xa = x.astype(acc)
    w = np.asarray(w, dtype=acc)
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    idx = np.asarray(idx, dtype=np.int64)
    cnt = np.diff(row_ptr)
    out = np.zeros((x.shape[0], len(cnt), x.shape[2]), acc)
    for e in range(int(cnt.max()) if len(cnt) else 0):
        rows = np.nonzero(cnt > e)[0]
        ent = row_ptr[rows] + e
        prod = w[ent][None, :, None] * xa[:, idx[ent], :]
        out[:, rows, :] = out[:, rows, :] + prod
    if out_u8:
        return np.round(np.clip(out, 0, 255)).astype(np.uint8)
    return out


def dense_matrix(left, w, n_in, pad_mode):
    """float64 [n_out][n_in]: the axis pass as a matrix, padded taps folded onto their source index, constant-pad taps dropped"""
    w = np.asarray(w, dtype=np.float64)
    src = source_rows(left, w.shape[1], n_in, pad_mode)
    m = np.zeros((len(left), n_in), np.float64)
    jj = np.broadcast_to(np.arange(len(left))[:, None], src.shape)
    keep = src >= 0
    np.add.at(m, (jj[keep], src[keep]), w[keep])
    return m


def adjoint_csr(left, w, n_in, pad_mode):
    """(row_ptr[n_in + 1], idx[nnz], wt[nnz]) from the library's lerf_rr_adjoint_csr (host code); w float32 or float64"""
    from lerf_pytorch_amd import _lib
    left = np.ascontiguousarray(left, dtype=np.int32)
    w = np.ascontiguousarray(w)
    n_out, taps = w.shape
    row_ptr = np.zeros(n_in + 1, np.int32)
    idx = np.zeros(n_out * taps, np.int32)
    wt = np.zeros(n_out * taps, w.dtype)
    nnz = _lib.lib().lerf_rr_adjoint_csr(n_in, n_out, taps, left.ctypes.data, w.ctypes.data, F64 if w.dtype == np.float64 else F32,
                                          pad_mode, row_ptr.ctypes.data, idx.ctypes.data, wt.ctypes.data)
    assert nnz >= 0, nnz
    return row_ptr, idx[:nnz].copy(), wt[:nnz].copy()


# ---------------------------------------------------------------------------------------------------------- the path rule
def workgroup_spans(n_out, inner, left, taps):
    """narrow kernel: [(j0, j1, sp)] per workgroup, sp = left[j1] + taps - left[j0] as the kernel computes it"""
    jt = kThreads // inner
    out = []
    for j0 in range(0, n_out, jt):
        j1 = min(j0 + jt, n_out) - 1
        out.append((j0, j1, int(left[j1]) + taps - int(left[j0])))
    return out


def paths(n_out, inner, left, taps):
    """"wide" (inner >= 64), or for the narrow kernel the source path of every workgroup: "lds" where the segment
    [left[j0], left[j1] + taps) is not empty and fits the window, else "global" (a CSR pass, taps == 0: always "global")"""
    if inner >= 64:
        return "wide"
    if taps == 0:
        return ["global"] * ((n_out + kThreads // inner - 1) // (kThreads // inner))
    return ["lds" if sp > 0 and sp * inner <= kWin else "global" for _, _, sp in workgroup_spans(n_out, inner, left, taps)]


def wide_x_blocks(inner):
    """wide kernel: workgroups along `inner`, each covering kThreads * kVec elements"""
    return (inner + kThreads * kVec - 1) // (kThreads * kVec)


# ---------------------------------------------------------------------------------------------------------- data
def make_values(rng, shape, zeros=0.05):
    """float64 values that are 0 (a fraction `zeros`) or +-2^u, u uniform in [-10, 10]: signed, mixed magnitude"""
    v = np.exp2(rng.uniform(-10.0, 10.0, shape)) * rng.choice([-1.0, 1.0], shape)
    v[rng.random(shape) < zeros] = 0.0
    return v


def case_data(case, in_code, acc_code):
    """(x [outer][n_in][inner] of the input type, w [n_out][taps] of the accumulator type) of a case, the same at every call"""
    rng = np.random.default_rng([case.seed, in_code, acc_code])
    shape = (case.outer, case.n_in, case.inner)
    if in_code == U8:
        x = rng.integers(0, 256, shape, dtype=np.uint8)
        x[rng.random(shape) < 0.05] = 0
    else:
        x = make_values(rng, shape).astype(NP_OF[in_code])
    w = make_values(rng, (case.n_out, case.taps)).astype(NP_OF[acc_code])
    assert not np.all(np.signbit(w) & (w == 0))
    return x, w


# ---------------------------------------------------------------------------------------------------------- crafted tables
Case = collections.namedtuple("Case", "name group outer n_in n_out inner taps left pad seed")


def _grid(n_out, stride, offset):
    return (np.arange(n_out, dtype=np.int64) * stride + offset).astype(np.int32)


def _n_in_for(left, taps, tail=3):
    """an n_in under which the last output's final `tail` taps lie in the high pad (the first output's lie in the low pad when
    its left is negative)"""
    return int(np.max(left)) + taps - tail


def _build_cases():
    cases = []

    def add(name, group, inner, taps, left, pad, n_in=None, outer=3):
        left = np.ascontiguousarray(left, dtype=np.int32)
        n_in = _n_in_for(left, taps) if n_in is None else n_in
        assert n_in >= 1
        cases.append(Case(name, group, outer, n_in, len(left), inner, taps, left, pad, len(cases) + 1))

    # -- the LDS window limit: sp * inner against kWin, one element either side
    add("window-1x4096", "window", 1, 271, _grid(600, 15, -7), 3)          # 255 * 15 + 271 = 4096: stages
    add("window-1x4097", "window", 1, 272, _grid(600, 15, -7), 2)          # 4097: full workgroups fall back, the last (88 outputs) stages
    add("window-3x1365", "window", 3, 21, _grid(200, 16, -5), 4)           # jt = 85: 84 * 16 + 21 = 1365, x3 = 4095: stages
    add("window-3x1366", "window", 3, 22, _grid(200, 16, -5), 0)           # 1366, x3 = 4098: falls back; the last workgroup stages
    # -- narrow lane mapping: idle tail lanes (256 % inner != 0), n_out no multiple of jt
    for inner, n_out in ((2, 259), (33, 17), (48, 13), (63, 11)):
        assert n_out % (kThreads // inner)
        add("lanes-%d" % inner, "lanes", inner, 5, _grid(n_out, 2, -3), 2 + inner % 3)
    # -- wide: 64 is the first wide size (64 live lanes of 1024); 1025 and 2049 put one live lane into a second / third x-block
    for inner in (64, 65, 255, 256, 257, 1023, 1024, 1025, 2049):
        add("wide-%d" % inner, "wide", inner, 5, _grid(3, 2, -2), inner % 5)
    # -- table order: the header places none on left[]
    for inner in (1, 3, 64):
        jt = max(kThreads // inner, 1)
        n_out = 2 * jt + jt // 3 + 2 if inner < 64 else 40
        mono = _grid(n_out, 2, -4)
        n_in = _n_in_for(mono, 6)
        rng = np.random.default_rng(1000 + inner)
        add("order-permuted-%d" % inner, "order", inner, 6, rng.permutation(mono), 3, n_in)
        add("order-descending-%d" % inner, "order", inner, 6, mono[::-1], 2, n_in)                # sp <= 0 in every full workgroup
        out = mono.copy()                          # ends of every workgroup stay put; between them: below left[j0], above left[j1]
        for j0 in range(0, n_out, jt):
            j1 = min(j0 + jt, n_out) - 1
            mid = np.arange(j0 + 1, j1)
            out[mid[0::3]] = mono[j0] - 5 - (mid[0::3] % 11)
            out[mid[1::3]] = mono[j1] + 9 + (mid[1::3] % 13)
        add("order-outliers-%d" % inner, "order", inner, 6, out, 4, n_in)
    # -- the pad rule far outside the image: tiny n_in, left from -40 upward; staged (inner 1), unstaged (inner 3, one workgroup
    #    whose span does not fit) and wide (inner 64)
    for place, inner, n_out, stride in (("staged", 1, 30, 3), ("unstaged", 3, 85, 17), ("wide", 64, 30, 3)):
        for pad in range(5):
            for n_in in (1, 2, 3, 5):
                for taps in (1, 7, 32):
                    add("pad-%s-%s-n%d-t%d" % (place, PAD_NAMES[pad], n_in, taps), "pad-" + place, inner, taps,
                        _grid(n_out, stride, -40), pad, n_in, outer=2)
    return cases


CASES = _build_cases()
