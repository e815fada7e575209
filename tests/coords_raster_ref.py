"""A numpy / plain-Python restatement of the rasterising inverse (lerf_coords_invert_raster), which does not import the library: the
statement order at the top of csrc/lerf_coords_models.h, one Python float operation per statement (IEEE double, each rounded, no
fused multiply-add), Python ints for the keys, `struct` for the bit-casts.  A sequential loop over the cells, row-major, with a plain
min -- the order cannot matter.

    raster(F, out_hw, depth=None, max_span=16, orient=0, origin=(0, 0)) -> (G float64 [oH, oW, 2], keys uint64 [oH, oW])
    tri_sample(F, t, u) -> (row, col): the linear interpolant of triangle t of F at the position u of F's index space
"""
import math
import struct

import numpy as np

NO_KEY = (1 << 64) - 1


def _finite(v):
    return v - v == 0.0


def edge(P, Q, qr, qc):
    return (Q[1] - P[1]) * (qr - P[0]) - (Q[0] - P[0]) * (qc - P[1])


def tri_vertices(t, fW):
    """the (row, col) indices of A, B, C of triangle t"""
    cell, odd = t >> 1, t & 1
    i, j = divmod(cell, fW - 1)
    return ((i + 1, j + 1), (i + 1, j), (i, j + 1)) if odd else ((i, j), (i, j + 1), (i + 1, j))


def tri_edges(A, B, C, odd, qr, qc):
    """(e_a, e_b, e_c): every edge with its endpoints in ascending source index, negated where the triangle runs the other way"""
    if odd:
        return -edge(C, B, qr, qc), edge(C, A, qr, qc), -edge(B, A, qr, qc)
    return edge(B, C, qr, qc), -edge(A, C, qr, qc), edge(A, B, qr, qc)


def sortable(z32):
    b = struct.unpack("<I", struct.pack("<f", z32))[0]
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def _axis(v, max_span, first, n):
    """(lo, hi) ints of one axis of the box, or None: torn or outside the tile; the clip precedes the conversion to int"""
    lo, hi = float(math.ceil(min(v))), float(math.floor(max(v)))          # exact for any finite double
    if (hi - lo) + 1.0 > float(max_span):
        return None
    lo, hi = max(lo, float(first)), min(hi, float(first) + float(n - 1))
    if lo > hi:
        return None
    return int(lo), int(hi)


def raster(F, out_hw, depth=None, max_span=16, orient=0, origin=(0, 0)):
    F = np.asarray(F)
    fH, fW = F.shape[:2]
    oH, oW = int(out_hw[0]), int(out_hw[1])
    i0, j0 = int(origin[0]), int(origin[1])
    P = [[(float(F[i, j, 0]), float(F[i, j, 1])) for j in range(fW)] for i in range(fH)]          # a float32 map is promoted exactly
    Z = None if depth is None else np.asarray(depth, dtype=np.float32)
    keys = [[NO_KEY] * oW for _ in range(oH)]
    for i in range(fH - 1):
        for j in range(fW - 1):
            for odd in (0, 1):
                t = 2 * (i * (fW - 1) + j) + odd
                ia, ib, ic = tri_vertices(t, fW)
                A, B, C = P[ia[0]][ia[1]], P[ib[0]][ib[1]], P[ic[0]][ic[1]]
                if not all(_finite(v) for v in A + B + C):
                    continue
                if Z is not None:
                    zA, zB, zC = (float(Z[k]) for k in (ia, ib, ic))
                    if zA != zA or zB != zB or zC != zC:
                        continue
                area2 = edge(A, B, C[0], C[1])
                if area2 == 0.0 or not _finite(area2) or (orient > 0 and area2 < 0.0) or (orient < 0 and area2 > 0.0):
                    continue
                rows = _axis((A[0], B[0], C[0]), max_span, i0, oH)
                cols = _axis((A[1], B[1], C[1]), max_span, j0, oW)
                if rows is None or cols is None:
                    continue
                for r in range(rows[0], rows[1] + 1):
                    for c in range(cols[0], cols[1] + 1):
                        ea, eb, ec = tri_edges(A, B, C, odd, float(r), float(c))
                        if not ((ea >= 0.0 and eb >= 0.0 and ec >= 0.0) if area2 > 0.0 else (ea <= 0.0 and eb <= 0.0 and ec <= 0.0)):
                            continue
                        z32 = 0.0
                        if Z is not None:
                            lb, lc = eb / area2, ec / area2
                            with np.errstate(all="ignore"):
                                z32 = float(np.float32(zA + (lb * (zB - zA) + lc * (zC - zA))))
                            if z32 != z32:
                                z32 = struct.unpack("<f", struct.pack("<I", 0x7FC00000))[0]
                        key = (sortable(z32) << 32) | t
                        if key < keys[r - i0][c - j0]:
                            keys[r - i0][c - j0] = key
    G = np.full((oH, oW, 2), np.nan)
    for r in range(oH):
        for c in range(oW):
            key = keys[r][c]
            if key == NO_KEY:
                continue
            t = key & 0xFFFFFFFF
            odd = t & 1
            i, j = divmod(t >> 1, fW - 1)
            ia, ib, ic = tri_vertices(t, fW)
            A, B, C = P[ia[0]][ia[1]], P[ib[0]][ib[1]], P[ic[0]][ic[1]]
            area2 = edge(A, B, C[0], C[1])
            _, eb, ec = tri_edges(A, B, C, odd, float(i0 + r), float(j0 + c))
            lb, lc = eb / area2, ec / area2
            G[r, c] = (float(i + 1) - lc, float(j + 1) - lb) if odd else (float(i) + lc, float(j) + lb)
    return G, np.array(keys, dtype=np.uint64)


def tri_sample(F, t, u):
    """T(u) of triangle t: A + l_b (B - A) + l_c (C - A) with (l_c, l_b) the offsets of u from A in F's index space (both signs
    flipped for an odd triangle, whose B and C lie at lower indices than A)"""
    F = np.asarray(F, dtype=np.float64)
    ia, ib, ic = tri_vertices(int(t), F.shape[1])
    A, B, C = F[ia], F[ib], F[ic]
    s = -1.0 if int(t) & 1 else 1.0
    lc, lb = s * (float(u[0]) - ia[0]), s * (float(u[1]) - ia[1])
    return A + lb * (B - A) + lc * (C - A)
