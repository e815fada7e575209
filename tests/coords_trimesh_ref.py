"""A plain-Python restatement of the triangle-mesh rasteriser (lerf_coords_trimesh), which does not import the library: the statement
order at the top of csrc/lerf_coords_models.h, one Python float operation per statement (IEEE double, each rounded, no fused
multiply-add), Python ints for the indices and keys, `struct` for the bit-casts, numpy only to hold the arrays and to round to
float32.  A sequential loop over the faces with a plain min -- the order cannot matter.

    trimesh(pos, attr, faces, out_hw, attr_faces=None, depth=None, w=None, max_span=0, orient=0, origin=(0, 0), out_dtype=np.float64)
        -> (out [oH, oW, 2] of out_dtype, keys uint64 [oH, oW], depth_out float32 [oH, oW])
"""
import math
import struct

import numpy as np

NO_KEY = (1 << 64) - 1
QUIET_NAN32 = struct.unpack("<f", struct.pack("<I", 0x7FC00000))[0]


def _finite(v):
    return v - v == 0.0


def edge(P, Q, qr, qc):
    return (Q[1] - P[1]) * (qr - P[0]) - (Q[0] - P[0]) * (qc - P[1])


def directed(P, Q, ip, iq, qr, qc):
    """the edge function of the directed edge P -> Q, evaluated from its lower vertex index"""
    return edge(P, Q, qr, qc) if ip < iq else -edge(Q, P, qr, qc)


def tri_edges(A, B, C, ia, ib, ic, qr, qc):
    """(e_a, e_b, e_c) over B -> C, C -> A, A -> B"""
    return directed(B, C, ib, ic, qr, qc), directed(C, A, ic, ia, qr, qc), directed(A, B, ia, ib, qr, qc)


def sortable(z32):
    b = struct.unpack("<I", struct.pack("<f", z32))[0]
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def unsortable(s):
    b = (s & 0x7FFFFFFF) if s & 0x80000000 else (~s & 0xFFFFFFFF)
    return struct.unpack("<f", struct.pack("<I", b))[0]


def _axis(v, max_span, first, n):
    """(lo, hi) ints of one axis of the box, or None: torn or outside the tile; the clip precedes the conversion to int"""
    lo, hi = float(math.ceil(min(v))), float(math.floor(max(v)))          # exact for any finite double
    if max_span > 0 and (hi - lo) + 1.0 > float(max_span):
        return None
    lo, hi = max(lo, float(first)), min(hi, float(first) + float(n - 1))
    if lo > hi:
        return None
    return int(lo), int(hi)


def _div(a, b):
    """IEEE division of two floats (Python raises on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _face(f, P, T, Z, Wv, faces, attr_faces):
    """the vertices of face f, or None: an index outside the mesh (nothing is read)"""
    idx = [int(k) for k in faces[f]]
    aidx = [int(k) for k in (faces if attr_faces is None else attr_faces)[f]]
    if not all(0 <= k < len(P) for k in idx) or not all(0 <= k < len(T) for k in aidx):
        return None
    z = [0.0] * 3 if Z is None else [float(Z[k]) for k in idx]
    wv = None if Wv is None else [float(Wv[k]) for k in idx]
    return idx, aidx, [P[k] for k in idx], z, wv


def trimesh(pos, attr, faces, out_hw, attr_faces=None, depth=None, w=None, max_span=0, orient=0, origin=(0, 0), out_dtype=np.float64):
    pos, attr = np.asarray(pos), np.asarray(attr)
    P = [(float(r), float(c)) for r, c in pos]          # a float32 operand is promoted exactly
    T = [(float(r), float(c)) for r, c in attr]
    faces = np.asarray(faces)
    attr_faces = None if attr_faces is None else np.asarray(attr_faces)
    Z = None if depth is None else np.asarray(depth, dtype=np.float32)
    Wv = None if w is None else np.asarray(w)          # float32 or float64
    oH, oW = int(out_hw[0]), int(out_hw[1])
    i0, j0 = int(origin[0]), int(origin[1])
    keys = [[NO_KEY] * oW for _ in range(oH)]
    for f in range(len(faces)):
        face = _face(f, P, T, Z, Wv, faces, attr_faces)
        if face is None:
            continue
        (ia, ib, ic), _, (A, B, C), (zA, zB, zC), wv = face
        if not all(_finite(v) for v in A + B + C):
            continue
        if Z is not None and (zA != zA or zB != zB or zC != zC):
            continue
        if wv is not None and not all(_finite(v) and v > 0.0 for v in wv):
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
                ea, eb, ec = tri_edges(A, B, C, ia, ib, ic, float(r), float(c))
                if not ((ea >= 0.0 and eb >= 0.0 and ec >= 0.0) if area2 > 0.0 else (ea <= 0.0 and eb <= 0.0 and ec <= 0.0)):
                    continue
                z32 = 0.0
                if Z is not None:
                    lb, lc = eb / area2, ec / area2
                    with np.errstate(all="ignore"):
                        z32 = float(np.float32(zA + (lb * (zB - zA) + lc * (zC - zA))))
                    if z32 != z32:
                        z32 = QUIET_NAN32
                key = (sortable(z32) << 32) | f
                if key < keys[r - i0][c - j0]:
                    keys[r - i0][c - j0] = key
    out = np.full((oH, oW, 2), np.nan, dtype=np.float64)
    zo = np.full((oH, oW), np.nan, dtype=np.float32)
    for r in range(oH):
        for c in range(oW):
            key = keys[r][c]
            if key == NO_KEY:
                continue
            (ia, ib, ic), (ja, jb, jc), (A, B, C), _, wv = _face(key & 0xFFFFFFFF, P, T, Z, Wv, faces, attr_faces)
            aA, aB, aC = T[ja], T[jb], T[jc]
            area2 = edge(A, B, C[0], C[1])
            _, eb, ec = tri_edges(A, B, C, ia, ib, ic, float(i0 + r), float(j0 + c))
            lb, lc = eb / area2, ec / area2
            if wv is None:
                out[r, c] = [aA[k] + (lb * (aB[k] - aA[k]) + lc * (aC[k] - aA[k])) for k in (0, 1)]
            else:
                qa, qb, qc = 1.0 / wv[0], 1.0 / wv[1], 1.0 / wv[2]
                d = qa + (lb * (qb - qa) + lc * (qc - qa))
                out[r, c] = [_div(aA[k] * qa + (lb * (aB[k] * qb - aA[k] * qa) + lc * (aC[k] * qc - aA[k] * qa)), d) for k in (0, 1)]
            zo[r, c] = np.float32(unsortable(key >> 32))
    with np.errstate(all="ignore"):
        return out.astype(out_dtype), np.array(keys, dtype=np.uint64), zo
