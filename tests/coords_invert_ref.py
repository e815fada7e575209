"""Independent numpy restatement of the map inverse (lerf_coords_invert; the contract in include/lerf_hip.h), vectorised over the
entries, written from the formulas and not from the library (nothing of it is imported): Newton's method on the piecewise-bilinear
interpolant of F, the affine start from three corners, NaN for what does not converge.  Besides the inverse it returns what a
test needs to judge its own inputs: per entry the number of passes run, the last residual max(|e_r|, |e_c|) seen, and the
largest norm of an inverse Jacobian computed on the way."""
import numpy as np


def _axis(v, n):
    """compose's per-axis rule: clip onto [0, n - 1] (-inf -> 0, +inf -> n - 1), i = min(floor(r), n - 2), t = r - i"""
    r = np.where(v >= 0.0, np.minimum(v, float(n - 1)), 0.0)
    i = np.minimum(np.floor(r), float(n - 2))
    return r, i.astype(np.int64), r - i


def sample(F, u):
    """(clipped u, V, Jr, Jc) of the bilinear patch of F at u [..., 2]; u must hold no NaN"""
    F = np.asarray(F).astype(np.float64)
    fH, fW = F.shape[:2]
    r, i, t = _axis(u[..., 0], fH)
    c, j, s = _axis(u[..., 1], fW)
    t, s = t[..., None], s[..., None]
    P00, P01, P10, P11 = F[i, j], F[i, j + 1], F[i + 1, j], F[i + 1, j + 1]
    V = (1.0 - t) * ((1.0 - s) * P00 + s * P01) + t * ((1.0 - s) * P10 + s * P11)
    Jr = (1.0 - s) * (P10 - P00) + s * (P11 - P01)
    Jc = (1.0 - t) * (P01 - P00) + t * (P11 - P10)
    return np.stack([r, c], axis=-1), V, Jr, Jc


def start(F, q):
    """the affine guess of the u with F(u) = q from F[0, 0], F[fH - 1, 0], F[0, fW - 1]; the middle of F when they are degenerate"""
    F = np.asarray(F).astype(np.float64)
    fH, fW = F.shape[:2]
    A = F[0, 0]
    B = (F[fH - 1, 0] - A) / float(fH - 1)
    C = (F[0, fW - 1] - A) / float(fW - 1)
    with np.errstate(all="ignore"):
        det = B[0] * C[1] - B[1] * C[0]
        if det == 0.0 or not np.isfinite(det):
            return np.broadcast_to(np.array([(fH - 1) / 2.0, (fW - 1) / 2.0]), q.shape).copy()
        d = q - A
        return np.stack([(d[..., 0] * C[1] - C[0] * d[..., 1]) / det, (B[0] * d[..., 1] - B[1] * d[..., 0]) / det], axis=-1)


def invert(F, out_hw, init=None, max_iter=16, tol=1e-9, origin=(0, 0), info=False):
    """G float64 [oH, oW, 2]; info=True: (G, passes int [oH, oW], last residual [oH, oW], largest ||J^-1||_inf seen)"""
    F = np.asarray(F).astype(np.float64)
    oH, oW = int(out_hw[0]), int(out_hw[1])
    ii, jj = np.meshgrid(np.arange(oH) + int(origin[0]), np.arange(oW) + int(origin[1]), indexing="ij")
    q = np.stack([ii, jj], axis=-1).astype(np.float64)
    u = start(F, q) if init is None else np.asarray(init).astype(np.float64).copy()
    G = np.full((oH, oW, 2), np.nan)
    live = np.ones((oH, oW), dtype=bool)                 # entries still iterating
    passes = np.zeros((oH, oW), dtype=np.int64)
    resid = np.full((oH, oW), np.inf)
    jinv = 0.0
    with np.errstate(all="ignore"):
        for _ in range(int(max_iter)):
            live &= ~(np.isnan(u[..., 0]) | np.isnan(u[..., 1]))           # a NaN iterate: NaN, nothing is read
            if not live.any():
                break
            uc, V, Jr, Jc = sample(F, np.where(live[..., None], u, 0.0))
            e = V - q
            passes += live
            bad = np.isnan(e[..., 0]) | np.isnan(e[..., 1])
            res = np.maximum(np.abs(e[..., 0]), np.abs(e[..., 1]))
            resid = np.where(live & ~bad, res, resid)
            live &= ~bad
            hit = live & (np.abs(e[..., 0]) <= tol) & (np.abs(e[..., 1]) <= tol)
            G[hit] = uc[hit]
            live &= ~hit
            det = Jr[..., 0] * Jc[..., 1] - Jr[..., 1] * Jc[..., 0]
            live &= (det != 0.0) & np.isfinite(det)
            if live.any():
                # ||J^-1||_inf of J = [[Jr.r, Jc.r], [Jr.c, Jc.c]]: the larger absolute row sum of adj(J) / det
                n = np.maximum(np.abs(Jc[..., 1]) + np.abs(Jc[..., 0]), np.abs(Jr[..., 1]) + np.abs(Jr[..., 0])) / np.abs(det)
                jinv = max(jinv, float(n[live].max()))
            du = np.stack([(e[..., 0] * Jc[..., 1] - Jc[..., 0] * e[..., 1]) / det, (Jr[..., 0] * e[..., 1] - Jr[..., 1] * e[..., 0]) / det], axis=-1)
            u = np.where(live[..., None], uc - du, u)
    return (G, passes, resid, jinv) if info else G
