"""A plain numpy restatement of the forward warp by summation splatting and of its adjoint, written from the statement of the
operation (include/lerf_hip.h above lerf_splat); it imports nothing of the library.  Float64 statements in the stated order, one
rounding to the image dtype T where a value is added (forward) or stored (backward).  The forward adds in row-major source order,
taps in the order (0,0) (0,1) (1,0) (1,1) -- the order of the host twin -- and also returns, per output element, the number n[q]
of contributions and the sum of their magnitudes: the two figures of the bound of a reordered sum."""
import numpy as np


def _axis(v, n):
    """floor, the two weights, the frame test in floating point, then the int base: for a finite v (others: masked by the caller)"""
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(v)
        t = v - f
        w = np.stack([1.0 - t, t], 0)
        last = float(n - 1)
        inside = np.stack([(f >= 0.0) & (f <= last), (f + 1.0 >= 0.0) & (f + 1.0 <= last)], 0)
        i0 = np.where(inside[0] | inside[1], f, 0.0).astype(np.int64)
    return i0, w, inside


def _taps(F, oH, oW):
    """per source pixel [H, W] and tap t = 2a + b: on, inside, w (float64), q (flat index into [oH, oW]); finite: the position counts"""
    F = np.asarray(F).astype(np.float64)                       # a float32 map is promoted exactly
    r, c = F[..., 0], F[..., 1]
    with np.errstate(invalid="ignore"):
        finite = ((r - r) == 0.0) & ((c - c) == 0.0)
    r, c = np.where(finite, r, 0.0), np.where(finite, c, 0.0)
    i0, wr, inr = _axis(r, oH)
    j0, wc, inc = _axis(c, oW)
    on, inside, w, q = [], [], [], []
    for a in range(2):
        for b in range(2):
            ins = inr[a] & inc[b] & finite
            inside.append(ins)
            on.append(ins & (wr[a] != 0.0) & (wc[b] != 0.0))
            w.append(wr[a] * wc[b])
            q.append(np.where(ins, (i0 + a) * oW + (j0 + b), 0))
    return finite, np.stack(on, -1), np.stack(inside, -1), np.stack(w, -1), np.stack(q, -1), wr, wc


def splat_one(X, F, M, out_hw, norm, acc=None):
    """one set: X [C, H, W] of dtype T, F [H, W, 2], M [H, W] of T or None -> (acc [C (+ 1), oH, oW] of T, n, mag); acc given:
    accumulated into.  n [C (+ 1), oH, oW] int64 and mag float64: the count and the sum of |term| of THIS call's contributions"""
    X = np.asarray(X)
    T = X.dtype
    C, H, W = X.shape
    oH, oW = out_hw
    planes = C + (1 if norm else 0)
    acc = np.zeros((planes, oH, oW), T) if acc is None else acc
    n = np.zeros((planes, oH * oW), np.int64)
    mag = np.zeros((planes, oH * oW), np.float64)
    finite, on, inside, w, q, _, _ = _taps(F, oH, oW)
    m = np.ones((H, W), np.float64) if M is None else np.asarray(M).astype(np.float64)
    wm = w * m[..., None]                                      # (wr[a] * wc[b]) * m
    sel = on.reshape(-1)                                       # source-major, tap-minor: row-major source order, taps in order
    idx = q.reshape(-1)[sel]
    flat = acc.reshape(planes, oH * oW)
    for k in range(planes):
        with np.errstate(invalid="ignore", over="ignore"):
            term = (wm * X[k].astype(np.float64)[..., None] if k < C else wm).astype(T)          # rounded once to T
        v = term.reshape(-1)[sel]
        np.add.at(flat[k], idx, v)                             # unbuffered, in index order: an add in T per contribution
        np.add.at(n[k], idx, 1)
        np.add.at(mag[k], idx, np.abs(v.astype(np.float64)))
    return acc, n.reshape(planes, oH, oW), mag.reshape(planes, oH, oW)


def splat(X, F, M, out_hw, norm, acc=None):
    """a batch: X [B, C, H, W], F [H, W, 2] (shared) or [B, H, W, 2], M [B, H, W] or None -> (acc, n, mag), each [B, C (+ 1), oH, oW]"""
    X = np.asarray(X)
    B = X.shape[0]
    outs = [splat_one(X[s], F if np.ndim(F) == 3 else F[s], None if M is None else M[s], out_hw, norm, None if acc is None else acc[s])
            for s in range(B)]
    return tuple(np.stack([o[k] for o in outs], 0) for k in range(3))


def splat_bwd_one(X, F, M, G, norm, need=(True, True, True)):
    """one set: the adjoint at G [C (+ 1), oH, oW] of T -> (grad_X [C, H, W] of T, grad_M [H, W] of T, grad_F [H, W, 2] float64); None
    for a half that need[k] skips.  Every sum starts at +0.0 and adds its terms in the stated order; a skipped term adds +0.0, which
    leaves such a sum unchanged bit for bit (it is never -0.0)."""
    X = np.asarray(X)
    T = X.dtype
    C, H, W = X.shape
    planes, oH, oW = G.shape
    assert planes == C + (1 if norm else 0)
    finite, on, inside, w, q, wr, wc = _taps(F, oH, oW)
    m = np.ones((H, W), np.float64) if M is None else np.asarray(M).astype(np.float64)
    Gf = np.asarray(G).reshape(planes, oH * oW)
    read = inside & (on | bool(need[2]))
    want_s = need[1] or need[2]
    S = np.zeros((H, W, 4), np.float64)
    gX = np.zeros((C, H, W), T) if need[0] else None
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(C):
            g = np.where(read, Gf[k][q].astype(np.float64), 0.0)
            if need[0]:
                s = np.zeros((H, W), np.float64)
                for t in range(4):
                    s = s + np.where(on[..., t], w[..., t] * g[..., t], 0.0)
                gX[k] = np.where(finite, m * s, 0.0).astype(T)
            if want_s:
                S = S + np.where(read, X[k].astype(np.float64)[..., None] * g, 0.0)
        if not want_s:
            return gX, None, None
        if norm:
            S = S + np.where(read, Gf[C][q].astype(np.float64), 0.0)
        sm = np.zeros((H, W), np.float64)
        for t in range(4):
            sm = sm + np.where(on[..., t], w[..., t] * S[..., t], 0.0)
        gM = np.where(finite, sm, 0.0).astype(T) if need[1] else None
        gF = None
        if need[2]:
            dr = np.zeros((H, W), np.float64)
            dc = np.zeros((H, W), np.float64)
            for b in range(2):
                dr = dr + np.where(wc[b] != 0.0, wc[b] * (S[..., 2 + b] - S[..., b]), 0.0)
            for a in range(2):
                dc = dc + np.where(wr[a] != 0.0, wr[a] * (S[..., 2 * a + 1] - S[..., 2 * a]), 0.0)
            gF = np.stack([np.where(finite, m * dr, 0.0), np.where(finite, m * dc, 0.0)], -1)
    return gX, gM, gF


def splat_bwd(X, F, M, G, norm, need=(True, True, True)):
    """a batch: per set like splat_bwd_one; grad_F [B, H, W, 2] (one per set, also for a shared map)"""
    X = np.asarray(X)
    outs = [splat_bwd_one(X[s], F if np.ndim(F) == 3 else F[s], None if M is None else M[s], G[s], norm, need) for s in range(X.shape[0])]
    return tuple(None if outs[0][k] is None else np.stack([o[k] for o in outs], 0) for k in range(3))


def torch_splat(X, F, M, out_hw, norm):
    """the forward in differentiable torch ops (index_add_ over the four taps), for autograd: X [C, H, W] or [B, C, H, W], F [H, W, 2] or
    [B, H, W, 2], M None or [H, W] / [B, H, W], on one device, float64 -> acc [.., C (+ 1), oH, oW].  floor is a constant of the graph:
    the derivative is that of the cell floor picked."""
    import torch
    if X.ndim == 4:
        return torch.stack([torch_splat(X[s], F if F.ndim == 3 else F[s], None if M is None else M[s], out_hw, norm) for s in range(X.shape[0])])
    oH, oW = out_hw
    C, H, W = X.shape
    r, c = F[..., 0].double(), F[..., 1].double()
    finite = torch.isfinite(r) & torch.isfinite(c)
    r, c = torch.where(finite, r, torch.zeros_like(r)), torch.where(finite, c, torch.zeros_like(c))
    fr, fc = torch.floor(r).detach(), torch.floor(c).detach()
    tr, tc = r - fr, c - fc
    wr, wc = (1.0 - tr, tr), (1.0 - tc, tc)
    Xa = X.double() if not norm else torch.cat([X.double(), torch.ones((1, H, W), dtype=torch.float64, device=X.device)])
    m = torch.ones_like(r) if M is None else M.double()
    acc = torch.zeros((Xa.shape[0], oH * oW), dtype=torch.float64, device=X.device)
    for a in range(2):
        for b in range(2):
            ri, ci = fr + a, fc + b
            inside = finite & (ri >= 0) & (ri <= oH - 1) & (ci >= 0) & (ci <= oW - 1)
            w = torch.where(inside, (wr[a] * wc[b]) * m, torch.zeros_like(r))
            q = torch.where(inside, ri * oW + ci, torch.zeros_like(r)).long()
            acc = acc.index_add(1, q.reshape(-1), (w[None] * Xa).reshape(Xa.shape[0], -1))
    return acc.reshape(Xa.shape[0], oH, oW)
