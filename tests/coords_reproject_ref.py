"""Restatement of coords.reproject and of its adjoint in numpy float64, statement by statement, written from the operation's
definition and not from the C++ text; and the same forward in torch float64 for autograd.  It does not import the
library.

    forward(kind, params, depth, origin)                 -> map [.., H, W, 2] float64, zo [.., H, W] float64 (before any rounding)
    entry_grads(kind, params, depth, g, gz, origin)      -> dp [H, W, 12], dd [H, W] of ONE set
    ordered_sum(x)                                       -> the sum of x [H, W] in the adjoint's fixed order (two passes, bands, trees)
    grads(kind, params, depth, g, gz, origin)            -> grad_depth [.., H, W], grad_params [.., 12]
    forward_torch(kind, params, depth, origin)           -> map, zo as float64 tensors, differentiable where the entry is valid
    params_torch(K_src, K_dst, R, t)                     -> the 12-vector in torch ops

numpy rounds every elementwise product and sum once, so the order of the Python expressions IS the rounding order.
"""
import numpy as np
import torch

Z, INVERSE = "z", "inverse"


def _xy(hw, origin):
    i = np.arange(hw[0], dtype=np.float64)[:, None] + float(origin[0])
    j = np.arange(hw[1], dtype=np.float64)[None, :] + float(origin[1])
    return np.broadcast_to(j, hw), np.broadcast_to(i, hw)          # x = column, y = row


def _one_forward(kind, p, depth, origin):
    """every intermediate of one set: dict of [H, W] float64 arrays; `ok` is the validity mask"""
    m, q = p[:9], p[9:]
    dep = np.asarray(depth).astype(np.float64)                        # float32 -> float64 is exact
    x, y = _xy(dep.shape, origin)
    with np.errstate(all="ignore"):
        a0 = (m[0] * x + m[1] * y) + m[2]
        a1 = (m[3] * x + m[4] * y) + m[5]
        a2 = (m[6] * x + m[7] * y) + m[8]
        if kind == Z:
            X, Y, W = a0 * dep + q[0], a1 * dep + q[1], a2 * dep + q[2]
            zo = W
            ok = dep > 0
        else:
            X, Y, W = a0 + q[0] * dep, a1 + q[1] * dep, a2 + q[2] * dep
            zo = np.where(dep == 0, np.inf, W / dep)
            ok = dep >= 0
        ok = ok & (dep - dep == 0) & (W > 0)
        col, row = X / W, Y / W
    return dict(x=x, y=y, a0=a0, a1=a1, a2=a2, W=W, dep=dep, ok=ok, col=np.where(ok, col, np.nan), row=np.where(ok, row, np.nan),
                zo=np.where(ok, zo, np.nan))


def forward(kind, params, depth, origin=(0, 0)):
    """params [12] with depth [H, W], or [B, 12] with depth [B, H, W] or one shared [H, W]"""
    p = np.asarray(params, np.float64)
    if p.ndim == 2:
        both = [forward(kind, p[s], depth[s] if np.ndim(depth) == 3 else depth, origin) for s in range(p.shape[0])]
        return np.stack([b[0] for b in both]), np.stack([b[1] for b in both])
    f = _one_forward(kind, p, depth, origin)
    return np.stack([f["row"], f["col"]], axis=-1), f["zo"]


def entry_grads(kind, p, depth, g, gz=None, origin=(0, 0)):
    """the adjoint of one set, entry by entry: dp [H, W, 12] (d loss / d params from that entry) and dd [H, W] (d loss / d depth)"""
    f = _one_forward(kind, np.asarray(p, np.float64), depth, origin)
    x, y, a0, a1, a2, W, dep, col, row, zo = (f[k] for k in ("x", "y", "a0", "a1", "a2", "W", "dep", "col", "row", "zo"))
    q = np.asarray(p, np.float64)[9:]
    gr, gc = g[..., 0], g[..., 1]
    gz = np.zeros_like(dep) if gz is None else np.asarray(gz, np.float64)
    with np.errstate(all="ignore"):
        zfin = zo - zo == 0
        fin = (row - row == 0) & (col - col == 0)
        dX, dY = gc / W, gr / W
        dWm = -((gc * col + gr * row) / W)
        if kind == Z:
            dW = dWm + np.where(zfin, gz, 0.0)
            dd = (dX * a0 + dY * a1) + dW * a2
            A = (dX * dep, dY * dep, dW * dep)
            Q = (dX, dY, dW)
        else:
            gzd = np.where(zfin, gz / dep, 0.0)
            gzz = np.where(zfin, gzd * zo, 0.0)
            dW = dWm + gzd
            dd = ((dX * q[0] + dY * q[1]) + dW * q[2]) - gzz
            A = (dX, dY, dW)
            Q = (dX * dep, dY * dep, dW * dep)
        dp = np.stack([A[0] * x, A[0] * y, A[0], A[1] * x, A[1] * y, A[1], A[2] * x, A[2] * y, A[2], Q[0], Q[1], Q[2]], axis=-1)
    return np.where(fin[..., None], dp, 0.0), np.where(fin, dd, 0.0)


def _tree64(v):
    """the 64 values on the last axis by the tree of offsets 32 .. 1 -> the last axis gone"""
    v = v.copy()
    off = 32
    while off:
        v[..., :off] = v[..., :off] + v[..., off:2 * off]
        off //= 2
    return v[..., 0]


def ordered_sum(x):
    """the sum of x [H, W] in the fixed order of the adjoint: bands of 64 rows x 64 columns, in a band 4 x 64 lanes (w, l), lane (w, l)
    adds rows w, w + 4, ... of column l in order; the 64 lanes of w by the tree; ((w0 + w1) + w2) + w3 = the band's partial; then 64 lanes
    over the partials (lane l: partials l, l + 64, ...), the tree again"""
    H, W = x.shape
    nby, nbx = -(-H // 64), -(-W // 64)
    with np.errstate(all="ignore"):
        pad = np.zeros((nby * 64, nbx * 64))
        pad[:H, :W] = x
        v = pad.reshape(nby, 16, 4, nbx, 64)                          # row = by * 64 + 4 * t + w
        acc = np.zeros((nby, 4, nbx, 64))
        for t in range(16):
            acc = acc + v[:, t]
        ws = _tree64(acc)                                             # [nby, 4, nbx]
        part = (((ws[:, 0] + ws[:, 1]) + ws[:, 2]) + ws[:, 3]).reshape(-1)          # [by * nbx + bx]
        n = -(-part.size // 64)
        pp = np.zeros(n * 64)
        pp[:part.size] = part
        pp = pp.reshape(n, 64)
        acc = np.zeros(64)
        for t in range(n):
            acc = acc + pp[t]
        return _tree64(acc)


def grads(kind, params, depth, g, gz=None, origin=(0, 0)):
    """(grad_depth [.., H, W], grad_params [.., 12]) from zero: what the adjoint ADDS to its buffers"""
    p = np.asarray(params, np.float64)
    if p.ndim == 2:
        both = [grads(kind, p[s], depth[s] if np.ndim(depth) == 3 else depth, g[s], None if gz is None else gz[s], origin)
                for s in range(p.shape[0])]
        return np.stack([b[0] for b in both]), np.stack([b[1] for b in both])
    dp, dd = entry_grads(kind, p, depth, g, gz, origin)
    return dd, np.array([ordered_sum(dp[..., k]) for k in range(12)])


# ---------------------------------------------------------------------------------------------- torch, for autograd
def params_torch(K_src, K_dst, R=None, t=None):
    """K_dst . R . inv(K_src) row-major, K_dst . t -> float64 [12]"""
    Ks, Kd = K_src.double(), K_dst.double()
    KR = Kd if R is None else Kd @ R.double()
    q = torch.zeros(3, dtype=torch.float64, device=Ks.device) if t is None else Kd @ t.double()
    return torch.cat([(KR @ torch.linalg.inv(Ks)).reshape(9), q])


def forward_torch(kind, params, depth, origin=(0, 0)):
    """the map [H, W, 2] and zo [H, W] of ONE set in stock torch float64, on params' device.  An entry that is not valid is NaN and is
    evaluated at harmless operands, so that autograd returns exactly 0 for it (the library's rule) instead of NaN; so is a zo of +inf."""
    p, dep = params.double(), depth.double()
    H, W = dep.shape
    y = (torch.arange(H, dtype=torch.float64, device=p.device) + float(origin[0]))[:, None].expand(H, W)
    x = (torch.arange(W, dtype=torch.float64, device=p.device) + float(origin[1]))[None, :].expand(H, W)
    a0 = p[0] * x + p[1] * y + p[2]
    a1 = p[3] * x + p[4] * y + p[5]
    a2 = p[6] * x + p[7] * y + p[8]
    finite = torch.isfinite(dep)
    one = torch.ones((), dtype=torch.float64, device=p.device)
    with torch.no_grad():
        Wt = a2 * dep + p[11] if kind == Z else a2 + p[11] * dep
        ok = (dep > 0 if kind == Z else dep >= 0) & finite & (Wt > 0)
    d = torch.where(ok, dep, one)
    if kind == Z:
        X, Y, Wh = a0 * d + p[9], a1 * d + p[10], a2 * d + p[11]
        zo = Wh
    else:
        X, Y, Wh = a0 + p[9] * d, a1 + p[10] * d, a2 + p[11] * d
        far = d == 0
        zo = torch.where(far, torch.full_like(d, float("inf")), Wh / torch.where(far, one, d))
    Wh = torch.where(ok, Wh, one)
    nan = torch.full_like(dep, float("nan"))
    return torch.stack([torch.where(ok, Y / Wh, nan), torch.where(ok, X / Wh, nan)], dim=-1), torch.where(ok, zo, nan)
