"""Reference side of the remap-gradient tests: a float64 torch autograd restatement of the remap, device-agnostic.

`restated_remap` is `_restated_warp` of tests/test_gpu_warp_grad.py with two changes: the projected point is READ from
`coords` (a tensor that may require grad) and clamped to [0, H] x [0, W], and the fixed kinds are evaluated by calling
lerf_pytorch_amd.resize_right.interp_methods on the float64 distances, so their derivative is what autograd gives for those
forms.  It is the yardstick for the map gradient; tests/test_remap_grad_cpu.py anchors it: its forward against the oracle's
remap forward, its map gradient against central finite differences of that forward.

`margins` is the distance of every map entry from the places where the remap is not differentiable in the point: the support's
left-boundary switch, the clip borders and (amplified linear) the class borders d = 0, +-1."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
NP_PAD = {"constant": "constant", "replicate": "edge", "reflect": "reflect", "circular": "wrap"}
FIXED = {"cubic": "cubic", "bilinear": "linear", "lanczos2": "lanczos2", "lanczos3": "lanczos3", "nearest": "box"}


def _pad_index(idx, n, mode, torch):
    """image pad rule of F.pad for unpadded index idx (any integer): (index, inside-or-remapped mask)"""
    if mode == "constant":
        return idx.clamp(0, n - 1), (idx >= 0) & (idx < n)
    if mode == "replicate":
        return idx.clamp(0, n - 1), torch.ones_like(idx, dtype=torch.bool)
    if mode == "reflect":
        p = 2 * (n - 1)
        m = torch.remainder(idx, p)
        return torch.where(m < n, m, p - m), torch.ones_like(idx, dtype=torch.bool)
    assert mode == "circular", mode
    return torch.remainder(idx, n), torch.ones_like(idx, dtype=torch.bool)


def restated_remap(kind, S, pad_mode, coords, pads, x, hs, max_sigma):
    """coords: [oH, oW, 2] (row, col) float32 / float64 tensor, may require grad; pads = (pad_r_lo, pad_c_lo); x: float32
    [N, H, W]; hs: float32 [N, H, W] hyper maps (3 gauss, 1 linear, none otherwise); pad_mode: F.pad's name.  Returns float64
    [N, oH, oW].  A NaN entry is read as 0 (it has no gradient path): the caller ignores the output there."""
    import torch
    from lerf_pytorch_amd.resize_right import interp_methods
    N, H, W = x.shape
    dev = x.device
    q = coords.double()
    q = torch.where(torch.isnan(q), torch.zeros((), dtype=torch.float64, device=q.device), q)
    r = q[..., 0].clamp(0, H)
    c = q[..., 1].clamp(0, W)
    prl, pcl = int(pads[0]), int(pads[1])
    lr = torch.ceil(r.detach() - S / 2 - EPS32).long() + prl
    lc = torch.ceil(c.detach() - S / 2 - EPS32).long() + pcl
    gr, gc = r + prl, c + pcl
    ws, vs = [], []
    for a in range(S):
        for b in range(S):
            pr = (lr + b).clamp(0, H - 1)
            pc = (lc + a).clamp(0, W - 1)
            dx, dy = gr - pr.double(), gc - pc.double()
            sr, sc = pr - prl, pc - pcl
            rcl, ccl = sr.clamp(0, H - 1), sc.clamp(0, W - 1)
            ri, rm = _pad_index(sr, H, pad_mode, torch)
            ci, cm = _pad_index(sc, W, pad_mode, torch)
            v = torch.where(rm & cm, x[:, ri, ci], torch.zeros((), dtype=x.dtype, device=dev))
            if kind == "gauss":
                rho = (hs[0] * 2 - 1)[:, rcl, ccl].double()
                sx = (hs[1] * max_sigma)[:, rcl, ccl].double()
                sy = (hs[2] * max_sigma)[:, rcl, ccl].double()
                e = (sx * dx) ** 2 - 2 * rho * (sx * dx * sy * dy) + (sy * dy) ** 2
                w = torch.exp(-0.5 * e)
            elif kind == "linear":
                al = (max_sigma * (hs[0] * 2 - 1))[:, rcl, ccl].double()

                def lin(t):
                    return (al * t + 1) * ((-1 <= t) & (t < 0)) + (1 - al * t) * ((0 <= t) & (t <= 1))
                w = torch.clamp(lin(dx), 0, None) * torch.clamp(lin(dy), 0, None)
            else:
                k1 = getattr(interp_methods, FIXED[kind])
                w = (k1(dx) * k1(dy))[None].expand(N, -1, -1)
            ws.append(w)
            vs.append(v)
    if kind not in ("gauss", "linear") and S == 1:        # warp() does not normalise the fixed kinds at S = 1
        return sum(v * w for v, w in zip(vs, ws))
    Wsum = sum(ws)
    return sum(v * (w / Wsum) for v, w in zip(vs, ws))


def pads_of(coords, in_hw, S):
    """(pad_r_lo, pad_c_lo) the remap derives from entry (0, 0): max(-left_boundary(clip(.)), 0) (calc_pad_sz)"""
    q = np.asarray(coords.detach().cpu().numpy() if hasattr(coords, "detach") else coords, np.float64)[0, 0]
    q = np.where(np.isnan(q), 0.0, q)
    return tuple(max(-int(np.ceil(min(max(float(q[k]), 0.0), in_hw[k]) - S / 2 - EPS32)), 0) for k in range(2))


def margins(kind, S, coords, pads, in_hw):
    """numpy [oH, oW]: per entry, the distance (in source pixels) of the point from the nearest place where the remap is not
    differentiable in it -- left-boundary switch of either axis, the clip borders 0 and n, and for kind == "linear" a tap
    distance at 0 or +-1"""
    q = np.asarray(coords, np.float64)
    out = np.full(q.shape[:2], np.inf)
    for k, n, pad in ((0, in_hw[0], pads[0]), (1, in_hw[1], pads[1])):
        u = q[..., k]
        m = np.minimum(np.abs(u), np.abs(u - n))                             # the clip borders (inside or outside)
        g = np.clip(u, 0, n)
        t = g - S / 2 - EPS32
        inner = np.abs(t - np.round(t))                                      # ceil switches at an integer
        if kind == "linear":
            left = np.ceil(t).astype(np.int64) + pad
            for j in range(S):
                d = g + pad - np.clip(left + j, 0, n - 1)
                for edge in (-1.0, 0.0, 1.0):
                    inner = np.minimum(inner, np.abs(d - edge))
        # a point outside the clip does not move with its entry: only the border itself is a discontinuity of that axis
        out = np.minimum(out, np.where((u > 0) & (u < n), np.minimum(m, inner), m))
    return out
