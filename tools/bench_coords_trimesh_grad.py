"""Times the adjoint of the triangle-mesh rasteriser (lerf_coords_trimesh_bwd behind ops.coords_trimesh_bwd) on the MI355X,
on a 2160 x 3840 map, float64:

  jittered  leg (b) of tools/bench_coords_trimesh.py -- a jittered 17 x 30 vertex grid, 928 triangles some 130 pixels wide: the backward
            for attr alone, for attr + pos, and with w for all three; the forward IN THE SAME RUN; and autograd (forward + backward)
            through a stock-torch restatement of the interpolation on the same device, given the same winning-face plane;
  quad      two faces over the whole frame: the KNOWN BAD CASE of one workgroup per face -- two workgroups walk 8.3 M pixels.  Reported,
            not gated.

Device times: device events around `--iters` calls after `--warmup` calls, median of `--repeats` windows; the calls that are compared
are timed in INTERLEAVED windows (one window of each per repeat), so clock and thermal drift meet all alike.  A backward call is what a
user runs: the zeroed gradients, the memsets, the face pass, the vertex passes and the 4-byte read-back of the largest valence (a
synchronisation) are all inside the window.  In-run checks: the device equals the host twin BY BITS on a 135 x 240 crop, and the
full-size gradients lie within 1e-9 * max(max |ref|, 1) of the torch restatement's.  Prints ONE JSON line; there is no speed gate.

    python tools/bench_coords_trimesh_grad.py [--iters 10] [--warmup 3] [--repeats 5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def interleaved_ms(fns, iters, warmup, repeats):
    """{name: (median, min, max) ms per call}: every repeat times one window of each fn in turn"""
    import torch
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / iters)
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ms.items()}


def restated(plane, pos, attr, faces, w, grad_out):
    """the interpolation over the winning faces in stock torch on pos's device, and autograd through it -> (grad_attr, grad_pos, grad_w)"""
    import torch
    P, A = pos.detach().clone().requires_grad_(True), attr.detach().clone().requires_grad_(True)
    Wv = None if w is None else w.detach().clone().requires_grad_(True)
    rows, cols = torch.nonzero(plane >= 0, as_tuple=True)
    f = plane[rows, cols]
    fc = faces.long()
    q = torch.stack([rows.double(), cols.double()], dim=1)

    def edge(P_, Q_):
        return (Q_[:, 1] - P_[:, 1]) * (q[:, 0] - P_[:, 0]) - (Q_[:, 0] - P_[:, 0]) * (q[:, 1] - P_[:, 1])
    a, b, c = P[fc[f, 0]], P[fc[f, 1]], P[fc[f, 2]]
    area2 = (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0]) - (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1])
    lb, lc = edge(c, a) / area2, edge(a, b) / area2
    lam = torch.stack([1.0 - lb - lc, lb, lc], dim=1)
    if Wv is not None:
        lam = lam / torch.stack([Wv[fc[f, 0]], Wv[fc[f, 1]], Wv[fc[f, 2]]], dim=1)
        lam = lam / lam.sum(dim=1, keepdim=True)
    u = (lam[:, :, None] * torch.stack([A[fc[f, 0]], A[fc[f, 1]], A[fc[f, 2]]], dim=1)).sum(dim=1)
    (u * grad_out[rows, cols]).sum().backward()
    return A.grad, P.grad, None if Wv is None else Wv.grad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out-hw", type=int, nargs=2, default=[2160, 3840])
    ap.add_argument("--grid-hw", type=int, nargs=2, default=[17, 30])
    a = ap.parse_args()
    import torch
    from lerf_pytorch_amd import _lib, coords, ops
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    hw, ghw = tuple(a.out_hw), tuple(a.grid_hw)
    res = {"tool": "bench_coords_trimesh_grad", "out_hw": list(hw), "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats}
    ok = True

    def row(t):
        return {"ms": round(t[0], 4), "ms_min": round(t[1], 4), "ms_max": round(t[2], 4)}

    def within(got, ref):
        err = float((got - ref).abs().max())
        return err, err <= 1e-9 * max(float(ref.abs().max()), 1.0)

    def leg(pos_np, attr_np, faces_np, w_np, with_restatement):
        nonlocal ok
        out = {"faces": int(len(faces_np)), "vertices": int(len(pos_np))}
        pd, ad, fd, wd = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (pos_np, attr_np, faces_np, w_np))
        m = torch.empty(hw + (2,), dtype=torch.float64, device=dev)
        keys, keys_w = torch.empty(hw, dtype=torch.int64, device=dev), torch.empty(hw, dtype=torch.int64, device=dev)
        ops.coords_trimesh(pd, ad, fd, hw, out=m, keys=keys)
        ops.coords_trimesh(pd, ad, fd, hw, w=wd, out=m, keys=keys_w)
        gen = torch.Generator(device=dev).manual_seed(3)
        g = torch.randn(hw + (2,), generator=gen, device=dev, dtype=torch.float64)
        plane = torch.where(keys == -1, keys, keys & 0xffffffff)
        calls = {"forward": lambda: ops.coords_trimesh(pd, ad, fd, hw, out=m, keys=keys),
                 "backward_attr": lambda: ops.coords_trimesh_bwd(pd, ad, fd, hw, keys, g, need=(True, False, False)),
                 "backward_attr_pos": lambda: ops.coords_trimesh_bwd(pd, ad, fd, hw, keys, g, need=(True, True, False)),
                 "backward_attr_pos_w": lambda: ops.coords_trimesh_bwd(pd, ad, fd, hw, keys_w, g, w=wd, need=(True, True, True))}
        if with_restatement:
            calls["torch_restatement_fwd_bwd"] = lambda: restated(plane, pd, ad, fd, None, g)
            calls["torch_restatement_fwd_bwd_w"] = lambda: restated(torch.where(keys_w == -1, keys_w, keys_w & 0xffffffff), pd, ad, fd, wd, g)
        t = interleaved_ms(calls, a.iters, a.warmup, a.repeats)
        for name in calls:
            out[name] = row(t[name])
        if with_restatement:
            out["restatement_over_forward_plus_backward"] = round(t["torch_restatement_fwd_bwd"][0] / (t["forward"][0] + t["backward_attr_pos"][0]), 2)
            out["restatement_w_over_forward_plus_backward_w"] = round(t["torch_restatement_fwd_bwd_w"][0] / (t["forward"][0] + t["backward_attr_pos_w"][0]), 2)
        out["covered_fraction"] = round(float((keys != -1).double().mean()), 4)
        # the full-size gradients against the restatement, within the family's bound
        got = ops.coords_trimesh_bwd(pd, ad, fd, hw, keys_w, g, w=wd, need=(True, True, True))
        again = ops.coords_trimesh_bwd(pd, ad, fd, hw, keys_w, g, w=wd, need=(True, True, True))
        ref = restated(torch.where(keys_w == -1, keys_w, keys_w & 0xffffffff), pd, ad, fd, wd, g)
        errs = [within(x, y) for x, y in zip(got, ref)]
        out["max_error_attr_pos_w"] = [float("%.3g" % e[0]) for e in errs]
        out["within_bound"] = all(e[1] for e in errs)
        out["two_runs_equal"] = all(bool(torch.equal(x, y)) for x, y in zip(got, again))
        # a crop against the host twin, by bits
        ch, cw = min(135, hw[0]), min(240, hw[1])
        origin = (hw[0] // 2 - ch // 2, hw[1] // 2 - cw // 2)
        h_out, h_keys = _lib.coords_trimesh_host(pos_np, attr_np, faces_np, (ch, cw), w=w_np, origin=origin, return_keys=True)
        gc = g[origin[0]:origin[0] + ch, origin[1]:origin[1] + cw].contiguous()
        host = _lib.coords_trimesh_bwd_host(pos_np, attr_np, faces_np, (ch, cw), h_keys, gc.cpu().numpy(), w=w_np, origin=origin, need=(True, True, True))
        d_out, d_keys = ops.coords_trimesh(pd, ad, fd, (ch, cw), w=wd, origin=origin, return_keys=True)
        devg = ops.coords_trimesh_bwd(pd, ad, fd, (ch, cw), d_keys, gc, w=wd, origin=origin, need=(True, True, True))
        out["equals_host_on_crop"] = all(np.array_equal(x.cpu().numpy().view(np.uint64), y.view(np.uint64)) for x, y in zip(devg, host))
        ok = ok and out["within_bound"] and out["two_runs_equal"] and out["equals_host_on_crop"]
        return out

    # ---- the jittered vertex grid of tools/bench_coords_trimesh.py, leg (b)
    rng = np.random.default_rng(0)
    gy, gx = np.meshgrid(np.linspace(0, hw[0] - 1, ghw[0]), np.linspace(0, hw[1] - 1, ghw[1]), indexing="ij")
    base = np.stack([gy, gx], axis=-1).reshape(-1, 2)
    step = min((hw[0] - 1) / (ghw[0] - 1), (hw[1] - 1) / (ghw[1] - 1))
    pos_np = base + rng.uniform(-0.2 * step, 0.2 * step, base.shape)
    attr_np = 0.5 * base + 3.0
    rng.uniform(1.0, 2.0, len(base))                                      # the depth draw of that tool: the same w follows
    w_np = 1.0 + 0.25 * rng.uniform(size=len(base))
    res["jittered"] = leg(pos_np, attr_np, coords.grid_faces(*ghw), w_np, True)
    # ---- two faces over the whole frame
    quad = np.array([[-0.5, -0.5], [-0.5, hw[1] - 0.5], [hw[0] - 0.5, -0.5], [hw[0] - 0.5, hw[1] - 0.5]])
    res["quad"] = leg(quad, 0.5 * quad + 3.0, np.array([[0, 1, 2], [3, 2, 1]], np.int32), np.array([1.0, 1.25, 0.8, 1.1]), False)
    res["checks_pass"] = ok
    print(json.dumps(res))
    if not ok:
        raise SystemExit("a gradient differs from the host twin or from the restatement")


if __name__ == "__main__":
    main()
