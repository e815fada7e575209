"""Times the model builders with device parameters and their adjoint on the MI355X for 2160 x 3840 float64 maps (133 MB each), the
homography, the brown, the fisheye and the equirect model, one parameter set and a batch of 8 (fisheye and equirect carry the
library's own square root and arc tangents, a chain of divisions: their times over brown's, in the same run, are reported as
over_brown):

  build_bwd     lerf_coords_build_bwd: grad_params[s][k] += sum over the entries of dp[k], two passes, no atomics
  build         lerf_coords_build_dev: the forward from parameters in device memory, in the same run
  torch         the only alternative a user had: autograd through a stock-torch restatement of the model (broadcast elementwise ops
                over the pixel grid) on the same device -- forward + backward for the parameter gradient, and its forward alone

Device events around windows of `--iters` calls (`--torch-iters` for the restatement, whose calls are long); the variants' windows
are INTERLEAVED (window k of every variant before window k + 1 of any) after `--warmup` calls of each; median of `--repeats` windows
with [min, max], and the ratios of the medians.  With each kernel go the bytes per entry that must cross HBM at least once.  Prints
ONE JSON line; no speed gate -- the in-run check is that the kernel's gradients agree with the restatement's autograd to
1e-9 max(max|ref|, 1).

    python tools/bench_coords_build_grad.py [--iters 20] [--torch-iters 3] [--warmup 3] [--repeats 5] [--hw 2160 3840] [--batch 8]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
M_ISC = np.array([[2.05, 0.12, 15.0], [-0.08, 1.95, 40.0], [1.5e-5, -1.0e-5, 1.0]])
K0 = np.array([[1900.0, 0.0, 1935.5], [0.0, 1890.0, 1071.25], [0.0, 0.0, 1.0]])               # a 4K camera, mild distortion
DIST8 = [0.11, -0.04, 0.002, -0.003, 0.013, 0.02, -0.007, 0.001]
FISH_DIST = [0.05, -0.012, 0.004, -0.0009]
PANO_HW = (4096, 8192)
VIEW_R = [[0.8660254037844387, 0.0, 0.5], [0.0, 1.0, 0.0], [-0.5, 0.0, 0.8660254037844387]]      # the view turned 30 degrees about y


def torch_model(torch, model, p, hw):
    """the map [B, oH, oW, 2] of parameters p [B, n] in stock torch ops, differentiable in p"""
    y = torch.arange(hw[0], dtype=torch.float64, device=p.device)[None, :, None]
    x = torch.arange(hw[1], dtype=torch.float64, device=p.device)[None, None, :]
    q = [p[:, k, None, None] for k in range(p.shape[1])]
    X, Y, Wh = q[0] * x + q[1] * y + q[2], q[3] * x + q[4] * y + q[5], q[6] * x + q[7] * y + q[8]
    if model == "equirect":
        sx, sy, cxp, cyp = q[9:]
        return torch.stack([cyp + sy * torch.atan2(Y, torch.sqrt(X * X + Wh * Wh)), cxp + sx * torch.atan2(X, Wh)], dim=-1)
    u, v = X / Wh, Y / Wh
    if model == "fisheye":
        fx, fy, cx, cy, k1, k2, k3, k4 = q[9:]
        r = torch.sqrt(u * u + v * v)
        th = torch.atan(r)
        th2 = th * th
        s = th * (1 + th2 * (k1 + th2 * (k2 + th2 * (k3 + th2 * k4)))) / r
        return torch.stack([fy * (v * s) + cy, fx * (u * s) + cx], dim=-1)
    if model == "homography":
        return torch.stack([v, u], dim=-1)
    fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 = q[9:]
    r2 = u * u + v * v
    rad = (1 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1 + r2 * (k4 + r2 * (k5 + r2 * k6)))
    xd = u * rad + 2 * p1 * u * v + p2 * (r2 + 2 * u * u)
    yd = v * rad + p1 * (r2 + 2 * v * v) + 2 * p2 * u * v
    return torch.stack([fy * yd + cy, fx * xd + cx], dim=-1)


def interleaved_ms(fns, iters, warmup, repeats):
    """{name: (median, min, max) ms per call}; window k of every variant runs before window k + 1 of any; iters: {name: calls}"""
    import torch
    for k, fn in fns.items():
        for _ in range(min(warmup, iters[k])):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters[k]):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / iters[k])
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--torch-iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hw", type=int, nargs=2, default=[2160, 3840])
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    import torch
    from lerf_pytorch_amd import _lib, coords, ops
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    hw = tuple(a.hw)
    entries = hw[0] * hw[1]
    base = {"homography": np.linalg.inv(M_ISC).reshape(9), "brown": coords.brown_params(K0, DIST8, None, None),
            "fisheye": coords.fisheye_params(K0, FISH_DIST, None, None), "equirect": coords.equirect_params(PANO_HW, K0, VIEW_R)}
    res = {"tool": "bench_coords_build_grad", "hw": list(hw), "dtype": "float64", "iters": a.iters, "torch_iters": a.torch_iters,
           "warmup": a.warmup, "repeats": a.repeats, "map_bytes": 16 * entries, "cases": {}}
    ok = True
    for model in ("homography", "brown", "fisheye", "equirect"):
        for B in (1, a.batch):
            n = base[model].size
            p = torch.from_numpy(np.stack([base[model] * (1.0 + 1e-3 * s) for s in range(B)])).to(dev)
            g = torch.randn((B,) + hw + (2,), dtype=torch.float64, device=dev)
            out = torch.empty((B,) + hw + (2,), dtype=torch.float64, device=dev)
            gp = torch.zeros((B, n), dtype=torch.float64, device=dev)
            leaf = p.clone().requires_grad_(True)

            def torch_fwd_bwd():
                leaf.grad = None
                torch_model(torch, model, leaf, hw).backward(g)

            def torch_fwd():
                with torch.no_grad():
                    torch_model(torch, model, leaf, hw)

            fns = {"build_bwd": lambda: ops.coords_build_bwd(model, p, g, gp), "build": lambda: ops.coords_build_params(model, p, hw, out=out),
                   "torch_fwd_bwd": torch_fwd_bwd, "torch_fwd": torch_fwd}
            iters = {"build_bwd": a.iters, "build": a.iters, "torch_fwd_bwd": a.torch_iters, "torch_fwd": a.torch_iters}
            ms = interleaved_ms(fns, iters, a.warmup, a.repeats)
            per_entry = {"build_bwd": 16, "build": 16}           # grad_map read once / the map written once; the partials are KBs
            case = {"n_params": n, "workspace_bytes": int(_lib.lib().lerf_coords_build_bwd_workspace_bytes(n, B, hw[0], hw[1]))}
            for k, t in ms.items():
                case[k] = {"ms": round(t[0], 4), "ms_min": round(t[1], 4), "ms_max": round(t[2], 4)}
                if k in per_entry:
                    case[k]["bytes_per_entry"] = per_entry[k]
                    case[k]["hbm_fraction"] = round(per_entry[k] * entries * B / (t[0] * 1e-3) / HBM_PEAK, 4)
            case["ratios"] = {"torch_fwd_bwd_over_build_bwd": round(ms["torch_fwd_bwd"][0] / ms["build_bwd"][0], 2),
                              "torch_fwd_bwd_over_build_plus_bwd": round(ms["torch_fwd_bwd"][0] / (ms["build"][0] + ms["build_bwd"][0]), 2),
                              "torch_fwd_over_build": round(ms["torch_fwd"][0] / ms["build"][0], 2),
                              "build_bwd_over_build": round(ms["build_bwd"][0] / ms["build"][0], 2)}
            # the in-run check: one fresh backward against the restatement's autograd
            got = ops.coords_build_bwd(model, p, g)
            torch_fwd_bwd()
            scale = max(float(leaf.grad.abs().max()), 1.0)
            err = float((got - leaf.grad).abs().max())
            case["grad_max_error"], case["grad_scale"] = err, scale
            ok = ok and err <= 1e-9 * scale
            if model in ("fisheye", "equirect"):
                brown = res["cases"]["brown_B%d" % B]
                case["over_brown"] = {k: round(case[k]["ms"] / brown[k]["ms"], 2) for k in ("build", "build_bwd")}
            res["cases"]["%s_B%d" % (model, B)] = case
            del g, out, leaf
            torch.cuda.empty_cache()
    res["agrees_with_torch_autograd"] = ok
    print(json.dumps(res))
    if not ok:
        raise SystemExit("the kernel's gradients differ from the restatement's autograd")


if __name__ == "__main__":
    main()
