"""Times reproject by depth and its adjoint on the MI355X for 2160 x 3840 maps -- float32 depth in, float64 map plus float32 zo out --
one view and a batch of 8:

  reproject            lerf_coords_reproject: one launch, 24 B per entry (4 in, 16 + 4 out)
  bwd_depth            lerf_coords_reproject_bwd, grad_depth only   (depth 4, grad_map 16, grad_depth_out 8, grad_depth 8 + 8: 44 B)
  bwd_params           grad_params only: the two fixed-order passes (depth 4, grad_map 16, grad_depth_out 8: 28 B)
  bwd_both             both halves in one call                      (44 B)
  brown / brown_bwd    in the same run, the heaviest closed-form builder through lerf_coords_build_dev and lerf_coords_build_bwd (16 B each):
                       the yardstick the forward's share of the HBM rate is stated against
  torch_fwd / torch_fwd_bwd   the alternative a user had: a stock-torch restatement of reproject (broadcast elementwise ops over the pixel
                       grid) on the same device, and autograd through it for depth and the 12 parameters

Device events around windows of `--iters` calls (`--torch-iters` for the restatement); the variants' windows are INTERLEAVED after
`--warmup` calls of each; median of `--repeats` windows with [min, max], and the ratios of the medians.  Prints ONE JSON line; no
speed gate -- the in-run check is that the kernel's gradients agree with the restatement's float64 autograd to 1e-9 max(max|ref|, 1).

    python tools/bench_coords_reproject.py [--iters 20] [--torch-iters 3] [--warmup 3] [--repeats 5] [--hw 2160 3840] [--batch 8]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_coords_build_grad import DIST8, HBM_PEAK, K0, interleaved_ms          # noqa: E402  (the same camera, the same timing loop)

K1 = np.array([[1850.0, 0.0, 1919.5], [0.0, 1850.0, 1079.5], [0.0, 0.0, 1.0]])
POSE_R = [[0.9998000066665778, -0.009999333346666653, 0.017298268171065984],
          [0.010171632387547942, 0.9998994169453621, -0.009901005854503532],
          [-0.017197525080241446, 0.010074974809025127, 0.999801350553843]]
POSE_T = [0.12, -0.05, 0.08]
BYTES = {"reproject": 24, "bwd_depth": 44, "bwd_params": 28, "bwd_both": 44, "brown": 16, "brown_bwd": 16}


def torch_reproject(torch, p, depth):
    """(map [B, H, W, 2] float64, zo [B, H, W] in depth's dtype) of parameters p [B, 12] and depth [B, H, W] in stock torch ops"""
    d = depth.double()
    y = torch.arange(d.shape[1], dtype=torch.float64, device=p.device)[None, :, None]
    x = torch.arange(d.shape[2], dtype=torch.float64, device=p.device)[None, None, :]
    q = [p[:, k, None, None] for k in range(12)]
    a0, a1, a2 = q[0] * x + q[1] * y + q[2], q[3] * x + q[4] * y + q[5], q[6] * x + q[7] * y + q[8]
    X, Y, W = a0 * d + q[9], a1 * d + q[10], a2 * d + q[11]
    ok = (d > 0) & torch.isfinite(d) & (W > 0)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=p.device)
    return torch.where(ok[..., None], torch.stack([Y / W, X / W], dim=-1), nan), torch.where(ok, W, nan).to(depth.dtype)


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
    base = coords.reproject_params(K0, K1, POSE_R, POSE_T)
    brown0 = coords.brown_params(K0, DIST8, None, None)
    ii, jj = np.meshgrid(np.arange(hw[0], dtype=np.float32), np.arange(hw[1], dtype=np.float32), indexing="ij")
    depth0 = (3.0 + np.sin(ii / 97.0) + 0.5 * np.cos(jj / 131.0)).astype(np.float32)
    res = {"tool": "bench_coords_reproject", "hw": list(hw), "depth": "float32", "map": "float64", "zo": "float32", "iters": a.iters,
           "torch_iters": a.torch_iters, "warmup": a.warmup, "repeats": a.repeats, "cases": {}}
    ok = True
    for B in (1, a.batch):
        p = torch.from_numpy(np.stack([base * (1.0 + 1e-3 * s) for s in range(B)])).to(dev)
        pb = torch.from_numpy(np.stack([brown0 * (1.0 + 1e-3 * s) for s in range(B)])).to(dev)
        depth = torch.from_numpy(np.stack([depth0 + 0.01 * s for s in range(B)])).to(dev)
        g = torch.randn((B,) + hw + (2,), dtype=torch.float64, device=dev)
        gz = torch.randn((B,) + hw, dtype=torch.float64, device=dev)
        gz32 = gz.float()
        out = torch.empty((B,) + hw + (2,), dtype=torch.float64, device=dev)
        zo = torch.empty((B,) + hw, dtype=torch.float32, device=dev)
        gd = torch.zeros((B,) + hw, dtype=torch.float64, device=dev)
        gp = torch.zeros((B, 12), dtype=torch.float64, device=dev)
        gpb = torch.zeros((B, 21), dtype=torch.float64, device=dev)
        leaf_p, leaf_d = p.clone().requires_grad_(True), depth.clone().requires_grad_(True)

        def torch_fwd_bwd():
            leaf_p.grad = leaf_d.grad = None
            torch.autograd.backward(torch_reproject(torch, leaf_p, leaf_d), [g, gz32])

        def torch_fwd():
            with torch.no_grad():
                torch_reproject(torch, leaf_p, leaf_d)

        fns = {"reproject": lambda: ops.coords_reproject("z", p, depth, out=out, depth_out=zo),
               "bwd_depth": lambda: ops.coords_reproject_bwd("z", p, depth, g, gz, grad_depth=gd, need=(True, False)),
               "bwd_params": lambda: ops.coords_reproject_bwd("z", p, depth, g, gz, grad_params=gp, need=(False, True)),
               "bwd_both": lambda: ops.coords_reproject_bwd("z", p, depth, g, gz, grad_depth=gd, grad_params=gp),
               "brown": lambda: ops.coords_build_params("brown", pb, hw, out=out),
               "brown_bwd": lambda: ops.coords_build_bwd("brown", pb, g, gpb),
               "torch_fwd": torch_fwd, "torch_fwd_bwd": torch_fwd_bwd}
        iters = {k: (a.torch_iters if k.startswith("torch") else a.iters) for k in fns}
        ms = interleaved_ms(fns, iters, a.warmup, a.repeats)
        case = {"workspace_bytes": int(_lib.lib().lerf_coords_reproject_bwd_workspace_bytes(B, hw[0], hw[1]))}
        for k, t in ms.items():
            case[k] = {"ms": round(t[0], 4), "ms_min": round(t[1], 4), "ms_max": round(t[2], 4)}
            if k in BYTES:
                case[k]["bytes_per_entry"] = BYTES[k]
                case[k]["hbm_fraction"] = round(BYTES[k] * entries * B / (t[0] * 1e-3) / HBM_PEAK, 4)
        case["ratios"] = {"torch_fwd_over_reproject": round(ms["torch_fwd"][0] / ms["reproject"][0], 2),
                          "torch_fwd_bwd_over_reproject_plus_bwd_both": round(ms["torch_fwd_bwd"][0] / (ms["reproject"][0] + ms["bwd_both"][0]), 2),
                          "reproject_over_brown": round(ms["reproject"][0] / ms["brown"][0], 2),
                          "bwd_both_over_brown_bwd": round(ms["bwd_both"][0] / ms["brown_bwd"][0], 2)}
        # the in-run check: one fresh backward against float64 autograd of the restatement (a float64 leaf of the same depths)
        got_d, got_p = ops.coords_reproject_bwd("z", p, depth, g, gz)
        leaf_p.grad = None
        d64 = depth.double().requires_grad_(True)
        torch.autograd.backward(torch_reproject(torch, leaf_p, d64), [g, gz])
        for name, got, ref in (("grad_depth", got_d, d64.grad), ("grad_params", got_p, leaf_p.grad)):
            scale = max(float(ref.abs().max()), 1.0)
            err = float((got - ref).abs().max())
            case[name + "_max_error"], case[name + "_scale"] = err, scale
            ok = ok and err <= 1e-9 * scale
        res["cases"]["B%d" % B] = case
        del g, gz, gz32, out, zo, gd, leaf_p, leaf_d, d64
        torch.cuda.empty_cache()
    res["agrees_with_torch_autograd"] = ok
    print(json.dumps(res))
    if not ok:
        raise SystemExit("the kernel's gradients differ from the restatement's autograd")


if __name__ == "__main__":
    main()
