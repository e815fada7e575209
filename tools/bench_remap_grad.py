"""Times the remap backward (lerf_remap_bwd) against the homographic warp backward (lerf_warp_bwd) of the same run on the MI355X:
Gaussian kind, S = 2, one float32 plane, 1920x1080 -> 3840x2160, the config-4 matrix of bench.py (M_ISC) and the map
coords.from_homography makes of it (float64, device-resident).

  warp_bwd          lerf_warp_bwd: image and three hyper-map gradients
  remap_bwd         lerf_remap_bwd, grad_coords = NULL: the same four gradients, the point read from the map
  remap_bwd_coords  lerf_remap_bwd with grad_coords: plus the float64 map gradient [1, oH, oW, 2]

The launches alone: operands, the map and every gradient buffer are on the device before the clock starts, and the buffers are
accumulated into from call to call (the contract; no memset inside the window).  Device events around `--iters` calls after
`--warmup` calls, median of `--repeats` windows, the three variants interleaved window by window so that they share whatever the
machine does meanwhile.

Bytes per output pixel that must cross HBM at least once: 8 read (grad_out), the four float32 source maps read and their four
gradients updated (32 B per SOURCE pixel, 8 B per output pixel at this scale) -- and for the remap the map entry, 16 B, and for
the map gradient 32 B more (load-add-store of a 16-byte entry).  Prints ONE JSON line; the in-run check is that the remap of the
homography's map returns the warp backward's gradients (GRAD_RTOL rule of the tests: float atomics sum in arrival order).

    python tools/bench_remap_grad.py [--iters 100] [--warmup 10] [--repeats 7]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

M_ISC = [[2.05, 0.12, 15.0], [-0.08, 1.95, 40.0], [1.5e-5, -1.0e-5, 1.0]]     # bench.py config 4
HBM_PEAK = 8.0e12
GRAD_RTOL = 2e-5


def time_interleaved(fns, iters, warmup, repeats):
    """{name: (median, min, max) ms per call}, the functions timed in turn inside every repeat"""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--in-hw", type=int, nargs=2, default=[1080, 1920])
    ap.add_argument("--out-hw", type=int, nargs=2, default=[2160, 3840])
    a = ap.parse_args()
    import torch
    from lerf_pytorch_amd import _lib, coords, ops
    _lib.require_gpu()
    (H, W), out_hw = a.in_hw, tuple(a.out_hw)
    M = np.array(M_ISC)
    S, kind, max_sigma = 2, "gauss", 10.0
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand((1, H, W), generator=gen, device="cuda") * 255
    hs = [torch.rand((1, H, W), generator=gen, device="cuda")]
    hs += [torch.rand((1, H, W), generator=gen, device="cuda") * 0.3 for _ in range(2)]      # sigma <= 3: no vanishing weight sums
    G = torch.randn((1,) + out_hw, generator=gen, device="cuda", dtype=torch.float64)
    wgeo = ops.WarpGeometry((H, W), M, out_hw, S)
    rgeo = ops.RemapGeometry((H, W), torch.from_numpy(coords.from_homography(M, out_hw)).cuda(), S)

    def buffers():
        return [torch.zeros_like(x) for _ in range(4)]

    # in-run check: the map of the homography gives the warp backward's gradients; the map gradient is finite and deterministic
    gw, gr, gr2 = buffers(), buffers(), buffers()
    gc = torch.zeros((1,) + out_hw + (2,), dtype=torch.float64, device="cuda")
    gc2 = torch.zeros_like(gc)
    ops.warp_bwd_planar(x, hs, wgeo, kind, max_sigma, G, gw)
    ops.remap_bwd_planar(x, hs, rgeo, kind, max_sigma, G, gr)
    ops.remap_bwd_planar(x, hs, rgeo, kind, max_sigma, G, gr2, gc)
    ops.remap_bwd_planar(x, hs, rgeo, kind, max_sigma, G, buffers(), gc2)
    worst = 0.0
    for ref, got in zip(gw + gw, gr + gr2):
        scale = max(float(ref.abs().max()), 1.0)
        worst = max(worst, float((got - ref).abs().max()) / scale)
    coords_ok = bool(torch.isfinite(gc).all()) and bool(torch.equal(gc, gc2)) and bool((gc != 0).any())

    t = time_interleaved({
        "warp_bwd": lambda: ops.warp_bwd_planar(x, hs, wgeo, kind, max_sigma, G, gw),
        "remap_bwd": lambda: ops.remap_bwd_planar(x, hs, rgeo, kind, max_sigma, G, gr),
        "remap_bwd_coords": lambda: ops.remap_bwd_planar(x, hs, rgeo, kind, max_sigma, G, gr2, gc)}, a.iters, a.warmup, a.repeats)

    opix = out_hw[0] * out_hw[1]
    src_per_out = 32.0 * H * W / opix
    bytes_px = {"warp_bwd": 8 + src_per_out, "remap_bwd": 8 + src_per_out + 16, "remap_bwd_coords": 8 + src_per_out + 16 + 32}
    res = {"tool": "bench_remap_grad", "kind": kind, "S": S, "planes": 1, "in_hw": [H, W], "out_hw": list(out_hw),
           "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats,
           "ms": {k: {"ms": round(v[0], 4), "ms_min": round(v[1], 4), "ms_max": round(v[2], 4), "gpix_per_s": round(opix / v[0] / 1e6, 3)}
                  for k, v in t.items()},
           "ratio_to_warp_bwd": {k: round(t[k][0] / t["warp_bwd"][0], 3) for k in ("remap_bwd", "remap_bwd_coords")},
           "coords_over_no_coords": round(t["remap_bwd_coords"][0] / t["remap_bwd"][0], 3),
           "bytes_per_out_px": {k: round(v, 2) for k, v in bytes_px.items()},
           "hbm_fraction": {k: round(bytes_px[k] * opix / (t[k][0] * 1e-3) / HBM_PEAK, 4) for k in bytes_px},
           "grads_vs_warp_bwd_rel": worst, "grads_equal_warp_bwd": worst <= GRAD_RTOL, "map_gradient_ok": coords_ok}
    print(json.dumps(res))
    if worst > GRAD_RTOL or not coords_ok:
        raise SystemExit("the remap backward of the homography's map does not reproduce the warp backward")


if __name__ == "__main__":
    main()
