"""Times the adjoints of compose and invert on the MI355X for 2160 x 3840 float64 maps (133 MB each; the radial map of
tools/bench_coords.py's invert section):

  compose_bwd   lerf_coords_compose_bwd of the radial map (outer) sampled at a gentle homography's map (inner): both halves, the
                outer half alone (the atomic scatter), the inner half alone (no atomics)
  invert_bwd    lerf_coords_invert_bwd of the radial map at the inverse lerf_coords_invert returned for it
  compose       the forward lerf_coords_compose of the same operands, in the same run
  torch         the only alternative a user had: autograd through a stock-torch restatement of the bilinear sample (clamp, floor,
                four advanced-index gathers, the four-term formula) on the same device -- forward + backward for both gradients,
                and its forward alone

Device events around windows of `--iters` calls; the variants' windows are INTERLEAVED (window k of every variant before window
k + 1 of any) after `--warmup` calls of each; median of `--repeats` windows with [min, max], and the ratios of the medians.  With
each kernel go the bytes per entry that must cross HBM at least once, counted by hand.  Prints ONE JSON line; no
speed gate -- the in-run check is that the kernel's gradients agree with the restatement's to 1e-9 max(max|ref|, 1).

    python tools/bench_coords_grad.py [--iters 20] [--warmup 5] [--repeats 7] [--hw 2160 3840]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12


def torch_compose(torch, a, b):
    """the bilinear sample in stock torch ops, differentiable in both maps"""
    def axis(v, n):
        r = torch.clamp(v, 0.0, float(n - 1))
        i0 = torch.clamp(torch.floor(r.detach()), max=float(n - 2)).long()
        t = r - i0.to(r.dtype)
        return i0, (1.0 - t)[..., None], t[..., None]
    i0, wr0, wr1 = axis(b[..., 0], a.shape[0])
    j0, wc0, wc1 = axis(b[..., 1], a.shape[1])
    return wr0 * (wc0 * a[i0, j0] + wc1 * a[i0, j0 + 1]) + wr1 * (wc0 * a[i0 + 1, j0] + wc1 * a[i0 + 1, j0 + 1])


def interleaved_ms(fns, iters, warmup, repeats):
    """{name: (median, min, max) ms per call}; window k of every variant runs before window k + 1 of any"""
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--hw", type=int, nargs=2, default=[2160, 3840])
    a = ap.parse_args()
    import torch
    from lerf_pytorch_amd import _lib, coords, ops
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    hw = tuple(a.hw)
    entries = hw[0] * hw[1]
    F = coords.radial(hw, hw, 0.08, -0.02, device=dev)
    inner = coords.from_homography(np.array([[1.01, 0.004, 3.0], [-0.003, 0.99, 5.0], [1e-6, -1e-6, 1.0]]), hw, device=dev)
    G = ops.coords_invert(F, hw)
    g = torch.randn(hw + (2,), dtype=torch.float64, device=dev)
    out = torch.empty(hw + (2,), dtype=torch.float64, device=dev)
    ga, gb, gf = (torch.zeros(hw + (2,), dtype=torch.float64, device=dev) for _ in range(3))
    la, lb = F.clone().requires_grad_(True), inner.clone().requires_grad_(True)

    def torch_fwd_bwd():
        la.grad = lb.grad = None
        torch_compose(torch, la, lb).backward(g)

    def torch_fwd():
        with torch.no_grad():
            torch_compose(torch, la, lb)

    fns = {
        "compose_bwd_both": lambda: ops.coords_compose_bwd(F, inner, g, ga, gb),
        "compose_bwd_outer": lambda: ops.coords_compose_bwd(F, inner, g, ga, None, need=(True, False)),
        "compose_bwd_inner": lambda: ops.coords_compose_bwd(F, inner, g, None, gb, need=(False, True)),
        "invert_bwd": lambda: ops.coords_invert_bwd(F, G, g, gf),
        "compose": lambda: ops.coords_compose(F, inner, out=out),
        "torch_fwd_bwd": torch_fwd_bwd,
        "torch_fwd": torch_fwd,
    }
    # bytes per entry that must cross HBM at least once (the gathers of A / F are neighbours' gathers: the map is read once)
    per_entry = {"compose_bwd_both": 16 + 16 + 16 + 32 + 32, "compose_bwd_outer": 16 + 16 + 32, "compose_bwd_inner": 16 + 16 + 16 + 32,
                 "invert_bwd": 16 + 16 + 16 + 32, "compose": 48}
    ms = interleaved_ms(fns, a.iters, a.warmup, a.repeats)
    res = {"tool": "bench_coords_grad", "hw": list(hw), "dtype": "float64", "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats,
           "map_bytes": 16 * entries, "nan_fraction_of_inverse": round(float(torch.isnan(G[..., 0]).float().mean()), 4)}
    for k, t in ms.items():
        res[k] = {"ms": round(t[0], 4), "ms_min": round(t[1], 4), "ms_max": round(t[2], 4)}
        if k in per_entry:
            res[k]["bytes_per_entry"] = per_entry[k]
            res[k]["hbm_fraction"] = round(per_entry[k] * entries / (t[0] * 1e-3) / HBM_PEAK, 4)
    res["ratios"] = {"torch_fwd_bwd_over_compose_bwd_both": round(ms["torch_fwd_bwd"][0] / ms["compose_bwd_both"][0], 2),
                     "torch_fwd_bwd_over_compose_plus_bwd": round(ms["torch_fwd_bwd"][0] / (ms["compose"][0] + ms["compose_bwd_both"][0]), 2),
                     "torch_fwd_over_compose": round(ms["torch_fwd"][0] / ms["compose"][0], 2),
                     "compose_bwd_both_over_compose": round(ms["compose_bwd_both"][0] / ms["compose"][0], 2),
                     "invert_bwd_over_compose_bwd_outer": round(ms["invert_bwd"][0] / ms["compose_bwd_outer"][0], 2)}
    # the in-run check: one fresh backward against the restatement's autograd
    ga.zero_(), gb.zero_()
    ops.coords_compose_bwd(F, inner, g, ga, gb)
    torch_fwd_bwd()
    ok = True
    for name, got, ref in (("grad_outer", ga, la.grad), ("grad_inner", gb, lb.grad)):
        scale = max(float(ref.abs().max()), 1.0)
        err = float((got - ref).abs().max())
        res[name + "_max_error"], res[name + "_scale"] = err, scale
        ok = ok and err <= 1e-9 * scale
    res["agrees_with_torch_autograd"] = ok
    print(json.dumps(res))
    if not ok:
        raise SystemExit("the kernel's gradients differ from the restatement's autograd")


if __name__ == "__main__":
    main()
