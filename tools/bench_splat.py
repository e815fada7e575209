"""Times the forward warp by summation splatting and its adjoint on the MI355X: 1080 x 1920 -> 1080 x 1920, float32, C = 3 + the norm
plane, a float32 map, one frame and a batch of 8.  The map is a smooth flow of a few pixels.

  splat                lerf_splat: one launch, one no-return float atomic add per tap and plane; ADDED bytes = H W 4 taps (C + 1) 4 B
  bwd_all              lerf_splat_bwd, all three halves (grad_src, grad_weight, grad_map): a gather, no atomics
  bwd_image            lerf_splat_bwd, grad_src only
  torch_fwd / torch_fwd_bwd   the alternative a user had: a stock-torch restatement on the same device -- index_add_ over the four taps of
                       the C + 1 planes -- and autograd through it for src, weight and map

Device events around windows of `--iters` calls (`--torch-iters` for the restatement); the variants' windows are INTERLEAVED after
`--warmup` calls of each; median of `--repeats` windows with [min, max], and the ratios of the medians.  The forward's added bytes over
its time are printed next to the float-atomic rate of the chip (about 1.3 TB/s of added bytes for 256-byte contiguous wave accesses).
Prints ONE JSON line; no speed gate -- the in-run check is that the kernel's forward and gradients agree with the restatement's.

    python tools/bench_splat.py [--iters 20] [--torch-iters 3] [--warmup 3] [--repeats 5] [--hw 1080 1920] [--batch 8]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_coords_build_grad import interleaved_ms          # noqa: E402  (the same timing loop)

ATOMIC_RATE = 1.3e12          # added bytes per second, float atomics in 256-byte contiguous wave accesses


def torch_splat(torch, x, f, m, ohw):
    """acc [B, C + 1, oH, oW] of x [B, C, H, W], f [B, H, W, 2] and m [B, H, W] in stock torch ops, differentiable in all three"""
    B, C, H, W = x.shape
    oH, oW = ohw
    r, c = f[..., 0], f[..., 1]
    fr, fc = torch.floor(r).detach(), torch.floor(c).detach()
    tr, tc = r - fr, c - fc
    wr, wc = (1 - tr, tr), (1 - tc, tc)
    xa = torch.cat([x, torch.ones_like(x[:, :1])], 1).permute(1, 0, 2, 3).reshape(C + 1, -1)          # [C + 1, B H W]
    acc = torch.zeros((C + 1, B * oH * oW), dtype=x.dtype, device=x.device)
    base = (torch.arange(B, device=x.device) * (oH * oW))[:, None, None]
    for a in range(2):
        for b in range(2):
            ri, ci = fr + a, fc + b
            inside = (ri >= 0) & (ri <= oH - 1) & (ci >= 0) & (ci <= oW - 1)
            w = torch.where(inside, wr[a] * wc[b] * m, torch.zeros_like(m))
            q = torch.where(inside, ri * oW + ci, torch.zeros_like(ri)).long() + base
            acc = acc.index_add(1, q.reshape(-1), w.reshape(1, -1) * xa)
    return acc.reshape(C + 1, B, oH, oW).permute(1, 0, 2, 3)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--torch-iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hw", type=int, nargs=2, default=[1080, 1920])
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    import torch
    from lerf_pytorch_amd import _lib, ops
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    hw = tuple(a.hw)
    C = 3
    ii, jj = np.meshgrid(np.arange(hw[0], dtype=np.float64), np.arange(hw[1], dtype=np.float64), indexing="ij")
    res = {"tool": "bench_splat", "hw": list(hw), "out_hw": list(hw), "dtype": "float32", "map": "float32", "C": C, "norm": True, "iters": a.iters,
           "torch_iters": a.torch_iters, "warmup": a.warmup, "repeats": a.repeats, "atomic_rate_reference_tb_s": ATOMIC_RATE / 1e12, "cases": {}}
    ok = True
    for B in (1, a.batch):
        flow = np.stack([np.stack([2.7 * np.sin(jj / 97.0 + 0.3 * s) + 1.1 * np.cos(ii / 61.0), 3.4 * np.cos(ii / 131.0 + 0.2 * s) + 0.9 * np.sin(jj / 43.0)], -1)
                         for s in range(B)])
        f = torch.from_numpy((np.stack([ii, jj], -1)[None] + flow).astype(np.float32)).to(dev)
        x = torch.rand((B, C) + hw, dtype=torch.float32, device=dev)
        m = torch.rand((B,) + hw, dtype=torch.float32, device=dev) + 0.5
        g = torch.randn((B, C + 1) + hw, dtype=torch.float32, device=dev)
        acc = torch.zeros((B, C + 1) + hw, dtype=torch.float32, device=dev)
        lx, lm, lf = (t.clone().requires_grad_(True) for t in (x, m, f))

        def torch_fwd():
            with torch.no_grad():
                torch_splat(torch, x, f, m, hw)

        def torch_fwd_bwd():
            lx.grad = lm.grad = lf.grad = None
            torch.autograd.backward(torch_splat(torch, lx, lf, lm, hw), g)

        fns = {"splat": lambda: ops.splat(x, f, hw, m, True, acc=acc),
               "bwd_all": lambda: ops.splat_bwd(x, f, g, m, True),
               "bwd_image": lambda: ops.splat_bwd(x, f, g, m, True, (True, False, False)),
               "torch_fwd": torch_fwd, "torch_fwd_bwd": torch_fwd_bwd}
        iters = {k: (a.torch_iters if k.startswith("torch") else a.iters) for k in fns}
        ms = interleaved_ms(fns, iters, a.warmup, a.repeats)
        case = {}
        for k, t in ms.items():
            case[k] = {"ms": round(t[0], 4), "ms_min": round(t[1], 4), "ms_max": round(t[2], 4)}
        added = B * hw[0] * hw[1] * 4 * (C + 1) * 4
        case["splat"]["added_bytes"] = added
        case["splat"]["added_tb_s"] = round(added / (ms["splat"][0] * 1e-3) / 1e12, 4)
        case["splat"]["fraction_of_atomic_rate"] = round(added / (ms["splat"][0] * 1e-3) / ATOMIC_RATE, 4)
        case["ratios"] = {"torch_fwd_over_splat": round(ms["torch_fwd"][0] / ms["splat"][0], 2),
                          "torch_fwd_bwd_over_splat_plus_bwd_all": round(ms["torch_fwd_bwd"][0] / (ms["splat"][0] + ms["bwd_all"][0]), 2),
                          "bwd_all_over_bwd_image": round(ms["bwd_all"][0] / ms["bwd_image"][0], 2)}
        # the in-run check: one fresh forward and backward against the restatement and its autograd (float32 both: a few ulp of a sum of 16)
        got = ops.splat(x, f, hw, m, True)
        torch_fwd_bwd()
        ref = torch_splat(torch, x, f, m, hw)
        gx, gm, gf = ops.splat_bwd(x, f, g, m, True)
        for name, u, v in (("forward", got, ref), ("grad_src", gx, lx.grad), ("grad_weight", gm, lm.grad), ("grad_map", gf.float(), lf.grad)):
            scale = max(float(v.abs().max()), 1.0)
            err = float((u - v).abs().max())
            case[name + "_max_error"], case[name + "_scale"] = err, scale
            ok = ok and err <= 1e-4 * scale
        res["cases"]["B%d" % B] = case
        del f, x, m, g, acc, lx, lm, lf, got, ref, gx, gm, gf
        torch.cuda.empty_cache()
    res["agrees_with_torch"] = ok
    print(json.dumps(res))
    if not ok:
        raise SystemExit("the kernel differs from the stock-torch restatement")


if __name__ == "__main__":
    main()
