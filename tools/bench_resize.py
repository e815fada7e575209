"""Times resize_right.resize on the MI355X: 4K -> 1080p and 1080p -> 4K, cubic, for
  u8 HWC numpy-side operands (float64 sums; with and without the uint8 epilogue) and f32 NCHW torch tensors (float32 sums),
  plus f64 NCHW (float64 sums on the torch side).
The operands are on the device before the clock starts (a lazy.DeviceArray for the numpy side), so the figures are the
axis passes alone: device events around `--iters` calls after `--warmup` calls, median of `--repeats` windows.

Per row: ms per call, Gpix/s of OUTPUT pixels, and the bytes the passes must move (every pass reads its input once and
writes its output once; tables are negligible) over the time, as a fraction of the HBM peak (8 TB/s).  The same bytes over
the peak is the least time a memory-bound resize could take; the float64 multiply-adds of the pass (2 flops per tap and
output element) over the float64 vector peak (78.6 TFLOP/s) is the compute bound, printed beside it.
`torch.nn.functional.interpolate(mode="bicubic", antialias=True)` on the same f32 tensors is printed as an outside
yardstick only: it is a different filter at the borders and not a pass criterion.

    python tools/bench_resize.py [--iters 20] [--warmup 5] [--repeats 5] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
F64_PEAK = 78.6e12
F32_PEAK = 157.3e12


def time_ms(fn, iters, warmup, repeats):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return float(np.median(out)), float(min(out)), float(max(out))


def traffic_and_flops(shape, plan, in_bytes, acc_bytes, last_bytes):
    """bytes read + written and multiply-adds * 2 over the passes of `plan` ([(dim, AxisTable)])"""
    shape = list(shape)
    total = flops = 0
    for n, (dim, tab) in enumerate(plan):
        src = int(np.prod(shape)) * (in_bytes if n == 0 else acc_bytes)
        shape[dim] = tab.n_out
        dst = int(np.prod(shape)) * (last_bytes if n == len(plan) - 1 else acc_bytes)
        total += src + dst
        flops += 2 * tab.taps * int(np.prod(shape))
    return total, flops


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", type=str, default="")
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import lerf_pytorch_amd as L  # noqa: F401
    from lerf_pytorch_amd import _lib, lazy
    from lerf_pytorch_amd.resize_right import interp_methods as IM
    from lerf_pytorch_amd.resize_right import resize_right as R
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    rows = []
    for name, (H, W), s in (("4K->1080p", (2160, 3840), 0.5), ("1080p->4K", (1080, 1920), 2.0)):
        u8 = lazy.DeviceArray(torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda())
        f32 = torch.from_numpy(rng.uniform(0, 255, (1, 3, H, W)).astype(np.float32)).cuda()
        f64 = f32.double()
        oh, ow = int(np.ceil(H * s)), int(np.ceil(W * s))
        opix = oh * ow

        def plan_of(shape, is_np):
            sc, sz = R._scales_and_sizes(shape, None, [s, s], False, is_np)
            return R._plan(shape, sc, sz, IM.cubic, None, True, 0, is_np)

        configs = [
            ("u8 HWC, f64 sums -> f64", lambda: R.resize(u8, [s, s]), traffic_and_flops((H, W, 3), plan_of((H, W, 3), True), 1, 8, 8), F64_PEAK),
            ("u8 HWC, f64 sums -> u8", lambda: R.resize_to_uint8(u8, [s, s]), traffic_and_flops((H, W, 3), plan_of((H, W, 3), True), 1, 8, 1), F64_PEAK),
            ("f32 NCHW, f32 sums", lambda: R.resize(f32, [s, s]), traffic_and_flops((1, 3, H, W), plan_of((1, 3, H, W), False), 4, 4, 4), F32_PEAK),
            ("f64 NCHW, f64 sums", lambda: R.resize(f64, [s, s]), traffic_and_flops((1, 3, H, W), plan_of((1, 3, H, W), False), 8, 8, 8), F64_PEAK),
        ]
        for label, fn, (nbytes, flops), peak in configs:
            ms, lo, hi = time_ms(fn, a.iters, a.warmup, a.repeats)
            t_mem, t_alu = nbytes / HBM_PEAK * 1e3, flops / peak * 1e3
            rows.append({"case": name, "config": label, "ms": ms, "ms_min": lo, "ms_max": hi, "gpix_per_s": opix / ms / 1e6,
                         "bytes": nbytes, "hbm_fraction": t_mem / ms, "flops": flops, "alu_fraction": t_alu / ms,
                         "bound_ms": max(t_mem, t_alu), "binding": "memory" if t_mem >= t_alu else "multiply-adds"})
        ms, lo, hi = time_ms(lambda: F.interpolate(f32, size=(oh, ow), mode="bicubic", antialias=True, align_corners=False),
                             a.iters, a.warmup, a.repeats)
        rows.append({"case": name, "config": "yardstick: F.interpolate bicubic antialias f32", "ms": ms, "ms_min": lo, "ms_max": hi,
                     "gpix_per_s": opix / ms / 1e6})
    for r in rows:
        extra = ""
        if "bytes" in r:
            extra = "  %6.1f MB  %5.1f %% of HBM peak  %5.1f %% of the multiply-add peak  (lower bound %.3f ms, %s)" % (
                r["bytes"] / 1e6, 100 * r["hbm_fraction"], 100 * r["alu_fraction"], r["bound_ms"], r["binding"])
        print("%-10s %-48s %8.3f ms [%.3f, %.3f]  %6.2f Gpix/s%s" % (r["case"], r["config"], r["ms"], r["ms_min"], r["ms_max"],
                                                                     r["gpix_per_s"], extra))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
