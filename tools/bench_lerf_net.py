#!/usr/bin/env python3
"""LeRF-Net (IMDN2, nf 64, inC 3, outC 3) forward on the HIP path (lerf_imdn_fwd_f32) against the same network as stock
PyTorch float32 convolutions (F.conv2d, MIOpen: what the reference's module runs), on seeded weights.  Prints one JSON line.

    python tools/bench_lerf_net.py [--steps K] [--warmup W] [--nf 64]

Sizes: a 1x3x1080x1920 frame, and the Set5 x2 LR images (tests/data/Set5/LR_bicubic/rrLR_X2.00_2.00, one launch each,
summed per set).  FLOPs = 2 x the network's multiply-adds per pixel x pixels; utilisation = those FLOPs / time / 157.3
TFLOP/s (the float32-input MFMA peak).  max_abs_diff: HIP against stock torch, stage 1 and 2 raw outputs, 1080p frame."""
import argparse
import glob
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import imdn_ref64 as R  # noqa: E402
from lerf_pytorch_amd.resample.model import IMDN2  # noqa: E402

PEAK_F32_MFMA = 157.3e12


def macs_per_pixel(nf, in_nc, out_nc):
    return sum(int(np.prod(s)) for k, s in R.state_keys(nf, in_nc, out_nc) if k.endswith(".weight"))


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nf", type=int, default=64)
    args = ap.parse_args()
    nf, inC, outC = args.nf, 3, 3
    sd = R.weight_rule(nf, inC, outC, 2701)
    m = IMDN2(types.SimpleNamespace(nf=nf, norm=255), inC=inC, outC=outC)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m.cuda().eval()
    sdt = {k: torch.from_numpy(v).cuda() for k, v in sd.items()}
    mac = {1: macs_per_pixel(nf, inC, inC), 2: macs_per_pixel(nf, inC, inC * outC)}
    frame = torch.rand((1, inC, 1080, 1920), generator=torch.Generator().manual_seed(0)).cuda()
    from PIL import Image
    lr_dir = os.path.join(ROOT, "tests", "data", "Set5", "LR_bicubic", "rrLR_X2.00_2.00")
    set5 = [torch.from_numpy(np.asarray(Image.open(p).convert("RGB"), np.float32) / 255.0).permute(2, 0, 1)[None].contiguous().cuda()
            for p in sorted(glob.glob(os.path.join(lr_dir, "*.png")))]
    res = {"tool": "bench_lerf_net", "nf": nf, "inC": inC, "outC": outC, "steps": args.steps, "warmup": args.warmup}
    for name, xs in (("1080p", [frame]), ("set5_x2", set5)):
        px = sum(x.shape[2] * x.shape[3] for x in xs)
        with torch.no_grad():
            t1 = timed(lambda: [m.stage1(x) for x in xs], args.steps, args.warmup)
            t2 = timed(lambda: [m.stage2(x) for x in xs], args.steps, args.warmup)
            tt = timed(lambda: [m.predict(m.predict(x, 1) / 255.0, 2) for x in xs], args.steps, args.warmup)
            r1 = timed(lambda: [R.torch_imdn_rtc(sdt, "stage1.", x) for x in xs], args.steps, args.warmup)
            r2 = timed(lambda: [R.torch_imdn_rtc(sdt, "stage2.", x) for x in xs], args.steps, args.warmup)
        flop = 2.0 * px * (mac[1] + mac[2])
        res[name] = {"pixels": px, "ms_stage1": round(t1, 3), "ms_stage2": round(t2, 3), "ms_both": round(tt, 3),
                     "tflops": round(flop / (tt * 1e-3) / 1e12, 2), "frac_peak": round(flop / (tt * 1e-3) / PEAK_F32_MFMA, 4),
                     "torch_ms_stage1": round(r1, 3), "torch_ms_stage2": round(r2, 3), "torch_ms_both": round(r1 + r2, 3)}
    with torch.no_grad():
        diff = max(float((m.stage1(frame) - R.torch_imdn_rtc(sdt, "stage1.", frame)).abs().max()),
                   float((m.stage2(frame) - R.torch_imdn_rtc(sdt, "stage2.", frame)).abs().max()))
    res["max_abs_diff_vs_torch"] = diff
    print(json.dumps(res))


if __name__ == "__main__":
    main()
