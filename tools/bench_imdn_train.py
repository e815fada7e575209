#!/usr/bin/env python3
"""One LeRF-Net training iteration (train_model.py:416-441, --twoStage, model IMDN2 nf 64, inC 3, outC 3; forward + backward,
no optimiser) at the reference's shapes -- batch 16, 48x48 LR crops, x4, SteeringGaussianResize2dTorch S = 2 -- through
lutft_step's loss path: on the HIP nets (lerf_imdn_fwd_train_f32 / lerf_imdn_bwd_f32) and, as the baseline, on the same
network as stock float32 F.conv2d autograd (imdn_ref64.torch_imdn_rtc: MIOpen) with the same resampler, on seeded weights.
Prints one JSON line.

    python tools/bench_imdn_train.py [--steps K] [--warmup W] [--batch 16] [--crop 48] [--scale 4] [--no-profile]

Net FLOPs per iteration = 2 x the networks' multiply-adds per pixel x pixels x 3 (forward, data gradient, weight gradient);
frac_peak = those FLOPs / the iteration's time / 157.3 TFLOP/s (the float32-input MFMA peak; the iteration includes the
resampler, so the figure is a lower bound for the nets).  kernels: the per-kernel split (total ms over the profiled
iterations, calls) of one `rocprofv3 --kernel-trace --stats` run per path, each in a child process of its own."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import imdn_ref64 as R  # noqa: E402
from lerf_pytorch_amd.resample.model import IMDN2, lutft_step  # noqa: E402
from lerf_pytorch_amd.resize_right.resize_right2d_torch import SteeringGaussianResize2dTorch  # noqa: E402

PEAK_F32_MFMA = 157.3e12


class TorchIMDN2(torch.nn.Module):
    """IMDN2.predict over stock F.conv2d autograd, the same parameters"""

    def __init__(self, sd):
        super().__init__()
        self.names = list(sd)
        self.params = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(v.copy())) for v in sd.values()])

    def predict(self, x, stage=1):
        y = torch.clamp(R.torch_imdn_rtc(dict(zip(self.names, self.params)), "stage%d." % stage, x), -1, 1)
        return y / 2 + 0.5 if stage == 2 else y * 127 + 127


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


def setup(a, path):
    nf, inC, outC = a.nf, 3, 3
    sd = R.weight_rule(nf, inC, outC, 2701)
    if path == "hip":
        m = IMDN2(types.SimpleNamespace(nf=nf, norm=255), inC=inC, outC=outC)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        m.enable_backward()
    else:
        m = TorchIMDN2(sd)
    m.cuda()
    rng = np.random.default_rng(0)
    S = int(round(a.crop * a.scale))
    im = torch.tensor(rng.random((a.batch, 3, a.crop, a.crop), dtype=np.float32), device="cuda")
    lb = torch.tensor(rng.random((a.batch, 3, S, S), dtype=np.float32), device="cuda")
    r = SteeringGaussianResize2dTorch(support_sz=2, device=torch.device("cuda"), max_sigma=10)
    r.set_shape([a.batch, 1, a.crop, a.crop], scale_factors=a.scale)

    def step():
        m.zero_grad(set_to_none=True)
        return lutft_step(m, r, im, lb, None, featC=3, inC=3)
    return m, step


def kernel_split(a, path):
    """{kernel: [ms, calls]} of `steps` iterations of one path under rocprofv3 (a child process), largest first"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--output-format", "csv", "--", sys.executable,
               os.path.abspath(__file__), "--child", path, "--steps", str(a.steps), "--warmup", "1", "--batch", str(a.batch),
               "--crop", str(a.crop), "--scale", str(a.scale), "--nf", str(a.nf)]
        try:
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
        except (OSError, subprocess.SubprocessError) as e:
            return {"error": str(e)[:200]}
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"error": "no kernel_stats.csv"}
        rows = list(csv.DictReader(open(files[0])))
    out = {}
    for row in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:12]:
        out[row["Name"].split("(")[0][:60]] = [round(float(row["TotalDurationNs"]) / 1e6, 3), int(row["Calls"])]
    out["_total_ms"] = round(sum(float(r["TotalDurationNs"]) for r in rows) / 1e6, 3)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--crop", type=int, default=48)
    ap.add_argument("--scale", type=float, default=4.0)
    ap.add_argument("--nf", type=int, default=64)
    ap.add_argument("--no-profile", action="store_true", help="skip the two rocprofv3 runs")
    ap.add_argument("--child", choices=["hip", "torch"], help="(internal) run one path's iterations and exit")
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_imdn_train measures on the GPU"
    if a.child:
        _, step = setup(a, a.child)
        timed(step, a.steps, a.warmup)
        return
    res = {"tool": "bench_imdn_train", "nf": a.nf, "batch": a.batch, "crop": a.crop, "scale": a.scale, "steps": a.steps,
           "warmup": a.warmup}
    if not a.no_profile:                                  # each path in a child of its own, before this process's timing
        res["kernels"] = {p: kernel_split(a, p) for p in ("hip", "torch")}
    macs = sum(int(np.prod(s)) for k, s in R.imdn2_keys(a.nf, 3, 3) if k.endswith(".weight"))
    flops = 2.0 * macs * a.batch * a.crop * a.crop * 3
    res["net_gflop_iter"] = round(flops / 1e9, 2)
    losses = {}
    for p in ("hip", "torch"):
        _, step = setup(a, p)
        losses[p] = float(step().detach())
        ms = timed(step, a.steps, a.warmup)
        res[p + "_ms_iter"] = round(ms, 3)
        res[p + "_frac_peak"] = round(flops / (ms * 1e-3) / PEAK_F32_MFMA, 4)
    res["loss_hip"], res["loss_torch"] = losses["hip"], losses["torch"]
    res["speedup_vs_torch"] = round(res["torch_ms_iter"] / res["hip_ms_iter"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
