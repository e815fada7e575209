#!/usr/bin/env python3
"""One hyper-network training iteration (train_model.py:416-442, --twoStage, model SRNetsSWF2) at the reference's defaults:
batch 16, 48x48 LR crops, x4, SteeringGaussianResize2dTorch S = 2, modes sct / sct, Adam -- on the HIP nets
(lerf_srnet_fwd_f32 / lerf_srnet_bwd_f32) and, for comparison, on a stock-torch float32 restatement of the same nets
(unfold + Linear layers, the same weights, the same glue and resize).  Prints one JSON line.

    python tools/bench_srnet_train.py [--steps K] [--warmup W] [--batch 16] [--crop 48] [--scale 4]

Net FLOPs per step = 2 x (multiply-adds of one forward) x 4 (forward, recompute, data gradient, weight gradient) over the
24 net passes (3 modes x 4 rotations x 2 stages); MFMA utilisation = those FLOPs / net time / 157.3 TFLOP/s (the
float32-input MFMA peak).  The stock-torch path does no recompute; it is charged the same FLOPs for comparability."""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import lerf_pytorch_amd  # noqa: E402,F401
from lerf_pytorch_amd.resample.model import SRNetsSWF2, lutft_step, mode_pad_dict, mulut_predict  # noqa: E402
from lerf_pytorch_amd.resize_right.resize_right2d_torch import SteeringGaussianResize2dTorch  # noqa: E402

PEAK_F32_MFMA = 157.3e12
PICK = {"s": [(0, 0), (0, 1), (1, 0), (1, 1)], "c": [(0, 0), (0, 1), (0, 2), (0, 3)], "t": [(0, 0), (1, 1), (2, 2), (3, 3)],
        "d": [(0, 0), (0, 2), (2, 0), (2, 2)], "y": [(0, 0), (1, 1), (1, 2), (2, 1)]}


class TorchNet(nn.Module):
    """one SRNet as stock torch: F.unfold over the K x K field, the mode's four pixels, Linear layers with concatenation"""

    def __init__(self, hip_net, mode):
        super().__init__()
        self.mode, self.K = mode, mode_pad_dict[mode] + 1
        ps = [p.detach().clone() for p in hip_net.parameters()]
        self.lin = nn.ModuleList()
        for i in range(0, 12, 2):
            w = ps[i].reshape(ps[i].shape[0], -1)
            lin = nn.Linear(w.shape[1], w.shape[0])
            lin.weight.data.copy_(w)
            lin.bias.data.copy_(ps[i + 1])
            self.lin.append(lin)
        self.sel = [dy * self.K + dx for dy, dx in PICK[mode]]

    def forward(self, x):
        B, C, H, W = x.shape
        h, w = H - self.K + 1, W - self.K + 1
        u = F.unfold(x, self.K)                                          # [B, C*K*K, h*w]
        u = u.view(B, C, self.K * self.K, h * w).permute(0, 1, 3, 2)[..., self.sel].reshape(-1, 4)
        a = torch.relu(self.lin[0](u))
        for lin in self.lin[1:5]:
            a = torch.cat([a, torch.relu(lin(a))], dim=1)
        y = torch.tanh(self.lin[5](a))                                   # [B*C*h*w, oC]
        return y.view(B, C, h * w, -1).permute(0, 1, 3, 2).reshape(B, -1, h, w)


class TorchSRNets(SRNetsSWF2):
    """SRNetsSWF2's glue (predict) over TorchNet nets"""

    def __init__(self, hip_model):
        nn.Module.__init__(self)
        self.modes, self.modes2, self.stages, self.norm, self.outC = (hip_model.modes, hip_model.modes2, hip_model.stages,
                                                                     hip_model.norm, hip_model.outC)
        self.nets = nn.ModuleDict({name: TorchNet(net, name[3]) for name, net in hip_model.named_children()})

    def forward(self, x, stage, mode, r):
        return self.nets["s{}_{}r{}".format(stage, mode, r)](x)


def net_flops(B, crop, modes, modes2, outC):
    px = B * crop * crop
    hidden = 4 * 64 + sum(k * 64 for k in (64, 128, 192, 256))
    macs = 4 * px * ((hidden + 320) * len(modes) + (hidden + 320 * outC) * len(modes2))     # 4 rotations per mode
    return 2 * macs * 4


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


def phases(m, r, im, lb, opt_G, steps, warmup):
    """ms of: the whole lutft_step; net forward; resize forward + loss; resize backward; net backward; optimiser"""
    def nets_fwd():
        feat = mulut_predict(m, im, 1)
        return feat, mulut_predict(m, feat / 255.0, 2)

    def head(feat, hyper):
        pred = r.resize(feat, hyper[:, :1], hyper[:, 1:2], hyper[:, 2:])
        return F.mse_loss(torch.clamp(pred, 0, 255) / 255.0, lb)

    feat0, hyper0 = [t.detach().requires_grad_() for t in nets_fwd()]

    def net_fwd_bwd():
        feat, hyper = nets_fwd()
        torch.autograd.backward([feat, hyper], [gf, gh])

    def resize_fwd_bwd():
        torch.autograd.grad(head(feat0, hyper0), [feat0, hyper0])

    with torch.no_grad():
        t_net_fwd = timed(nets_fwd, steps, warmup)
        t_resize_fwd = timed(lambda: head(feat0, hyper0), steps, warmup)
    gf, gh = torch.autograd.grad(head(feat0, hyper0), [feat0, hyper0])
    t_net_fb = timed(net_fwd_bwd, steps, warmup)
    t_resize_fb = timed(resize_fwd_bwd, steps, warmup)
    t_opt = timed(opt_G.step, steps, warmup)
    t_step = timed(lambda: lutft_step(m, r, im, lb, opt_G), steps, warmup)
    return {"step": t_step, "net_fwd": t_net_fwd, "net_bwd": t_net_fb - t_net_fwd, "net_fwd_bwd": t_net_fb,
            "resize_fwd": t_resize_fwd, "resize_bwd": t_resize_fb - t_resize_fwd, "opt": t_opt}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--crop", type=int, default=48)
    ap.add_argument("--scale", type=float, default=4.0)
    ap.add_argument("--hip-only", action="store_true", help="skip the stock-torch restatement (profiling runs)")
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_srnet_train measures on the GPU"
    torch.manual_seed(0)
    opt = types.SimpleNamespace(nf=64, modes="sct", modes2="sct", stages=2, norm=255)
    m = SRNetsSWF2(opt, inC=1, outC=3).cuda()
    rng = np.random.default_rng(0)
    S = int(round(a.crop * a.scale))
    im = torch.tensor(rng.random((a.batch, 1, a.crop, a.crop), dtype=np.float32), device="cuda")
    lb = torch.tensor(rng.random((a.batch, 1, S, S), dtype=np.float32), device="cuda")
    r = SteeringGaussianResize2dTorch(support_sz=2, device=torch.device("cuda"), max_sigma=10)
    r.set_shape([a.batch, 1, a.crop, a.crop], scale_factors=a.scale)
    flops = net_flops(a.batch, a.crop, opt.modes, opt.modes2, 3)
    res = {"tool": "bench_srnet_train", "batch": a.batch, "crop": a.crop, "scale": a.scale, "net_gflop_step": flops / 1e9}
    tm = TorchSRNets(m).cuda() if not a.hip_only else None
    hip = phases(m, r, im, lb, torch.optim.Adam(m.parameters(), lr=1e-4), a.steps, a.warmup)
    res.update({"hip_ms_" + k: round(v, 3) for k, v in hip.items()})
    res["hip_mfma_util"] = round(flops / (hip["net_fwd_bwd"] * 1e-3) / PEAK_F32_MFMA, 4)
    if tm is not None:
        tt = phases(tm, r, im, lb, torch.optim.Adam(tm.parameters(), lr=1e-4), a.steps, a.warmup)
        res.update({"torch_ms_" + k: round(v, 3) for k, v in tt.items()})
        res["torch_mfma_util"] = round(flops / (tt["net_fwd_bwd"] * 1e-3) / PEAK_F32_MFMA, 4)
        res["net_speedup_vs_torch"] = round(tt["net_fwd_bwd"] / hip["net_fwd_bwd"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
