"""Network evaluation on the MI355X path: the counterpart of the reference's resample/eval_model.py, which scores a
*network* (LeRF-Net `IMDN2`, or the hyper-networks `SRNetsSWF2` before their transfer to LUTs) instead of LUTs.  Same
options, directory layout, result files and printed tables:

    python -m lerf_pytorch_amd.resample.eval_model --model SRNetsSWF2 -e models/lerf-g --twoStage --testDir data/rrBenchmark
    python -m lerf_pytorch_amd.resample.eval_model --model IMDN2 -e models/lerf-net --inC 3 --featC 3 --twoStage \
        --testDir data/WarpBenchmark --resultRoot results/warp

Weights under -e: `imdn2_weights.npz` / `srnets_weights.npz` (model.export_imdn2 / export_srnets) if present, else
`Model_{loadIter:06d}.pth` holding a plain state dict.  "warp" in --resultRoot selects the warp table (Set5, isc / osc),
otherwise the SR table (Set5 at x2, x3, x4).  The nets (lerf_imdn_fwd_f32 / lerf_srnet_fwd_f32), the resampling twins and
the metrics run on the GPU; PNG decoding and encoding stay on the host.
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from .. import metrics
from ..resize_right.resize_right2d_torch import (AmplifiedLinearResize2dTorch, AmplifiedLinearWarp2dTorch, NearestWarp2dTorch,
                                                  SteeringGaussianResize2dTorch, SteeringGaussianWarp2dTorch)
from . import model as M
from .eval_harness import _load_matrix, _load_rgb

PRE_UPSAMPLE = [[0.5, 0, -0.25], [0, 0.5, -0.25], [0, 0, 1]]
WEIGHT_FILES = {"IMDN2": "imdn2_weights.npz", "SRNetsSWF2": "srnets_weights.npz"}


def mulut_predict(model_G, x, stage, opt):
    """eval_model.py:23-32: one channel at a time when inC == 1"""
    with torch.no_grad():
        if opt.inC == 1:
            return torch.cat([model_G.predict(x[:, i:i + 1], stage=stage) for i in range(x.shape[1])], dim=1)
        return model_G.predict(x, stage=stage)


def split_hyper(pred_hyper, opt):
    """the three hyper-parameter maps: interleaved ([0::3], [1::3], [2::3]) for inC 1, blocks of featC for inC 3; the one
    amplitude map of the linear resampling function (train_model.py:116-118)"""
    if getattr(opt, "linear", False):
        return (pred_hyper,)
    if opt.inC == 1:
        return pred_hyper[:, 0::3], pred_hyper[:, 1::3], pred_hyper[:, 2::3]
    f = opt.featC
    return pred_hyper[:, :f], pred_hyper[:, f:2 * f], pred_hyper[:, 2 * f:]


class Eltr:
    """eltr of eval_model.py:35-300 with the per-image work on the GPU"""

    def __init__(self, opt, model_G):
        self.opt = opt
        self.model_G = model_G
        self.norm = 255
        if getattr(opt, "linear", False):
            self.resizer = AmplifiedLinearResize2dTorch(support_sz=opt.suppSize)
            self.warper = AmplifiedLinearWarp2dTorch(support_sz=opt.suppSize)
        else:
            self.resizer = SteeringGaussianResize2dTorch(support_sz=opt.suppSize, max_sigma=opt.maxSigma)
            self.warper = SteeringGaussianWarp2dTorch(support_sz=opt.suppSize, max_sigma=opt.maxSigma)
        self.nn_warper = NearestWarp2dTorch()

    def _files(self, dataset):
        folder = os.path.join(self.opt.testDir, dataset, "HR")
        return sorted(f for f in os.listdir(folder) if "png" in f)

    def _stages(self, img_lr):
        opt = self.opt
        if opt.twoStage:
            feat_im = mulut_predict(self.model_G, img_lr, 1, opt)
            hyper_in = feat_im / float(opt.norm)
        else:
            feat_im = torch.round(img_lr * opt.norm)
            hyper_in = img_lr
        return feat_im, mulut_predict(self.model_G, hyper_in, 2, opt)

    @staticmethod
    def _dev(a):
        return (torch.from_numpy(a.astype(np.float32))[None].permute(0, 3, 1, 2) / 255.0).contiguous().cuda()

    def sr_image(self, lr, scale_h, scale_w):
        """uint8 [H', W', 3] output of eval_model.py:_worker for one uint8 LR image"""
        img_lr = self._dev(lr)
        feat_im, pred_hyper = self._stages(img_lr)
        post = 2 if "PreUpsample" in self.opt.testDir else 1
        ish, isw = scale_h / post, scale_w / post
        if ish == 1 and isw == 1:                                   # the scale-1 skip
            pred = torch.round(img_lr * self.opt.norm)
        else:
            self.resizer.set_shape(list(img_lr.shape), [ish, isw])
            pred = self.resizer.resize(feat_im, *split_hyper(pred_hyper, self.opt))
        pred = pred[0].permute(1, 2, 0)
        return torch.clamp(torch.round(pred), 0, self.norm).to(torch.uint8).contiguous()

    def run(self, dataset, scale_h, scale_w):
        """[[psnr, ssim], ...] per image"""
        from PIL import Image
        rdir = None
        if self.opt.resultRoot:
            rdir = os.path.join(self.opt.resultRoot, os.path.basename(os.path.normpath(self.opt.expDir)),
                                "X{:.2f}_{:.2f}".format(scale_h, scale_w), dataset)
            os.makedirs(rdir, exist_ok=True)
        res = []
        for f in self._files(dataset):
            lr = _load_rgb(os.path.join(self.opt.testDir, dataset, "LR_bicubic/rrLR_X{:.2f}_{:.2f}".format(scale_h, scale_w), f))
            gt = _load_rgb(os.path.join(self.opt.testDir, dataset, "HR", f))
            out = self.sr_image(lr, scale_h, scale_w)
            if rdir:
                Image.fromarray(out.cpu().numpy()).save(os.path.join(rdir, "{}.png".format(f[:-4])))
            shave = max(int(scale_h), int(scale_w))
            res.append([metrics.psnr_y(gt, out, shave), metrics.ssim_y(gt, out)])
        return res

    def warp_image(self, lr, matrix, gt_hw):
        """(uint8 [1, 3, H', W'] output, bool mask) of eval_model.py:_worker_warp for one uint8 LR image"""
        img_lr = self._dev(lr)
        m = torch.as_tensor(np.asarray(matrix, np.float64)).cuda()
        if "PreUpsample" in self.opt.testDir:
            m = torch.matmul(m, torch.tensor(PRE_UPSAMPLE, dtype=torch.float64, device=m.device))
        feat_im, pred_hyper = self._stages(img_lr)
        out_shape = [1, 3, int(gt_hw[0]), int(gt_hw[1])]
        white = torch.zeros_like(img_lr)                            # the mask: a border-4 white image, nearest-warped
        border = 4
        h, w = white.shape[-2:]
        white[:, :, border:h - border, border:w - border] = 255
        self.nn_warper.set_shape(list(img_lr.shape), m, out_shape)
        mask = self.nn_warper.warp(white).bool()
        self.warper.set_shape(list(img_lr.shape), m, out_shape)
        pred = self.warper.warp(feat_im, *split_hyper(pred_hyper, self.opt))
        pred = torch.nan_to_num(pred, nan=0.0, posinf=float("inf"), neginf=float("-inf"))
        pred = torch.round(pred.clip(0, 255)).to(torch.uint8)
        return pred, mask

    def run_warp(self, scale, dataset):
        """[[mpsnr, 0], ...] per image"""
        from PIL import Image
        rdir = None
        if self.opt.resultRoot:
            rdir = os.path.join(self.opt.resultRoot, dataset, "warp_{}".format(scale))
            os.makedirs(rdir, exist_ok=True)
        res = []
        for f in self._files(dataset):
            lr = _load_rgb(os.path.join(self.opt.testDir, dataset, scale, f))
            gt = _load_rgb(os.path.join(self.opt.testDir, dataset, "HR", f))
            matrix = _load_matrix(os.path.join(self.opt.testDir, dataset, scale, f[:-4]))
            pred, mask = self.warp_image(lr, matrix, gt.shape[:2])
            lb = torch.from_numpy(gt).permute(2, 0, 1)[None].contiguous().cuda()
            res.append([metrics.mpsnr(pred, lb, mask), 0])
            if rdir:
                Image.fromarray(pred[0].permute(1, 2, 0).cpu().numpy()).save(os.path.join(rdir, "{}.png".format(f[:-4])))
        return res


def sr_table(etr, datasets=("Set5",), scales=((2, 2), (3, 3), (4, 4))):
    lines = ["\t".join(["Scale".ljust(15, " ")] + ["{:.1f}x{:.1f}\t".format(a, b) for a, b in scales])]
    for ds in datasets:
        row = [ds.ljust(15, " ")]
        for a, b in scales:
            r = np.asarray(etr.run(ds, a, b))
            row.append("{:.2f}/{:.4f}".format(np.mean(r[:, 0]), np.mean(r[:, 1])))
        lines.append("\t".join(row))
    return lines


def warp_table(etr, datasets=("Set5",), scales=("isc", "osc")):
    lines = ["\t".join(["Scale".ljust(15, " ")] + ["{}\t".format(s) for s in scales])]
    for ds in datasets:
        row = [ds.ljust(15, " ")]
        for s in scales:
            r = np.asarray(etr.run_warp(s, ds))
            row.append("{:.2f}".format(np.mean(r[:, 0])))
        lines.append("\t".join(row))
    return lines


def parse(argv=None):
    """common/option.py's BaseOptions + TestOptions (the options eval_model.py reads, with their defaults); the training
    and bookkeeping options are accepted and ignored"""
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--name", type=str, default="lerf")
    ap.add_argument("--model", type=str, default="SRNetsSWF2", choices=["IMDN2", "SRNetsSWF2"])
    ap.add_argument("--scale", "-r", type=str, default="4")
    ap.add_argument("--nsigma", type=int, default=-1)
    ap.add_argument("--nf", type=int, default=64)
    ap.add_argument("--modes", type=str, default="sct")
    ap.add_argument("--modes2", type=str, default="sct")
    ap.add_argument("--interval", type=int, default=4)
    ap.add_argument("--norm", type=int, default=255)
    ap.add_argument("--suppSize", type=int, default=2)
    ap.add_argument("--inC", type=int, default=1)
    ap.add_argument("--outC", type=int, default=3)
    ap.add_argument("--featC", type=int, default=1)
    ap.add_argument("--maxSigma", type=int, default=10)
    ap.add_argument("--stages", type=int, default=2)
    ap.add_argument("--twoStage", action="store_true", default=False)
    ap.add_argument("--linear", action="store_true", default=False)
    ap.add_argument("--modelRoot", type=str, default="./models")
    ap.add_argument("--expDir", "-e", type=str, default="")
    ap.add_argument("--load_from_opt_file", action="store_true", default=False)
    ap.add_argument("--debug", default=False, action="store_true")
    ap.add_argument("--testDir", type=str, default="./data/rrBenchmark")
    ap.add_argument("--resultRoot", type=str, default="./results")
    ap.add_argument("--loadIter", type=int, default=50000)
    ap.add_argument("--lutName", type=str, default="LUTft")
    return ap.parse_args(argv)


def weights_path(opt):
    p = os.path.join(opt.expDir, WEIGHT_FILES[opt.model])
    return p if os.path.exists(p) else os.path.join(opt.expDir, "Model_{:06d}.pth".format(opt.loadIter))


def load_model(opt):
    model_G = getattr(M, opt.model)(opt, inC=opt.inC, outC=opt.outC)
    model_G.load_state_dict(M.load_state(weights_path(opt)), strict=True)
    return model_G.cuda().eval()


def main(argv=None):
    opt = parse(argv)
    etr = Eltr(opt, load_model(opt))
    for line in (warp_table(etr) if "warp" in opt.resultRoot else sr_table(etr)):
        print(line)


if __name__ == "__main__":
    main()
