"""Training and LUT fine-tuning on the MI355X path: the counterpart of the reference's resample/train_model.py, with the
options of common/option.py's TrainOptions (same names, same defaults):

    python -m lerf_pytorch_amd.resample.train_model -e models/lerf-g/ --twoStage --outC 3                      # scripts.sh step 1
    python -m lerf_pytorch_amd.resample.transfer_to_lut -e models/lerf-g/ --outC 3                              # step 2
    python -m lerf_pytorch_amd.resample.train_model -e models/lerf-g/ --lutft --model SWF2LUT --twoStage --outC 3 --batchSize 256   # step 3

The batch comes from data.Provider (one HIP launch over the device-resident DIV2K pool), the iteration is
model.lutft_step (HIP forward and backward of SWF2LUT / SRNetsSWF2 / IMDN2 and of the resampler), Adam and the cosine
LambdaLR are the reference's (:360-369), the log line is its `Iter / Sample / GPixel / dT / rT`, validation is
eval_model.Eltr on the live model.

Every --saveStep iterations `Checkpoint_{i:06d}.pth` holds the model's state dict, the optimiser's, the iteration and the
provider's generator state, and the network models also write the export file transfer_to_lut / eval_model read
(srnets_weights.npz / imdn2_weights.npz).  `--startIter N` restores all four and positions the schedule at N, so a resumed
run continues the run it came from; the reference restores the weights only and restarts its schedule.  `save_code` (a copy
of every .py under the experiment) and --load_from_opt_file are not mirrored.
"""
from __future__ import annotations

import argparse
import copy
import logging
import math
import os
import time

import numpy as np
import torch
import torch.optim as optim

from ..resize_right.resize_right2d_torch import AmplifiedLinearResize2dTorch, SteeringGaussianResize2dTorch
from . import eval_model
from . import model as M
from .data import Provider

MODELS = ("SRNetsSWF2", "SWF2LUT", "IMDN2")


def build_parser():
    """common/option.py:13-41 (BaseOptions) and :180-204 (TrainOptions)"""
    ap = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--name", type=str, default="lerf")
    ap.add_argument("--model", type=str, default="SRNetsSWF2")
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
    ap.add_argument("--batchSize", type=int, default=16)
    ap.add_argument("--cropSize", type=int, default=48)
    ap.add_argument("--cropSizeLR", type=int, default=48)
    ap.add_argument("--trainDir", type=str, default="./data/DIV2K")
    ap.add_argument("--valDir", type=str, default="./data/rrBenchmark")
    ap.add_argument("--valWDir", type=str, default="./data/WarpBenchmark")
    ap.add_argument("--lutft", action="store_true", default=False)
    ap.add_argument("--startIter", type=int, default=0)
    ap.add_argument("--totalIter", type=int, default=50000)
    ap.add_argument("--displayStep", type=int, default=100)
    ap.add_argument("--valStep", type=int, default=2000)
    ap.add_argument("--saveStep", type=int, default=2000)
    ap.add_argument("--lr0", type=float, default=1e-3)
    ap.add_argument("--lr1", type=float, default=1e-4)
    ap.add_argument("--weightDecay", type=float, default=0)
    ap.add_argument("--gpuNum", "-g", type=int, default=1)
    ap.add_argument("--workerNum", "-n", type=int, default=8)
    return ap


def options_text(ap, opt):
    """option.py:63-83: one line per option, the default noted where it was changed"""
    lines = []
    for k, v in sorted(vars(opt).items()):
        default = ap.get_default(k)
        comment = "\t[default: %s]" % str(default) if v != default else ""
        lines.append("{:>25}: {:<30}{}".format(str(k), str(v), comment))
    return "\n".join(lines)


def parse(argv=None, make_dirs=True):
    """option.py:121-176 for TrainOptions: --scale to int or float, the experiment / val / lutft directories, opt.txt, the
    --debug overrides.  `make_dirs=False` only parses (no directory is made, nothing is written)."""
    ap = build_parser()
    opt = ap.parse_args(argv)
    opt.isTrain = True
    opt.scale = float(opt.scale) if "." in opt.scale else int(opt.scale)
    if opt.load_from_opt_file:
        raise NotImplementedError("--load_from_opt_file is not mirrored: repeat the options on the command line")
    if make_dirs:
        if opt.expDir == "":
            opt.modelDir = os.path.join(opt.modelRoot, opt.name)
            os.makedirs(opt.modelDir, exist_ok=True)
            count = 1
            while os.path.isdir(os.path.join(opt.modelDir, "expr_{}".format(count))):
                count += 1
            opt.expDir = os.path.join(opt.modelDir, "expr_{}".format(count))
            os.mkdir(opt.expDir)
        else:
            os.makedirs(opt.expDir, exist_ok=True)
            opt.name = opt.expDir.split("/")[-1] + "-" + opt.model
        opt.modelPath = os.path.join(opt.expDir, "Model.pth")
        opt.valoutDir = os.path.join(opt.expDir, "lutft" if opt.lutft else "val")
        os.makedirs(opt.valoutDir, exist_ok=True)
        with open(os.path.join(opt.valoutDir, "opt.txt"), "wt") as f:
            f.write(options_text(ap, opt) + "\n")
    if opt.debug:
        opt.displayStep = 10
        opt.saveStep = 100
        opt.valStep = 50
        opt.totalIter = 200
        opt.batchSize = 4
        opt.nf = 16
    opt._parser = ap
    return opt


def lr_lambda(opt):
    """train_model.py:363-368: cosine from 1 to 0.2 (lr1 < 0), or from 1 to lr1 / lr0, over totalIter"""
    if opt.lr1 < 0:
        lr_a, lr_b = 0.8, 0.2
    else:
        lr_b = opt.lr1 / opt.lr0
        lr_a = 1 - lr_b
    return lambda x: (((1 + math.cos(x * math.pi / opt.totalIter)) / 2) ** 1.0) * lr_a + lr_b


def _logger(name, path):
    """common/utils.py:8-28 logger_info, with the handlers of an earlier run in this process dropped"""
    log = logging.getLogger(name)
    for h in list(log.handlers):
        log.removeHandler(h)
        h.close()
    fmt = logging.Formatter("%(asctime)s.%(msecs)03d : %(message)s", datefmt="%y-%m-%d %H:%M:%S")
    log.setLevel(logging.INFO)
    log.propagate = False
    for h in (logging.FileHandler(path, mode="a"), logging.StreamHandler()):
        h.setFormatter(fmt)
        log.addHandler(h)
    return log


def _summary_writer(log_dir):
    try:
        from torch.utils.tensorboard import SummaryWriter
    except ImportError:
        return None
    return SummaryWriter(log_dir=log_dir)


def build_model(opt):
    if opt.model not in MODELS:
        raise ValueError("--model must be one of {}".format(", ".join(MODELS)))
    model_G = getattr(M, opt.model)(opt, inC=opt.inC, outC=opt.outC).cuda()
    if opt.model == "IMDN2":
        model_G.enable_backward()
    return model_G


def save_checkpoint(model_G, opt_G, train_iter, opt, i, logger):
    torch.save({"model": model_G.state_dict(), "optimizer": opt_G.state_dict(), "iteration": i,
                "provider": train_iter.state_dict()}, os.path.join(opt.expDir, "Checkpoint_{:06d}.pth".format(i)))
    if opt.model == "SRNetsSWF2":
        M.export_srnets(model_G, opt.expDir)
    elif opt.model == "IMDN2":
        M.export_imdn2(model_G, opt.expDir)
    logger.info("Checkpoint saved {}".format(str(i)))


def load_checkpoint(model_G, opt_G, scheduler, train_iter, opt):
    """--startIter N: weights, optimiser state, provider generators, and the schedule at N"""
    path = os.path.join(opt.expDir, "Checkpoint_{:06d}.pth".format(opt.startIter))
    ck = torch.load(path, map_location="cpu", weights_only=True)
    if int(ck["iteration"]) != opt.startIter:
        raise ValueError("{} holds iteration {}".format(path, ck["iteration"]))
    model_G.load_state_dict(ck["model"], strict=True)
    opt_G.load_state_dict(ck["optimizer"])
    train_iter.load_state_dict(ck["provider"])
    scheduler.last_epoch = opt.startIter                      # N scheduler steps have been taken
    scheduler._step_count = opt.startIter + 1
    for group, base, lf in zip(opt_G.param_groups, scheduler.base_lrs, scheduler.lr_lambdas):
        group["lr"] = base * lf(opt.startIter)
    scheduler._last_lr = [g["lr"] for g in opt_G.param_groups]
    return path


def validate(model_G, opt, i, logger, writer):
    """train_model.py:68-314 valid_steps_warp + valid_steps: the warp table over valWDir, the SR table over valDir"""
    model_G.eval()
    for kind, root in (("warp", opt.valWDir), ("sr", opt.valDir)):
        if not os.path.isdir(os.path.join(root, "Set5", "HR")):
            logger.info("validation ({}) skipped: {} holds no Set5/HR".format(kind, root))
            continue
        vopt = copy.copy(opt)
        vopt.testDir, vopt.resultRoot = root, opt.valoutDir
        etr = eval_model.Eltr(vopt, model_G)
        lines = eval_model.warp_table(etr) if kind == "warp" else eval_model.sr_table(etr)
        logger.info("Iter {:06d}".format(i).ljust(15, " ") + lines[0][15:])
        for line in lines[1:]:
            logger.info(line)
            if writer is not None:
                cells = line.split("\t")
                for head, cell in zip(lines[0].split("\t")[1:], cells[1:]):
                    if head and cell:
                        writer.add_scalar("{}_{}/{}".format("mPSNR" if kind == "warp" else "PSNR", head.strip(), cells[0].strip()),
                                          float(cell.split("/")[0]), i)
    model_G.train()


def main(argv=None, on_step=None):
    """Run the training the options describe.  `on_step(i, lr, loss)`, if given, is called at the end of every iteration with
    the learning rate its optimiser step used; returning False ends the run after that iteration.  Returns a namespace of the live objects (opt, model_G, opt_G, scheduler,
    train_iter)."""
    opt = parse(argv, make_dirs=False)
    if opt.gpuNum > 1:
        raise NotImplementedError("--gpuNum > 1 (nn.DataParallel) is not mirrored: run one process per GPU and pass "
                                  "dist.allreduce_grads as lutft_step's reduce_grads")
    if opt.scale < 1:
        raise NotImplementedError("scale < 1 (LR decoded on the fly, data.py:82-83, 114) is not implemented")
    opt = parse(argv)
    ap = opt._parser
    del opt._parser

    logger_name = "lutft" if opt.lutft else "train"
    writer = None if opt.lutft else _summary_writer(opt.expDir)
    logger = _logger(logger_name, os.path.join(opt.expDir, logger_name + ".log"))
    logger.info("----------------- Options ---------------\n" + options_text(ap, opt) + "\n----------------- End -------------------")

    model_G = build_model(opt)
    if opt.linear:
        train_resizer = AmplifiedLinearResize2dTorch(support_sz=opt.suppSize, device=torch.device("cuda"))
    else:
        train_resizer = SteeringGaussianResize2dTorch(support_sz=opt.suppSize, device=torch.device("cuda"), max_sigma=opt.maxSigma)
    train_resizer.set_shape([opt.batchSize, 1, opt.cropSize, opt.cropSize], scale_factors=opt.scale)

    params_G = list(filter(lambda p: p.requires_grad, model_G.parameters()))
    opt_G = optim.Adam(params_G, lr=opt.lr0, betas=(0.9, 0.999), eps=1e-8, weight_decay=opt.weightDecay, amsgrad=False)
    scheduler = optim.lr_scheduler.LambdaLR(opt_G, lr_lambda=lr_lambda(opt))

    train_iter = Provider(opt.batchSize, opt.workerNum, opt.scale, opt.trainDir, opt.cropSize, opt.nsigma, inC=opt.inC)
    train_iter.data.upload()
    if opt.startIter > 0:
        logger.info("load Checkpoint from: " + load_checkpoint(model_G, opt_G, scheduler, train_iter, opt))

    l_accum = 0.
    dT = 0.
    rT = 0.
    accum_samples = 0
    for i in range(opt.startIter + 1, opt.totalIter + 1):
        model_G.train()

        st = time.time()
        im, lb = train_iter.next()
        dT += time.time() - st

        st = time.time()
        lr = opt_G.param_groups[0]["lr"]
        loss_G = M.lutft_step(model_G, train_resizer, im, lb, opt_G, linear=opt.linear, norm=opt.norm, featC=opt.featC,
                              inC=opt.inC, two_stage=opt.twoStage)
        scheduler.step()
        rT += time.time() - st

        accum_samples += opt.batchSize
        loss = loss_G.item()
        l_accum += loss

        if i % opt.displayStep == 0:
            if writer is not None:
                writer.add_scalar("loss_Pixel", l_accum / opt.displayStep, i)
            logger.info("{} | Iter:{:6d}, Sample:{:6d}, GPixel:{:.2e}, dT:{:.4f}, rT:{:.4f}".format(
                opt.expDir, i, accum_samples, l_accum / opt.displayStep, dT / opt.displayStep, rT / opt.displayStep))
            l_accum = 0.
            dT = 0.
            rT = 0.

        if i % opt.saveStep == 0:
            save_checkpoint(model_G, opt_G, train_iter, opt, i, logger)

        if (i % opt.valStep == 0) or (opt.debug and i == 1):
            validate(model_G, opt, i, logger, writer)

        if on_step is not None and on_step(i, lr, loss) is False:
            break

    if opt.lutft:
        M.export_luts(model_G, opt.expDir)
        logger.info("Finetuned LUT saved to {}".format(opt.expDir))
    logger.info("Complete")
    if writer is not None:
        writer.close()
    for h in list(logger.handlers):
        logger.removeHandler(h)
        h.close()
    return argparse.Namespace(opt=opt, model_G=model_G, opt_G=opt_G, scheduler=scheduler, train_iter=train_iter)


if __name__ == "__main__":
    main()
