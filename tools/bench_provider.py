#!/usr/bin/env python3
"""One training batch of the DIV2K provider, two ways, on the same synthetic pool (DIV2K-sized random images, B 16, crop 48,
x4, inC 1 and 3):

  numpy : the reference's host path restated (resample/data.py:107-165 per sample, in this process, no worker processes),
          the default collate (stack), then .cuda() of both tensors
  hip   : data.Provider.next() -- descriptors drawn on the host, one small upload, one launch of lerf_patch_batch_u8

Per path: the median over --iters batches of the wall clock (synchronised at the end of the batch) and of the hipEvent
time on the stream.  Then the `dT` share of one train_model iteration (SWF2LUT lerf-g through lutft_step) with either
path feeding it, timed the way train_model's log line does, with a synchronise closing each part.

    python tools/bench_provider.py [--iters 200] [--images 16]
"""
import argparse
import os
import random
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import lerf_pytorch_amd  # noqa: F401,E402
from lerf_pytorch_amd.resample.data import DIV2K, Provider  # noqa: E402
from lerf_pytorch_amd.resample.model import SWF2LUT, lutft_step  # noqa: E402
from lerf_pytorch_amd.resize_right.resize_right2d_torch import SteeringGaussianResize2dTorch  # noqa: E402

B, SZ, SCALE = 16, 48, 4


class NumpyProvider:
    """data.py:107-165 and :33-42, statement for statement"""

    def __init__(self, lr_ims, hr_ims, inC):
        self.lr_ims, self.hr_ims, self.inC = lr_ims, hr_ims, inC
        self.file_list = sorted(hr_ims)
        self.scale, self.sz = SCALE, SZ

    def item(self):
        key = random.choice(self.file_list)
        lb = self.hr_ims[key]
        im = self.lr_ims[key]
        shape = im.shape
        i = random.randint(0, shape[0] - self.sz)
        j = random.randint(0, shape[1] - self.sz)
        lb = lb[int(i * self.scale):int(i * self.scale) + int(self.sz * self.scale),
                int(j * self.scale):int(j * self.scale) + int(self.sz * self.scale), :]
        im = im[i:i + self.sz, j:j + self.sz, :]
        if self.inC == 1:
            c = random.choice([0, 1, 2])
            im = im[:, :, c]
            lb = lb[:, :, c]
        if random.uniform(0, 1) < 0.5:
            lb = np.fliplr(lb)
            im = np.fliplr(im)
        if random.uniform(0, 1) < 0.5:
            lb = np.flipud(lb)
            im = np.flipud(im)
        k = random.choice([0, 1, 2, 3])
        lb = np.rot90(lb, k)
        im = np.rot90(im, k)
        lb = lb.astype(np.float32) / 255.0
        im = im.astype(np.float32) / 255.0
        if self.inC == 1:
            lb = np.expand_dims(lb, axis=0)
            im = np.expand_dims(im, axis=0)
        else:
            lb = np.transpose(lb, [2, 0, 1])
            im = np.transpose(im, [2, 0, 1])
        im = im + 0
        return im, lb

    def next(self):
        items = [self.item() for _ in range(B)]
        im = torch.stack([torch.as_tensor(np.ascontiguousarray(a)) for a, _ in items])      # default_collate
        lb = torch.stack([torch.as_tensor(np.ascontiguousarray(b)) for _, b in items])
        return im.cuda(), lb.cuda()


def median_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    wall, dev = [], []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t) * 1e3)
        dev.append(e0.elapsed_time(e1))
    return float(np.median(wall)), float(np.median(dev))


def iteration_split(provider, inC, iters, warmup):
    """(dT, rT) ms per iteration of provider.next() + lutft_step, each part closed by a synchronise"""
    opt = types.SimpleNamespace(modes="sct", modes2="sct", stages=2, norm=255, interval=4, lutName="LUTft",
                                expDir=os.path.join(ROOT, "lerf-pytorch_amd", "assets", "models", "lerf-g"))
    m = SWF2LUT(opt, inC=1, outC=3).cuda()
    r = SteeringGaussianResize2dTorch(support_sz=2, device=torch.device("cuda"), max_sigma=10)
    r.set_shape([B, 1, SZ, SZ], scale_factors=SCALE)
    opt_G = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    dT, rT = [], []
    for n in range(warmup + iters):
        t = time.perf_counter()
        im, lb = provider.next()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        lutft_step(m, r, im, lb, opt_G, featC=1, inC=1)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if n >= warmup:
            dT.append((t1 - t) * 1e3)
            rT.append((t2 - t1) * 1e3)
    return float(np.median(dT)), float(np.median(rT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--train-iters", type=int, default=30)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    files = ["%04d" % (n + 1) for n in range(a.images)]
    hr = {f: rng.integers(0, 256, (1400 - 4 * (n % 5), 2040, 3), dtype=np.uint8) for n, f in enumerate(files)}
    lr = {f: rng.integers(0, 256, (hr[f].shape[0] // SCALE, 2040 // SCALE, 3), dtype=np.uint8) for f in files}
    print("pool: %d images of about 1400x2040 (HR) and 350x510 (LR), B %d, crop %d, x%d; medians of %d batches" % (a.images, B, SZ, SCALE, a.iters))
    print("%-6s %-6s %12s %12s" % ("inC", "path", "wall ms", "hipEvent ms"))
    for inC in (1, 3):
        random.seed(1)
        host = NumpyProvider(lr, hr, inC)
        dev = Provider.__new__(Provider)
        dev.data = DIV2K.from_arrays(SCALE, lr, hr, SZ, inC=inC, file_list=files, seed=1).upload()
        dev.batch_size, dev.num_workers, dev.iteration, dev.epoch = B, 0, 0, 1
        wn, dn = median_ms(host.next, a.iters, a.warmup)
        wh, dh = median_ms(dev.next, a.iters, a.warmup)
        print("%-6d %-6s %12.3f %12.3f" % (inC, "numpy", wn, dn))
        print("%-6d %-6s %12.3f %12.3f" % (inC, "hip", wh, dh))
        print("%-6d %-6s %12.2f %12.2f" % (inC, "ratio", wn / wh, dn / dh))
        if inC == 1:
            keep = (host, dev)
    print("one train_model iteration (SWF2LUT lerf-g, lutft_step, inC 1), medians of %d:" % a.train_iters)
    for name, p in zip(("numpy", "hip"), keep):
        dT, rT = iteration_split(p, 1, a.train_iters, 5)
        print("%-6s dT %8.3f ms  rT %8.3f ms  dT share %5.1f %%" % (name, dT, rT, 100 * dT / (dT + rT)))


if __name__ == "__main__":
    main()
