"""The reference's training data, resample/data.py, with the batch made on the GPU.

`DIV2K` decodes the train split once (same `cache_hr.npy` / `cache_lr_x{scale}.npy` files as the reference, so a reference
cache is reused as is), uploads every image into ONE packed uint8 device pool, and from then on a sample is a descriptor:
`draw()` makes the reference's random draws in the reference's order (:108-140) on the host, and `lerf_patch_batch_u8`
(csrc/lerf_patch.hip) cuts, flips, rotates and converts the whole batch in one launch.  There are no worker processes, no
pinned staging and no per-sample host arithmetic; `Provider.next()` returns `(im, lb)` on the device.

`MultiSRBenchmark` and `SRBenchmarkW` are the reference's validation dict loaders (:171-283), on the host.

Differences from the reference, all refusals: `nsigma == 0` (its blind-noise branch reads `self.max_nsigma`, which nothing
sets) and `scale <= 1` (LR decoded on the fly) raise; a crop whose HR window leaves the HR image -- possible only when the LR
image is larger than HR / scale -- raises instead of returning a label smaller than the patch, which the reference's
DataLoader could not collate either.
"""
from __future__ import annotations

import collections
import os
import random
import sys

import numpy as np

from .. import _lib, ops
from .eval_harness import _load_matrix, _load_rgb

Draw = collections.namedtuple("Draw", "file li lj hi hj chan fliplr flipud k")


def _decode(path):
    from PIL import Image
    return np.array(Image.open(path))


class DIV2K(object):
    """data.py:54-168.  `file_list`: the image stems (default 0001..0800); `device`: where the pool lives (default: the
    current GPU); `seed`: None draws from the global `random` module like the reference, an int from a private
    random.Random(seed) -- the same sequence as random.seed(seed) there."""

    def __init__(self, scale, path, patch_size, nsigma=-1, inC=1, rigid_aug=True, *, file_list=None, device=None, seed=None):
        self._configure(scale, path, patch_size, nsigma, inC, rigid_aug, file_list, device, seed)
        self.hr_cache = os.path.join(path, "cache_hr.npy")
        if not os.path.exists(self.hr_cache):
            self.cache_hr()
            print("HR image cache to:", self.hr_cache)
        hr_ims = np.load(self.hr_cache, allow_pickle=True).item()
        print("HR image cache from:", self.hr_cache)
        self.lr_cache = os.path.join(path, "cache_lr_x{}.npy".format(self.scale))
        if not os.path.exists(self.lr_cache):
            self.cache_lr()
            print("LR image cache to:", self.lr_cache)
        lr_ims = np.load(self.lr_cache, allow_pickle=True).item()
        print("LR image cache from:", self.lr_cache)
        self._adopt(lr_ims, hr_ims)

    @classmethod
    def from_arrays(cls, scale, lr_ims, hr_ims, patch_size, nsigma=-1, inC=1, rigid_aug=True, *, file_list=None, device=None,
                    seed=None):
        """A dataset over decoded images already in memory ({stem: uint8 HWC array} each): no disk, no cache files"""
        self = cls.__new__(cls)
        self._configure(scale, None, patch_size, nsigma, inC, rigid_aug, sorted(hr_ims) if file_list is None else file_list,
                        device, seed)
        self._adopt(lr_ims, hr_ims)
        return self

    def _configure(self, scale, path, patch_size, nsigma, inC, rigid_aug, file_list, device, seed):
        if scale <= 1:
            raise NotImplementedError("scale <= 1 (LR decoded on the fly, data.py:82-83, 114) is not implemented")
        if nsigma == 0:
            raise ValueError("nsigma == 0 selects the reference's blind-noise branch, which reads self.max_nsigma that "
                             "nothing sets (data.py:154-157); give nsigma > 0, or < 0 for no noise")
        if inC not in (1, 3):
            raise ValueError("inC must be 1 or 3")
        self.scale = scale
        self.sz = patch_size
        self.hsz = int(patch_size * scale)
        self.rigid_aug = rigid_aug
        self.path = path
        self.inC = inC
        self.nsigma = nsigma
        self.file_list = [str(i).zfill(4) for i in range(1, 801)] if file_list is None else list(file_list)
        self.rng = random if seed is None else random.Random(seed)
        self.device = device
        self.pool = None

    def _adopt(self, lr_ims, hr_ims):
        """lay the images out in the pool: [file][lr, hr] = (byte offset, h, w, row pitch); the upload itself is upload()"""
        geo = np.zeros((len(self.file_list), 2, 4), np.int64)
        off = 0
        for n, f in enumerate(self.file_list):
            for s, ims in enumerate((lr_ims, hr_ims)):
                a = ims[f]
                if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
                    raise ValueError("image {} is not uint8 RGB: {} {}".format(f, a.shape, a.dtype))
                geo[n, s] = (off, a.shape[0], a.shape[1], 3 * a.shape[1])
                off += a.size
        self.geo = geo
        self.pool_bytes = off
        self._host = (lr_ims, hr_ims)
        self._index = {f: n for n, f in enumerate(self.file_list)}

    # -- caches: the reference's own format, a pickled {stem: uint8 HWC array}
    def cache_lr(self):
        dataLR = os.path.join(self.path, "LR", "X{}".format(self.scale))
        lr_dict = {f: _decode(os.path.join(dataLR, f + "x{}.png".format(self.scale))) for f in self.file_list}
        np.save(self.lr_cache, lr_dict, allow_pickle=True)

    def cache_hr(self):
        dataHR = os.path.join(self.path, "HR")
        hr_dict = {f: _decode(os.path.join(dataHR, f + ".png")) for f in self.file_list}
        np.save(self.hr_cache, hr_dict, allow_pickle=True)

    # -- the device pool
    def upload(self):
        """Copy every image into the packed device pool, once; the host copies are dropped.  batch() calls it on first use."""
        if self.pool is not None:
            return self
        torch = _lib.require_gpu()
        self.device = torch.device("cuda", torch.cuda.current_device()) if self.device is None else torch.device(self.device)
        pool = torch.empty((self.pool_bytes,), dtype=torch.uint8, device=self.device)
        for n, f in enumerate(self.file_list):
            for s, ims in enumerate(self._host):
                o, h, w, p = (int(v) for v in self.geo[n, s])
                pool[o:o + h * p].copy_(torch.from_numpy(np.ascontiguousarray(ims[f]).reshape(-1)))
        self.pool = pool
        self._host = None
        return self

    # -- one sample = one descriptor
    def draw(self):
        """The reference's draws of one __getitem__, in its order (:108, 117, 118, 126, 132, 136, 140)."""
        rng = self.rng
        n = self._index[rng.choice(self.file_list)]
        i = rng.randint(0, int(self.geo[n, 0, 1]) - self.sz)
        j = rng.randint(0, int(self.geo[n, 0, 2]) - self.sz)
        chan = rng.choice([0, 1, 2]) if self.inC == 1 else 0
        fl = fu = k = 0
        if self.rigid_aug:
            fl = int(rng.uniform(0, 1) < 0.5)
            fu = int(rng.uniform(0, 1) < 0.5)
            k = rng.choice([0, 1, 2, 3])
        return Draw(n, i, j, int(i * self.scale), int(j * self.scale), chan, fl, fu, k)

    def descriptors(self, draws):
        """lerf_patch_desc_t records (numpy, _lib.PATCH_DESC_DTYPE) of a list of draws"""
        w = np.asarray(draws, dtype=np.int64).reshape(-1, 9)
        g = self.geo[w[:, 0]]                                         # [n][lr, hr][off, h, w, pitch]
        bad = np.nonzero((w[:, 3] + self.hsz > g[:, 1, 1]) | (w[:, 4] + self.hsz > g[:, 1, 2]))[0]
        if bad.size:
            n = bad[0]
            raise ValueError("the HR window of LR crop ({}, {}) of image {} leaves the HR image ({} x {}): the LR image is "
                             "larger than HR / scale".format(w[n, 1], w[n, 2], self.file_list[w[n, 0]], g[n, 1, 1], g[n, 1, 2]))
        d = np.zeros(len(w), _lib.PATCH_DESC_DTYPE)
        for s, side in enumerate(("lr", "hr")):
            for c, name in enumerate(("off", "h", "w", "pitch")):
                d[side + "_" + name] = g[:, s, c]
        for c, name in enumerate(("li", "lj", "hi", "hj", "chan", "fliplr", "flipud", "k")):
            d[name] = w[:, 1 + c]
        return d

    def batch(self, n):
        """n samples: (im [n, C, sz, sz], lb [n, C, hsz, hsz]) float32 on the device, one launch"""
        torch = _lib.require_gpu()
        self.upload()
        desc = self.descriptors([self.draw() for _ in range(n)])
        noise = None
        if self.nsigma > 0:                                          # :159, one host draw per batch, sample after sample
            noise = torch.from_numpy(np.random.normal(0, self.nsigma / 255.0, (n, self.inC, self.sz, self.sz)).astype(np.float32))
            noise = noise.to(self.device)
        return ops.patch_batch(self.pool, desc, self.inC, self.sz, self.hsz, noise=noise)

    def __getitem__(self, _dump):
        im, lb = self.batch(1)
        return im[0].cpu().numpy(), lb[0].cpu().numpy()

    def __len__(self):
        return int(sys.maxsize)


class Provider(object):
    """data.py:15-51.  `num_workers` is accepted and ignored: the batch is one kernel launch.  Keyword extras go to DIV2K."""

    def __init__(self, batch_size, num_workers, scale, path, patch_size, nsigma=-1, inC=1, **kw):
        self.data = DIV2K(scale, path, patch_size, nsigma, inC=inC, **kw)
        self.batch_size = batch_size
        self.num_workers = num_workers
        self.is_cuda = True
        self.iteration = 0
        self.epoch = 1

    def __len__(self):
        return int(sys.maxsize)

    def next(self):
        self.iteration += 1
        return self.data.batch(self.batch_size)

    def state_dict(self):
        """iteration, epoch and the state of every generator a batch draws from (plain containers: torch.save-able)"""
        rng = self.data.rng.getstate()
        sd = {"iteration": self.iteration, "epoch": self.epoch, "rng": [rng[0], list(rng[1]), rng[2]]}
        if self.data.nsigma > 0:
            s = np.random.get_state()
            sd["np_rng"] = [s[0], [int(v) for v in s[1]], int(s[2]), int(s[3]), float(s[4])]
        return sd

    def load_state_dict(self, sd):
        self.iteration, self.epoch = int(sd["iteration"]), int(sd["epoch"])
        v, words, g = sd["rng"]
        self.data.rng.setstate((v, tuple(words), g))
        if "np_rng" in sd:
            s = sd["np_rng"]
            np.random.set_state((s[0], np.array(s[1], dtype=np.uint32), s[2], s[3], s[4]))


class SRBenchmarkW(object):
    """data.py:171-208: {<dataset>_<stem>_hr, _isc, _osc: uint8 HWC; _isc_matrix, _osc_matrix: 3x3}"""

    def __init__(self, path, datasets):
        self.ims = dict()
        self.files = dict()
        self.datasets = datasets
        for dataset in datasets:
            files = sorted(os.listdir(os.path.join(path, dataset, "HR")))
            self.files[dataset] = files
            for f in files:
                key = dataset + "_" + f[:-4]
                self.ims[key + "_hr"] = _load_rgb(os.path.join(path, dataset, "HR", f))
                for scale in ("isc", "osc"):
                    self.ims[key + "_" + scale] = _load_rgb(os.path.join(path, dataset, scale, f))
                    self.ims[key + "_" + scale + "_matrix"] = _load_matrix(os.path.join(path, dataset, scale, f[:-4]))


class MultiSRBenchmark(object):
    """data.py:247-283: {<dataset>_<stem>hr, <dataset>_<stem>X{int(scale_h)}: uint8 HWC}"""

    def __init__(self, path, datasets=["Set5", "Set14", "B100", "Urban100", "Manga109"], scale_pairs=[[2, 2], [3, 3], [4, 4]],
                 nsigma=-1):
        self.ims = dict()
        self.files = dict()
        self.datasets = datasets
        for dataset in datasets:
            files = sorted(f for f in os.listdir(os.path.join(path, dataset, "HR")) if "png" in f)
            self.files[dataset] = files
            for f in files:
                self.ims[dataset + "_" + f[:-4] + "hr"] = _load_rgb(os.path.join(path, dataset, "HR", f))
                for scale_h, scale_w in scale_pairs:
                    self.ims[dataset + "_" + f[:-4] + "X{}".format(int(scale_h))] = _load_rgb(
                        os.path.join(path, dataset, "LR_bicubic", "rrLR_X{:.2f}_{:.2f}".format(scale_h, scale_w), f))
