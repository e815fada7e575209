"""GPU tests of lerf_patch_batch_u8 (csrc/lerf_patch.hip) through ctypes: the batch of the DIV2K provider against samples
recorded from the reference (tests/golden/g30_div2k.npz) and against the numpy restatement tests/patch_ref.py.

Everything is compared on bit patterns: the kernel permutes bytes and makes one IEEE division (and one float32 addition
for the noise), so there is no tolerance.  Outputs sit between sentinel floats that must survive every launch."""
import ctypes as C
import json

import numpy as np
import pytest

import patch_ref

pytestmark = pytest.mark.gpu
GUARD = 64                    # sentinel floats before and after each output
SENTINEL = -12345.0
EINVAL = -1


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


@pytest.fixture(scope="module")
def g(golden):
    return golden("g30_div2k.npz")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def pack(images, extra_pitch=0):
    """[(lr, hr), ...] uint8 HWC -> (pool bytes, geo [file][lr, hr] = (off, h, w, pitch)); rows `extra_pitch` bytes apart
    more than dense, the gaps filled with 0xEE"""
    geo, chunks, off = [], [], 0
    for pair in images:
        row = []
        for a in pair:
            h, w = a.shape[:2]
            pitch = 3 * w + extra_pitch
            buf = np.full((h, pitch), 0xEE, np.uint8)
            buf[:, :3 * w] = a.reshape(h, 3 * w)
            row.append((off, h, w, pitch))
            chunks.append(buf.reshape(-1))
            off += h * pitch
        geo.append(row)
    return np.concatenate(chunks), geo


def records(draws, geo):
    from lerf_pytorch_amd import _lib
    d = np.zeros(len(draws), _lib.PATCH_DESC_DTYPE)
    for r, w in zip(d, draws):
        (r["lr_off"], r["lr_h"], r["lr_w"], r["lr_pitch"]), (r["hr_off"], r["hr_h"], r["hr_w"], r["hr_pitch"]) = geo[int(w[0])]
        for name, v in zip(("li", "lj", "hi", "hj", "chan", "fliplr", "flipud", "k"), w[1:]):
            r[name] = int(v)
    return d


class Launch:
    """one call of the C entry point with guarded outputs"""

    def __init__(self, torch, pool, desc, Cn, sz, hsz, noise=None):
        self.torch = torch
        self.B, self.Cn, self.sz, self.hsz = len(desc), Cn, sz, hsz
        self.pool = torch.from_numpy(pool).cuda()
        self.desc = desc
        self.desc_dev = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
        self.noise = None if noise is None else torch.from_numpy(np.ascontiguousarray(noise)).cuda()
        self.n_im, self.n_lb = self.B * Cn * sz * sz, self.B * Cn * hsz * hsz
        self.im = torch.full((self.n_im + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        self.lb = torch.full((self.n_lb + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")

    def run(self, **over):
        from lerf_pytorch_amd import _lib
        a = dict(pool=self.pool.data_ptr(), pool_bytes=self.pool.numel(), desc=self.desc_dev.data_ptr(), desc_host=self.desc.ctypes.data,
                 B=self.B, C=self.Cn, sz=self.sz, hsz=self.hsz, noise=None if self.noise is None else self.noise.data_ptr(),
                 im=self.im.data_ptr() + 4 * GUARD, lb=self.lb.data_ptr() + 4 * GUARD)
        a.update(over)
        rc = _lib.lib().lerf_patch_batch_u8(a["pool"], a["pool_bytes"], a["desc"], a["desc_host"], a["B"], a["C"], a["sz"], a["hsz"],
                                            a["noise"], a["im"], a["lb"], _lib.current_stream())
        self.torch.cuda.synchronize()
        return rc

    def outputs(self):
        """(im, lb) as numpy, after checking the sentinels around them"""
        im, lb = self.im.cpu().numpy(), self.lb.cpu().numpy()
        for buf in (im, lb):
            assert np.all(buf[:GUARD] == SENTINEL) and np.all(buf[-GUARD:] == SENTINEL), "a sentinel was overwritten"
        return (im[GUARD:-GUARD].reshape(self.B, self.Cn, self.sz, self.sz), lb[GUARD:-GUARD].reshape(self.B, self.Cn, self.hsz, self.hsz))

    def untouched(self):
        return bool((self.im == SENTINEL).all()) and bool((self.lb == SENTINEL).all())


def fixture_case(g, ci, n=5):
    """the first n samples of a case whose HR window is inside the image (the kernel's precondition)"""
    case = json.loads(str(g["cases"]))[ci]
    images = [(g["lr_%d_%d" % (ci, f)], g["hr_%d" % f]) for f in range(4)]
    pick = np.nonzero(g["inside_%d" % ci])[0][:n]
    assert len(pick) == n
    sz, Cn = case["sz"], case["inC"]
    ref_im = g["im_%d" % ci][pick]
    ref_lb = np.stack([g["lb_%d_%d" % (ci, p)] for p in pick])
    noise = g["noise_%d" % ci][pick] if case["nsigma"] > 0 else None
    return case, images, g["draws_%d" % ci][pick], sz, int(sz * case["scale"]), Cn, ref_im, ref_lb, noise


@pytest.mark.parametrize("ci", range(5))
def test_fixture_batches_bit_equal(torch, g, ci):
    """B = 5 per case, the fixture's descriptors (case 4: with the fixture's noise); dense and pitched pools; twice"""
    case, images, draws, sz, hsz, Cn, ref_im, ref_lb, noise = fixture_case(g, ci)
    outs = []
    for extra in (0, 7):
        pool, geo = pack(images, extra)
        L = Launch(torch, pool, records(draws, geo), Cn, sz, hsz, noise)
        assert L.run() == 0
        im, lb = L.outputs()
        assert np.array_equal(_bits(im), _bits(ref_im)) and np.array_equal(_bits(lb), _bits(ref_lb))
        assert L.run() == 0                                  # a second launch of the same batch
        im2, lb2 = L.outputs()
        assert np.array_equal(_bits(im2), _bits(im)) and np.array_equal(_bits(lb2), _bits(lb))
        outs.append((im, lb))
    assert np.array_equal(_bits(outs[0][0]), _bits(outs[1][0])) and np.array_equal(_bits(outs[0][1]), _bits(outs[1][1]))


@pytest.mark.parametrize("scale", [2, 3])
@pytest.mark.parametrize("sz", [1, 6, 7, 65])
def test_exhaustive_sweep_against_patch_ref(torch, sz, scale):
    """all 16 (fliplr, flipud, k) x the four corner crops (i = H - sz and j = W - sz among them) x the three channels at
    C = 1, and the same 64 at C = 3; sz 1 (one pixel), 6 and 7 (inside one tile), 65 (three tiles a side, the last one
    pixel wide; hsz 130 and 195: five and seven tiles)"""
    rng = np.random.default_rng(1000 * sz + scale)
    H, W = sz + 3, sz + 5
    lr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    hr = rng.integers(0, 256, (H * scale, W * scale, 3), dtype=np.uint8)
    hsz = sz * scale
    pool, geo = pack([(lr, hr)])
    base = [(0, i, j, i * scale, j * scale, 0, fl, fu, k)
            for (i, j) in ((0, 0), (0, W - sz), (H - sz, 0), (H - sz, W - sz)) for fl in (0, 1) for fu in (0, 1) for k in range(4)]
    for Cn in (1, 3):
        draws = [d[:5] + (c,) + d[6:] for d in base for c in range(3)] if Cn == 1 else base
        L = Launch(torch, pool, records(draws, geo), Cn, sz, hsz)
        assert L.run() == 0
        im, lb = L.outputs()
        for n, d in enumerate(draws):
            rim, rlb = patch_ref.sample(lr, hr, d, sz, hsz, Cn)
            assert np.array_equal(_bits(im[n]), _bits(rim)), (Cn, d)
            assert np.array_equal(_bits(lb[n]), _bits(rlb)), (Cn, d)


def test_refused_arguments_leave_the_outputs_untouched(torch, g):
    case, images, draws, sz, hsz, Cn, _, _, _ = fixture_case(g, 0)
    pool, geo = pack(images)
    desc = records(draws, geo)
    L = Launch(torch, pool, desc, Cn, sz, hsz)
    refused = [dict(pool=None), dict(desc=None), dict(im=None), dict(lb=None), dict(pool_bytes=0), dict(B=0), dict(B=-1),
               dict(C=0), dict(C=2), dict(C=4), dict(sz=0), dict(sz=-3), dict(hsz=0)]
    for over in refused:
        assert L.run(**over) == EINVAL, over
        assert L.untouched(), over
    lh, lw, hh, hw = desc["lr_h"][2], desc["lr_w"][2], desc["hr_h"][2], desc["hr_w"][2]
    bad_fields = [("li", lh - sz + 1), ("lj", lw - sz + 1), ("li", -1), ("hi", hh - hsz + 1), ("hj", hw - hsz + 1), ("hj", -1),
                  ("chan", 3), ("chan", -1), ("k", 4), ("k", -1), ("lr_off", -1), ("hr_off", len(pool)), ("hr_pitch", 3 * hw - 1),
                  ("lr_h", 0)]
    for name, value in bad_fields:                           # checked on the host copy: nothing is launched
        d = desc.copy()
        d[name][2] = value
        assert L.run(desc_host=d.ctypes.data) == EINVAL, (name, value)
        assert L.untouched(), (name, value)
    # a pool one byte shorter than the end of the last image the batch reads: that image would leave the pool
    end = int((desc["hr_off"] + desc["hr_h"].astype(np.int64) * desc["hr_pitch"]).max())
    assert L.run(pool_bytes=end - 1) == EINVAL and L.untouched()
    assert end == len(pool) or L.run(pool_bytes=end) == 0                   # images the batch does not read may lie beyond
    L.im.fill_(SENTINEL)
    L.lb.fill_(SENTINEL)
    assert L.run() == 0 and not L.untouched()
    L.outputs()


def test_ops_wrapper_matches_the_entry_point(torch, g):
    from lerf_pytorch_amd import ops
    case, images, draws, sz, hsz, Cn, ref_im, ref_lb, noise = fixture_case(g, 4)
    pool, geo = pack(images)
    im, lb = ops.patch_batch(torch.from_numpy(pool).cuda(), records(draws, geo), Cn, sz, hsz, noise=torch.from_numpy(noise).cuda())
    assert np.array_equal(_bits(im.cpu().numpy()), _bits(ref_im)) and np.array_equal(_bits(lb.cpu().numpy()), _bits(ref_lb))
    bad = records(draws, geo)
    bad["k"][0] = 7
    with pytest.raises(ValueError, match="lerf_patch_batch_u8"):
        ops.patch_batch(torch.from_numpy(pool).cuda(), bad, Cn, sz, hsz)
