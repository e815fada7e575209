"""GPU tests of resample/data.py's Provider and of resample/train_model.py: batches against the samples recorded from the
reference (tests/golden/g30_div2k.npz), and short end-to-end runs of main() on a DIV2K folder of eight 64x64 crops of Set5.

Weights of two runs are never compared: the resampler and LUT backwards add with float atomics, so two runs differ in the
last bits.  What must be equal is what is deterministic: the batches and the learning rates."""
import json
import os
import shutil

import numpy as np
import pytest

from conftest import ASSETS, DATA, REPO

pytestmark = pytest.mark.gpu
FILES = ["%04d" % n for n in range(1, 9)]


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


def _provider(g, ci, batch, seed):
    from lerf_pytorch_amd.resample.data import DIV2K, Provider
    case = json.loads(str(g["cases"]))[ci]
    files = json.loads(str(g["files"]))
    hr = {f: g["hr_%d" % n] for n, f in enumerate(files)}
    lr = {f: g["lr_%d_%d" % (ci, n)] for n, f in enumerate(files)}
    p = Provider.__new__(Provider)
    p.data = DIV2K.from_arrays(case["scale"], lr, hr, case["sz"], case["nsigma"], inC=case["inC"], file_list=files,
                               seed=case["seed"] if seed is None else seed)
    p.batch_size, p.num_workers, p.is_cuda, p.iteration, p.epoch = batch, 0, True, 0, 1
    return p, case


@pytest.mark.parametrize("ci", [1, 3])
def test_provider_batches_equal_the_fixture(torch, g, ci):
    """cases 1 (x3, inC 3) and 3 (x1.5, inC 3): every HR window is inside its image, so 2 x 8 consecutive samples stack"""
    B = 8
    p, case = _provider(g, ci, B, None)
    for call in range(2):
        im, lb = p.next()
        assert im.is_cuda and lb.is_cuda and im.dtype == torch.float32 and p.iteration == call + 1
        ref_lb = np.stack([g["lb_%d_%d" % (ci, n)] for n in range(call * B, (call + 1) * B)])
        assert np.array_equal(_bits(im.cpu().numpy()), _bits(g["im_%d" % ci][call * B:(call + 1) * B]))
        assert np.array_equal(_bits(lb.cpu().numpy()), _bits(ref_lb))


def test_getitem_with_noise_equals_the_fixture(torch, g):
    p, case = _provider(g, 4, 1, None)
    state = np.random.get_state()
    try:
        np.random.seed(case["np_seed"])
        for n in range(3):
            im, lb = p.data[0]
            assert isinstance(im, np.ndarray) and im.shape == (1, case["sz"], case["sz"])
            assert np.array_equal(_bits(im), _bits(g["im_4"][n])) and np.array_equal(_bits(lb), _bits(g["lb_4_%d" % n]))
    finally:
        np.random.set_state(state)


def test_provider_state_dict_round_trip(torch, g):
    a, _ = _provider(g, 1, 4, 77)
    a.next()
    sd = a.state_dict()
    want = [tuple(t.cpu().numpy() for t in a.next()) for _ in range(3)]
    b, _ = _provider(g, 1, 4, 12345)                         # another seed: only the restored state can make it agree
    b.load_state_dict(sd)
    assert b.iteration == 1
    for im, lb in want:
        bim, blb = b.next()
        assert np.array_equal(_bits(bim.cpu().numpy()), _bits(im)) and np.array_equal(_bits(blb.cpu().numpy()), _bits(lb))


# ------------------------------------------------------------------ main() on a small DIV2K folder
@pytest.fixture(scope="module")
def div2k(torch, tmp_path_factory):
    """<tmp>/HR/000N.png: eight 64x64 crops of the Set5 HR images; <tmp>/LR/X4/000Nx4.png: resize_right's x1/4 of them"""
    from PIL import Image
    from lerf_pytorch_amd.resample.make_lr import make_lr_image
    root = tmp_path_factory.mktemp("DIV2K")
    os.makedirs(root / "HR")
    os.makedirs(root / "LR" / "X4")
    stems = ["baby", "bird", "butterfly", "head", "woman"]
    for n, f in enumerate(FILES):
        img = np.array(Image.open(os.path.join(DATA, "HR", stems[n % 5] + ".png")))
        y, x = 40 + 70 * (n // 5), 60 + 50 * (n // 5)
        hr = np.ascontiguousarray(img[y:y + 64, x:x + 64, :3])
        Image.fromarray(hr).save(root / "HR" / (f + ".png"))
        Image.fromarray(make_lr_image(hr, 4, 4)).save(root / "LR" / "X4" / (f + "x4.png"))
    return str(root)


@pytest.fixture()
def recording(monkeypatch):
    """train_model.Provider replaced by a subclass over the eight files, seeded, that keeps every batch it hands out"""
    from lerf_pytorch_amd.resample import data, train_model
    batches = []

    class Recording(data.Provider):
        def __init__(self, *a, **kw):
            super().__init__(*a, file_list=FILES, seed=11, **kw)

        def next(self):
            im, lb = super().next()
            batches.append((im.cpu().numpy(), lb.cpu().numpy()))
            return im, lb

    monkeypatch.setattr(train_model, "Provider", Recording)
    return batches


COMMON = ["--batchSize", "4", "--cropSize", "12", "--totalIter", "6", "--displayStep", "2", "--saveStep", "3", "--valStep", "6"]


def _lut_dir(tmp_path, name="exp"):
    """an experiment folder holding the shipped lerf-g LUTs under the names train_model --lutft reads (LUT_*.npy)"""
    exp = tmp_path / name
    os.makedirs(exp)
    for f in os.listdir(os.path.join(ASSETS, "lerf-g")):
        if f.startswith("LUTft_"):
            shutil.copy(os.path.join(ASSETS, "lerf-g", f), exp / f.replace("LUTft_", "LUT_"))
    return str(exp)


def test_lutft_run_logs_validates_checkpoints_and_exports(torch, div2k, recording, tmp_path):
    from lerf_pytorch_amd.resample import train_model
    exp = _lut_dir(tmp_path)
    steps = []
    train_model.main(["-e", exp, "--lutft", "--model", "SWF2LUT", "--twoStage", "--trainDir", div2k,
                      "--valDir", os.path.join(REPO, "tests", "data"), "--valWDir", str(tmp_path / "nowhere")] + COMMON,
                     on_step=lambda i, lr, loss: steps.append((i, lr, loss)))
    log = open(os.path.join(exp, "lutft.log")).read().splitlines()
    shown = [l for l in log if "GPixel:" in l]
    assert len(shown) == 3 and ["Iter:%6d" % i in l for i, l in zip((2, 4, 6), shown)] == [True] * 3
    assert all("Sample:" in l and "dT:" in l and "rT:" in l for l in shown)
    assert [i for i, _, _ in steps] == [1, 2, 3, 4, 5, 6] and all(np.isfinite(loss) for _, _, loss in steps)
    heads = [l for l in log if "Iter 000006" in l]
    rows = [l for l in log if " : Set5" in l]
    assert len(heads) == 1 and "2.0x2.0" in heads[0] and len(rows) == 1              # one validation table: SR over valDir
    cells = rows[0].split("\t")[1:]
    assert len(cells) == 3 and all(np.isfinite(float(v)) for c in cells for v in c.split("/"))
    assert sum("validation (warp) skipped" in l for l in log) == 1
    assert os.path.exists(os.path.join(exp, "lutft", "opt.txt"))
    for i in (3, 6):
        ck = torch.load(os.path.join(exp, "Checkpoint_%06d.pth" % i), map_location="cpu", weights_only=True)
        assert sorted(ck) == ["iteration", "model", "optimizer", "provider"] and ck["iteration"] == i
    for key in ["s1_%sr0" % m for m in "sct"] + ["s2_%sr%d" % (m, r) for m in "sct" for r in (0, 1)]:
        a = np.load(os.path.join(exp, "LUTft_%s.npy" % key))
        assert a.dtype == np.int8 and a.shape == np.load(os.path.join(ASSETS, "lerf-g", "LUTft_%s.npy" % key)).shape
    assert len(recording) == 6 and recording[0][0].shape == (4, 1, 12, 12) and recording[0][1].shape == (4, 1, 48, 48)


@pytest.mark.parametrize("model,extra,weights", [("SRNetsSWF2", ["--nf", "64"], "srnets_weights.npz"),
                                                 ("IMDN2", ["--inC", "3", "--featC", "3"], "imdn2_weights.npz")])
def test_network_runs_write_their_export(torch, div2k, recording, tmp_path, model, extra, weights):
    from lerf_pytorch_amd.resample import eval_model, train_model
    exp = str(tmp_path / "net")
    losses = []
    train_model.main(["-e", exp, "--model", model, "--twoStage", "--trainDir", div2k, "--valDir", str(tmp_path / "none"),
                      "--valWDir", str(tmp_path / "none")] + extra + COMMON, on_step=lambda i, lr, loss: losses.append(loss))
    assert len(losses) == 6 and all(np.isfinite(losses))
    assert os.path.exists(os.path.join(exp, weights)) and os.path.exists(os.path.join(exp, "train.log"))
    opt = eval_model.parse(["--model", model, "-e", exp, "--twoStage"] + extra)
    m = eval_model.load_model(opt)
    assert sum(p.numel() for p in m.parameters()) > 0


def test_resume_continues_the_schedule_and_the_batches(torch, div2k, recording, tmp_path):
    from lerf_pytorch_amd.resample import train_model
    base = ["--lutft", "--model", "SWF2LUT", "--twoStage", "--trainDir", div2k, "--valDir", str(tmp_path / "none"),
            "--valWDir", str(tmp_path / "none")] + COMMON
    whole, first, second = [], [], []
    train_model.main(["-e", _lut_dir(tmp_path, "whole")] + base, on_step=lambda i, lr, loss: whole.append((i, lr)))
    whole_batches = list(recording)
    del recording[:]
    exp = _lut_dir(tmp_path, "parts")

    def until3(i, lr, loss):                                 # the same 6-iteration cosine, stopped after iteration 3
        first.append((i, lr))
        return i < 3

    train_model.main(["-e", exp] + base, on_step=until3)
    out = train_model.main(["-e", exp, "--startIter", "3"] + base, on_step=lambda i, lr, loss: second.append((i, lr)))
    assert [i for i, _ in first + second] == [1, 2, 3, 4, 5, 6]
    lf = train_model.lr_lambda(out.opt)
    assert [lr for _, lr in whole] == [out.opt.lr0 * lf(i - 1) for i in range(1, 7)]
    assert [lr for _, lr in first + second] == [lr for _, lr in whole]
    assert len(recording) == 6
    for (im, lb), (wim, wlb) in zip(recording, whole_batches):
        assert np.array_equal(_bits(im), _bits(wim)) and np.array_equal(_bits(lb), _bits(wlb))
    assert {int(s["step"]) for s in out.opt_G.state.values()} == {6}
    assert out.scheduler.last_epoch == 6
