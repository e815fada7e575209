"""CPU-only tests of resample/data.py and resample/train_model.py: the host side of the DIV2K provider against samples
recorded from the reference (tests/golden/g30_div2k.npz, written by gen_div2k_golden.py), the cache files, the validation
loaders, the options and the learning-rate schedule.  The kernel itself is tested in test_gpu_patch.py."""
import json
import math
import os
import random

import numpy as np
import pytest

from conftest import REPO

import patch_ref

import lerf_pytorch_amd  # noqa: F401
from lerf_pytorch_amd.resample import data as D
from lerf_pytorch_amd.resample import train_model as T

N_CASES = 5


@pytest.fixture(scope="module")
def g(golden):
    return golden("g30_div2k.npz")


def _case(g, ci):
    case = json.loads(str(g["cases"]))[ci]
    files = json.loads(str(g["files"]))
    hr = {f: g["hr_%d" % n] for n, f in enumerate(files)}
    lr = {f: g["lr_%d_%d" % (ci, n)] for n, f in enumerate(files)}
    return case, files, lr, hr


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("ci", range(N_CASES))
def test_patch_ref_reproduces_the_reference(g, ci):
    case, files, lr, hr = _case(g, ci)
    sz, C = case["sz"], case["inC"]
    hsz = int(sz * case["scale"])
    draws, ims = g["draws_%d" % ci], g["im_%d" % ci]
    n_short = 0
    for n, d in enumerate(draws):
        noise = g["noise_%d" % ci][n] if case["nsigma"] > 0 else None
        im, lb = patch_ref.sample(lr[files[d[0]]], hr[files[d[0]]], d, sz, hsz, C, noise)
        ref_lb = g["lb_%d_%d" % (ci, n)]
        assert im.dtype == np.float32 and np.array_equal(_bits(im), _bits(ims[n]))
        assert lb.shape == ref_lb.shape and np.array_equal(_bits(lb), _bits(ref_lb))
        ins = patch_ref.inside(hr[files[d[0]]].shape, d, hsz)
        assert ins == bool(g["inside_%d" % ci][n]) == (lb.shape == (C, hsz, hsz))
        n_short += not ins
    if case["scale"] in (3, 1.5):                       # HR sizes are multiples of 3: LR * scale == HR
        assert n_short == 0


def _dataset(g, ci, seed):
    case, files, lr, hr = _case(g, ci)
    return D.DIV2K.from_arrays(case["scale"], lr, hr, case["sz"], case["nsigma"], inC=case["inC"], file_list=files, seed=seed), case


@pytest.mark.parametrize("ci", range(N_CASES))
def test_draw_reproduces_every_fixture_descriptor(g, ci):
    ds, case = _dataset(g, ci, case_seed(g, ci))
    draws = [ds.draw() for _ in range(24)]
    assert np.array_equal(np.array(draws, dtype=np.int64), g["draws_%d" % ci])
    assert ds.hsz == int(case["sz"] * case["scale"])
    inside = g["inside_%d" % ci]
    good = [d for d, ok in zip(draws, inside) if ok]
    desc = ds.descriptors(good)
    assert desc.dtype.itemsize == 72 and len(desc) == len(good)
    for r, d in zip(desc, good):                        # the pool layout: LR then HR of every file, dense
        lh, lw = g["lr_%d_%d" % (ci, d.file)].shape[:2]
        hh, hw = g["hr_%d" % d.file].shape[:2]
        assert (r["lr_h"], r["lr_w"], r["lr_pitch"], r["hr_h"], r["hr_w"], r["hr_pitch"]) == (lh, lw, 3 * lw, hh, hw, 3 * hw)
        assert r["hr_off"] == r["lr_off"] + lh * lw * 3
        assert tuple(r[k] for k in ("li", "lj", "hi", "hj", "chan", "fliplr", "flipud", "k")) == tuple(d[1:])
    assert int((desc["hr_off"] + desc["hr_h"].astype(np.int64) * desc["hr_pitch"]).max()) <= ds.pool_bytes
    for d, ok in zip(draws, inside):
        if not ok:
            with pytest.raises(ValueError, match="leaves the HR image"):
                ds.descriptors([d])


def case_seed(g, ci):
    return json.loads(str(g["cases"]))[ci]["seed"]


def test_global_random_mode_matches_private_seed(g):
    saved = random.getstate()
    try:
        for ci in (0, 3):
            seed = case_seed(g, ci)
            private, _ = _dataset(g, ci, seed)
            shared, _ = _dataset(g, ci, None)
            assert shared.rng is random
            random.seed(seed)
            assert [shared.draw() for _ in range(24)] == [private.draw() for _ in range(24)]
    finally:
        random.setstate(saved)


def test_provider_state_dict_is_plain_and_restores_the_draws(g):
    case, files, lr, hr = _case(g, 1)
    p = D.Provider.__new__(D.Provider)
    p.data, _ = _dataset(g, 1, 5)
    p.batch_size, p.num_workers, p.iteration, p.epoch = 4, 0, 7, 1
    [p.data.draw() for _ in range(3)]
    sd = p.state_dict()
    json.dumps(sd)                                       # ints, strings, lists, None only
    after = [p.data.draw() for _ in range(6)]
    p.iteration = 99
    p.load_state_dict(sd)
    assert p.iteration == 7 and [p.data.draw() for _ in range(6)] == after


def test_refusals():
    img = {"a": np.zeros((8, 8, 3), np.uint8)}
    with pytest.raises(NotImplementedError, match="scale <= 1"):
        D.DIV2K.from_arrays(0.5, img, img, 4)
    with pytest.raises(ValueError, match="max_nsigma"):
        D.DIV2K.from_arrays(2, img, img, 4, nsigma=0)
    with pytest.raises(ValueError, match="not uint8 RGB"):
        D.DIV2K.from_arrays(2, img, {"a": np.zeros((8, 8), np.uint8)}, 4)


def test_cache_files_round_trip(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(3)
    files = ["0001", "0002", "0003"]
    hr = {f: rng.integers(0, 256, (12 + 2 * n, 16, 3), dtype=np.uint8) for n, f in enumerate(files)}
    lr = {f: rng.integers(0, 256, (6 + n, 8, 3), dtype=np.uint8) for n, f in enumerate(files)}
    os.makedirs(tmp_path / "HR")
    os.makedirs(tmp_path / "LR" / "X2")
    for f in files:
        Image.fromarray(hr[f]).save(tmp_path / "HR" / (f + ".png"))
        Image.fromarray(lr[f]).save(tmp_path / "LR" / "X2" / (f + "x2.png"))
    ds = D.DIV2K(2, str(tmp_path), 4, file_list=files, seed=0)
    for name, ims in (("cache_hr.npy", hr), ("cache_lr_x2.npy", lr)):
        cached = np.load(tmp_path / name, allow_pickle=True).item()          # the reference's format: a pickled dict
        assert sorted(cached) == files and all(np.array_equal(cached[f], ims[f]) for f in files)
    assert [tuple(ds.geo[n, 1, 1:3]) for n in range(3)] == [hr[f].shape[:2] for f in files]
    assert ds.pool_bytes == sum(a.size for a in hr.values()) + sum(a.size for a in lr.values())
    # a cache written the reference's way (np.save of the dict) is used as is: no PNG is needed any more
    other = tmp_path / "other"
    os.makedirs(other)
    np.save(other / "cache_hr.npy", hr, allow_pickle=True)
    np.save(other / "cache_lr_x2.npy", lr, allow_pickle=True)
    ds2 = D.DIV2K(2, str(other), 4, file_list=files, seed=0)
    assert np.array_equal(ds2.geo, ds.geo)
    assert [ds2.draw() for _ in range(5)] == [ds.draw() for _ in range(5)]


def test_benchmark_loaders_keys_and_shapes():
    root = os.path.join(REPO, "tests", "data")
    stems = ["baby", "bird", "butterfly", "head", "woman"]
    v = D.MultiSRBenchmark(root, ["Set5"])
    assert v.datasets == ["Set5"] and v.files["Set5"] == [s + ".png" for s in stems]
    assert sorted(v.ims) == sorted("Set5_" + s + t for s in stems for t in ("hr", "X2", "X3", "X4"))
    assert v.ims["Set5_babyhr"].shape == (512, 512, 3) and v.ims["Set5_babyX4"].shape == (128, 128, 3)
    assert v.ims["Set5_womanhr"].shape == (344, 228, 3) and v.ims["Set5_womanX3"].shape == (114, 76, 3)
    assert all(a.dtype == np.uint8 for a in v.ims.values())
    w = D.SRBenchmarkW(root, ["Set5"])
    assert sorted(w.ims) == sorted("Set5_" + s + t for s in stems for t in ("_hr", "_isc", "_osc", "_isc_matrix", "_osc_matrix"))
    assert w.ims["Set5_bird_isc_matrix"].shape == (3, 3) and w.ims["Set5_bird_isc"].ndim == 3
    assert w.ims["Set5_bird_hr"].shape == (288, 288, 3)


def test_parse_defaults_equal_the_reference(g):
    ref = json.loads(str(g["options"]))
    ap = T.build_parser()
    ours = {a.dest: a.default for a in ap._actions if a.dest != "help"}
    assert sorted(ours) == sorted(name for name, _ in ref)
    for name, value in ref:
        assert ours[name] == value, name
    opt = T.parse([], make_dirs=False)
    assert opt.scale == 4 and isinstance(opt.scale, int)
    assert T.parse(["--scale", "1.5"], make_dirs=False).scale == 1.5
    dbg = T.parse(["--debug"], make_dirs=False)
    assert (dbg.displayStep, dbg.saveStep, dbg.valStep, dbg.totalIter, dbg.batchSize, dbg.nf) == (10, 100, 50, 200, 4, 16)


def test_parse_directories_and_opt_txt(tmp_path):
    opt = T.parse(["-e", str(tmp_path / "exp"), "--lutft", "--batchSize", "256"])
    assert opt.valoutDir == os.path.join(str(tmp_path / "exp"), "lutft") and os.path.isdir(opt.valoutDir)
    text = open(os.path.join(opt.valoutDir, "opt.txt")).read()
    assert "batchSize: 256" in text and "[default: 16]" in text
    assert opt.name == "exp-SRNetsSWF2"
    opt = T.parse(["--modelRoot", str(tmp_path), "--name", "auto"])
    assert opt.expDir == os.path.join(str(tmp_path), "auto", "expr_1") and os.path.isdir(os.path.join(opt.expDir, "val"))
    assert T.parse(["--modelRoot", str(tmp_path), "--name", "auto"]).expDir.endswith("expr_2")


@pytest.mark.parametrize("lr1", [-1.0, 1e-4])
def test_lr_multiplier_is_the_reference_formula(lr1):
    opt = T.parse(["--lr1", str(lr1), "--totalIter", "5000"], make_dirs=False)
    lf = T.lr_lambda(opt)
    a, b = (0.8, 0.2) if lr1 < 0 else (1 - lr1 / opt.lr0, lr1 / opt.lr0)
    for x in (0, opt.totalIter / 2, opt.totalIter):
        assert lf(x) == (((1 + math.cos(x * math.pi / opt.totalIter)) / 2) ** 1.0) * a + b
    assert lf(0) == 1.0 and abs(lf(opt.totalIter) - b) < 1e-15


def test_refused_runs():
    with pytest.raises(NotImplementedError, match="allreduce_grads"):
        T.main(["--gpuNum", "2"])
    with pytest.raises(NotImplementedError, match="scale < 1"):
        T.main(["--scale", "0.5"])
