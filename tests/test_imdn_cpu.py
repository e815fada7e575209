"""CPU-only checks of the LeRF-Net (IMDN2) port: the fixtures g27_imdn.npz / g28_eval_model.json are well formed, the
seeded weight rule and the float64 restatement (imdn_ref64.py) reproduce the reference's IMDN2, the model's state_dict
keys are the reference's, and eval_model accepts the reference's options.  No device code runs here."""
import json
import os
import types

import numpy as np
import pytest

from conftest import GOLDEN

import imdn_ref64 as R

CASES = [(64, 3, 3, 2, 17, 23), (16, 1, 3, 1, 33, 65), (64, 3, 1, 1, 1, 1), (16, 3, 3, 1, 40, 9)]


def test_g27_well_formed(golden):
    g = golden("g27_imdn.npz")
    for i, (nf, inC, outC, B, H, W) in enumerate(CASES):
        cfg = g["%d/cfg" % i]
        assert tuple(int(v) for v in cfg[:6]) == (nf, inC, outC, B, H, W)
        assert g["%d/x" % i].shape == (B, inC, H, W) and g["%d/x" % i].dtype == np.float32
        assert g["%d/y1" % i].shape == g["%d/p1" % i].shape == (B, inC, H, W)
        assert g["%d/y2" % i].shape == g["%d/p2" % i].shape == (B, inC * outC, H, W)
        for k in ("y1", "y2", "p1", "p2"):
            assert np.isfinite(g["%d/%s" % (i, k)]).all()
        assert 0 <= g["%d/p1" % i].min() and g["%d/p1" % i].max() <= 254
        assert 0 <= g["%d/p2" % i].min() and g["%d/p2" % i].max() <= 1


def test_g28_well_formed():
    g = json.load(open(os.path.join(GOLDEN, "g28_eval_model.json")))
    assert g["files"] == ["baby.png", "bird.png", "butterfly.png", "head.png", "woman.png"]
    assert set(g["cases"]) == {"lerf-g", "imdn2"}
    for c in g["cases"].values():
        for rows in c["sr"].values():
            assert len(rows) == 5 and all(5 < p < 60 and 0 < s <= 1 for p, s in rows)
        assert len(c["u8"]["md5"]) == 32
        for rows in c["warp"].values():
            assert len(rows) == 5 and all(5 < p < 60 for p in rows)


@pytest.mark.parametrize("i", range(4))
def test_weight_rule_reproduces_digest(golden, i):
    g = golden("g27_imdn.npz")
    nf, inC, outC, _, _, _, seed = [int(v) for v in g["%d/cfg" % i]]
    assert R.digest(R.weight_rule(nf, inC, outC, seed)) == bytes(g["%d/digest" % i]).hex()


@pytest.mark.parametrize("i", range(4))
def test_float64_restatement_matches_reference(golden, i):
    g = golden("g27_imdn.npz")
    nf, inC, outC, _, _, _, seed = [int(v) for v in g["%d/cfg" % i]]
    sd = R.weight_rule(nf, inC, outC, seed)
    x = g["%d/x" % i]
    for key, y64 in (("y1", R.imdn_rtc(sd, "stage1.", x)), ("y2", R.imdn_rtc(sd, "stage2.", x)),
                     ("p2", R.post(R.imdn_rtc(sd, "stage2.", g["%d/p1" % i] / np.float32(255.0)), 2))):
        ref = g["%d/%s" % (i, key)]
        assert np.abs(y64 - ref).max() <= 1e-4 * max(1.0, float(np.abs(ref).max())), key
    assert np.abs(R.post(R.imdn_rtc(sd, "stage1.", x), 1) - g["%d/p1" % i]).max() <= 127 * 1e-4


@pytest.mark.parametrize("nf,inC,outC", [(16, 1, 3), (64, 3, 3), (64, 3, 1), (16, 3, 3)])
def test_state_dict_keys_are_the_reference_keys(golden, nf, inC, outC):
    import torch  # noqa: F401
    from lerf_pytorch_amd.resample.model import IMDN2
    g = golden("g27_imdn.npz")
    want = [str(s) for s in g["keys/%d/%d/%d" % (nf, inC, outC)]]
    m = IMDN2(types.SimpleNamespace(nf=nf, norm=255), inC=inC, outC=outC)
    got = ["%s:%s" % (k, "x".join(str(s) for s in v.shape)) for k, v in m.state_dict().items()]
    assert got == want
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == R.imdn2_keys(nf, inC, outC)


def test_eval_model_parse_accepts_reference_options():
    from lerf_pytorch_amd.resample import eval_model as E
    opt = E.parse(["--model", "IMDN2", "-e", "models/x", "--loadIter", "1000", "--testDir", "data/rrBenchmark",
                   "--resultRoot", "results/warp", "--twoStage", "--inC", "3", "--outC", "3", "--featC", "3", "--nf", "16",
                   "--suppSize", "2", "--maxSigma", "10", "--norm", "255", "--modes", "sct", "--modes2", "sct"])
    assert (opt.model, opt.expDir, opt.loadIter, opt.twoStage, opt.inC, opt.featC, opt.nf) == ("IMDN2", "models/x", 1000, True, 3, 3, 16)
    d = E.parse([])
    assert (d.model, d.nf, d.inC, d.outC, d.featC, d.norm, d.loadIter, d.twoStage) == ("SRNetsSWF2", 64, 1, 3, 1, 255, 50000, False)
    assert E.weights_path(opt) == os.path.join("models/x", "Model_001000.pth")


def test_imdn_abi_host_queries():
    from lerf_pytorch_amd import _lib
    lib = _lib.lib()
    for nf, inC, outC in [(16, 1, 1), (16, 3, 9), (48, 1, 3), (64, 3, 3), (64, 3, 9)]:
        assert lib.lerf_imdn_weight_floats(nf, inC, outC) == sum(int(np.prod(s)) for _, s in R.state_keys(nf, inC, outC))
    for bad in [(24, 3, 3), (8, 3, 3), (80, 3, 3), (16, 2, 3), (16, 3, 4)]:
        assert lib.lerf_imdn_weight_floats(*bad) == 0
    assert lib.lerf_imdn_workspace_bytes(64, 2, 17, 23) == 2 * 17 * 23 * 18 * 64
    assert lib.lerf_imdn_workspace_bytes(64, 0, 17, 23) == 0
