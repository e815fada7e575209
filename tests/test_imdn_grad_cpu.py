"""CPU-only checks of LeRF-Net training: the new entry points are declared and exported, the host size queries, and the
float64 checker of test_gpu_imdn_train.py (imdn_grad_ref.net_grads) pinned to the reference's own gradients
(tests/golden/g28_imdn_grads.npz, the reference's IMDN2 in float32 on the CPU).

Tolerance of the checker against the golden: 1e-4 of the golden tensor's largest entry.  The golden is a float32 run of
28 convolutions forward and backward (dot products of up to 576 terms); its own rounding error is a few 1e-6 of the largest
entry, while a wrong clamp mask, slope, tap or residual is off by 1e-2 or more."""
import os
import re

import numpy as np
import pytest

import imdn_grad_ref as GR
import imdn_ref64 as R

NEW = ["lerf_imdn_saved_bytes", "lerf_imdn_fwd_train_f32", "lerf_imdn_bwd_workspace_bytes", "lerf_imdn_bwd_f32"]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_declared_and_exported():
    from lerf_pytorch_amd import _lib
    header = open(os.path.join(REPO, "include", "lerf_hip.h")).read()
    declared = set(re.findall(r"\b(lerf_\w+)\(", header))
    lib = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS and name in declared and hasattr(lib, name), name
    assert lib.lerf_abi_version() == 7


def test_size_queries():
    lib = __import__("lerf_pytorch_amd")._lib.lib()
    # saved: fea, 5 module outputs, the upsampler input (7 nf), per module cat (nf) and r1..r3 (3 * 3/4 nf), y (out_nc)
    assert lib.lerf_imdn_saved_bytes(64, 3, 9, 2, 17, 23) == 2 * 17 * 23 * (7 * 64 + 5 * (64 + 3 * 48) + 9) * 4
    assert lib.lerf_imdn_saved_bytes(16, 1, 1, 3, 1, 1) == 3 * (7 * 16 + 5 * (16 + 36) + 1) * 4
    assert lib.lerf_imdn_bwd_workspace_bytes(16, 3, 3, 2, 17, 23) > 2 * 17 * 23 * 16 * 4
    for bad in ((24, 3, 3, 1, 8, 8), (16, 2, 3, 1, 8, 8), (16, 3, 5, 1, 8, 8), (16, 3, 3, 0, 8, 8)):
        assert lib.lerf_imdn_saved_bytes(*bad) == 0 and lib.lerf_imdn_bwd_workspace_bytes(*bad) == 0


def test_fixture_is_well_formed(golden):
    g = golden("g28_imdn_grads.npz")
    for c, n_grads in (("a", 112), ("b", 59)):
        nf, inC, outC, B, H, W, seed = [int(v) for v in g[c + "/cfg"]]
        sd = R.weight_rule(nf, inC, outC, seed)
        assert bytes(g[c + "/digest"]).hex() == R.digest(sd)
        names = [k for k in g.files if k.startswith(c + "/grad/")]
        assert len(names) == n_grads
        for k in names:
            assert g[k].shape == sd[k[len(c + "/grad/"):]].shape and np.abs(g[k]).max() > 0
        assert g[c + "/im"].shape == (B, 3, H, W) and g[c + "/lb"].shape == (B, 3, 2 * H, 2 * W)
        assert np.isfinite(g[c + "/loss"][0]) and g[c + "/loss"][0] > 0


@pytest.mark.parametrize("c", ["a", "b"])
def test_float64_checker_reproduces_the_reference(golden, c):
    import torch
    g = golden("g28_imdn_grads.npz")
    nf, inC, outC, B, H, W, seed = [int(v) for v in g[c + "/cfg"]]
    sd = R.weight_rule(nf, inC, outC, seed)
    for stage, x in ((1, g[c + "/im"]), (2, g[c + "/feat"] / np.float32(255.0))):
        prefix = "stage%d." % stage
        y, grads, gx = GR.net_grads(torch, sd, prefix, x, g[c + "/G%d" % stage], stage, torch.float64)
        assert np.abs(np.abs(y) - 1).min() > 1e-4                      # no float32 run can flip the mask
        frac = float((np.abs(y) > 1).mean())
        assert 0.02 <= frac <= 0.5, frac
        n = 0
        for k in [k for k in g.files if k.startswith(c + "/net/" + prefix)]:
            e = GR.rel_err(g[k], grads[k[len(c + "/net/"):]])
            assert e <= 1e-4, (k, e)
            n += 1
        assert n == 28 + 4                                              # 28 convolutions: every bias, four weights
        e = GR.rel_err(g[c + "/net/x%d" % stage], gx)
        assert e <= 1e-4, ("x", e)
