"""GPU: seeded programs over the deferred sum / expression layer (tests/lazy_programs.py), lazy on against plain numpy.

Each program runs twice on the same mirrors: with `lazy.set_enabled(False)` on plain ndarrays -- numpy itself is the
expectation, every statement is numpy's own -- and with lazy results on.  Every value the program names must come back with
numpy's dtype, shape and BIT PATTERN (the sign of zero counts; NaN must be NaN, any payload).  Both launch paths of the LUT pass
(41 x 57: the direct kernel; 260 x 330: the LDS-resident one) and both kinds of image (device, host).  The passes themselves are
pinned to the oracle in test_gpu_lut_interp.py; here they are the same kernels on both sides.  A failure prints the seed and the
program, so one failing seed is one pytest id."""
import os
import sys

import numpy as np
import pytest

from conftest import ASSETS
import lazy_programs as lp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(oracle):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import callsite_driver as cd
    luts = cd.float_luts(oracle.load_luts(os.path.join(ASSETS, "lerf-g"), linear=False))
    interp, pads, _ = cd.mirror_api(linear=False)
    return interp, pads, luts


def bits(a):
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def differences(got, want):
    """[text] of what differs between the named values of the two runs"""
    out = []
    if [n for n, _ in got] != [n for n, _ in want]:
        return ["names %s != %s" % ([n for n, _ in got], [n for n, _ in want])]
    for (name, g), (_, w) in zip(got, want):
        gn, wn = np.asarray(g), np.asarray(w)
        if gn.dtype != wn.dtype or gn.shape != wn.shape:
            out.append("%s: %s %s, numpy %s %s" % (name, gn.dtype, gn.shape, wn.dtype, wn.shape))
            continue
        gn, wn = np.ascontiguousarray(gn).reshape(-1), np.ascontiguousarray(wn).reshape(-1)
        ok = (bits(gn) == bits(wn)) | (np.isnan(gn) & np.isnan(wn))
        if not ok.all():
            k = int(np.flatnonzero(~ok)[0])
            out.append("%s: %d of %d elements differ; first at %d: got %r (0x%x), numpy %r (0x%x)"
                       % (name, int((~ok).sum()), ok.size, k, gn[k].item(), int(bits(gn)[k]), wn[k].item(), int(bits(wn)[k])))
    return out


@pytest.mark.parametrize("hw", [(41, 57), (260, 330)])
@pytest.mark.parametrize("device_image", [True, False])
@pytest.mark.parametrize("seed", lp.SEEDS)
def test_program_gives_numpys_bits(env, seed, device_image, hw):
    from lerf_pytorch_amd import lazy
    interp, pads, luts = env
    prog = lp.generate(seed)
    lazy.set_enabled(False)
    try:
        want = lp.execute(prog, interp, pads, luts, lambda a: a, hw)            # plain numpy all the way
    finally:
        lazy.set_enabled(True)
    for _, w in want:
        assert isinstance(w, (np.ndarray, np.generic)), type(w)
    got = lp.execute(prog, interp, pads, luts, (lambda a: lazy.asdevice(a)) if device_image else (lambda a: a), hw)
    diff = differences(got, want)
    if diff:
        pytest.fail("seed %d, %s image, %d x %d:\n  %s\nprogram:\n%s" % (seed, "device" if device_image else "host", hw[0], hw[1],
                                                                       "\n  ".join(diff), lp.render(prog)))
