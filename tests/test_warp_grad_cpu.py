"""CPU-only: the warp backward's C entry point is exported, and the g24 warp-gradient fixture is well formed."""
import ctypes

import numpy as np

import lerf_pytorch_amd as L
from lerf_pytorch_amd import _lib


def test_warp_bwd_is_exported():
    assert "lerf_warp_bwd" in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "lerf_warp_bwd")
    assert _lib.lib().lerf_warp_bwd.argtypes is not None


def test_g24_fixture_shapes(golden):
    g, g13 = golden("g24_warp_grads.npz"), golden("g13_torch_warp.npz")
    cases = list(g["cases"])
    assert len(cases) >= 30
    kinds, pads, layouts = set(), set(), set()
    n_nan = 0
    for c in cases:
        kind, S, pad, layout = str(g[c + "/kind"]), int(g[c + "/S"]), str(g[c + "/pad_mode"]), str(g[c + "/layout"])
        kinds.add(kind)
        pads.add(pad)
        layouts.add(layout)
        assert g[c + "/matrix"].shape == (3, 3) and S >= 1
        B, C = {"b2c1": (2, 1), "b1c1": (1, 1), "b1c3": (1, 3)}[layout]
        Gi, gx = g[c + "/Gi"], g[c + "/gx"]
        assert Gi.dtype == np.int8 and Gi.shape[:2] == (B, C) and np.abs(Gi).max() <= 2 and Gi.any()
        oH, oW = Gi.shape[2:]
        if c + "/out" in g.files:                       # the forward output, or a pointer to the same in g13
            out = g[c + "/out"]
        else:
            base = g13[str(g[c + "/out_g13"])]
            assert base.shape == (2, 1, oH, oW)
            out = base if layout == "b2c1" else np.concatenate([base[:, 0], g[c + "/out_c2"][None]])[None]
        assert out.dtype == np.float64 and out.shape == Gi.shape
        assert gx.dtype == np.float32 and gx.shape == (B, C, 52, 52)
        assert np.nanmax(np.abs(gx)) > 0
        nh = {"gauss": 3, "linear": 1}.get(kind, 0)
        if nh:
            gh = g[c + "/gh"]
            assert gh.dtype == np.float32 and gh.shape == (nh, B, C, 52, 52)
            for k in range(nh):
                assert np.nanmax(np.abs(gh[k])) > 0
        else:
            assert c + "/gh" not in g.files
        n_nan += int(np.isnan(out).any())
    assert kinds == {"gauss", "linear", "nearest", "cubic"}
    assert pads == {"constant", "replicate", "reflect", "circular"}
    assert layouts == {"b2c1", "b1c1", "b1c3"}
    assert n_nan >= 1
