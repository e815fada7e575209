"""CPU-only: the g25 resize-gradient fixture is well formed, and its Bicubic image gradients are the transposed resize
A^T G, restated in numpy float64 from the float32 torch-geometry tables of the host export lerf_sr_axis_tables_f32."""
import numpy as np

from lerf_pytorch_amd import _lib


def _cubic(x):
    # resize_right/interp_methods.py:35-43
    a = np.abs(x)
    return (1.5 * a ** 3 - 2.5 * a ** 2 + 1) * (a <= 1) + (-0.5 * a ** 3 + 2.5 * a ** 2 - 4 * a + 2) * ((1 < a) & (a <= 2))


def _axis_matrix(n_in, scale, S, pad_mode):
    """[n_out, n_in] float64: the normalised 1-D cubic resize along one axis, F.pad's rule folded in (A = R (x) C)"""
    n_out = _lib.out_size(n_in, scale)
    left, _, dis32, _ = _lib.sr_axis_tables_f32(n_in, n_out, scale, S)
    k = _cubic(dis32.astype(np.float64))
    k = k / k.sum(axis=1, keepdims=True)
    A = np.zeros((n_out, n_in))
    for i in range(n_out):
        for b in range(S):
            s = int(left[i]) + b
            if pad_mode == "constant" and not 0 <= s < n_in:
                continue
            A[i, min(max(s, 0), n_in - 1)] += k[i, b]
    return A


def test_resize_bwd_is_exported():
    assert "lerf_resize_bwd_f32" in _lib.EXPORTS
    assert _lib.lib().lerf_resize_bwd_f32.argtypes is not None


def test_g25_fixture_shapes(golden):
    g = golden("g25_resize_grads.npz")
    cases = list(g["cases"])
    assert len(cases) >= 30
    seen = set()
    for c in cases:
        kind, S, pad = str(g[c + "/kind"]), int(g[c + "/S"]), str(g[c + "/pad_mode"])
        seen.add((kind, pad))
        assert S == {"gauss": S, "linear": 2, "cubic": 4, "bilinear": 2, "lanczos2": 4, "lanczos3": 6}[kind]
        x, Gi, gx, out = g[c + "/x"], g[c + "/Gi"], g[c + "/gx"], g[c + "/out"]
        scale = g[c + "/scale"]
        assert x.dtype == np.uint8 and x.ndim == 4
        assert scale.dtype == np.float64 and scale.shape == (2,) and scale[0] == scale[1]
        B, C, H, W = x.shape
        oH, oW = _lib.out_size(H, float(scale[0])), _lib.out_size(W, float(scale[1]))
        assert out.dtype == np.float32 and out.shape == (B, C, oH, oW) and not np.isnan(out).any()
        assert Gi.dtype == np.int8 and Gi.shape == out.shape and np.abs(Gi).max() <= 2 and Gi.any()
        assert gx.dtype == np.float32 and gx.shape == x.shape and np.abs(gx).max() > 0
        nh = {"gauss": 3, "linear": 1}.get(kind, 0)
        if nh:
            hy, gh = g[c + "/hy"], g[c + "/gh"]
            assert hy.dtype == np.float32 and hy.shape == (nh,) + x.shape and 0 <= hy.min() and hy.max() <= 1
            assert gh.dtype == np.float32 and gh.shape == (nh,) + x.shape
            assert all(np.abs(gh[k]).max() > 0 for k in range(nh))
        else:
            assert c + "/hy" not in g.files and c + "/gh" not in g.files
    pads = ("constant", "replicate", "reflect", "circular")
    assert {("cubic", p) for p in pads} <= seen
    assert {(k, p) for k in ("gauss", "linear") for p in pads[1:]} <= seen
    assert {k for k, _ in seen} == {"gauss", "linear", "cubic", "bilinear", "lanczos2", "lanczos3"}


def test_g25_bicubic_gradient_is_the_transposed_resize(golden):
    g = golden("g25_resize_grads.npz")
    n = 0
    for c in g["cases"]:
        pad = str(g[c + "/pad_mode"])
        if str(g[c + "/kind"]) != "cubic" or pad not in ("constant", "replicate"):
            continue
        x, gx = g[c + "/x"], g[c + "/gx"].astype(np.float64)
        G = g[c + "/Gi"].astype(np.float64) / 2
        s = float(g[c + "/scale"][0])
        R = _axis_matrix(x.shape[2], s, 4, pad)
        Cm = _axis_matrix(x.shape[3], s, 4, pad)
        want = np.einsum("ih,bcij,jw->bchw", R, G, Cm)               # A^T G with A = R (x) C
        assert np.abs(gx - want).max() <= 1e-4 * np.abs(want).max(), c
        fwd = np.einsum("ih,bchw,jw->bcij", R, x.astype(np.float64), Cm)
        assert np.abs(g[c + "/out"] - fwd).max() <= 1e-4 * np.abs(fwd).max(), c
        n += 1
    assert n == 8
