"""CPU-only: the host side of resize_right.resize -- interp_methods values, the per-axis tables (left index, weights) and
the argument handling -- against the reference's own results recorded in tests/golden/g29_rr.npz
(tests/golden/gen_rr_golden.py).  Bit-equal: the tables decide which pixels a resize reads and with what weights."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import gen_rr_golden as G                                                     # noqa: E402  (the case list and the seeded inputs)

import lerf_pytorch_amd as L                                                  # noqa: E402,F401
from lerf_pytorch_amd import _lib                                             # noqa: E402
from lerf_pytorch_amd.resize_right import interp_methods as IM                # noqa: E402
from lerf_pytorch_amd.resize_right import resize_right as R                   # noqa: E402
from lerf_pytorch_amd.resize_right.resize_right import resize                 # noqa: E402


@pytest.fixture(scope="module")
def g29():
    return np.load(os.path.join(GOLDEN, "g29_rr.npz"))


def plan_of(c):
    kw = dict(c["kw"])
    name = kw.pop("interp_method", "cubic")
    method = G.gauss5 if name == "gauss5" else getattr(IM, name)
    is_np = c["fw"] == "np"
    pad = _lib.pad_mode_code(kw.get("pad_mode", "constant"), _lib.NUMPY_PAD_MODES if is_np else _lib.TORCH_PAD_MODES)
    scales, sizes = R._scales_and_sizes(c["shape"], kw.get("out_shape"), kw.get("scale_factors"), False, is_np)
    return R._plan(c["shape"], scales, sizes, method, kw.get("support_sz"), kw.get("antialiasing", True), pad, is_np), sizes


@pytest.mark.parametrize("name", G.KERNELS)
def test_interp_methods_bit_equal_numpy_float64(g29, name):
    got = getattr(IM, name)(g29["im_x"])
    assert np.asarray(got, dtype=np.float64).tobytes() == g29["im_" + name].tobytes()


def test_interp_methods_surface():
    for name, sz in (("cubic", 4), ("lanczos2", 4), ("lanczos3", 6), ("linear", 2), ("box", 1), ("cubic2d", 4), ("linear2d", 2),
                     ("box2d", 1), ("lanczos2d", 4), ("lanczos3d", 6)):
        assert getattr(IM, name).support_sz == sz
    x, y = np.linspace(-2, 2, 9), np.linspace(-1, 1, 9)
    assert np.array_equal(IM.cubic2d(x, y), IM.cubic(x) * IM.cubic(y))
    assert np.array_equal(IM.lanczos3d(x, y), IM.lanczos3(x) * IM.lanczos3(y))

    @IM.support_sz(3)
    def f(v):
        return v
    assert f.support_sz == 3


def test_interp_methods_torch_keep_dtype():
    import torch
    for dt in (torch.float32, torch.float64):
        x = torch.linspace(-3, 3, 25, dtype=dt)
        for name in G.KERNELS:
            y = getattr(IM, name)(x)
            assert y.dtype == dt and y.shape == x.shape
            ref = getattr(IM, name)(x.double().numpy())
            assert np.allclose(y.double().numpy(), ref, atol=1e-5)


def test_tables_bit_equal_golden(g29):
    cases = json.loads(str(g29["cases"]))
    assert len(cases) > 150
    for i, c in enumerate(cases):
        plan, sizes = plan_of(c)
        dim, tab = plan[-1]
        assert dim == c["table_dim"], (i, c)
        assert list(g29["out_%d" % i].shape) == [int(s) for s in sizes], (i, c)
        left, w = g29["left_%d" % i], g29["w_%d" % i]
        assert np.array_equal(tab.left, left), (i, c)
        assert tab.w.dtype == (np.float64 if c["fw"] == "np" else np.float32)
        assert tab.w.tobytes() == np.ascontiguousarray(w.astype(tab.w.dtype)).tobytes(), (i, c)


def test_pass_order_is_ascending_scale_and_stable():
    scales, sizes = R._scales_and_sizes([6, 7, 5, 2], None, [2, 0.5, 0.5], False, True)
    plan = R._plan([6, 7, 5, 2], scales, sizes, IM.cubic, None, True, 0, True)
    assert [d for d, _ in plan] == [1, 2, 0]                                   # equal scales keep their dim order; scale 1 is skipped
    scales, sizes = R._scales_and_sizes([2, 3, 8, 8], None, 0.5, False, False)
    assert scales == [1.0, 1.0, 0.5, 0.5] and sizes == [2, 3, 4, 4]            # torch: the last dims
    scales, sizes = R._scales_and_sizes([8, 8, 3], None, 0.5, False, True)
    assert scales == [0.5, 0.5, 1.0] and sizes == [4, 4, 3]                    # numpy: the first dims
    scales, sizes = R._scales_and_sizes([15, 14, 3], [9, 20], None, False, True)
    assert scales == [9 / 15, 20 / 14, 1.0] and sizes == [9, 20, 3]


def test_adjoint_csr_is_the_transpose():
    rng = np.random.default_rng(3)
    for pad in range(5):
        for n_in, scale in ((9, 0.4), (5, 0.125), (7, 2.3), (1, 3.0)):
            n_out = int(np.ceil(n_in * scale))
            tab = R.axis_table(n_in, n_out, scale, IM.cubic, 4, True, pad, True)
            dense = np.zeros((n_out, n_in))
            for j in range(n_out):
                for k in range(tab.taps):
                    s = int(tab.left[j]) + k
                    if pad == 0:
                        if not 0 <= s < n_in:
                            continue
                    else:
                        s = np.pad(np.arange(n_in), 64, mode=_lib.NUMPY_PAD_MODES[pad])[s + 64]
                    dense[j, s] += tab.w[j, k]
            row_ptr, idx, wt = tab.adjoint(np.float64)
            back = np.zeros((n_in, n_out))
            for s in range(n_in):
                e = slice(row_ptr[s], row_ptr[s + 1])
                assert list(idx[e]) == sorted(idx[e])                          # fixed (j, k) order
                np.add.at(back[s], idx[e], wt[e])
            y = rng.normal(size=n_out)
            assert np.allclose(back, dense.T, rtol=0, atol=1e-15), (pad, n_in, scale)
            assert np.allclose(back @ y, dense.T @ y)


def test_bad_arguments_raise():
    x = np.zeros((8, 8))
    with pytest.raises(NotImplementedError, match="default path"):
        resize(x, 0.5, by_convs=True)
    with pytest.raises(NotImplementedError, match="default path"):
        resize(x, [0.5, 0.5], by_convs=[False, True])
    with pytest.raises(ValueError, match="scale_factors or out_shape"):
        resize(x)
    with pytest.raises(NotImplementedError, match="pad_mode"):
        resize(x, 0.5, pad_mode="mean")
    with pytest.raises(NotImplementedError, match="pad_mode"):
        resize(x, 0.5, pad_mode="replicate")                                   # a torch name on a numpy input
    with pytest.raises(ValueError):
        resize(x, [0.5, 0.5, 0.5])
    with pytest.raises(ValueError):
        resize(x, -1.0)
    with pytest.raises(ValueError, match="support_sz"):
        resize(x, 0.5, interp_method=lambda d: d)
    with pytest.raises(TypeError):
        resize([[1.0, 2.0]], 0.5)


def test_scale_one_returns_the_input_without_a_gpu():
    x = np.arange(12.0).reshape(3, 4)
    assert resize(x, [1, 1]) is x
