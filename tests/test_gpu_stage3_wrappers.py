"""The Python side of the eleven stage-3 wrappers of ops.py (resize / warp / remap; hwc, planar, packed, backward): what they
turn down -- exception type and message, word for word -- and the caller-owned `out` of the packed warps.  The values the
wrappers compute are pinned elsewhere (test_gpu_parity, test_gpu_general, test_gpu_remap*, test_gpu_*_grad); the refusals that
test_gpu_remap_batch.py::test_refusals_on_the_device_path already pins (plane and frame counts of a batched geometry) are not
repeated.  Every refused call below is refused before a launch: by the wrapper itself, or by the C ABI's argument checks.

Smallest shapes that reach every branch: a 6 x 5 RGB frame to a 4 x 7 output, S = 2, N = 2, a two-map batched RemapGeometry."""
import contextlib
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W, CN, OH, OW, N = 6, 5, 3, 4, 7, 2
FRAME = "the maps do not match the geometry's frame"
PACKED_FRAME = "packed maps do not match the geometry's frame"
HYPER = "hyper shape mismatch"
GRAD_OUT = "grad_out must be [N, out_h, out_w] of the geometry"
BUFFERS = "gradient buffers must be contiguous float32 [N, H, W]"
COORDS = "grad_coords must be contiguous float64 [N, out_h, out_w, 2]"


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import lerf_pytorch_amd as L
    from lerf_pytorch_amd import ops

    class E:
        pass
    e = E()
    e.torch, e.ops, e.L = torch, ops, L
    rng = np.random.default_rng(7)
    m = np.array([[1.2, 0.1, -0.5], [-0.05, 0.7, 0.4], [1e-3, -2e-3, 1.0]])
    cm = np.stack([rng.uniform(-1.0, H + 1.0, (N, OH, OW)), rng.uniform(-1.0, W + 1.0, (N, OH, OW))], axis=-1)
    e.sr = ops.SrGeometry((H, W), out_hw=(OH, OW), support=2)
    e.sr32 = ops.SrGeometry((H, W), out_hw=(OH, OW), support=2, arithmetic="torch32")
    e.warp = ops.WarpGeometry((H, W), m, (OH, OW), 2)
    e.remap = ops.RemapGeometry((H, W), cm[0], 2)
    e.remap2 = ops.RemapGeometry((H, W), np.ascontiguousarray(cm), 2)
    dev = lambda a: torch.from_numpy(a).cuda()
    e.feat = dev(rng.integers(0, 256, (H, W, CN), dtype=np.uint8))
    e.hq = dev(rng.integers(0, 256, (H, W, CN, 3), dtype=np.uint8))
    e.feat2 = dev(rng.integers(0, 256, (N, H, W, CN), dtype=np.uint8))
    e.hq2 = dev(rng.integers(0, 256, (N, H, W, CN, 3), dtype=np.uint8))
    e.x = dev(rng.random((N, H, W), dtype=np.float32))
    e.hs = [dev(rng.random((N, H, W), dtype=np.float32)) for _ in range(3)]
    e.packed = dev(rng.integers(-2 ** 31, 2 ** 31, (N, H, W, CN), dtype=np.int64).astype(np.int32))
    return e


@contextlib.contextmanager
def raises(exc, text):
    """the exception's type exactly (no subclass of it) and its whole message"""
    with pytest.raises(exc, match="^" + re.escape(text) + "$") as e:
        yield
    assert type(e.value) is exc


# ---------------------------------------------------------------------------------------------- forward wrappers
def test_hwc_wrappers_refuse(env):
    o, t = env.ops, env.torch
    for bad in (env.hq[:, :4], env.hq[..., :2], env.hq[:5]):                    # wrong shape; two maps for the three of gauss
        with raises(ValueError, HYPER):
            o.resize_hwc_u8(env.feat, bad, env.sr, "gauss")
    with raises(o._lib.LerfError, "lerf_resize: unsupported configuration (code -2)"):
        o.resize_hwc_u8(env.feat.float(), env.hq, env.sr, "gauss")             # float32 image, uint8 maps
    for fn, geo in ((o.resize_hwc_u8, env.sr), (o.warp_hwc_u8, env.warp), (o.remap_hwc_u8, env.remap)):
        with pytest.raises(KeyError, match="^'f16'$"):
            fn(env.feat, env.hq, geo, "gauss", out="f16")
    for fn, geo, what in ((o.warp_hwc_u8, env.warp, "lerf_warp"), (o.remap_hwc_u8, env.remap, "lerf_remap")):
        for bad in (env.feat[:, :4], t.zeros((H + 1, W, CN), dtype=t.uint8, device="cuda")):
            with raises(ValueError, FRAME):
                fn(bad, env.hq, geo, "gauss")
        with raises(o._lib.LerfError, what + ": unsupported configuration (code -2)"):
            fn(env.feat.float(), env.hq, geo, "gauss")
    # the batched geometry: frame-major [N,H,W,C] operands, one frame per map
    with raises(ValueError, FRAME):
        o.remap_hwc_u8(env.feat2[:, :, :4], env.hq2, env.remap2, "gauss")
    for bad in (env.hq2[0], env.hq2[:, :5], env.hq2[..., :2], env.hq2[:1]):
        with raises(ValueError, HYPER):
            o.remap_hwc_u8(env.feat2, bad, env.remap2, "gauss")
    assert tuple(o.remap_hwc_u8(env.feat2, env.hq2[..., :1], env.remap2, "linear").shape) == (N, OH, OW, CN)


def test_planar_wrappers_refuse(env):
    o, t = env.ops, env.torch
    with raises(ValueError, "hyper maps must have the shape of the input"):
        o.resize_planar(env.x, [env.hs[0], env.hs[1][:, :5], env.hs[2]], env.sr, "gauss")
    for fn, geo in ((o.resize_planar, env.sr), (o.warp_planar, env.warp), (o.remap_planar, env.remap)):
        with pytest.raises(IndexError):
            fn(env.x, env.hs[:2], geo, "gauss")                                # two maps for the three of gauss
        with pytest.raises(KeyError, match="^'u16'$"):
            fn(env.x, env.hs, geo, "gauss", out="u16")
        with pytest.raises(KeyError, match="^'sinc'$"):
            fn(env.x, env.hs, geo, "sinc")
    with raises(ValueError, FRAME):
        o.remap_planar(env.x[:, :5], env.hs, env.remap, "gauss")
    # resize_planar_u8: uint8 maps, the two kinds with hyper-parameter maps only
    xu, hu = (env.x * 255).to(t.uint8), [(h * 255).to(t.uint8) for h in env.hs]
    for f, h in ((env.x, hu), (xu, [hu[0], env.hs[1], hu[2]]), (xu, [hu[0], hu[1][:, :5], hu[2]])):
        with raises(ValueError, "uint8 maps of the input's shape"):
            o.resize_planar_u8(f, h, env.sr, "gauss")
    with pytest.raises(KeyError, match="^'cubic'$"):
        o.resize_planar_u8(xu, hu, env.sr, "cubic")
    with pytest.raises(IndexError):
        o.resize_planar_u8(xu, hu[:2], env.sr, "gauss")
    assert tuple(o.resize_planar_u8(xu, hu, env.sr, "linear").shape) == (OH, OW, N)


# ---------------------------------------------------------------------------------------------- backward wrappers
def test_backward_wrappers_refuse(env):
    o, t = env.ops, env.torch
    z = lambda *shape, dtype=t.float32: t.zeros(shape, dtype=dtype, device="cuda")
    for fn, geo, what in ((o.resize_bwd_planar, env.sr32, "lerf_resize_bwd_f32"), (o.warp_bwd_planar, env.warp, "lerf_warp_bwd"),
                          (o.remap_bwd_planar, env.remap, "lerf_remap_bwd"), (o.remap_bwd_planar, env.remap2, "lerf_remap_bwd_batched")):
        go = z(N, OH, OW)
        for bad in (z(N, OH, OW + 1), z(N + 1, OH, OW), z(OH, OW)):
            with raises(ValueError, GRAD_OUT):
                fn(env.x, env.hs, geo, "gauss", 10.0, bad, [z(N, H, W)])
        for bad in (z(N, H, W, dtype=t.float64), z(N, H, W + 1), z(N, H, 2 * W)[:, :, ::2], z(H, W)):
            with raises(ValueError, BUFFERS):
                fn(env.x, env.hs, geo, "gauss", 10.0, go, [z(N, H, W), None, bad])
        with raises(ValueError, what + ": invalid argument"):                 # two maps for the three of gauss: the C ABI's refusal
            fn(env.x, env.hs[:2], geo, "gauss", 10.0, go, [z(N, H, W)])
        with pytest.raises(KeyError, match="^'sinc'$"):
            fn(env.x, env.hs, geo, "sinc", 10.0, go, [z(N, H, W)])
        padded = fn(env.x, env.hs, geo, "linear", 1.0, go, [z(N, H, W)])        # a short list is padded with None
        assert len(padded) == 4 and padded[1:] == [None, None, None]
    for geo in (env.remap, env.remap2):
        with raises(ValueError, FRAME):
            o.remap_bwd_planar(env.x[:, :5], env.hs, geo, "gauss", 10.0, z(N, OH, OW), [z(N, 5, W)])
        for bad in (z(N, OH, OW, 2), z(N, OH, OW, dtype=t.float64), z(N, OH, OW, 4, dtype=t.float64)[..., ::2],
                    z(N + 1, OH, OW, 2, dtype=t.float64)):
            with raises(ValueError, COORDS):
                o.remap_bwd_planar(env.x, env.hs, geo, "gauss", 10.0, z(N, OH, OW), [z(N, H, W)], grad_coords=bad)


# ---------------------------------------------------------------------------------------------- packed warps: refusals and `out`
def _packed_calls(env):
    o = env.ops
    return ((lambda p, **kw: o.warp_packed(p, env.warp, "gauss", 10.0, **kw)),
            (lambda p, **kw: o.remap_packed(p, env.remap, "gauss", 10.0, **kw)),
            (lambda p, **kw: o.remap_packed(p, env.remap2, "gauss", 10.0, **kw)))


def test_packed_wrappers_refuse(env):
    t = env.torch
    z = lambda *shape, dtype=t.uint8: t.zeros(shape, dtype=dtype, device="cuda")
    for k, call in enumerate(_packed_calls(env)):
        for bad in (env.packed[:, :, :4], t.zeros((N, H + 1, W, CN), dtype=t.int32, device="cuda")):
            with raises(ValueError, PACKED_FRAME):
                call(bad)
        with pytest.raises(KeyError, match="^'f16'$"):
            call(env.packed, out="f16")
        what = "lerf_warp_packed" if k == 0 else ("lerf_remap_packed" if k == 1 else "lerf_remap_packed_batched")
        with raises(env.ops._lib.LerfError, what + ": unsupported configuration (code -2)"):
            call(env.packed, out="f64")                                          # a dtype the C ABI's packed warps do not write
        msg = "out must be a uint8/float32 tensor of shape %s on the input's device"
        for bad in (z(N, OH, OW + 1, CN), z(N, OH, OW, CN, dtype=t.float64), z(N, OH, OW, CN, dtype=t.int32), z(OH, OW, CN),
                    z(N, OH, OW, 2 * CN)[..., ::2], z(N, OH, OW, CN).cpu()):
            with raises(ValueError, msg % ((N, OH, OW, CN),)):
                call(env.packed, out=bad)
        if k < 2:                                                                # one frame: the message names the 3-D shape
            for bad in (z(OH, OW + 1, CN), z(2, OH, OW, CN), z(OH, OW, CN, dtype=t.float64)):
                with raises(ValueError, msg % ((OH, OW, CN),)):
                    call(env.packed[0], out=bad)


@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_packed_caller_owned_out_has_the_bytes_of_a_fresh_one(env, dtype):
    t = env.torch
    td = {"u8": t.uint8, "f32": t.float32}[dtype]
    same = lambda a, b: a.dtype == b.dtype and a.shape == b.shape and bool((a.contiguous().view(t.uint8) == b.contiguous().view(t.uint8)).all())
    for k, call in enumerate(_packed_calls(env)):
        want = call(env.packed, out=dtype)
        assert want.dtype == td and tuple(want.shape) == (N, OH, OW, CN) and want.is_contiguous()
        own = t.full((N, OH, OW, CN), 7, dtype=td, device="cuda")
        got = call(env.packed, out=own)
        assert got.data_ptr() == own.data_ptr() and same(own, want)
        # frames a gap apart (stride(0) is not dense): the gap stays as it was
        wide = t.full((N, OH + 2, OW, CN), 7, dtype=td, device="cuda")
        view = wide[:, :OH]
        assert view.stride(0) != OH * OW * CN
        got = call(env.packed, out=view)
        assert got.data_ptr() == wide.data_ptr() and same(view, want) and bool((wide[:, OH:] == 7).all())
        # a packed batch that is a strided view itself (dense frames, a gap between them) is read in place
        pw = t.zeros((N, H + 1, W, CN), dtype=t.int32, device="cuda")
        pw[:, :H] = env.packed
        assert same(call(pw[:, :H], out=dtype), want)
        if k < 2:                                                                # a 3-D input: 3-D out, or its [1, ...] form
            one = call(env.packed[0], out=dtype)
            assert tuple(one.shape) == (OH, OW, CN) and same(one, want[0])
            own3 = t.full((OH, OW, CN), 7, dtype=td, device="cuda")
            got = call(env.packed[0], out=own3)
            assert tuple(got.shape) == (OH, OW, CN) and got.data_ptr() == own3.data_ptr() and same(own3, want[0])
            own4 = t.full((1, OH, OW, CN), 7, dtype=td, device="cuda")
            got = call(env.packed[0], out=own4)
            assert tuple(got.shape) == (OH, OW, CN) and same(own4[0], want[0])
