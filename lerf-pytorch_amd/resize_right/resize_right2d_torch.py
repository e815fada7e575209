"""torch-facing resampler classes: drop-in for the LeRF classes of the
reference's resize_right/resize_right2d_torch.py ([B,C,H,W] tensors on the GPU).

SR geometry follows the torch classes' own float32 arithmetic (resize_right2d_torch.py:48-103, bit-equal tables:
lerf_sr_axis_tables_f32), warp geometry the float64 one; SR returns float32, warps return float64 like
the reference (its warp distances are double, resize_right2d_torch.py:286-296).
The SR classes carry autograd (`_ResizeFn`, HIP backward lerf_resize_bwd_f32: every kind -- gauss, linear and the
fixed-kernel subclasses -- and every pad mode, the gradient autograd derives for resize_right2d_torch.py:105-247), and so
do the warp classes (`_WarpFn`, every kind and pad mode: the gradient autograd derives for the reference's torch warps,
resize_right2d_torch.py:249-487).  With no operand requiring grad, both run the plain forward and return no graph.
The remap twins (set_shape takes a coordinate map) differentiate after enable_backward() (`_RemapFn`, lerf_remap_bwd),
the map included when it is a device tensor that requires grad.
"""
from __future__ import annotations

from math import ceil

import torch

from .. import _lib, ops


class _ResizeFn(torch.autograd.Function):
    """lerf_resize forward, lerf_resize_bwd_f32 backward (the gradient autograd derives for resize_right2d_torch.py:105-247,
    every kind and image pad mode) -- used when an input of resize() requires grad (train_model.py:431-441).  Gradients
    come back in each leaf's dtype."""

    @staticmethod
    def forward(ctx, geo, kind, max_sigma, x, *hs):
        xf = x.detach().contiguous().float()
        hf = [h.detach().contiguous().float() for h in hs]
        out = ops.resize_planar(xf, hf, geo, kind, max_sigma, out="f32")
        ctx.save_for_backward(xf, *hf)
        ctx.meta = (geo, kind, float(max_sigma), [t.dtype for t in (x,) + hs])
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, *hs = ctx.saved_tensors
        geo, kind, max_sigma, dtypes = ctx.meta
        need = ctx.needs_input_grad[3:]
        grads = [torch.zeros_like(x) if need[k] else None for k in range(1 + len(hs))]
        ops.resize_bwd_planar(x, hs, geo, kind, max_sigma, grad_out, grads)
        return (None, None, None) + tuple(g.to(dt) if g is not None else None for g, dt in zip(grads, dtypes))


class _WarpFn(torch.autograd.Function):
    """lerf_warp forward (float64 out), lerf_warp_bwd backward (what autograd derives for resize_right2d_torch.py:249-487)
    -- used when an input of warp() requires grad.  Gradients come back in each leaf's dtype."""

    @staticmethod
    def forward(ctx, geo, kind, max_sigma, x, *hs):
        xf = x.detach().contiguous().float()
        hf = [h.detach().contiguous().float() for h in hs]
        out = ops.warp_planar(xf, hf, geo, kind, max_sigma, out="f64")
        ctx.save_for_backward(xf, *hf)
        ctx.meta = (geo, kind, float(max_sigma), [t.dtype for t in (x,) + hs])
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, *hs = ctx.saved_tensors
        geo, kind, max_sigma, dtypes = ctx.meta
        need = ctx.needs_input_grad[3:]
        grads = [torch.zeros_like(x) if need[k] else None for k in range(1 + len(hs))]
        ops.warp_bwd_planar(x, hs, geo, kind, max_sigma, grad_out, grads)
        return (None, None, None) + tuple(g.to(dt) if g is not None else None for g, dt in zip(grads, dtypes))


def _check_dev(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError("{} must be a tensor on the GPU (there is no CPU path)".format(name))


class Resize2dTorch(object):
    def __init__(self, support_sz=4, device="GPU", pad_mode="constant"):
        self._pad_code = _lib.pad_mode_code(pad_mode, _lib.TORCH_PAD_MODES)     # F.pad(input, ..., mode=pad_mode) (:189, :362)
        self.eps = torch.finfo(torch.float32).eps
        self.device = device
        self.init_support_sz = support_sz
        self.pad_mode = pad_mode
        self.antialias = False

    def set_shape(self, in_shape, scale_factors=None, out_shape=None):
        self.support_sz = self.init_support_sz                 # :19
        in_shape = list(in_shape)
        if len(in_shape) != 4:
            raise ValueError("in_shape must be [B, C, H, W]")
        out_hw = None
        if out_shape is not None:                              # :26-29
            out_shape = list(in_shape[:-len(out_shape)]) + list(out_shape)
            out_hw = (out_shape[2], out_shape[3])
            if scale_factors is None:
                scale_factors = [o / i for o, i in zip(out_shape, in_shape)][2:]
        if scale_factors is None:
            raise ValueError("either scale_factors or out_shape is required")
        if not isinstance(scale_factors, (list, tuple)):
            scale_factors = [scale_factors, scale_factors]
        scale_factors = [1] * (4 - len(scale_factors)) + list(scale_factors)
        self.in_shape = in_shape
        self.scale_factors = [float(s) for s in scale_factors]
        self.geo = ops.SrGeometry(in_shape[2:], self.scale_factors[2:], out_hw, self.support_sz, arithmetic="torch32",
                                  pad_mode=self._pad_code)
        self.out_shape = [ceil(self.scale_factors[0] * in_shape[0]), ceil(self.scale_factors[1] * in_shape[1]),
                          self.geo.out_hw[0], self.geo.out_hw[1]]
        pr, pc = self.geo.pad_vec[1], self.geo.pad_vec[2]
        self.pad_vec = [pr[0], pr[1], pc[0], pc[1]]            # the reference's ordering (:93-95)
        if tuple(pr) != tuple(pc):
            # F.pad consumes pad_vec last-dimension first, so the reference pads the columns with the ROW pads and
            # vice versa (:189); harmless while both are (S/2, S/2) -- every up-sampling -- but a shifted / out-of-range
            # gather when they differ (some down-samplings).  That case is not reproduced.
            raise NotImplementedError("row pads {} != column pads {}: the reference mis-pads this geometry".format(pr, pc))

    # dense geometry attributes of the reference object (:48-103), materialised on access only; torch.meshgrid 'ij'
    # (:72-76): inside a patch the row offset varies along the ROW index; dis_* are [B, 1, oH*S, oW*S] float32
    def _dense(self):
        import numpy as np
        h, S = self.geo.host, self.support_sz
        oH, oW = self.geo.out_hw
        k = np.arange(S)
        pr, pc = self.geo.pad_vec[1][0], self.geo.pad_vec[2][0]
        fx = (np.repeat(h["left_r"].astype(np.int64) + pr, S) + np.tile(k, oH))[:, None] + np.zeros((1, oW * S), np.int64)
        fy = (np.repeat(h["left_c"].astype(np.int64) + pc, S) + np.tile(k, oW))[None, :] + np.zeros((oH * S, 1), np.int64)
        dx = np.repeat(h["dis_r32"].reshape(-1)[:, None], oW * S, axis=1)
        dy = np.repeat(h["dis_c32"].reshape(-1)[None, :], oH * S, axis=0)
        B = self.in_shape[0]
        dev = self.geo.device
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return t(fx), t(fy), t(dx)[None, None].repeat(B, 1, 1, 1), t(dy)[None, None].repeat(B, 1, 1, 1)

    field_of_view_x = property(lambda self: self._dense()[0])
    field_of_view_y = property(lambda self: self._dense()[1])
    dis_x = property(lambda self: self._dense()[2])
    dis_y = property(lambda self: self._dense()[3])

    def _run(self, kind, input, hypers, max_sigma):
        _check_dev(input, "input")
        B, Cn, H, W = input.shape
        if [H, W] != list(self.in_shape[2:]):
            raise ValueError("input shape does not match set_shape")
        x = input.reshape(B * Cn, H, W)
        hs = []
        for h in hypers:
            _check_dev(h, "hyper-parameter map")
            hs.append(h.reshape(B * Cn, H, W))
        if torch.is_grad_enabled() and any(t.requires_grad for t in [x] + hs):
            out = _ResizeFn.apply(self.geo, kind, max_sigma, x, *hs)
        else:
            out = ops.resize_planar(x, hs, self.geo, kind, max_sigma, out="f32")
        return out.reshape(B, Cn, self.geo.out_hw[0], self.geo.out_hw[1])


    kind = None                                                # fixed-kernel subclasses name their interp_methods kernel

    def resize(self, input):
        """default interpolation process (:105-129): weight(dis_x, dis_y) normalised over the patch."""
        if self.kind is None:
            raise NotImplementedError("Resize2dTorch.resize needs a subclass with a weight kernel")
        return self._run(self.kind, input, [], 1.0)


class BicubicResize2dTorch(Resize2dTorch):                     # :131-138, interp_methods.cubic2d
    kind = "cubic"

    def __init__(self, support_sz=4, device="CPU", pad_mode="constant"):
        super().__init__(support_sz, device, pad_mode)


class BilinearResize2dTorch(Resize2dTorch):                    # interp_methods.linear2d on the same base class
    kind = "bilinear"

    def __init__(self, support_sz=2, device="CPU", pad_mode="constant"):
        super().__init__(support_sz, device, pad_mode)


class Lanczos2Resize2dTorch(Resize2dTorch):                    # interp_methods.lanczos2d
    kind = "lanczos2"

    def __init__(self, support_sz=4, device="CPU", pad_mode="constant"):
        super().__init__(support_sz, device, pad_mode)


class Lanczos3Resize2dTorch(Resize2dTorch):                    # interp_methods.lanczos3d
    kind = "lanczos3"

    def __init__(self, support_sz=6, device="CPU", pad_mode="constant"):
        super().__init__(support_sz, device, pad_mode)


class SteeringGaussianResize2dTorch(Resize2dTorch):
    def __init__(self, support_sz=4, device="GPU", pad_mode="constant", max_sigma=10):
        super().__init__(support_sz, device, pad_mode)
        self.max_sigma = max_sigma

    def resize(self, input, rho, sigma_x, sigma_y):
        return self._run("gauss", input, [rho, sigma_x, sigma_y], self.max_sigma)


class AmplifiedLinearResize2dTorch(Resize2dTorch):
    def __init__(self, support_sz=2, device="GPU", pad_mode="constant", max_sigma=1):
        super().__init__(support_sz, device, pad_mode)
        self.max_sigma = max_sigma

    def resize(self, input, alpha):
        return self._run("linear", input, [alpha], self.max_sigma)


class Warp2dTorch(object):
    def __init__(self, support_sz=4, device="GPU", pad_mode="constant"):
        self._pad_code = _lib.pad_mode_code(pad_mode, _lib.TORCH_PAD_MODES)     # F.pad(input, ..., mode=pad_mode) (:189, :362)
        self.eps = torch.finfo(torch.float32).eps
        self.device = device
        self.support_sz = support_sz
        self.pad_mode = pad_mode

    def set_shape(self, in_shape, matrix, out_shape):
        in_shape = list(in_shape)
        out_shape = list(out_shape) + list(in_shape[len(out_shape):])      # :263
        self.in_shape, self.out_shape, self.matrix = in_shape, out_shape, matrix
        self.in_sz = [in_shape[2], in_shape[3]]
        self.out_sz = [out_shape[2], out_shape[3]]
        self.geo = ops.WarpGeometry(self.in_sz, matrix, self.out_sz, self.support_sz, pad_mode=self._pad_code)
        pr, pc = self.geo.pad_vec[1], self.geo.pad_vec[2]
        self.pad_vec = [pc[0], pc[1], pr[0], pr[1]]                         # last dim first (:330-332)

    def _run(self, kind, input, hypers, max_sigma):
        _check_dev(input, "input")
        B, Cn, H, W = input.shape
        if [H, W] != list(self.in_sz):
            raise ValueError("input shape does not match set_shape")
        x = input.reshape(B * Cn, H, W)
        hs = []
        for h in hypers:
            _check_dev(h, "hyper-parameter map")
            hs.append(h.reshape(B * Cn, H, W))
        if torch.is_grad_enabled() and any(t.requires_grad for t in [x] + hs):
            out = _WarpFn.apply(self.geo, kind, max_sigma, x, *hs)
        else:
            out = ops.warp_planar(x, hs, self.geo, kind, max_sigma, out="f64")
        return out.reshape(B, Cn, self.out_sz[0], self.out_sz[1])


class NearestWarp2dTorch(Warp2dTorch):
    def __init__(self, support_sz=1, device="CPU", pad_mode="constant"):
        super().__init__(support_sz, device, pad_mode)

    def warp(self, input):
        return self._run("nearest", input, [], 1.0)


class SteeringGaussianWarp2dTorch(Warp2dTorch):
    def __init__(self, support_sz=4, device="GPU", pad_mode="constant", max_sigma=10):
        super().__init__(support_sz, device, pad_mode)
        self.max_sigma = max_sigma

    def warp(self, input, rho, sigma_x, sigma_y):
        return self._run("gauss", input, [rho, sigma_x, sigma_y], self.max_sigma)


class AmplifiedLinearWarp2dTorch(Warp2dTorch):
    def __init__(self, support_sz=2, device="GPU", pad_mode="constant", max_sigma=1):
        super().__init__(support_sz, device, pad_mode)
        self.max_sigma = max_sigma

    def warp(self, input, alpha):
        return self._run("linear", input, [alpha], self.max_sigma)


# fixed-kernel baselines of the reference (resize_right2d_numpy.py:451-494, resize_right2d_torch.py:372-388);
# weights from resize_right/interp_methods.py evaluated in float64 on the device
class BicubicWarp2dTorch(Warp2dTorch):
    def __init__(self, support_sz=4, device="CPU", pad_mode="constant"):
        super().__init__(support_sz, device, pad_mode)

    def warp(self, input):
        return self._run("cubic", input, [], 1.0)


class BilinearWarp2dTorch(Warp2dTorch):
    def __init__(self, support_sz=2, device="CPU", pad_mode="constant"):
        super().__init__(support_sz, device, pad_mode)

    def warp(self, input):
        return self._run("bilinear", input, [], 1.0)


class Lanczos2Warp2dTorch(Warp2dTorch):
    def __init__(self, support_sz=4, device="CPU", pad_mode="constant"):
        super().__init__(support_sz, device, pad_mode)

    def warp(self, input):
        return self._run("lanczos2", input, [], 1.0)


class Lanczos3Warp2dTorch(Warp2dTorch):
    def __init__(self, support_sz=6, device="CPU", pad_mode="constant"):
        super().__init__(support_sz, device, pad_mode)

    def warp(self, input):
        return self._run("lanczos3", input, [], 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# Remap twins: the *Warp2dTorch classes with set_shape(in_shape, coords) in place of (in_shape, matrix, out_shape) -- the
# projected grid comes from a dense coordinate map ([oH, oW, 2] (row, col), unclipped: coords.py; numpy or a device tensor; or
# [B, oH, oW, 2], one map per sample of the batch, one launch) instead of a matrix (ops.RemapGeometry).  Forward-only by
# default: an input that requires grad is an error rather than a silently detached result.  enable_backward() (opt-in, like IMDN2's) turns autograd on: `_RemapFn`, HIP backward
# lerf_remap_bwd -- the image and hyper-parameter gradients of the warp classes and, when the map given to set_shape is a
# device tensor that requires grad, the gradient with respect to the map (a flow field, a mesh, a lens model fitted by
# gradient: coords.from_flow_torch keeps a flow in the graph).
# ---------------------------------------------------------------------------------------------------------------------
class _RemapFn(torch.autograd.Function):
    """lerf_remap forward (float64 out), lerf_remap_bwd backward.  `cm` is the map given to set_shape when it is a device
    tensor that requires grad (else None): its gradient is the per-plane map gradient summed over the planes, in the map's
    dtype and shape (autograd carries it through a strided view) -- for a [B, oH, oW, 2] map, every sample's gradient summed
    over that sample's planes only.  Leaf gradients come back in each leaf's dtype."""

    @staticmethod
    def forward(ctx, geo, kind, max_sigma, cm, x, *hs):
        xf = x.detach().contiguous().float()
        hf = [h.detach().contiguous().float() for h in hs]
        out = ops.remap_planar(xf, hf, geo, kind, max_sigma, out="f64")
        # the kernels read the map through the geometry's detached alias; saving the map itself lets autograd's version counter
        # refuse a backward after the map was modified in place (it would differentiate another map than the forward used)
        ctx.save_for_backward(xf, *hf, *([] if cm is None else [cm]))
        ctx.meta = (geo, kind, float(max_sigma), [t.dtype for t in (x,) + hs], None if cm is None else cm.dtype)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        geo, kind, max_sigma, dtypes, cdtype = ctx.meta
        saved = ctx.saved_tensors                                          # raises if a saved tensor was modified in place
        x, *hs = saved if cdtype is None else saved[:-1]
        need = ctx.needs_input_grad[4:]
        grads = [torch.zeros_like(x) if need[k] else None for k in range(1 + len(hs))]
        gc = None
        if cdtype is not None and ctx.needs_input_grad[3]:
            gc = torch.zeros((x.shape[0],) + tuple(geo.out_hw) + (2,), dtype=torch.float64, device=x.device)
        ops.remap_bwd_planar(x, hs, geo, kind, max_sigma, grad_out, grads, gc)
        if gc is not None:                                                 # planes [b * P, (b + 1) * P) read map b
            gc = (gc.view((geo.n_maps, -1) + tuple(gc.shape[1:])).sum(1) if geo.batched else gc.sum(0)).to(cdtype)
        return (None, None, None, gc) + \
            tuple(g.to(dt) if g is not None else None for g, dt in zip(grads, dtypes))


class Remap2dTorch(Warp2dTorch):
    _backward = False

    def enable_backward(self):
        """Opt in to autograd through warp(): image, hyper-parameter and map gradients by lerf_remap_bwd.  Returns self.
        The map gets a gradient when the tensor given to set_shape lives on the GPU and requires grad; a numpy map is data; a
        HOST tensor that requires grad is refused (ValueError) rather than silently detached.  The geometry reads the map's
        memory in place: modifying a leaf map in place between warp() and backward() is an error autograd reports."""
        self._backward = True
        return self

    def set_shape(self, in_shape, coords):
        in_shape = list(in_shape)                                           # [B, C, H, W]
        self.in_shape, self.coords = in_shape, coords
        self.in_sz = [in_shape[2], in_shape[3]]
        self.geo = ops.RemapGeometry(self.in_sz, coords, self.support_sz, pad_mode=self._pad_code)
        if self.geo.batched and self.geo.n_maps != in_shape[0]:            # [B, oH, oW, 2]: sample b's C planes read map b
            raise ValueError("a 4-D coordinate map holds one map per sample: its leading size must equal in_shape[0]")
        self.out_sz = list(self.geo.out_hw)
        self.out_shape = in_shape[:2] + self.out_sz

    def _run(self, kind, input, hypers, max_sigma):
        _check_dev(input, "input")
        B, Cn, H, W = input.shape
        if [H, W] != list(self.in_sz):
            raise ValueError("input shape does not match set_shape")
        if self.geo.batched and B != self.geo.n_maps:
            raise ValueError("input batch does not match the %d maps of set_shape" % self.geo.n_maps)
        x = input.reshape(B * Cn, H, W)
        hs = []
        for h in hypers:
            _check_dev(h, "hyper-parameter map")
            hs.append(h.reshape(B * Cn, H, W))
        cm = self.coords if isinstance(self.coords, torch.Tensor) and self.coords.requires_grad else None
        if cm is not None and not cm.is_cuda and torch.is_grad_enabled():
            raise ValueError("the coordinate map requires grad but lives on the host: it was uploaded as data and would get no "
                             "gradient (build it on the GPU, e.g. coords.from_flow_torch of a device flow, or detach it)")
        if cm is not None and not cm.is_cuda:
            cm = None
        if torch.is_grad_enabled() and (cm is not None or any(t.requires_grad for t in [x] + hs)):
            if not self._backward:
                raise NotImplementedError("the remap classes are forward-only: an input requires grad and there is no remap backward "
                                          "(detach the inputs or run under torch.no_grad(); the *Warp2dTorch classes differentiate) "
                                          "unless the class has opted in with enable_backward()")
            out = _RemapFn.apply(self.geo, kind, max_sigma, cm, x, *hs)
        else:
            out = ops.remap_planar(x, hs, self.geo, kind, max_sigma, out="f64")
        return out.reshape(B, Cn, self.out_sz[0], self.out_sz[1])


class NearestRemap2dTorch(Remap2dTorch):
    def __init__(self, support_sz=1, device="CPU", pad_mode="constant"):
        super().__init__(support_sz, device, pad_mode)

    def warp(self, input):
        return self._run("nearest", input, [], 1.0)


class SteeringGaussianRemap2dTorch(Remap2dTorch):
    def __init__(self, support_sz=4, device="GPU", pad_mode="constant", max_sigma=10):
        super().__init__(support_sz, device, pad_mode)
        self.max_sigma = max_sigma

    def warp(self, input, rho, sigma_x, sigma_y):
        return self._run("gauss", input, [rho, sigma_x, sigma_y], self.max_sigma)


class AmplifiedLinearRemap2dTorch(Remap2dTorch):
    def __init__(self, support_sz=2, device="GPU", pad_mode="constant", max_sigma=1):
        super().__init__(support_sz, device, pad_mode)
        self.max_sigma = max_sigma

    def warp(self, input, alpha):
        return self._run("linear", input, [alpha], self.max_sigma)


class BicubicRemap2dTorch(Remap2dTorch):
    def __init__(self, support_sz=4, device="CPU", pad_mode="constant"):
        super().__init__(support_sz, device, pad_mode)

    def warp(self, input):
        return self._run("cubic", input, [], 1.0)


class BilinearRemap2dTorch(Remap2dTorch):
    def __init__(self, support_sz=2, device="CPU", pad_mode="constant"):
        super().__init__(support_sz, device, pad_mode)

    def warp(self, input):
        return self._run("bilinear", input, [], 1.0)


class Lanczos2Remap2dTorch(Remap2dTorch):
    def __init__(self, support_sz=4, device="CPU", pad_mode="constant"):
        super().__init__(support_sz, device, pad_mode)

    def warp(self, input):
        return self._run("lanczos2", input, [], 1.0)


class Lanczos3Remap2dTorch(Remap2dTorch):
    def __init__(self, support_sz=6, device="CPU", pad_mode="constant"):
        super().__init__(support_sz, device, pad_mode)

    def warp(self, input):
        return self._run("lanczos3", input, [], 1.0)
