"""`resize`: the separable, anti-aliased, any-scale resize of the reference's resize_right/resize_right.py (same
signature and defaults) for numpy arrays and torch tensors -- the function that made every `rrLR_X*` low-resolution
folder this project evaluates on.

Where the work runs.  Per resized dim the host builds two small tables, O(n_out * taps): the first source index of every
output and its normalised weights, by calling the interpolation callable exactly as the reference does (numpy: float64;
torch: float32 grid and weights, as the reference's torch branch computes them) -- which is also how any user callable
with a `support_sz` is supported.  Everything O(pixels) runs on the MI355X: one HIP axis pass per resized dim
(lerf_rr_axis, csrc/lerf_rr.hip), dims in ascending order of scale like the reference, sums in tap order.  numpy inputs
are uploaded and come back like the results of resize_right2d_numpy.py (a device-backed array while lazy results are
enabled, else a numpy array); torch inputs must be on the GPU and stay there.  There is no CPU path.

torch results are differentiable with respect to the input (a torch.autograd.Function per axis pass; the backward gathers
over the transposed table, no atomics).  `by_convs=True` is refused: it is an optimisation switch of the reference with a
torch-only implementation, and the default path computes the same resize.

`resize_to_uint8` is this project's addition: the same resize of a numpy image with the last pass writing
`np.round(np.clip(x, 0, 255)).astype(np.uint8)` from its float64 sums (resample/make_lr.py).
"""
from __future__ import annotations

import ctypes as C
from math import ceil

import numpy

try:
    import torch
except ImportError:
    torch = None

from .. import _lib
from . import interp_methods

_NP_EPS = numpy.finfo(numpy.float32).eps


# ------------------------------------------------------------------ arguments (reference :284-344)
def _is_numpy_like(x):
    from .. import lazy
    return isinstance(x, (numpy.ndarray, lazy.DeviceArray))


def _scales_and_sizes(in_shape, out_shape, scale_factors, by_convs, is_numpy):
    """full-length scale and size lists.  Fewer entries than dims: numpy resizes the FIRST dims, torch the LAST; a scalar scale
    means two dims; out_shape alone derives the scales, scales alone give ceil(scale * in)."""
    if scale_factors is None and out_shape is None:
        raise ValueError("either scale_factors or out_shape should be provided")
    flags = by_convs if isinstance(by_convs, (list, tuple)) else [by_convs]
    if any(bool(f) for f in flags):
        raise NotImplementedError(
            "by_convs=True is not implemented: it is an optimisation switch of the reference (torch only); the default "
            "path, by_convs=False, computes the same resize")
    in_shape = list(in_shape)
    nd = len(in_shape)
    if out_shape is not None:
        out_shape = list(out_shape)
        if len(out_shape) > nd:
            raise ValueError("out_shape has more entries than the input has dims")
        out_shape = out_shape + in_shape[len(out_shape):] if is_numpy else in_shape[:nd - len(out_shape)] + out_shape
        if any(int(o) != o or o < 1 for o in out_shape):
            raise ValueError("out_shape entries must be positive integers")
        out_shape = [int(o) for o in out_shape]
        if scale_factors is None:
            scale_factors = [o / i for o, i in zip(out_shape, in_shape)]
    if not isinstance(scale_factors, (list, tuple)):
        scale_factors = [scale_factors, scale_factors]
    scale_factors = list(scale_factors)
    if len(scale_factors) > nd:
        raise ValueError("more scale factors than the input has dims")
    fill = [1] * (nd - len(scale_factors))
    scale_factors = scale_factors + fill if is_numpy else fill + scale_factors
    if any(not (s > 0) for s in scale_factors):
        raise ValueError("scale factors must be positive")
    if out_shape is None:
        out_shape = [ceil(s * i) for s, i in zip(scale_factors, in_shape)]
    return [float(s) for s in scale_factors], out_shape


# ------------------------------------------------------------------ per-axis tables (reference :130-218, :347-359)
class AxisTable(object):
    """left[n_out] int32 (first source index of each output, unpadded coordinates), w[n_out][taps] (normalised weights,
    float64 for numpy inputs, float32 for torch), the pad rule; device copies and the adjoint CSR are made on demand."""

    def __init__(self, n_in, n_out, left, w, pad_code):
        self.n_in, self.n_out, self.taps = int(n_in), int(n_out), int(w.shape[1])
        self.left = numpy.ascontiguousarray(left, dtype=numpy.int32)
        self.w = numpy.ascontiguousarray(w)
        self.pad_code = int(pad_code)
        self._dev = {}

    def weights_as(self, np_dtype):
        return self.w if self.w.dtype == np_dtype else self.w.astype(np_dtype)      # float32 -> float64 is exact

    def adjoint(self, np_dtype):
        """host CSR of the transposed map: (row_ptr[n_in + 1], idx[nnz], wt[nnz])"""
        w = numpy.ascontiguousarray(self.weights_as(np_dtype))
        row_ptr = numpy.zeros(self.n_in + 1, numpy.int32)
        idx = numpy.zeros(self.n_out * self.taps, numpy.int32)
        wt = numpy.zeros(self.n_out * self.taps, np_dtype)
        code = _lib.LERF_F64 if numpy.dtype(np_dtype) == numpy.float64 else _lib.LERF_F32
        nnz = _lib.lib().lerf_rr_adjoint_csr(self.n_in, self.n_out, self.taps, self.left.ctypes.data, w.ctypes.data, code,
                                              self.pad_code, row_ptr.ctypes.data, idx.ctypes.data, wt.ctypes.data)
        if nnz < 0:
            _lib.check(nnz, "lerf_rr_adjoint_csr")
        return row_ptr, idx[:max(nnz, 1)].copy(), wt[:max(nnz, 1)].copy()

    def device(self, dev, np_dtype, adjoint=False):
        key = (str(dev), numpy.dtype(np_dtype).str, adjoint)
        hit = self._dev.get(key)
        if hit is None:
            if adjoint:
                hit = tuple(torch.from_numpy(a).to(dev) for a in self.adjoint(np_dtype))
            else:
                hit = (torch.from_numpy(self.left).to(dev), torch.from_numpy(numpy.ascontiguousarray(self.weights_as(np_dtype))).to(dev))
            self._dev[key] = hit
        return hit


def axis_table(in_sz, out_sz, scale, interp_method, support_sz, antialiasing, pad_code, is_numpy):
    """the tables of one dim, by the reference's own steps: projected grid, anti-aliasing, field of view, pad shift, weights"""
    scale = float(scale)
    method, support = interp_method, support_sz
    if scale < 1.0 and antialiasing:
        # low-pass by stretching: the kernel is evaluated at scale * distance and multiplied by scale, the window grows
        def method(d, _f=interp_method, _s=scale):
            return _s * _f(_s * d)
        support = support_sz / scale
    if is_numpy:
        eps = _NP_EPS
        grid = numpy.arange(out_sz) / scale + (in_sz - 1) / 2 - (out_sz - 1) / (2 * scale)
        left = numpy.int_(numpy.ceil(grid - support / 2 - eps))
        taps = ceil(support - eps)
        if taps < 1:
            raise ValueError("support_sz {} gives no taps".format(support_sz))
        fov = left[:, None] + numpy.arange(taps)
        shift = -fov[0, 0].item()           # the reference pads by this and moves both coordinates: it changes the float bits
        fov = fov + shift
        grid = grid + shift
        w = method(grid[:, None] - fov)
        total = w.sum(1, keepdims=True)
        total[total == 0] = 1
        w = numpy.asarray(w / total, dtype=numpy.float64)
        left = numpy.asarray(left, dtype=numpy.int64)
    else:
        eps = torch.finfo(torch.float32).eps
        grid = torch.arange(out_sz) / scale + (in_sz - 1) / 2 - (out_sz - 1) / (2 * scale)
        left = (grid - support / 2 - eps).ceil().long()
        taps = ceil(support - eps)
        if taps < 1:
            raise ValueError("support_sz {} gives no taps".format(support_sz))
        fov = left[:, None] + torch.arange(taps)
        shift = -fov[0, 0].item()
        fov = fov + shift
        grid = grid + shift
        w = method(grid[:, None] - fov)
        total = w.sum(1, keepdim=True)
        total[total == 0] = 1
        w = (w / total).to(torch.float32).numpy()
        left = left.numpy()
    if tuple(w.shape) != (out_sz, taps):
        raise ValueError("interp_method returned shape {} for distances of shape {}".format(tuple(w.shape), (out_sz, taps)))
    if left.min() < -(1 << 30) or left.max() > (1 << 30):
        raise ValueError("field of view out of range")
    return AxisTable(in_sz, out_sz, left, w, pad_code)


_TABLES = {}


def _cached_table(*key):
    try:
        hit = _TABLES.get(key)
    except TypeError:                       # an unhashable callable: build every time
        return axis_table(*key)
    if hit is None:
        if len(_TABLES) >= 64:
            _TABLES.pop(next(iter(_TABLES)))
        hit = _TABLES[key] = axis_table(*key)
    return hit


def _plan(in_shape, scale_factors, out_shape, interp_method, support_sz, antialiasing, pad_code, is_numpy):
    """[(dim, AxisTable)] in the order the passes run: ascending scale, stable; dims of scale 1 are skipped"""
    if support_sz is None:
        support_sz = interp_method.support_sz
    order = [d for d in sorted(range(len(in_shape)), key=lambda d: scale_factors[d]) if scale_factors[d] != 1.]
    return [(d, _cached_table(int(in_shape[d]), int(out_shape[d]), scale_factors[d], interp_method, support_sz, bool(antialiasing),
                              pad_code, is_numpy)) for d in order]


# ------------------------------------------------------------------ device passes
_NP_OF = None


def _np_dtype_of(t):
    global _NP_OF
    if _NP_OF is None:
        _NP_OF = {torch.float32: numpy.float32, torch.float64: numpy.float64}
    return _NP_OF[t]


def _launch(x, dim, n_out, acc, out_dtype, tabs, taps, n_src, pad_code):
    """x: contiguous device tensor; one lerf_rr_axis launch along `dim` -> tensor with shape[dim] = n_out"""
    shape = list(x.shape)
    outer = 1
    for s in shape[:dim]:
        outer *= s
    inner = 1
    for s in shape[dim + 1:]:
        inner *= s
    shape[dim] = n_out
    out = torch.empty(shape, dtype=out_dtype, device=x.device)
    if out.numel() == 0:
        return out
    ax = _lib.RrAxis(n_src, n_out, taps, None, None, None, None, pad_code)
    if taps > 0:
        ax.left, ax.w = tabs[0].data_ptr(), tabs[1].data_ptr()
    else:
        ax.row_ptr, ax.idx, ax.w = tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr()
    with _lib.on_device(x):
        _lib.check(_lib.lib().lerf_rr_axis(x.data_ptr(), _lib._dt(x), outer, inner, C.byref(ax), _lib.LERF_F64 if acc == torch.float64 else _lib.LERF_F32,
                                           out.data_ptr(), _lib._dt(out), _lib.current_stream(x.device)), "lerf_rr_axis")
    return out


def _forward_pass(x, dim, tab, acc, out_dtype):
    tabs = tab.device(x.device, _np_dtype_of(acc))
    return _launch(x, dim, tab.n_out, acc, out_dtype, tabs, tab.taps, tab.n_in, tab.pad_code)


def _adjoint_pass(g, dim, tab, acc):
    tabs = tab.device(g.device, _np_dtype_of(acc), adjoint=True)
    return _launch(g, dim, tab.n_in, acc, acc, tabs, 0, tab.n_out, 0)


if torch is not None:
    class _AxisPass(torch.autograd.Function):
        """one axis pass with its adjoint as the backward (the reference's torch resize is differentiable through autograd)"""

        @staticmethod
        def forward(ctx, x, dim, tab, acc):
            ctx.dim, ctx.tab, ctx.acc, ctx.in_dtype = dim, tab, acc, x.dtype
            return _forward_pass(x, dim, tab, acc, acc)

        @staticmethod
        def backward(ctx, g):
            gi = _adjoint_pass(g.contiguous().to(ctx.acc), ctx.dim, ctx.tab, ctx.acc)
            return gi.to(ctx.in_dtype), None, None, None


def _run(x, plan, acc, last_dtype=None):
    """all passes on a device tensor; `last_dtype`: output type of the final pass (the uint8 epilogue), default `acc`"""
    for n, (dim, tab) in enumerate(plan):
        x = x.contiguous()
        out_dtype = last_dtype if (last_dtype is not None and n == len(plan) - 1) else acc
        if x.requires_grad and torch.is_grad_enabled():
            x = _AxisPass.apply(x, dim, tab, acc)
        else:
            x = _forward_pass(x, dim, tab, acc, out_dtype)
    return x


def _numpy_operand(input):
    """numpy array / device-backed array -> device tensor of a dtype the kernels read (uint8, float32, float64)"""
    from .. import lazy
    _lib.require_gpu()
    if isinstance(input, lazy.DeviceArray):
        t = input.t
        if t.dtype not in (torch.uint8, torch.float32, torch.float64):
            t = t.to(torch.float64)
        return t
    a = input
    if a.dtype not in (numpy.uint8, numpy.float32, numpy.float64):
        if a.dtype.kind not in "iubf":
            raise TypeError("resize: unsupported dtype {}".format(a.dtype))
        a = a.astype(numpy.float64)         # the value numpy's product with the float64 weights would see
    return lazy.upload(numpy.ascontiguousarray(a))


def resize(input, scale_factors=None, out_shape=None,
           interp_method=interp_methods.cubic, support_sz=None,
           antialiasing=True, by_convs=False, scale_tolerance=None,
           max_numerator=10, pad_mode='constant'):
    """See the module docstring.  numpy uint8 / float32 / float64 in -> float64 out (float64 tables and sums); torch float32
    (and uint8) in -> float32 out with float32 tables and sums; torch float64 in -> float64 out, the float32 weights
    promoted -- the reference's own dtypes.  `scale_tolerance` and `max_numerator` only concern `by_convs` and are ignored."""
    is_numpy = _is_numpy_like(input)
    if not is_numpy and not (torch is not None and isinstance(input, torch.Tensor)):
        raise TypeError("resize: input must be a numpy array or a torch tensor, not {}".format(type(input).__name__))
    if not callable(interp_method) or (support_sz is None and not hasattr(interp_method, "support_sz")):
        raise ValueError("interp_method must be a callable with a support_sz attribute (or pass support_sz=)")
    pad_code = _lib.pad_mode_code(pad_mode, _lib.NUMPY_PAD_MODES if is_numpy else _lib.TORCH_PAD_MODES)
    scales, out_shape = _scales_and_sizes(input.shape, out_shape, scale_factors, by_convs, is_numpy)
    plan = _plan(input.shape, scales, out_shape, interp_method, support_sz, antialiasing, pad_code, is_numpy)
    if not plan:
        return input                                            # every scale is 1: the reference hands the input back
    if is_numpy:
        from .resize_right2d_numpy import _result
        return _result(_run(_numpy_operand(input), plan, torch.float64), [input])
    if not input.is_cuda:
        raise _lib.LerfError("resize: torch inputs must be on the GPU (there is no CPU path)")
    _lib.require_gpu()
    if input.dtype == torch.float64:
        acc = torch.float64
    elif input.dtype in (torch.float32, torch.uint8):
        acc = torch.float32
    else:
        raise TypeError("resize: unsupported torch dtype {}".format(input.dtype))
    return _run(input, plan, acc)


def resize_to_uint8(input, scale_factors=None, out_shape=None, interp_method=interp_methods.cubic, support_sz=None,
                    antialiasing=True, pad_mode='constant'):
    """`np.round(np.clip(resize(input, ...), 0, 255)).astype(np.uint8)` of a numpy image with the rounding fused into the last
    axis pass: the float64 sums never reach memory.  Same bytes as the three numpy steps."""
    if not _is_numpy_like(input):
        raise TypeError("resize_to_uint8 takes numpy arrays")
    from .resize_right2d_numpy import _result
    pad_code = _lib.pad_mode_code(pad_mode, _lib.NUMPY_PAD_MODES)
    scales, out_shape = _scales_and_sizes(input.shape, out_shape, scale_factors, False, True)
    plan = _plan(input.shape, scales, out_shape, interp_method, support_sz, antialiasing, pad_code, True)
    x = _numpy_operand(input)
    if not plan:
        return _result(x.to(torch.float64).clamp(0, 255).round().to(torch.uint8), [input])
    return _result(_run(x, plan, torch.float64, last_dtype=torch.uint8), [input])
