"""Interpolation kernels of the reference's resize_right/interp_methods.py: `cubic`, `lanczos2`, `lanczos3`, `linear`,
`box`, their 2-D products and the `support_sz` attribute each carries.  Same names, signatures and values; polymorphic over
numpy arrays and torch tensors (the masks take the argument's dtype on the torch side, as there).

Host-side.  `resize_right.resize` fills its per-axis weight tables by calling these (or any user callable with a
`support_sz`), so for numpy float64 arguments they return the reference's values bit for bit: the same operations in the
same order, `absx ** 3` as a power and not a product, and the float32 machine epsilon in the Lanczos quotients.
"""
from math import pi

import numpy

try:
    import torch
except ImportError:          # the numpy side works without it
    torch = None

_EPS32 = float(numpy.finfo(numpy.float32).eps)


def _mask_caster(x):
    """boolean mask -> factor: numpy multiplies booleans as they are, torch casts them to the argument's dtype"""
    if type(x) is numpy.ndarray:
        return lambda m: m
    return lambda m: m.to(x.dtype)


def _sin(x):
    return numpy.sin(x) if type(x) is numpy.ndarray else torch.sin(x)


def _abs(x):
    return numpy.abs(x) if type(x) is numpy.ndarray else torch.abs(x)


def support_sz(sz):
    """decorator: attach the width of the kernel's support, which `resize` reads unless `support_sz=` overrides it"""
    def tag(f):
        f.support_sz = sz
        return f
    return tag


@support_sz(4)
def cubic(x):
    """Keys' cubic convolution kernel, a = -0.5 (:35-43)"""
    as_factor = _mask_caster(x)
    a1 = _abs(x)
    a2 = a1 ** 2
    a3 = a1 ** 3
    near = 1.5 * a3 - 2.5 * a2 + 1.
    far = -0.5 * a3 + 2.5 * a2 - 4. * a1 + 2.
    return near * as_factor(a1 <= 1.) + far * as_factor((1. < a1) & (a1 <= 2.))


def _lanczos(x, a):
    """sinc(x) sinc(x / a) on |x| < a, with the reference's eps in numerator and denominator (:46-57)"""
    as_factor = _mask_caster(x)
    num = _sin(pi * x) * _sin(pi * x / a) + _EPS32
    den = (pi ** 2 * x ** 2 / a) + _EPS32
    return (num / den) * as_factor(abs(x) < a)


@support_sz(4)
def lanczos2(x):
    return _lanczos(x, 2)


@support_sz(6)
def lanczos3(x):
    return _lanczos(x, 3)


@support_sz(2)
def linear(x):
    """the hat function; the half-open masks of the reference (:60-64)"""
    as_factor = _mask_caster(x)
    return (x + 1) * as_factor((-1 <= x) & (x < 0)) + (1 - x) * as_factor((0 <= x) & (x <= 1))


@support_sz(1)
def box(x):
    as_factor = _mask_caster(x)
    return as_factor((-1 <= x) & (x < 0)) + as_factor((0 <= x) & (x <= 1))


@support_sz(4)
def cubic2d(x, y):
    return cubic(x) * cubic(y)


@support_sz(2)
def linear2d(x, y):
    return linear(x) * linear(y)


@support_sz(1)
def box2d(x, y):
    return box(x) * box(y)


@support_sz(4)
def lanczos2d(x, y):
    return lanczos2(x) * lanczos2(y)


@support_sz(6)
def lanczos3d(x, y):
    return lanczos3(x) * lanczos3(y)
