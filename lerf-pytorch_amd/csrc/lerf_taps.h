// The taps of both resamplers in the form the per-tap kernels take them: SrTap for the separable SR geometry (resize_kernel,
// resize_cells_u8_kernel, resize_fixed_kernel and the backward, lerf_resize_bwd.hip), WarpTap for the homographic warp on planar
// operands (Warp2dTorch.get_distance / warp, resize_right2d_torch.py:249-487; warp_kernel, warp_packed_kernel and the backward,
// lerf_warp_bwd.hip), plus the fixed interpolation kernels.  The geometry itself (source_tap: clamps and pad rule; warp_pixel /
// axis_tap: projection, support boundary, distances) is lerf_host_geometry.h's, which lerf_warp_px.h shares.
#pragma once

#include "lerf_kernels.h"

namespace lerf {

// fixed interpolation kernels of resize_right/interp_methods.py:35-70 (the reference's non-learned warps,
// resize_right2d_numpy.py:451-494); evaluated in float64 like the reference, eps = float32 eps
__device__ __forceinline__ double fixed_kernel_1d(int kind, double x) {
#pragma clang fp contract(off)
    const double pi = 3.141592653589793;
    const double eps = (double)kEps32;
    if (kind == LERF_KIND_CUBIC) {                                        // :35-43
        const double a = fabs(x), a2 = a * a, a3 = a * a * a;
        return (1.5 * a3 - 2.5 * a2 + 1.0) * (a <= 1.0 ? 1.0 : 0.0) +
               (-0.5 * a3 + 2.5 * a2 - 4.0 * a + 2.0) * ((1.0 < a && a <= 2.0) ? 1.0 : 0.0);
    }
    if (kind == LERF_KIND_LANCZOS2)                                       // :46-50
        return ((sin(pi * x) * sin(pi * x / 2) + eps) / ((pi * pi * (x * x) / 2) + eps)) * (fabs(x) < 2.0 ? 1.0 : 0.0);
    if (kind == LERF_KIND_LANCZOS3)                                       // :53-57
        return ((sin(pi * x) * sin(pi * x / 3) + eps) / ((pi * pi * (x * x) / 3) + eps)) * (fabs(x) < 3.0 ? 1.0 : 0.0);
    if (kind == LERF_KIND_BILINEAR)                                       // :60-64
        return (x + 1.0) * ((-1.0 <= x && x < 0.0) ? 1.0 : 0.0) + (1.0 - x) * ((0.0 <= x && x <= 1.0) ? 1.0 : 0.0);
    return ((-1.0 <= x && x < 0.0) ? 1.0 : 0.0) + ((0.0 <= x && x <= 1.0) ? 1.0 : 0.0);   // box :67-70
}

// d/dx of fixed_kernel_1d as autograd derives it for the forms of interp_methods.py (the remap's map gradient, lerf_warp_bwd_kernels.h):
// the support masks are constants, |x|' = sign(x) with sign(0) = 0, the hat's kink at 0 belongs to its right branch (-1), the
// Lanczos quotient (sin sin + eps) / (pi^2 x^2 / a + eps) is differentiated with its eps, box has no gradient.
__device__ __forceinline__ double fixed_kernel_1d_deriv(int kind, double x) {
#pragma clang fp contract(off)
    const double pi = 3.141592653589793;
    const double eps = (double)kEps32;
    if (kind == LERF_KIND_CUBIC) {
        const double a = fabs(x), sg = x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0);
        return sg * ((4.5 * (a * a) - 5.0 * a) * (a <= 1.0 ? 1.0 : 0.0) +
                     (-1.5 * (a * a) + 5.0 * a - 4.0) * ((1.0 < a && a <= 2.0) ? 1.0 : 0.0));
    }
    if (kind == LERF_KIND_LANCZOS2 || kind == LERF_KIND_LANCZOS3) {
        const double a = kind == LERF_KIND_LANCZOS2 ? 2.0 : 3.0;
        const double s1 = sin(pi * x), c1 = cos(pi * x), s2 = sin(pi * x / a), c2 = cos(pi * x / a);
        const double num = s1 * s2 + eps, den = (pi * pi * (x * x) / a) + eps;
        const double dnum = pi * c1 * s2 + (pi / a) * (s1 * c2), dden = 2.0 * (pi * pi) * x / a;
        return (dnum / den - num * dden / (den * den)) * (fabs(x) < a ? 1.0 : 0.0);
    }
    if (kind == LERF_KIND_BILINEAR)
        return ((-1.0 <= x && x < 0.0) ? 1.0 : 0.0) - ((0.0 <= x && x <= 1.0) ? 1.0 : 0.0);
    return 0.0;                                                             // box
}

// tap (a, b) of SR output pixel (i, j) -- column offset a, row offset b -- from its support's left boundaries lr = left_r[i],
// lc = left_c[j]
struct SrTap {
    int rcl, ccl;       // clamped source pixel: where the replicate-padded hyper-parameter maps are read (:172-174)
    int rs, cs;         // image pixel under the image's pad rule (:208)
    bool z;             // the image value is the constant pad (0)
    bool inside;        // the tap lies inside the frame
};

__device__ __forceinline__ SrTap sr_tap(int lr, int lc, int a, int b, int H, int W, int pad_mode) {
    const SourceTap r = source_tap(lr + b, H, pad_mode), c = source_tap(lc + a, W, pad_mode);
    return {r.cl, c.cl, r.s, c.s, r.z || c.z, r.inside && c.inside};
}

// output pixel (i, j) of the launch's rectangle
__device__ __forceinline__ WarpPixel warp_pixel(const WarpGeo& g, int i, int j, int H, int W) {
    return warp_pixel(g.minv, g.S, g.pad_r_lo, g.pad_c_lo, i + g.oy0, j + g.ox0, H, W);
}

template <typename A>
struct WarpTap {
    double dxd, dyd;    // float64 distances (row, column)
    A dx, dy;           // the same in the arithmetic type of the weights
    int rcl, ccl;       // clamped source pixel: where the replicate-padded hyper-parameter maps are read
    int rs, cs;         // image pixel under the image's pad rule
    bool zr, zc;        // the image value is the constant pad (0)
    bool inside;        // the tap lies inside the frame
};

// tap (a, b) of the patch: column offset a, row offset b
template <typename A>
__device__ __forceinline__ WarpTap<A> warp_tap(const WarpGeo& g, const WarpPixel& p, int a, int b, int H, int W) {
    const AxisTap r = axis_tap(p.gr, p.lr, b, H, g.pad_r_lo, g.pad_mode), c = axis_tap(p.gc, p.lc, a, W, g.pad_c_lo, g.pad_mode);
    return {r.d, c.d, (A)r.d, (A)c.d, r.cl, c.cl, r.s, c.s, r.z, c.z, r.inside && c.inside};
}

}  // namespace lerf
