// Per-output-pixel geometry of the homographic warp on planar operands (Warp2dTorch.get_distance / warp,
// resize_right2d_torch.py:249-487, float64 like the reference's distances): the projection, the support's left
// boundary, the pad shift, the taps of the S x S patch and the fixed interpolation kernels.  Shared by the forward
// (warp_kernel, lerf_kernels.hip) and the backward (lerf_warp_bwd.hip) so that the two enumerate the same taps with the
// same float64 distances and weights.
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

struct WarpPixel {
    double gr, gc;      // projected point, clipped to [0, in] and shifted by the low pads (padded coordinates)
    int lr, lc;         // left boundary of the support in padded coordinates
};

// output pixel (i, j) of the launch's rectangle
__device__ __forceinline__ WarpPixel warp_pixel(const WarpGeo& g, int i, int j, int H, int W) {
    WarpPixel p;
    project_point(g.minv, i + g.oy0, j + g.ox0, H, W, &p.gr, &p.gc);
    p.lr = left_boundary(p.gr, g.S) + g.pad_r_lo;
    p.lc = left_boundary(p.gc, g.S) + g.pad_c_lo;
    p.gr += (double)g.pad_r_lo;      // calc_pad_sz shifts grid and field of view (:366-367)
    p.gc += (double)g.pad_c_lo;
    return p;
}

template <typename A>
struct WarpTap {
    double dxd, dyd;    // float64 distances (row, column)
    A dx, dy;           // the same in the arithmetic type of the weights
    int rcl, ccl;       // clamped source pixel: where the replicate-padded hyper-parameter maps are read
    int rs, cs;         // image pixel under the image's pad rule
    bool zr, zc;        // the image value is the constant pad (0)
};

// tap (a, b) of the patch: column offset a, row offset b
template <typename A>
__device__ __forceinline__ WarpTap<A> warp_tap(const WarpGeo& g, const WarpPixel& p, int a, int b, int H, int W) {
    WarpTap<A> t;
    // field of view clipped to [0, in-1] while indexing the PADDED arrays (:396-398)
    const int pr = clampi(p.lr + b, 0, H - 1), pc = clampi(p.lc + a, 0, W - 1);
    t.dxd = p.gr - (double)pr;
    t.dyd = p.gc - (double)pc;
    t.dx = (A)t.dxd;
    t.dy = (A)t.dyd;
    const int sr = pr - g.pad_r_lo, sc = pc - g.pad_c_lo;      // unpadded source coordinates
    t.rcl = clampi(sr, 0, H - 1);
    t.ccl = clampi(sc, 0, W - 1);
    t.rs = pad_index(sr, H, g.pad_mode, &t.zr);                // image pad rule (:560)
    t.cs = pad_index(sc, W, g.pad_mode, &t.zc);
    return t;
}

}  // namespace lerf
