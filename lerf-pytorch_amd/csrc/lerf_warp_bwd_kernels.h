// The backward of the float warps from "the pixel's point is known" onward, shared by the homographic backward (lerf_warp_bwd.hip:
// the point is projected, warp_pixel) and the remap backward (lerf_remap_bwd.hip: the point is read from a coordinate map,
// remap_pixel) -- the split lerf_warp_kernels.h makes for the forward.  warp_bwd_body is the block's window reduction, the two
// tap loops, `put` and the LDS / global flush; the formulas are at the top of lerf_warp_bwd.hip.
//
// COORD (compile time) adds the gradient with respect to the POINT, which only a map has as a tensor.  The point enters through
// the distances alone (d_row,k = clip(row) + pad - p_k), the tap set, the pads and the amplified-linear classes are piecewise
// constant, so per pixel
//   d loss / d row = sum_t (d loss / d w_t) (d w_t / d dx_t),   d loss / d w_t = G (v_t - out) / W   (G v_t where warp() does not
//                                                                                                    normalise: fixed kinds, S = 1)
//   gauss:  d w / d dx = -1/2 w 2 sx (tx - rho ty),  d w / d dy = -1/2 w 2 sy (ty - rho tx)
//   linear: d l / d x = alpha [class 1] - alpha [class 2] where l >= 0 (x = 0 is class 2)
//   fixed:  k'(dx) k(dy), k(dx) k'(dy)  (fixed_kernel_1d_deriv, lerf_taps.h);  nearest: identically 0 (box has no gradient)
// summed in float64 (the map is a float64 quantity in the reference's geometry; nothing is rounded to float32 on the way).  The
// clip's own derivative (pass / block) is the caller's: it knows the unclipped entry.  Off, the body is the homographic kernel's
// arithmetic unchanged.
#pragma once

#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "lerf_warp_px.h"
#include "lerf_taps.h"

namespace lerf {
namespace warp_bwd {

// One workgroup = a 16 x 16 block of outputs of one plane.  A homography's footprint is not a rectangle spanned by the
// block's corners (the projection can cross the horizon), and a map's is whatever the map says, so the block reduces the clamped
// rows and columns its own taps touch (LDS min / max) and takes that as its window.  When the window fits, the gradient maps are
// summed in LDS (ds_add_f32) and flushed with one global atomic per non-zero window element; otherwise every tap adds to global
// memory.
constexpr int WB_ROWS = 16, WB_COLS = 16, WB_NT = WB_ROWS * WB_COLS;
constexpr int WB_LDS = 8192;         // floats of window, shared by the kind's maps (32 KiB)

template <int KIND>
struct Kind {
    static constexpr bool hyper = KIND == LERF_KIND_GAUSS || KIND == LERF_KIND_LINEAR;
    static constexpr int maps = KIND == LERF_KIND_GAUSS ? 4 : (KIND == LERF_KIND_LINEAR ? 2 : 1);
};

// one tap's weight and what its gradient needs, float64
struct TapW {
    double w, v;
    double rho, tx, ty;      // gauss
    double sx, sy;           // gauss: the scales behind tx, ty
    double lx, ly;           // linear: the unclamped factors (alpha = rho)
};

template <int KIND>
__device__ __forceinline__ TapW tap_weight(const float* __restrict__ feat, const float* __restrict__ h0, const float* __restrict__ h1,
                                           const float* __restrict__ h2, int64_t plane, int W, const WarpTap<double>& t, float ms) {
    TapW r;
    r.v = (t.zr || t.zc) ? 0.0 : (double)feat[plane + (int64_t)t.rs * W + t.cs];
    const int64_t ho = plane + (int64_t)t.rcl * W + t.ccl;
    if (KIND == LERF_KIND_GAUSS) {
        r.rho = (double)(h0[ho] * 2.0f - 1.0f);
        r.sx = (double)(h1[ho] * ms);
        r.sy = (double)(h2[ho] * ms);
        r.tx = r.sx * t.dx;
        r.ty = r.sy * t.dy;
        const double e = r.tx * r.tx - 2.0 * r.rho * (r.tx * r.ty) + r.ty * r.ty;
        r.w = exp(-0.5 * e);
    } else if (KIND == LERF_KIND_LINEAR) {
        r.rho = (double)(ms * (h0[ho] * 2.0f - 1.0f));
        const int cx = dist_class(t.dxd), cy = dist_class(t.dyd);
        r.lx = cx == 1 ? r.rho * t.dx + 1.0 : (cx == 2 ? 1.0 - r.rho * t.dx : 0.0);
        r.ly = cy == 1 ? r.rho * t.dy + 1.0 : (cy == 2 ? 1.0 - r.rho * t.dy : 0.0);
        r.w = (r.lx < 0.0 ? 0.0 : r.lx) * (r.ly < 0.0 ? 0.0 : r.ly);
    } else if (KIND == LERF_KIND_NEAREST) {
        r.w = (dist_class(t.dxd) != 0 && dist_class(t.dyd) != 0) ? 1.0 : 0.0;     // box2d
    } else {
        r.w = fixed_kernel_1d(KIND, t.dxd) * fixed_kernel_1d(KIND, t.dyd);         // cubic2d / linear2d / lanczos
    }
    return r;
}

// d l / d alpha of the linear factor behind clamp(l, 0): x [-1 <= x < 0] - x [0 <= x <= 1] where l >= 0
__device__ __forceinline__ double dlin(double l, double x, int cls) {
    return l >= 0.0 ? (cls == 1 ? x : (cls == 2 ? -x : 0.0)) : 0.0;
}

// d l / d x of the same factor: alpha [-1 <= x < 0] - alpha [0 <= x <= 1] where l >= 0
__device__ __forceinline__ double dlin_dx(double l, double alpha, int cls) {
    return l >= 0.0 ? (cls == 1 ? alpha : (cls == 2 ? -alpha : 0.0)) : 0.0;
}

// d w / d dx and d w / d dy of tap t (the tap set and the class masks held fixed)
template <int KIND>
__device__ __forceinline__ void tap_weight_dpoint(const WarpTap<double>& t, const TapW& tw, double* dwx, double* dwy) {
    if (KIND == LERF_KIND_GAUSS) {
        *dwx = -0.5 * tw.w * (2.0 * tw.sx * (tw.tx - tw.rho * tw.ty));
        *dwy = -0.5 * tw.w * (2.0 * tw.sy * (tw.ty - tw.rho * tw.tx));
    } else if (KIND == LERF_KIND_LINEAR) {
        const double cx = tw.lx < 0.0 ? 0.0 : tw.lx, cy = tw.ly < 0.0 ? 0.0 : tw.ly;
        *dwx = dlin_dx(tw.lx, tw.rho, dist_class(t.dxd)) * cy;
        *dwy = cx * dlin_dx(tw.ly, tw.rho, dist_class(t.dyd));
    } else if (KIND == LERF_KIND_NEAREST) {
        *dwx = 0.0;
        *dwy = 0.0;
    } else {
        *dwx = fixed_kernel_1d_deriv(KIND, t.dxd) * fixed_kernel_1d(KIND, t.dyd);
        *dwy = fixed_kernel_1d(KIND, t.dxd) * fixed_kernel_1d_deriv(KIND, t.dyd);
    }
}

// The block's work once every thread knows its pixel: `act` = this thread has an output pixel (i, j) of plane n with point px.
// Called by all WB_NT threads of the block (it synchronises).  COORD: *gdx, *gdy receive d loss / d (row distance) and
// d loss / d (column distance) of an active pixel (0 otherwise, and 0 for the nearest kind).
template <int KIND, bool COORD>
__device__ __forceinline__ void warp_bwd_body(const float* __restrict__ feat, const float* __restrict__ h0, const float* __restrict__ h1,
                                              const float* __restrict__ h2, int H, int W, const WarpGeo& g, float ms,
                                              const double* __restrict__ gout, float* __restrict__ gfeat, float* __restrict__ gh0,
                                              float* __restrict__ gh1, float* __restrict__ gh2, const WarpPixel& px, bool act, int i,
                                              int j, int n, double* gdx, double* gdy) {
    constexpr int NM = Kind<KIND>::maps, CAP = WB_LDS / NM;
    __shared__ float win[WB_LDS];
    __shared__ int rng[4];           // window: first row, last row, first column, last column
    const int tid = threadIdx.x;
    const int S = g.S;
    const int64_t plane = (int64_t)n * H * W;
    if (COORD) { *gdx = 0.0; *gdy = 0.0; }
    if (tid == 0) { rng[0] = INT_MAX; rng[1] = -1; rng[2] = INT_MAX; rng[3] = -1; }
    __syncthreads();
    if (act) {
        // the clamped tap rows (columns) are non-decreasing in the tap index: the first and the last tap bound them
        const WarpTap<double> t0 = warp_tap<double>(g, px, 0, 0, H, W), t1 = warp_tap<double>(g, px, S - 1, S - 1, H, W);
        atomicMin(&rng[0], t0.rcl);
        atomicMax(&rng[1], t1.rcl);
        atomicMin(&rng[2], t0.ccl);
        atomicMax(&rng[3], t1.ccl);
    }
    __syncthreads();
    const int wr0 = rng[0], wc0 = rng[2];
    if (rng[1] < 0) return;          // no output pixel in this block (uniform across the block)
    const int wh = rng[1] - wr0 + 1, ww = rng[3] - wc0 + 1;
    const bool lds = (int64_t)wh * ww <= CAP;
    float* const dst[4] = {gfeat, gh0, gh1, gh2};
    if (lds) {
        for (int k = tid; k < wh * ww; k += WB_NT)
#pragma unroll
            for (int m = 0; m < NM; ++m) win[m * CAP + k] = 0.0f;
        __syncthreads();
    }
    auto put = [&](int m, int r, int c, float v) {
        if (!dst[m]) return;
        const int kr = r - wr0, kc = c - wc0;
        if (lds && kr >= 0 && kr < wh && kc >= 0 && kc < ww) atomicAdd(&win[m * CAP + kr * ww + kc], v);
        else if (v != 0.0f) atomicAdd(dst[m] + plane + (int64_t)r * W + c, v);
    };
    if (act) {
        double Wsum = 0.0, num = 0.0;
        for (int a = 0; a < S; ++a)
            for (int b = 0; b < S; ++b) {
                const WarpTap<double> t = warp_tap<double>(g, px, a, b, H, W);
                const TapW tw = tap_weight<KIND>(feat, h0, h1, h2, plane, W, t, ms);
                num += tw.w * tw.v;
                Wsum += tw.w;
            }
        const bool norm = Kind<KIND>::hyper || S != 1;
        const double out = num / Wsum;
        const double G = gout[((int64_t)n * g.oH + i) * g.oW + j];
        const double gn = norm ? G / Wsum : G;
        double ax = 0.0, ay = 0.0;
        for (int a = 0; a < S; ++a)
            for (int b = 0; b < S; ++b) {
                const WarpTap<double> t = warp_tap<double>(g, px, a, b, H, W);
                const TapW tw = tap_weight<KIND>(feat, h0, h1, h2, plane, W, t, ms);
                if (!(t.zr || t.zc)) put(0, t.rs, t.cs, (float)(gn * tw.w));
                if (KIND == LERF_KIND_GAUSS) {
                    const double c = G * (tw.v - out) / Wsum * (-0.5 * tw.w);     // d loss / d e_t
                    put(1, t.rcl, t.ccl, (float)(c * (-2.0 * tw.tx * tw.ty)) * 2.0f);
                    put(2, t.rcl, t.ccl, (float)(c * (2.0 * t.dx * (tw.tx - tw.rho * tw.ty))) * ms);
                    put(3, t.rcl, t.ccl, (float)(c * (2.0 * t.dy * (tw.ty - tw.rho * tw.tx))) * ms);
                } else if (KIND == LERF_KIND_LINEAR) {
                    const double gw = G * (tw.v - out) / Wsum;                      // d loss / d w_t
                    const double cx = tw.lx < 0.0 ? 0.0 : tw.lx, cy = tw.ly < 0.0 ? 0.0 : tw.ly;
                    const double da = dlin(tw.lx, t.dx, dist_class(t.dxd)) * cy + cx * dlin(tw.ly, t.dy, dist_class(t.dyd));
                    put(1, t.rcl, t.ccl, (float)(gw * da) * ms * 2.0f);
                }
                if (COORD && KIND != LERF_KIND_NEAREST) {
                    const double gw = norm ? G * (tw.v - out) / Wsum : G * tw.v;   // d loss / d w_t
                    double dwx, dwy;
                    tap_weight_dpoint<KIND>(t, tw, &dwx, &dwy);
                    ax += gw * dwx;
                    ay += gw * dwy;
                }
            }
        if (COORD) { *gdx = ax; *gdy = ay; }
    }
    if (lds) {
        __syncthreads();
        for (int k = tid; k < wh * ww; k += WB_NT) {
            const int64_t pos = plane + (int64_t)(wr0 + k / ww) * W + wc0 + k % ww;
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                const float v = win[m * CAP + k];
                if (dst[m] && v != 0.0f) atomicAdd(dst[m] + pos, v);
            }
        }
    }
}

}  // namespace warp_bwd
}  // namespace lerf
