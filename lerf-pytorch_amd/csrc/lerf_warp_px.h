// The S = 2 RGB homographic warp on the PACKED stage outputs (hq0 | hq1 << 8 | hq2 << 16 | feat << 24 per pixel-channel) and
// the float64 tie guard of every uint8 warp.  WarpPx2 is the per-pixel tap geometry of warp_pixel / axis_tap
// (lerf_host_geometry.h) evaluated once for the two rows and two columns of taps; warp_px_value_u8 is the float32
// production arithmetic (max_sigma <= s3::kNoShiftMaxSigma), warp_px_value the exact float32 parameter formation.  Shared by
// warp_packed_px_kernel (taps from the packed maps in HBM / L2) and the tile-fused warp (taps from the tile's packed dwords in
// LDS, lerf_fused_impl.h): the same instructions in both, so fused == unfused bit for bit.  warp_px_geometry takes the pixel's
// point as a WarpPixel, so the remap (lerf_remap.hip: the point is read from a coordinate map) shares all of it as well.
#pragma once

#include "lerf_kernels.h"
#include "lerf_stage3.h"

namespace lerf {

// amplified-linear 1-D factor (resize_right2d_numpy.py:233-241), cls = class of
// the float64 distance: 0 outside [-1,1], 1 for [-1,0), 2 for [0,1]
template <typename A>
__device__ __forceinline__ A lin_factor(A alpha, A x, int cls) {
    A f = cls == 1 ? alpha * x + (A)1 : (cls == 2 ? (A)1 - alpha * x : (A)0);
    return f < (A)0 ? (A)0 : f;
}
template <typename A>
__device__ __forceinline__ int dist_class(A x) {
    return (x >= (A)-1 && x < (A)0) ? 1 : ((x >= (A)0 && x <= (A)1) ? 2 : 0);
}

// Tie guard of the uint8 warps: an output within kTieEps of a half-integer is resolved in float64 (s3::resolve_u8: the
// reference's float64 forms, and its whole dtype chain where that is still undecided), like the SR kernels do, on the taps of
// pixel p rebuilt with axis_tap; `tap(r, c)` returns (k0 | k1<<8 | k2<<16 | val<<24) of the clamped source pixel.
template <int KIND, int S, typename F>
__device__ __forceinline__ uint8_t warp_resolve_u8(int H, int W, const WarpGeo& g, const WarpPixel& p, float max_sigma, F tap) {
    uint32_t dd[S * S];
    double dx[S], dy[S];
#pragma unroll
    for (int k = 0; k < S; ++k) {
        dx[k] = axis_tap(p.gr, p.lr, k, H, g.pad_r_lo, g.pad_mode).d;
        dy[k] = axis_tap(p.gc, p.lc, k, W, g.pad_c_lo, g.pad_mode).d;
    }
#pragma unroll
    for (int a = 0; a < S; ++a)
#pragma unroll
        for (int b = 0; b < S; ++b) {
            const AxisTap r = axis_tap(p.gr, p.lr, b, H, g.pad_r_lo, g.pad_mode), c = axis_tap(p.gc, p.lc, a, W, g.pad_c_lo, g.pad_mode);
            const uint32_t d = tap(r.cl, c.cl);
            dd[a * S + b] = (r.inside && c.inside) ? d : (d & 0x00FFFFFFu);      // zero image outside the frame
        }
    return s3::resolve_u8<KIND == LERF_KIND_GAUSS, S>(dd, dx, dy, max_sigma);
}

template <int KIND, typename F>
__device__ __forceinline__ bool warp_tie_guard(float res, int S, int H, int W, const WarpGeo& g, const WarpPixel& p, float max_sigma,
                                               F tap, uint8_t* dst) {
    if (!(KIND == LERF_KIND_GAUSS || KIND == LERF_KIND_LINEAR) || !s3::near_tie(res)) return false;
    if (S == 2) *dst = warp_resolve_u8<KIND, 2>(H, W, g, p, max_sigma, tap);
    else if (S == 4) *dst = warp_resolve_u8<KIND, 4>(H, W, g, p, max_sigma, tap);
    else return false;
    return true;
}

struct WarpPx2 {
    WarpPixel p;               // projected position and first tap (padded coordinates)
    float dx[2], dy[2];        // distances to the two rows / columns of taps
    int cx[2], cy[2];          // their classes for the amplified-linear kernel
    int rrow[2], rcol[2];      // the taps' source rows / columns, clamped into the frame (where the hyper-parameters are read)
    bool in_r[2], in_c[2];     // the tap lies inside the frame (the image is zero outside)
};

// ... of a pixel whose point is known (projected: the overload below; read from a coordinate map: lerf_remap.hip)
__device__ __forceinline__ WarpPx2 warp_px_geometry(const WarpGeo& g, const WarpPixel& p, int H, int W) {
    WarpPx2 G;
    G.p = p;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const AxisTap r = axis_tap(G.p.gr, G.p.lr, k, H, g.pad_r_lo, g.pad_mode);
        G.dx[k] = (float)r.d;
        G.cx[k] = dist_class(r.d);
        G.rrow[k] = r.cl;
        G.in_r[k] = r.inside;
        const AxisTap c = axis_tap(G.p.gc, G.p.lc, k, W, g.pad_c_lo, g.pad_mode);
        G.dy[k] = (float)c.d;
        G.cy[k] = dist_class(c.d);
        G.rcol[k] = c.cl;
        G.in_c[k] = c.inside;
    }
    return G;
}

__device__ __forceinline__ WarpPx2 warp_px_geometry(const WarpGeo& g, int i, int j, int H, int W) {
    return warp_px_geometry(g, warp_pixel(g.minv, 2, g.pad_r_lo, g.pad_c_lo, i + g.oy0, j + g.ox0, H, W), H, W);
}

// channel value of the pixel in production arithmetic; tap(r, c) -> packed dword of the clamped source pixel (this channel).
// Returns true when the byte was written by the tie guard (float64), else *res holds the float32 value to be stored.
template <int KIND, typename Tap>
__device__ __forceinline__ bool warp_px_value_u8(const WarpPx2& G, const WarpGeo& g, int H, int W, float max_sigma, const float (&dxs)[2],
                                                 const float (&dys)[2], Tap tap, uint8_t* dst, float* res_out) {
    constexpr int S = 2;
    const float ms255 = max_sigma * (1.0f / 255.0f);
    uint32_t d[S * S];
#pragma unroll
    for (int a = 0; a < S; ++a)
#pragma unroll
        for (int b = 0; b < S; ++b) d[a * S + b] = tap(G.rrow[b], G.rcol[a]);
    float e[S * S], v[S * S];
#pragma unroll
    for (int a = 0; a < S; ++a)
#pragma unroll
        for (int b = 0; b < S; ++b) {
            const uint32_t q = d[a * S + b];
            if (KIND == LERF_KIND_GAUSS) {
                e[a * S + b] = s3::gauss_form_u8((float)(q & 0xFFu), (float)((q >> 8) & 0xFFu), (float)((q >> 16) & 0xFFu), dxs[b], dys[a]);
            } else {
                const float alpha = s3::lin_alpha_u8((float)(q & 0xFFu), ms255);
                e[a * S + b] = s3::lin_factor(alpha, G.dx[b], G.cx[b]) * s3::lin_factor(alpha, G.dy[a], G.cy[a]);
            }
            v[a * S + b] = (G.in_r[b] && G.in_c[a]) ? (float)(q >> 24) : 0.0f;
        }
    float res = s3::finish<KIND == LERF_KIND_GAUSS, S * S, true, true, false>(e, v);
    if (KIND == LERF_KIND_GAUSS) {
        // every weight underflows in the reference's float64 (exp(-e/2) = 0 for e/2 > 745.2): its 0/0 = NaN; in the
        // pre-scaled units e' = 0.5 log2(e) e that is e' > 1075.1
        const float emin = fminf(fminf(e[0], e[1]), fminf(e[2], e[3]));
        if (emin > 1075.1f) res = __builtin_nanf("");
    }
    *res_out = res;
    return warp_tie_guard<KIND>(res, S, H, W, g, G.p, max_sigma, tap, dst);
}

// channel value of the pixel with the exact float32 parameter formation (float outputs, and uint8 outputs above
// s3::kNoShiftMaxSigma); d[a * 2 + b] = packed dword of tap (a, b), this channel.  NaN where every weight vanishes.
template <int KIND>
__device__ __forceinline__ float warp_px_value(const WarpPx2& G, float max_sigma, const uint32_t (&d)[4]) {
    constexpr int S = 2;
    float e[S * S], emin = 0.0f, num = 0.0f, den = 0.0f;
#pragma unroll
    for (int a = 0; a < S; ++a)
#pragma unroll
        for (int b = 0; b < S; ++b) {
            const uint32_t q = d[a * S + b];
            if (KIND == LERF_KIND_GAUSS) {
                e[a * S + b] = s3::gauss_form(s3::u8_over_255((float)(q & 0xFFu)), s3::u8_over_255((float)((q >> 8) & 0xFFu)),
                                              s3::u8_over_255((float)((q >> 16) & 0xFFu)), max_sigma, G.dx[b], G.dy[a]);
                emin = (a == 0 && b == 0) ? e[0] : fminf(e[a * S + b], emin);
            } else {
                const float alpha = s3::lin_alpha_of(s3::u8_over_255((float)(q & 0xFFu)), max_sigma);
                e[a * S + b] = s3::lin_factor(alpha, G.dx[b], G.cx[b]) * s3::lin_factor(alpha, G.dy[a], G.cy[a]);
            }
        }
#pragma unroll
    for (int a = 0; a < S; ++a)
#pragma unroll
        for (int b = 0; b < S; ++b) {
            const float w = KIND == LERF_KIND_GAUSS ? s3::gauss_weight(e[a * S + b], emin) : e[a * S + b];
            const float val = (G.in_r[b] && G.in_c[a]) ? (float)(d[a * S + b] >> 24) : 0.0f;
            num += w * val;
            den += w;
        }
    float res = num / den;
    if (KIND == LERF_KIND_GAUSS && emin * 0.5f > 745.2f) res = __builtin_nanf("");
    return res;
}

}  // namespace lerf
