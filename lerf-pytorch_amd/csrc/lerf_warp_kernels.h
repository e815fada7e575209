// The bodies of the three stage-3 warp kernels FROM THE POINT ON: everything an output pixel does once its WarpPixel is known.
// The homographic kernels (lerf_kernels.hip: the point is projected through the inverse matrix, warp_pixel) and the remap kernels
// (lerf_remap.hip: the point is read from a dense coordinate map, remap_pixel) are thin shells around these bodies -- the same
// instructions in both families, so the remap of a homography's map equals the warp bit for bit and the two cannot drift (the
// argument lerf_warp_px.h makes for the tile-fused warp against the unfused one).
#pragma once

#include "lerf_kernels.h"
#include "lerf_stage3.h"
#include "lerf_warp_px.h"
#include "lerf_taps.h"

namespace lerf {

// ---------------------------------------------------------------------------
// stage 3 building blocks
// ---------------------------------------------------------------------------
template <typename T> struct Loader;
template <> struct Loader<uint8_t> {
    // hyper numerators: h = float32(u8) / 255 exactly as eval_lut_sr.py:623-628
    static __device__ __forceinline__ float hyper(const uint8_t* p) { return s3::u8_over_255((float)(*p)); }
    static __device__ __forceinline__ float pixel(const uint8_t* p) { return (float)(*p); }
};
template <> struct Loader<float> {
    static __device__ __forceinline__ float hyper(const float* p) { return *p; }
    static __device__ __forceinline__ float pixel(const float* p) { return *p; }
};

// the reference's float32 Gaussian parameters of the tap at offset o of the hyper-parameter maps
template <typename TH>
__device__ __forceinline__ s3::GaussParams gauss_params(const TH* h0, const TH* h1, const TH* h2, int64_t o, float max_sigma) {
    return s3::gauss_params_of(Loader<TH>::hyper(h0 + o), Loader<TH>::hyper(h1 + o), Loader<TH>::hyper(h2 + o), max_sigma);
}

template <typename T> struct Storer;
template <> struct Storer<uint8_t> {
    // clip(np.round(x), 0, 255).astype(uint8)  (eval_lut_sr.py:663-665); NaN -> 0
    template <typename A> static __device__ __forceinline__ void put(uint8_t* p, A v) {
        if (sizeof(A) == 8) *p = s3::to_u8_d((double)v);      // float64 arithmetic: rounded once, from the double
        else *p = s3::to_u8((float)v);
    }
};
template <> struct Storer<float> {
    template <typename A> static __device__ __forceinline__ void put(float* p, A v) { *p = (float)v; }
};
template <> struct Storer<double> {
    template <typename A> static __device__ __forceinline__ void put(double* p, A v) { *p = (double)v; }
};

// what a pixel without a source position holds (every weight vanished; a NaN entry of a coordinate map): the reference's
// 0/0 = NaN in float outputs, 0 in uint8 outputs
template <typename TO>
__device__ __forceinline__ void store_no_value(TO* dst) {
    if constexpr (sizeof(TO) == 1) *dst = 0;
    else *dst = (TO)__builtin_nanf("");
}

// ---------------------------------------------------------------------------
// A7/A8 on planar / strided operands: channel c of the pixel with point px -> *dst
// ---------------------------------------------------------------------------
template <typename TI, typename TH, typename TO, typename A, int KIND>
__device__ __forceinline__ void warp_body(const TI* __restrict__ feat, int64_t fy, int64_t fx, int64_t fc,
                                          const TH* __restrict__ h0, const TH* __restrict__ h1, const TH* __restrict__ h2,
                                          int64_t hy, int64_t hx, int64_t hc, int H, int W, const WarpGeo& g, const WarpPixel& px,
                                          int c, A max_sigma, TO* __restrict__ dst) {
    const int S = g.S;
    A emin = 0, num = 0, den = 0;
    for (int pass = (KIND == LERF_KIND_GAUSS ? 0 : 1); pass < 2; ++pass) {
        for (int a = 0; a < S; ++a)
            for (int b = 0; b < S; ++b) {
                const WarpTap<A> tp = warp_tap<A>(g, px, a, b, H, W);
                const double dxd = tp.dxd, dyd = tp.dyd;
                const A dx = tp.dx, dy = tp.dy;
                const int rs = tp.rs, cs = tp.cs;
                const bool zr = tp.zr, zc = tp.zc;
                int64_t ho = tp.rcl * hy + tp.ccl * hx + c * hc;
                A w;
                if (KIND == LERF_KIND_GAUSS) {
                    const s3::GaussParams p = gauss_params(h0, h1, h2, ho, (float)max_sigma);
                    A rho = (A)p.rho, sx = (A)p.sx, sy = (A)p.sy;
                    A tx = sx * dx, ty = sy * dy;
                    A e = tx * tx - (A)2 * rho * (tx * ty) + ty * ty;
                    if (pass == 0) {
                        emin = sizeof(A) == 8 ? (A)0 : ((a == 0 && b == 0) ? e : (e < emin ? e : emin));   // float64: unshifted, as TapAcc
                        continue;
                    }
                    w = sizeof(A) == 4 ? (A)__expf((float)((A)-0.5 * (e - emin))) : (A)exp((double)((A)-0.5 * (e - emin)));
                } else if (KIND == LERF_KIND_LINEAR) {
                    A alpha = (A)s3::lin_alpha_ref(Loader<TH>::hyper(h0 + ho), (float)max_sigma);
                    // class decisions on the float64 distances
                    w = lin_factor<A>(alpha, dx, dist_class(dxd)) * lin_factor<A>(alpha, dy, dist_class(dyd));
                } else if (KIND == LERF_KIND_NEAREST) {
                    w = (dist_class(dxd) != 0 && dist_class(dyd) != 0) ? (A)1 : (A)0;     // box2d
                } else {
                    w = (A)(fixed_kernel_1d(KIND, dxd) * fixed_kernel_1d(KIND, dyd));     // cubic2d / linear2d / lanczos
                }
                A val = (zr || zc) ? (A)0 : (A)Loader<TI>::pixel(feat + rs * fy + cs * fx + c * fc);
                num += w * val;
                den += w;
            }
    }
    A res = num / den;
    if (KIND == LERF_KIND_GAUSS && emin * (A)0.5 > (A)745.2) res = (A)(0.0 / 0.0);
    if (sizeof(TI) == 1 && sizeof(TH) == 1 && sizeof(TO) == 1) {
        auto tap = [&](int rcl, int ccl) -> uint32_t {
            const int64_t ho = rcl * hy + ccl * hx + c * hc;
            const uint32_t k0 = (uint32_t)h0[ho];
            const uint32_t k12 = KIND == LERF_KIND_GAUSS ? (((uint32_t)h1[ho]) << 8) | (((uint32_t)h2[ho]) << 16) : 0u;
            return k0 | k12 | ((uint32_t)feat[rcl * fy + ccl * fx + c * fc] << 24);
        };
        if (warp_tie_guard<KIND>((float)res, S, H, W, g, px, (float)max_sigma, tap, reinterpret_cast<uint8_t*>(dst)))
            return;
    }
    Storer<TO>::put(dst, res);
}

// ---------------------------------------------------------------------------
// A7/A8 on packed stage outputs (dword = hq0 | hq1<<8 | hq2<<16 | feat<<24): one dword load per tap, channel c of one frame
// ---------------------------------------------------------------------------
template <typename TO, int KIND>
__device__ __forceinline__ void warp_packed_body(const uint32_t* __restrict__ packed, int H, int W, int C, const WarpGeo& g,
                                                 const WarpPixel& px, int c, float max_sigma, TO* __restrict__ dst) {
    const int S = g.S;
    float emin = 0, num = 0, den = 0;
    for (int pass = (KIND == LERF_KIND_GAUSS ? 0 : 1); pass < 2; ++pass) {
        for (int a = 0; a < S; ++a)
            for (int b = 0; b < S; ++b) {
                const WarpTap<float> tp = warp_tap<float>(g, px, a, b, H, W);
                const uint32_t d = packed[((int64_t)tp.rcl * W + tp.ccl) * C + c];
                float w;
                if (KIND == LERF_KIND_GAUSS) {
                    float e = s3::gauss_form(s3::u8_over_255((float)(d & 0xFFu)), s3::u8_over_255((float)((d >> 8) & 0xFFu)),
                                             s3::u8_over_255((float)((d >> 16) & 0xFFu)), max_sigma, tp.dx, tp.dy);
                    if (pass == 0) {
                        emin = (a == 0 && b == 0) ? e : fminf(e, emin);
                        continue;
                    }
                    w = s3::gauss_weight(e, emin);
                } else {
                    float alpha = s3::lin_alpha_of(s3::u8_over_255((float)(d & 0xFFu)), max_sigma);
                    w = s3::lin_factor(alpha, tp.dx, dist_class(tp.dxd)) * s3::lin_factor(alpha, tp.dy, dist_class(tp.dyd));
                }
                float val = tp.inside ? (float)(d >> 24) : 0.0f;
                num += w * val;
                den += w;
            }
    }
    float res = num / den;
    if (KIND == LERF_KIND_GAUSS && emin * 0.5f > 745.2f) res = __builtin_nanf("");
    if (sizeof(TO) == 1) {
        auto tap = [&](int rcl, int ccl) -> uint32_t { return packed[((int64_t)rcl * W + ccl) * C + c]; };
        if (warp_tie_guard<KIND>(res, S, H, W, g, px, max_sigma, tap, reinterpret_cast<uint8_t*>(dst)))
            return;
    }
    Storer<TO>::put(dst, res);
}

// ---------------------------------------------------------------------------
// The same, one thread per output PIXEL of an RGB frame with S = 2 (see warp_packed_px_kernel, lerf_kernels.hip).
// ---------------------------------------------------------------------------
// 1-D grid of (output row, 256-pixel segment) blocks in row-major order, each XCD on a contiguous eighth of it = a band of
// output rows: the packed-map rows two neighbouring output rows share are then fetched into ONE L2 (round 4, linear
// order: every map byte came from HBM 2.5 times, L2 hit 0.62 -- neighbouring rows sat on different XCDs)
__device__ __forceinline__ void warp_px_block(int oW, int* i, int* j) {
    const int gx = (oW + 255) >> 8;
    const int b = (int)gridDim.x >= 1024 ? xcd_contiguous((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
    *i = b / gx;
    *j = (b - *i * gx) * 256 + (int)threadIdx.x;
}

// pixel (i, j) of every frame of the batch from its tap geometry G
template <typename TO, int KIND, bool PROD>
__device__ __forceinline__ void warp_packed_px_body(const uint32_t* __restrict__ packed0, int64_t packed_sn, int n_frames, int H, int W,
                                                    const WarpGeo& g, const WarpPx2& G, int i, int j, float max_sigma,
                                                    TO* __restrict__ out0, int64_t oy, int64_t ox, int64_t oc, int64_t out_sn) {
    constexpr int S = 2, C = 3;
    int64_t pos[S * S];
#pragma unroll
    for (int a = 0; a < S; ++a)
#pragma unroll
        for (int b = 0; b < S; ++b) pos[a * S + b] = ((int64_t)G.rrow[b] * W + G.rcol[a]) * C;
    float dxs[S], dys[S];
    const float gsc = (PROD && KIND == LERF_KIND_GAUSS) ? s3::gauss_scale(max_sigma) : 1.0f;
#pragma unroll
    for (int b = 0; b < S; ++b) { dxs[b] = G.dx[b] * gsc; dys[b] = G.dy[b] * gsc; }
    // the frames of the batch share the geometry: the float64 point and the tap geometry are paid once per output pixel, not
    // once per frame (round 3: a fifth of this kernel's instructions went into repeating them)
#pragma unroll 1
    for (int fr = 0; fr < n_frames; ++fr) {
    const uint32_t* __restrict__ packed = packed0 + (int64_t)fr * packed_sn;
    TO* __restrict__ out = out0 + (int64_t)fr * out_sn;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        TO* dst = out + i * oy + j * ox + c * oc;
        auto tap = [&](int rcl, int ccl) -> uint32_t { return packed[((int64_t)rcl * W + ccl) * C + c]; };
        float res;
        if constexpr (PROD) {
            static_assert(sizeof(TO) == 1, "production arithmetic: uint8 outputs");
            if (warp_px_value_u8<KIND>(G, g, H, W, max_sigma, dxs, dys, tap, reinterpret_cast<uint8_t*>(dst), &res)) continue;
        } else {
            uint32_t d[S * S];
#pragma unroll
            for (int t = 0; t < S * S; ++t) d[t] = packed[pos[t] + c];
            res = warp_px_value<KIND>(G, max_sigma, d);
            if (sizeof(TO) == 1 && warp_tie_guard<KIND>(res, S, H, W, g, G.p, max_sigma, tap, reinterpret_cast<uint8_t*>(dst))) continue;
        }
        Storer<TO>::put(dst, res);
    }
    }
}

}  // namespace lerf
