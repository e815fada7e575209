// Backward of the float warps on planar maps (Warp2dTorch and its kinds, resize_right2d_torch.py:249-487), as autograd
// derives it for the reference's torch code.  The reference keeps its distances in float64, so its weights and their
// normalisation are float64; the gradients reach the float32 leaves through float32 index / pad backward.  Each tap's
// terms are therefore evaluated in float64 with the unshifted weights, rounded to float32, and summed in float32:
//   out = sum_t w_t v_t / W,  W = sum_t w_t          v_t = image at the tap (0 in a constant pad)
//   d out / d v_t = w_t / W                          (w_t alone for the fixed kinds at S = 1: warp() does not normalise)
//   d out / d w_t = (v_t - out) / W
//   gauss:  w = exp(-e/2), e = tx^2 - 2 rho tx ty + ty^2, tx = sx dx, ty = sy dy; rho = 2 h0 - 1, s = max_sigma h
//   linear: w = max(lx, 0) max(ly, 0), l(x) = (alpha x + 1)[-1 <= x < 0] + (1 - alpha x)[0 <= x <= 1],
//           alpha = max_sigma (2 h0 - 1); clamp passes the gradient where its argument is >= 0
// A pixel whose weights all vanish is NaN in the forward (0/0); the same formulas hand its taps NaN, as autograd does.
// Hyper-parameter gradients land on the clamped source pixel (the maps are replicate-padded), the image gradient on
// the pixel the image's pad rule names (nothing for a constant pad outside the frame: F.pad's backward).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <string.h>

#include "lerf_warp_px.h"
#include "lerf_taps.h"

namespace lerf {
namespace warp_bwd {

// One workgroup = a 16 x 16 block of outputs of one plane.  A homography's footprint is not a rectangle spanned by the
// block's corners (the projection can cross the horizon), so the block reduces the clamped rows and columns its own taps
// touch (LDS min / max) and takes that as its window.  When the window fits, the gradient maps are summed in LDS
// (ds_add_f32) and flushed with one global atomic per non-zero window element; otherwise every tap adds to global memory.
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
        const double sx = (double)(h1[ho] * ms), sy = (double)(h2[ho] * ms);
        r.tx = sx * t.dx;
        r.ty = sy * t.dy;
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

template <int KIND>
__global__ void __launch_bounds__(WB_NT)
warp_bwd_kernel(const float* __restrict__ feat, const float* __restrict__ h0, const float* __restrict__ h1, const float* __restrict__ h2,
                int H, int W, WarpGeo g, float ms, const double* __restrict__ gout, float* __restrict__ gfeat, float* __restrict__ gh0,
                float* __restrict__ gh1, float* __restrict__ gh2) {
    constexpr int NM = Kind<KIND>::maps, CAP = WB_LDS / NM;
    __shared__ float win[WB_LDS];
    __shared__ int rng[4];           // window: first row, last row, first column, last column
    const int tid = threadIdx.x;
    const int i = blockIdx.y * WB_ROWS + tid / WB_COLS, j = blockIdx.x * WB_COLS + tid % WB_COLS, n = blockIdx.z;
    const bool act = i < g.oH && j < g.oW;
    const int S = g.S;
    const int64_t plane = (int64_t)n * H * W;
    if (tid == 0) { rng[0] = INT_MAX; rng[1] = -1; rng[2] = INT_MAX; rng[3] = -1; }
    WarpPixel px{};
    if (act) px = warp_pixel(g, i, j, H, W);
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
            }
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

using namespace lerf;
using namespace lerf::warp_bwd;

extern "C" {

int lerf_warp_bwd(const float* feat, const float* h0, const float* h1, const float* h2, int N, int H, int W, const lerf_warp_geo_t* geo,
                  int kind, double max_sigma, const double* grad_out, float* grad_feat, float* grad_h0, float* grad_h1, float* grad_h2,
                  void* stream) {
    if (!feat || !geo || !grad_out || N < 1 || H < 1 || W < 1) return LERF_EINVAL;
    if (geo->out_h < 1 || geo->out_w < 1 || geo->pad_mode < LERF_PAD_CONSTANT || geo->pad_mode > LERF_PAD_WRAP) return LERF_EINVAL;
    if (kind < LERF_KIND_GAUSS || kind > LERF_KIND_LANCZOS3) return LERF_EUNSUPPORTED;
    if ((kind == LERF_KIND_GAUSS || kind == LERF_KIND_LINEAR) && !h0) return LERF_EINVAL;
    if (kind == LERF_KIND_GAUSS && (!h1 || !h2)) return LERF_EINVAL;
    if (geo->S < 1 || geo->S > LERF_MAX_SUPPORT) return LERF_EUNSUPPORTED;
    if (geo->out_y0 != 0 || geo->out_x0 != 0 || geo->src_y0 != 0) return LERF_EUNSUPPORTED;     // whole outputs only
    if (N > 65535 || geo->out_h > 65535 * WB_ROWS) return LERF_EINVAL;
    clear_stale_error();
    WarpGeo g{};
    g.S = geo->S; g.oH = geo->out_h; g.oW = geo->out_w;
    memcpy(g.minv, geo->minv, sizeof(g.minv));
    g.pad_r_lo = geo->pad_r_lo; g.pad_r_hi = geo->pad_r_hi;
    g.pad_c_lo = geo->pad_c_lo; g.pad_c_hi = geo->pad_c_hi;
    g.pad_mode = geo->pad_mode;
    dim3 block(WB_NT), grid((g.oW + WB_COLS - 1) / WB_COLS, (g.oH + WB_ROWS - 1) / WB_ROWS, N);
    hipStream_t st = (hipStream_t)stream;
    const float ms = (float)max_sigma;
#define LERF_WB(KIND, A1, A2, A3)                                                                                          \
    hipLaunchKernelGGL(warp_bwd_kernel<KIND>, grid, block, 0, st, feat, h0, h1, h2, H, W, g, ms, grad_out, grad_feat, A1, A2, A3)
    switch (kind) {
        case LERF_KIND_GAUSS: LERF_WB(LERF_KIND_GAUSS, grad_h0, grad_h1, grad_h2); break;
        case LERF_KIND_LINEAR: LERF_WB(LERF_KIND_LINEAR, grad_h0, nullptr, nullptr); break;
        case LERF_KIND_NEAREST: LERF_WB(LERF_KIND_NEAREST, nullptr, nullptr, nullptr); break;
        case LERF_KIND_CUBIC: LERF_WB(LERF_KIND_CUBIC, nullptr, nullptr, nullptr); break;
        case LERF_KIND_BILINEAR: LERF_WB(LERF_KIND_BILINEAR, nullptr, nullptr, nullptr); break;
        case LERF_KIND_LANCZOS2: LERF_WB(LERF_KIND_LANCZOS2, nullptr, nullptr, nullptr); break;
        case LERF_KIND_LANCZOS3: LERF_WB(LERF_KIND_LANCZOS3, nullptr, nullptr, nullptr); break;
    }
#undef LERF_WB
    return launch_status();
}

}  // extern "C"
