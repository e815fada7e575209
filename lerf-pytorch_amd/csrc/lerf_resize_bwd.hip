// Backward of the SR resamplers on planar float32 maps (Resize2dTorch.resize and its fixed-kernel subclasses,
// SteeringGaussianResize2dTorch.resize / AmplifiedLinearResize2dTorch.resize, resize_right2d_torch.py:105-247), as
// autograd derives it:
//   out = sum_t w_t v_t / W,  W = sum_t w_t          v_t = image at the tap under the image's pad rule (0 in a constant pad)
//   d out / d v_t = w_t / W                           (scattered to the pixel the pad rule names: F.pad's backward)
//   d out / d w_t = (v_t - out) / W
//   gauss:  w = exp(-e/2), e = tx^2 - 2 rho tx ty + ty^2, tx = sx dx, ty = sy dy, rho = 2 h0 - 1, s = max_sigma h
//   linear: w = max(lx, 0) max(ly, 0), l(x) = (alpha x + 1)[-1 <= x < 0] + (1 - alpha x)[0 <= x <= 1], alpha = max_sigma (2 h - 1)
//   fixed kinds (nearest, cubic, bilinear, lanczos2/3): w = k(dx) k(dy), the forward's float32 weights
//           (resize_fixed_kernel): d out / d v_t = k_r k_c / (sr sc), sr = sum_b k_r, sc = sum_a k_c; k_r k_c at S = 1
//           (not normalised, :119-121).  Image gradient only.
// Hyper-parameter gradients land on the CLAMPED tap position (the maps are replicate-padded).  Float atomics into the
// gradient maps (accumulating: the caller zeroes them or passes running sums).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lerf_common.h"
#include "lerf_dispatch.h"
#include "lerf_stage3.h"
#include "lerf_taps.h"

namespace lerf {
namespace resize_bwd {

struct Tap {
    float v, w, dx, dy, tx, ty, rho, alpha, lx, ly, cx, cy;
    int64_t pos;         // clamped tap pixel (hyper maps; the image too under a constant pad)
    int rs, cs;          // PADDED: the image pixel the pad rule names
    bool inside;         // the tap has an image pixel (outside the frame under a constant pad: none)
};

template <int KIND, bool PADDED>
__device__ __forceinline__ Tap load_tap(const float* __restrict__ feat, const float* __restrict__ h0, const float* __restrict__ h1,
                                        const float* __restrict__ h2, int64_t plane, int H, int W, int lr, int lc, int a, int b, float dx,
                                        float dy, float max_sigma, int pad_mode) {
    Tap t;
    const SrTap s = sr_tap(lr, lc, a, b, H, W, pad_mode);
    t.pos = plane + (int64_t)s.rcl * W + s.ccl;
    if (PADDED) {
        t.rs = s.rs;
        t.cs = s.cs;
        t.inside = !s.z;
        t.v = t.inside ? feat[plane + (int64_t)t.rs * W + t.cs] : 0.0f;
    } else {
        t.inside = s.inside;
        t.v = t.inside ? feat[t.pos] : 0.0f;
    }
    t.dx = dx;
    t.dy = dy;
    if (KIND == LERF_KIND_GAUSS) {
        const s3::GaussParams p = s3::gauss_params_of(h0[t.pos], h1[t.pos], h2[t.pos], max_sigma);
        t.rho = p.rho;
        t.tx = p.sx * dx;
        t.ty = p.sy * dy;
        t.w = t.tx * t.tx - 2.0f * t.rho * (t.tx * t.ty) + t.ty * t.ty;      // the exponent e; turned into a weight by the caller
    } else {
        t.alpha = s3::lin_alpha_ref(h0[t.pos], max_sigma);
        t.lx = (t.alpha * dx + 1.0f) * ((-1.0f <= dx && dx < 0.0f) ? 1.0f : 0.0f) + (1.0f - t.alpha * dx) * ((0.0f <= dx && dx <= 1.0f) ? 1.0f : 0.0f);
        t.ly = (t.alpha * dy + 1.0f) * ((-1.0f <= dy && dy < 0.0f) ? 1.0f : 0.0f) + (1.0f - t.alpha * dy) * ((0.0f <= dy && dy <= 1.0f) ? 1.0f : 0.0f);
        t.cx = fmaxf(t.lx, 0.0f);
        t.cy = fmaxf(t.ly, 0.0f);
        t.w = t.cx * t.cy;
    }
    return t;
}

// One workgroup = a 16 x 64 block of outputs of one plane.  Its taps fall into a small window of the input (about
// 16/s + S rows by 64/s + S columns), so the gradient maps of that window are accumulated in LDS (ds_add_f32) and
// flushed with one global atomic per window element: at x4 that is ~40x fewer global atomics than one per tap and map.
// The window is the span of the block's CLAMPED taps.  Windows that do not fit (down-sampling) fall back to global
// atomics per tap; so do image taps that a reflect / wrap pad sends outside the window (wrap: the far side of the frame).
constexpr int RB_ROWS = 16, RB_COLS = 64, RB_WIN_MAX = (RB_ROWS + LERF_MAX_SUPPORT + 1) * (RB_COLS + LERF_MAX_SUPPORT + 1);

// GAUSS / LINEAR.  PADDED = false: constant image pad (image taps outside the frame are 0 and get nothing, every other
// image tap is the clamped tap, inside the window); PADDED = true: the image follows pad_mode.
template <int KIND, bool PADDED>
__global__ void __launch_bounds__(256)
resize_bwd_kernel(const float* __restrict__ feat, const float* __restrict__ h0, const float* __restrict__ h1,
                  const float* __restrict__ h2, int N, int H, int W, int S, int oH, int oW, const int* __restrict__ left_r,
                  const float* __restrict__ dis_r, const int* __restrict__ left_c, const float* __restrict__ dis_c, float max_sigma,
                  int pad_mode, const float* __restrict__ gout, float* __restrict__ gfeat, float* __restrict__ gh0,
                  float* __restrict__ gh1, float* __restrict__ gh2) {
    __shared__ float win[4][RB_WIN_MAX];
    const int tid = threadIdx.x;
    const int j0 = blockIdx.x * RB_COLS, i0 = blockIdx.y * RB_ROWS, n = blockIdx.z;
    const int i1 = min(i0 + RB_ROWS, oH) - 1, j1 = min(j0 + RB_COLS, oW) - 1;
    // window of clamped source positions touched by this block (left tables are non-decreasing)
    const int wr0 = clampi(left_r[i0], 0, H - 1), wr1 = clampi(left_r[i1] + S - 1, 0, H - 1);
    const int wc0 = clampi(left_c[j0], 0, W - 1), wc1 = clampi(left_c[j1] + S - 1, 0, W - 1);
    const int wh = wr1 - wr0 + 1, ww = wc1 - wc0 + 1;
    const bool lds = wh * ww <= RB_WIN_MAX;
    if (lds) {
        for (int k = tid; k < wh * ww; k += 256) { win[0][k] = 0.0f; win[1][k] = 0.0f; win[2][k] = 0.0f; win[3][k] = 0.0f; }
        __syncthreads();
    }
    const int64_t plane = (int64_t)n * H * W;
    for (int e = tid; e < RB_ROWS * RB_COLS; e += 256) {
        const int i = i0 + e / RB_COLS, j = j0 + e % RB_COLS;
        if (i >= oH || j >= oW) continue;
        const int lr = left_r[i], lc = left_c[j];
        float emin = 0.0f;
        if (KIND == LERF_KIND_GAUSS) {
            for (int a = 0; a < S; ++a)
                for (int b = 0; b < S; ++b) {
                    const Tap t = load_tap<KIND, PADDED>(feat, h0, h1, h2, plane, H, W, lr, lc, a, b, dis_r[i * S + b], dis_c[j * S + a],
                                                         max_sigma, pad_mode);
                    emin = (a == 0 && b == 0) ? t.w : fminf(emin, t.w);
                }
        }
        float Wsum = 0.0f, num = 0.0f;
        for (int a = 0; a < S; ++a)
            for (int b = 0; b < S; ++b) {
                Tap t = load_tap<KIND, PADDED>(feat, h0, h1, h2, plane, H, W, lr, lc, a, b, dis_r[i * S + b], dis_c[j * S + a],
                                               max_sigma, pad_mode);
                const float w = KIND == LERF_KIND_GAUSS ? __expf(-0.5f * (t.w - emin)) : t.w;
                Wsum += w;
                num += w * t.v;
            }
        const float out = num / Wsum;
        const float g = gout[((int64_t)n * oH + i) * oW + j];
        for (int a = 0; a < S; ++a)
            for (int b = 0; b < S; ++b) {
                Tap t = load_tap<KIND, PADDED>(feat, h0, h1, h2, plane, H, W, lr, lc, a, b, dis_r[i * S + b], dis_c[j * S + a],
                                               max_sigma, pad_mode);
                const float w = KIND == LERF_KIND_GAUSS ? __expf(-0.5f * (t.w - emin)) : t.w;
                const int64_t rel = t.pos - plane;
                const int k = ((int)(rel / W) - wr0) * ww + ((int)(rel % W) - wc0);        // window slot of the clamped tap
                float gv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (t.inside) gv[0] = g * w / Wsum;
                const float gw = g * (t.v - out) / Wsum;          // d loss / d w_t
                if (KIND == LERF_KIND_GAUSS) {
                    const float c = gw * (-0.5f * w);               // d loss / d e_t
                    gv[1] = c * (-2.0f * t.tx * t.ty) * 2.0f;
                    gv[2] = c * (2.0f * t.dx * (t.tx - t.rho * t.ty)) * max_sigma;
                    gv[3] = c * (2.0f * t.dy * (t.ty - t.rho * t.tx)) * max_sigma;
                } else {
                    // clamp(l, 0) passes the gradient where l >= 0 (torch.clamp backward)
                    const float dlx = (t.lx >= 0.0f ? 1.0f : 0.0f) * (t.dx * ((-1.0f <= t.dx && t.dx < 0.0f) ? 1.0f : 0.0f) - t.dx * ((0.0f <= t.dx && t.dx <= 1.0f) ? 1.0f : 0.0f));
                    const float dly = (t.ly >= 0.0f ? 1.0f : 0.0f) * (t.dy * ((-1.0f <= t.dy && t.dy < 0.0f) ? 1.0f : 0.0f) - t.dy * ((0.0f <= t.dy && t.dy <= 1.0f) ? 1.0f : 0.0f));
                    gv[1] = gw * (dlx * t.cy + t.cx * dly) * 2.0f * max_sigma;
                }
                float* const dst[4] = {gfeat, gh0, gh1, gh2};
#pragma unroll
                for (int m = 0; m < (KIND == LERF_KIND_GAUSS ? 4 : 2); ++m) {
                    if (!dst[m] || (m == 0 && !t.inside)) continue;
                    if (PADDED && m == 0) {
                        // the pixel the pad rule names: in the window, or (reflected / wrapped beyond it) straight to memory
                        const int kr = t.rs - wr0, kc = t.cs - wc0;
                        if (lds && kr >= 0 && kr < wh && kc >= 0 && kc < ww) atomicAdd(&win[0][kr * ww + kc], gv[0]);
                        else if (gv[0] != 0.0f) atomicAdd(gfeat + plane + (int64_t)t.rs * W + t.cs, gv[0]);
                        continue;
                    }
                    if (lds) atomicAdd(&win[m][k], gv[m]);
                    else atomicAdd(dst[m] + t.pos, gv[m]);
                }
            }
    }
    if (lds) {
        __syncthreads();
        float* const dst[4] = {gfeat, gh0, gh1, gh2};
        for (int k = tid; k < wh * ww; k += 256) {
            const int64_t pos = plane + (int64_t)(wr0 + k / ww) * W + wc0 + k % ww;
#pragma unroll
            for (int m = 0; m < (KIND == LERF_KIND_GAUSS ? 4 : 2); ++m) {
                const float v = win[m][k];
                if (dst[m] && v != 0.0f) atomicAdd(dst[m] + pos, v);
            }
        }
    }
}

// Fixed kinds: one gradient map, so its window may take the LDS the four maps of resize_bwd_kernel share (4 x 1825
// floats: a 0.5x down-sampling at S = 4, ~34 x 130, still fits).  The block's row and column weights are evaluated once
// per block (S per output row / column, float64 like fixed_kernel_1d, rounded to float32 like the forward) and read back
// from LDS by every output.
constexpr int RF_WIN_MAX = 4 * RB_WIN_MAX;

template <int KIND>
__global__ void __launch_bounds__(256)
resize_bwd_fixed_kernel(int H, int W, int S, int oH, int oW, const int* __restrict__ left_r, const float* __restrict__ dis_r,
                        const int* __restrict__ left_c, const float* __restrict__ dis_c, int pad_mode, const float* __restrict__ gout,
                        float* __restrict__ gfeat) {
    __shared__ float win[RF_WIN_MAX];
    __shared__ float kr[RB_ROWS * LERF_MAX_SUPPORT], kc[RB_COLS * LERF_MAX_SUPPORT];
    __shared__ float sr[RB_ROWS], sc[RB_COLS];
    const int tid = threadIdx.x;
    const int j0 = blockIdx.x * RB_COLS, i0 = blockIdx.y * RB_ROWS, n = blockIdx.z;
    const int i1 = min(i0 + RB_ROWS, oH) - 1, j1 = min(j0 + RB_COLS, oW) - 1;
    const int wr0 = clampi(left_r[i0], 0, H - 1), wr1 = clampi(left_r[i1] + S - 1, 0, H - 1);
    const int wc0 = clampi(left_c[j0], 0, W - 1), wc1 = clampi(left_c[j1] + S - 1, 0, W - 1);
    const int wh = wr1 - wr0 + 1, ww = wc1 - wc0 + 1;
    const bool lds = wh * ww <= RF_WIN_MAX;
    if (lds)
        for (int k = tid; k < wh * ww; k += 256) win[k] = 0.0f;
    for (int e = tid; e < (RB_ROWS + RB_COLS) * S; e += 256) {
        const bool row = e < RB_ROWS * S;
        const int q = row ? e : e - RB_ROWS * S;          // (output row / column within the block) * S + tap
        const int o = (row ? i0 : j0) + q / S;
        float k = 0.0f;
        if (o < (row ? oH : oW)) k = (float)fixed_kernel_1d(KIND, (double)(row ? dis_r : dis_c)[o * S + q % S]);
        (row ? kr : kc)[q] = k;
    }
    __syncthreads();
    if (tid < RB_ROWS + RB_COLS) {                          // the forward's sums, in its order
        const float* k = tid < RB_ROWS ? kr + tid * S : kc + (tid - RB_ROWS) * S;
        float s = 0.0f;
        for (int b = 0; b < S; ++b) s += k[b];
        if (tid < RB_ROWS) sr[tid] = s;
        else sc[tid - RB_ROWS] = s;
    }
    __syncthreads();
    const int64_t plane = (int64_t)n * H * W;
    for (int e = tid; e < RB_ROWS * RB_COLS; e += 256) {
        const int ii = e / RB_COLS, jj = e % RB_COLS, i = i0 + ii, j = j0 + jj;
        if (i >= oH || j >= oW) continue;
        const int lr = left_r[i], lc = left_c[j];
        const float g = gout[((int64_t)n * oH + i) * oW + j];
        const float gn = S == 1 ? g : g / (sr[ii] * sc[jj]);
        for (int a = 0; a < S; ++a) {
            const SourceTap tc = source_tap(lc + a, W, pad_mode);
            if (tc.z) continue;
            const float ga = gn * kc[jj * S + a];
            for (int b = 0; b < S; ++b) {
                const SourceTap tr = source_tap(lr + b, H, pad_mode);
                if (tr.z) continue;
                const float v = ga * kr[ii * S + b];
                const int wr = tr.s - wr0, wc = tc.s - wc0;
                if (lds && wr >= 0 && wr < wh && wc >= 0 && wc < ww) atomicAdd(&win[wr * ww + wc], v);
                else if (v != 0.0f) atomicAdd(gfeat + plane + (int64_t)tr.s * W + tc.s, v);
            }
        }
    }
    if (lds) {
        __syncthreads();
        for (int k = tid; k < wh * ww; k += 256) {
            const float v = win[k];
            if (v != 0.0f) atomicAdd(gfeat + plane + (int64_t)(wr0 + k / ww) * W + wc0 + k % ww, v);
        }
    }
}

}  // namespace resize_bwd
}  // namespace lerf

using namespace lerf;
using namespace lerf::resize_bwd;

extern "C" {

int lerf_resize_bwd_f32(const float* feat, const float* h0, const float* h1, const float* h2, int N, int H, int W,
                        const lerf_sr_geo_t* geo, int kind, double max_sigma, const float* grad_out, float* grad_feat,
                        float* grad_h0, float* grad_h1, float* grad_h2, void* stream) {
    if (!bwd_operands_ok(feat, geo, grad_out, N, H, W)) return LERF_EINVAL;
    if (geo->pad_mode < LERF_PAD_CONSTANT || geo->pad_mode > LERF_PAD_WRAP) return LERF_EINVAL;
    const int rc = bwd_kind_check(kind, h0, h1, h2);
    if (rc != LERF_OK) return rc;
    if (!geo->left_r || !geo->left_c || !geo->dis_r || !geo->dis_c || geo->out_h < 1 || geo->out_w < 1) return LERF_EINVAL;
    if (geo->S < 1 || geo->S > LERF_MAX_SUPPORT) return LERF_EUNSUPPORTED;
    clear_stale_error();
    dim3 block(256), grid((geo->out_w + RB_COLS - 1) / RB_COLS, (geo->out_h + RB_ROWS - 1) / RB_ROWS, N);
    hipStream_t st = (hipStream_t)stream;
    const int pm = geo->pad_mode;
    const float ms = (float)max_sigma;
    if (kind == LERF_KIND_GAUSS || kind == LERF_KIND_LINEAR) {
        with_hyper_kind(kind, [&](auto K) {
            constexpr int KIND = decltype(K)::value;        // the linear kernel has one hyper-parameter map to differentiate
            return with_bool(pm == LERF_PAD_CONSTANT, [&](auto CONSTANT_PAD) {
                hipLaunchKernelGGL((resize_bwd_kernel<KIND, !decltype(CONSTANT_PAD)::value>), grid, block, 0, st, feat, h0, h1, h2, N, H, W,
                                   geo->S, geo->out_h, geo->out_w, geo->left_r, geo->dis_r, geo->left_c, geo->dis_c, ms, pm, grad_out,
                                   grad_feat, grad_h0, KIND == LERF_KIND_GAUSS ? grad_h1 : nullptr,
                                   KIND == LERF_KIND_GAUSS ? grad_h2 : nullptr);
                return LERF_OK;
            });
        });
    } else {
        if (!grad_feat) return LERF_OK;                     // nothing to compute: the fixed kinds have no other gradient
        with_fixed_kind(kind, [&](auto K) {
            hipLaunchKernelGGL(resize_bwd_fixed_kernel<decltype(K)::value>, grid, block, 0, st, H, W, geo->S, geo->out_h, geo->out_w,
                               geo->left_r, geo->dis_r, geo->left_c, geo->dis_c, pm, grad_out, grad_feat);
            return LERF_OK;
        });
    }
    return launch_status();
}

}  // extern "C"
