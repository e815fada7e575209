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
#include "lerf_dispatch.h"
#include "lerf_warp_bwd_kernels.h"

namespace lerf {
namespace warp_bwd {

// the point of pixel (i, j) projected through the inverse matrix, then the shared body (lerf_warp_bwd_kernels.h) without the
// gradient with respect to the point: a homography's grid is fixed data
template <int KIND>
__global__ void __launch_bounds__(WB_NT)
warp_bwd_kernel(const float* __restrict__ feat, const float* __restrict__ h0, const float* __restrict__ h1, const float* __restrict__ h2,
                int H, int W, WarpGeo g, float ms, const double* __restrict__ gout, float* __restrict__ gfeat, float* __restrict__ gh0,
                float* __restrict__ gh1, float* __restrict__ gh2) {
    const int tid = threadIdx.x;
    const int i = blockIdx.y * WB_ROWS + tid / WB_COLS, j = blockIdx.x * WB_COLS + tid % WB_COLS, n = blockIdx.z;
    const bool act = i < g.oH && j < g.oW;
    WarpPixel px{};
    if (act) px = warp_pixel(g, i, j, H, W);
    warp_bwd_body<KIND, false>(feat, h0, h1, h2, H, W, g, ms, gout, gfeat, gh0, gh1, gh2, px, act, i, j, n, nullptr, nullptr);
}

}  // namespace warp_bwd
}  // namespace lerf

using namespace lerf;
using namespace lerf::warp_bwd;

extern "C" {

int lerf_warp_bwd(const float* feat, const float* h0, const float* h1, const float* h2, int N, int H, int W, const lerf_warp_geo_t* geo,
                  int kind, double max_sigma, const double* grad_out, float* grad_feat, float* grad_h0, float* grad_h1, float* grad_h2,
                  void* stream) {
    if (!bwd_operands_ok(feat, geo, grad_out, N, H, W)) return LERF_EINVAL;
    if (geo->out_h < 1 || geo->out_w < 1 || geo->pad_mode < LERF_PAD_CONSTANT || geo->pad_mode > LERF_PAD_WRAP) return LERF_EINVAL;
    const int rc = bwd_kind_check(kind, h0, h1, h2);
    if (rc != LERF_OK) return rc;
    if (geo->S < 1 || geo->S > LERF_MAX_SUPPORT) return LERF_EUNSUPPORTED;
    if (geo->out_y0 != 0 || geo->out_x0 != 0 || geo->src_y0 != 0) return LERF_EUNSUPPORTED;     // whole outputs only
    if (N > 65535 || geo->out_h > 65535 * WB_ROWS) return LERF_EINVAL;
    clear_stale_error();
    const WarpGeo g = to_warp_geo(*geo);
    dim3 block(WB_NT), grid((g.oW + WB_COLS - 1) / WB_COLS, (g.oH + WB_ROWS - 1) / WB_ROWS, N);
    hipStream_t st = (hipStream_t)stream;
    const float ms = (float)max_sigma;
    with_kind(kind, [&](auto K) {
        constexpr int KIND = decltype(K)::value;            // a kind's kernel is handed the gradients of the maps it reads only
        hipLaunchKernelGGL(warp_bwd_kernel<KIND>, grid, block, 0, st, feat, h0, h1, h2, H, W, g, ms, grad_out, grad_feat,
                           KIND <= LERF_KIND_LINEAR ? grad_h0 : nullptr, KIND == LERF_KIND_GAUSS ? grad_h1 : nullptr,
                           KIND == LERF_KIND_GAUSS ? grad_h2 : nullptr);
        return LERF_OK;
    });
    return launch_status();
}

}  // extern "C"
