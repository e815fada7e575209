// Backward of the float remap on planar maps (lerf_remap with float32 planes and a float64 output; the *Remap2dTorch classes):
// lerf_warp_bwd with the point of every output pixel read from the coordinate map, plus the one gradient a homography has no use
// for -- d loss / d map.
//
// Image and hyper-parameter gradients are lerf_warp_bwd's, formula for formula (the top of lerf_warp_bwd.hip, its NaN rule for a
// pixel whose weights all vanish included): after the point is known the kernel runs the same body (lerf_warp_bwd_kernels.h), float
// atomics into an LDS window or, when the block's window does not fit -- a folded or scattered map -- into global memory.
//
// The map gradient: the point q = (row, col) enters only through the distances d_row,k = clip(row) + pad - p_k (columns alike); the
// tap set, the pads and the class masks are piecewise constant, so it is the gradient autograd gives with them held fixed,
//   d loss / d row = [0 <= row <= H] sum_t (d loss / d w_t) (d w_t / d dx_t)
// with torch.clamp's backward for the clip (it passes at the borders, is zero outside and for +-inf).  Float64 throughout.  Each
// element (n, i, j, .) has ONE writer, the thread of that pixel and plane, so grad_coords is per plane, updated with a plain
// load-add-store: no atomics, bit-equal from run to run, and the accumulate contract of the other gradients.  The sum over planes
// is the caller's.  A NaN entry is masked: it contributes to no gradient, adds nothing to its own, and takes no part in the block's
// window; a block with no pixel left returns before it touches anything.
//
// Addresses: as in lerf_remap.hip -- the map is read at (i, j) inside [oH][oW] only, the point is clipped before any conversion to
// int and every tap index passes axis_tap's clamps; grad_coords is written at the same (n, i, j).
#include "lerf_dispatch.h"
#include "lerf_warp_bwd_kernels.h"
#include "lerf_remap_point.h"

namespace lerf {
namespace warp_bwd {

// COORD: grad_coords is wanted (compile time, so that a call without it runs the homographic backward's arithmetic and nothing more)
template <int KIND, bool COORD>
__global__ void __launch_bounds__(WB_NT)
remap_bwd_kernel(const float* __restrict__ feat, const float* __restrict__ h0, const float* __restrict__ h1, const float* __restrict__ h2,
                 int H, int W, RemapGeo m, float ms, const double* __restrict__ gout, float* __restrict__ gfeat, float* __restrict__ gh0,
                 float* __restrict__ gh1, float* __restrict__ gh2, double* __restrict__ gcoords) {
    const int tid = threadIdx.x;
    const int i = blockIdx.y * WB_ROWS + tid / WB_COLS, j = blockIdx.x * WB_COLS + tid % WB_COLS, n = blockIdx.z;
    bool act = i < m.oH && j < m.oW;
    remap_select(m, n);                                    // plane n reads its sample's map (uniform over the block)
    const WarpGeo g = remap_warp_geo(m, H, W);
    MapPoint q{0.0, 0.0};
    WarpPixel px{};
    if (act) {
        q = remap_entry(m, i, j);
        act = !no_point(q);
        if (act) px = remap_pixel(g, q, H, W);
    }
    double gdx = 0.0, gdy = 0.0;
    warp_bwd_body<KIND, COORD>(feat, h0, h1, h2, H, W, g, ms, gout, gfeat, gh0, gh1, gh2, px, act, i, j, n, &gdx, &gdy);
    if (COORD && act) {
        // torch.clamp's backward: the gradient passes where the unclipped entry lies in [0, n] (borders included)
        double2* dst = reinterpret_cast<double2*>(gcoords) + ((int64_t)n * m.oH + i) * m.oW + j;
        double2 v = *dst;
        v.x += (q.r >= 0.0 && q.r <= (double)H) ? gdx : 0.0;
        v.y += (q.c >= 0.0 && q.c <= (double)W) ? gdy : 0.0;
        *dst = v;
    }
}

}  // namespace warp_bwd
}  // namespace lerf

using namespace lerf;
using namespace lerf::warp_bwd;

// both entry points: n_maps maps, planes_per_map planes each (the plain one: one map, N planes)
static int remap_bwd(const float* feat, const float* h0, const float* h1, const float* h2, int N, int H, int W, const lerf_remap_geo_t* geo,
                     int n_maps, int64_t map_stride, int planes_per_map, int kind, double max_sigma, const double* grad_out, float* grad_feat,
                     float* grad_h0, float* grad_h1, float* grad_h2, double* grad_coords, void* stream) {
    if (!bwd_operands_ok(feat, geo, grad_out, N, H, W)) return LERF_EINVAL;
    RemapGeo m{};
    int rc = remap_geo_batched(geo, n_maps, map_stride, N, planes_per_map, m);
    if (rc == LERF_OK) rc = bwd_kind_check(kind, h0, h1, h2);
    if (rc != LERF_OK) return rc;
    if (geo->S < 1 || geo->S > LERF_MAX_SUPPORT) return LERF_EUNSUPPORTED;
    if (N > 65535 || geo->out_h > 65535 * WB_ROWS) return LERF_EINVAL;
    if (grad_coords && (size_t)(uintptr_t)grad_coords % 16 != 0) return LERF_EINVAL;      // one 16-byte load / store per entry
    clear_stale_error();
    dim3 block(WB_NT), grid((m.oW + WB_COLS - 1) / WB_COLS, (m.oH + WB_ROWS - 1) / WB_ROWS, N);
    hipStream_t st = (hipStream_t)stream;
    const float ms = (float)max_sigma;
    with_kind(kind, [&](auto K) {
        constexpr int KIND = decltype(K)::value;            // a kind's kernel is handed the gradients of the maps it reads only
        return with_bool(grad_coords != nullptr, [&](auto COORD) {
            hipLaunchKernelGGL((remap_bwd_kernel<KIND, decltype(COORD)::value>), grid, block, 0, st, feat, h0, h1, h2, H, W, m, ms, grad_out,
                               grad_feat, KIND <= LERF_KIND_LINEAR ? grad_h0 : nullptr, KIND == LERF_KIND_GAUSS ? grad_h1 : nullptr,
                               KIND == LERF_KIND_GAUSS ? grad_h2 : nullptr, grad_coords);
            return LERF_OK;
        });
    });
    return launch_status();
}

extern "C" {

int lerf_remap_bwd(const float* feat, const float* h0, const float* h1, const float* h2, int N, int H, int W, const lerf_remap_geo_t* geo,
                   int kind, double max_sigma, const double* grad_out, float* grad_feat, float* grad_h0, float* grad_h1, float* grad_h2,
                   double* grad_coords, void* stream) {
    return remap_bwd(feat, h0, h1, h2, N, H, W, geo, 1, 0, N, kind, max_sigma, grad_out, grad_feat, grad_h0, grad_h1, grad_h2,
                     grad_coords, stream);
}

int lerf_remap_bwd_batched(const float* feat, const float* h0, const float* h1, const float* h2, int N, int H, int W,
                           const lerf_remap_geo_t* geo, int n_maps, int64_t map_stride, int planes_per_map, int kind, double max_sigma,
                           const double* grad_out, float* grad_feat, float* grad_h0, float* grad_h1, float* grad_h2, double* grad_coords,
                           void* stream) {
    return remap_bwd(feat, h0, h1, h2, N, H, W, geo, n_maps, map_stride, planes_per_map, kind, max_sigma, grad_out, grad_feat, grad_h0,
                     grad_h1, grad_h2, grad_coords, stream);
}

}  // extern "C"
