// Stage 3 by a DENSE COORDINATE MAP (lerf_remap_geo_t): the homographic warp with its projected grid read from memory --
// lens undistortion, rectification, optical-flow and mesh warps, one source position per output pixel with no matrix behind it.
//
//   remap_kernel             counterpart of warp_kernel            (planar / strided operands, every kind, S, pad mode, dtype)
//   remap_packed_kernel      counterpart of warp_packed_kernel     (packed stage dwords, any C, per channel)
//   remap_packed_px_kernel   counterpart of warp_packed_px_kernel  (packed stage dwords, RGB, S = 2, one thread per pixel: hot path)
//
// A kernel here differs from its counterpart in ONE statement: where that one projects (i, j) through the inverse matrix
// (warp_pixel), this one loads the map entry -- one 16-byte (float64) or 8-byte (float32) load per output pixel, consecutive
// lanes on consecutive entries -- and clips it (remap_entry / remap_pixel, lerf_remap_point.h, shared with the backward).
// Everything from the point on is the shared body of lerf_warp_kernels.h, so the map of a homography gives the homographic
// warp's bytes.
//
// One map per sample (lerf_remap*_batched, RemapGeo.map_stride != 0): the plane (remap_kernel) or the frame (the packed kernels)
// of a thread selects its map before the load (remap_select); pads left to the map come from THAT map's first entry.  With per-frame
// maps the per-pixel kernel has no pixel geometry to share between frames, so the frame goes on the grid (PER_FRAME).
//
// Addresses: the map is read at (i, j) inside the launch's [oH][oW] of one of the call's maps only (remap_geo_batched: the maps are
// n_maps disjoint extents, map_stride apart); the point is clipped to [0, H] x [0, W] BEFORE any
// conversion to int (clip_coord sends NaN to 0 and +-inf to the borders), and every tap index passes axis_tap's clamps, so no
// map value -- NaN, infinite, or 1e300 -- can form an address outside the operands.  A NaN entry reads nothing further and
// stores 0 (uint8) / NaN (float).
#include "lerf_dispatch.h"
#include "lerf_warp_kernels.h"
#include "lerf_remap_point.h"

namespace lerf {

// ---------------------------------------------------------------------------
// general remap
// ---------------------------------------------------------------------------
template <typename TI, typename TH, typename TO, typename A, int KIND>
__global__ void __launch_bounds__(256)
remap_kernel(const TI* __restrict__ feat, int64_t fy, int64_t fx, int64_t fc,
             const TH* __restrict__ h0, const TH* __restrict__ h1, const TH* __restrict__ h2,
             int64_t hy, int64_t hx, int64_t hc, int H, int W, int C, RemapGeo m,
             A max_sigma, TO* __restrict__ out, int64_t oy, int64_t ox, int64_t oc) {
    int xc = blockIdx.x * blockDim.x + threadIdx.x;
    int i = blockIdx.y;
    if (xc >= m.oW * C) return;
    int j = xc / C;
    int c = xc - j * C;
    TO* dst = out + i * oy + j * ox + c * oc;
    remap_select(m, c);                                    // plane c reads its sample's map
    const MapPoint q = remap_entry(m, i, j);
    if (no_point(q)) { store_no_value(dst); return; }
    const WarpGeo g = remap_warp_geo(m, H, W);
    warp_body<TI, TH, TO, A, KIND>(feat, fy, fx, fc, h0, h1, h2, hy, hx, hc, H, W, g, remap_pixel(g, q, H, W), c, max_sigma, dst);
}

int launch_remap(const WarpArgs& a, const RemapGeo& m, hipStream_t st) {
    if (m.S < 1 || m.S > LERF_MAX_SUPPORT || m.oH > 65535) return LERF_EUNSUPPORTED;
    dim3 block(256), grid((m.oW * a.C + 255) / 256, m.oH);
    const bool fixed = a.kind >= LERF_KIND_NEAREST;     // no hyper-parameter maps
    return with_stage3_types(a.in_dtype, a.h_dtype, a.out_dtype, fixed, [&](auto T) {
        using TI = typename decltype(T)::TI; using TH = typename decltype(T)::TH;
        using TO = typename decltype(T)::TO; using A = typename decltype(T)::A;
        return with_kind(a.kind, [&](auto K) {
            hipLaunchKernelGGL((remap_kernel<TI, TH, TO, A, decltype(K)::value>), grid, block, 0, st, (const TI*)a.feat, a.fy,
                               a.fx, a.fc, (const TH*)a.h[0], (const TH*)a.h[1], (const TH*)a.h[2], a.hy, a.hx,
                               a.hc, a.H, a.W, a.C, m, (A)a.max_sigma, (TO*)a.out, a.oy, a.ox, a.oc);
            return LERF_OK;
        });
    });
}

// ---------------------------------------------------------------------------
// packed stage outputs
// ---------------------------------------------------------------------------
template <typename TO, int KIND>
__global__ void __launch_bounds__(256)
remap_packed_kernel(const uint32_t* __restrict__ packed, int64_t packed_sn, int H, int W, int C, RemapGeo m, float max_sigma,
                    TO* __restrict__ out, int64_t oy, int64_t ox, int64_t oc, int64_t out_sn) {
    packed += (int64_t)blockIdx.z * packed_sn;             // frame of the batch (one map for all, or its own)
    out += (int64_t)blockIdx.z * out_sn;
    remap_select(m, (int)blockIdx.z);
    int xc = blockIdx.x * blockDim.x + threadIdx.x;
    int i = blockIdx.y;
    if (xc >= m.oW * C) return;
    int j = xc / C;
    int c = xc - j * C;
    TO* dst = out + i * oy + j * ox + c * oc;
    const MapPoint q = remap_entry(m, i, j);
    if (no_point(q)) { store_no_value(dst); return; }
    const WarpGeo g = remap_warp_geo(m, H, W);
    warp_packed_body<TO, KIND>(packed, H, W, C, g, remap_pixel(g, q, H, W), c, max_sigma, dst);
}

// one thread per output PIXEL of an RGB frame with S = 2; the block order of warp_packed_px_kernel (warp_px_block), so the
// lanes of a wave read 64 consecutive map entries (1 KiB of float64 entries per load instruction).
// PER_FRAME: every frame has its own map, so there is no pixel geometry to share between frames: the frame goes on the grid
// (blockIdx.y), one frame per thread, the block order inside a frame unchanged -- a wave still reads 64 consecutive entries of
// its frame's map.  Otherwise one thread walks the batch's frames with the geometry of the shared map
template <typename TO, int KIND, bool PROD = false, bool PER_FRAME = false>
__global__ void __launch_bounds__(256)
remap_packed_px_kernel(const uint32_t* __restrict__ packed0, int64_t packed_sn, int n_frames, int H, int W, RemapGeo m, float max_sigma,
                       TO* __restrict__ out0, int64_t oy, int64_t ox, int64_t oc, int64_t out_sn) {
    if constexpr (PER_FRAME) {
        const int fr = (int)blockIdx.y;
        packed0 += (int64_t)fr * packed_sn;
        out0 += (int64_t)fr * out_sn;
        remap_select(m, fr);
        n_frames = 1;
    }
    int i, j;
    warp_px_block(m.oW, &i, &j);
    if (j >= m.oW) return;
    const MapPoint q = remap_entry(m, i, j);
    if (no_point(q)) {
        for (int fr = 0; fr < n_frames; ++fr)
#pragma unroll
            for (int c = 0; c < 3; ++c) store_no_value(out0 + (int64_t)fr * out_sn + i * oy + j * ox + c * oc);
        return;
    }
    const WarpGeo g = remap_warp_geo(m, H, W);
    const WarpPx2 G = warp_px_geometry(g, remap_pixel(g, q, H, W), H, W);
    warp_packed_px_body<TO, KIND, PROD>(packed0, packed_sn, n_frames, H, W, g, G, i, j, max_sigma, out0, oy, ox, oc, out_sn);
}

// the path selection of launch_warp_packed
int launch_remap_packed(const uint32_t* packed, int64_t packed_sn, int n, int H, int W, int C, const RemapGeo& m, int kind,
                        float max_sigma, void* out, int out_dtype, int64_t oy, int64_t ox, int64_t oc, int64_t out_sn, hipStream_t st) {
    if (m.S < 1 || m.S > LERF_MAX_SUPPORT) return LERF_EUNSUPPORTED;
    if (n < 1 || n > 65535 || m.oH > 65535) return LERF_EUNSUPPORTED;
    if (C == 3 && m.S == 2 && (kind == LERF_KIND_GAUSS || kind == LERF_KIND_LINEAR) &&
        (out_dtype == LERF_U8 || out_dtype == LERF_F32)) {
        const bool per_frame = m.map_stride != 0;
        dim3 blockp(256), gridp((unsigned)(((m.oW + 255) / 256) * m.oH), per_frame ? n : 1, 1);
        const bool prod = out_dtype == LERF_U8 && max_sigma <= s3::kNoShiftMaxSigma;     // production arithmetic + tie guard
        return with_hyper_kind(kind, [&](auto K) {
            auto launch = [&](auto* o, auto PROD) {
                using TO = std::remove_pointer_t<decltype(o)>;
                with_bool(per_frame, [&](auto PER_FRAME) {
                    hipLaunchKernelGGL((remap_packed_px_kernel<TO, decltype(K)::value, decltype(PROD)::value, decltype(PER_FRAME)::value>),
                                       gridp, blockp, 0, st, packed, packed_sn, n, H, W, m, max_sigma, o, oy, ox, oc, out_sn);
                    return LERF_OK;
                });
            };
            if (prod) launch((uint8_t*)out, std::true_type{});
            else if (out_dtype == LERF_U8) launch((uint8_t*)out, std::false_type{});
            else launch((float*)out, std::false_type{});
            return LERF_OK;
        });
    }
    if (out_dtype != LERF_U8 && out_dtype != LERF_F32) return LERF_EUNSUPPORTED;
    dim3 block(256), grid((m.oW * C + 255) / 256, m.oH, n);
    return with_hyper_kind(kind, [&](auto K) {
        auto launch = [&](auto* o) {
            using TO = std::remove_pointer_t<decltype(o)>;
            hipLaunchKernelGGL((remap_packed_kernel<TO, decltype(K)::value>), grid, block, 0, st, packed, packed_sn, H, W, C, m, max_sigma,
                               o, oy, ox, oc, out_sn);
        };
        if (out_dtype == LERF_U8) launch((uint8_t*)out);
        else launch((float*)out);
        return LERF_OK;
    });
}

}  // namespace lerf
