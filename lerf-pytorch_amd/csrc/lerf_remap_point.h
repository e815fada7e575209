// The point of an output pixel of the remap: the map entry in one load, the NaN test, the WarpGeo the shared warp bodies read and
// the clipped point as a WarpPixel, plus the host-side check of a lerf_remap_geo_t.  Shared by the forward (lerf_remap.hip), the
// backward (lerf_remap_bwd.hip) and the entry points (lerf_api.hip), so all see the same point, pads and taps for the same map.
#pragma once

#include "lerf_kernels.h"
#include "lerf_host_geometry.h"

namespace lerf {

struct MapPoint {
    double r, c;
};

// entry (i, j) of the map in ONE load; float32 entries are promoted exactly
__device__ __forceinline__ MapPoint remap_entry(const RemapGeo& m, int i, int j) {
    const int64_t o = (int64_t)i * m.stride + 2 * (int64_t)j;
    if (m.f32) {
        const float2 v = *reinterpret_cast<const float2*>(static_cast<const float*>(m.coords) + o);
        return {(double)v.x, (double)v.y};
    }
    const double2 v = *reinterpret_cast<const double2*>(static_cast<const double*>(m.coords) + o);
    return {v.x, v.y};
}

// the map of plane (or frame) p of a call with one map per sample: `coords` moves to map p / ppm, everything else is shared.  A
// call with ONE map (map_stride == 0) takes the uniform branch and pays no division
__device__ __forceinline__ void remap_select(RemapGeo& m, int p) {
    if (m.map_stride == 0) return;
    const int64_t o = (int64_t)(p / m.ppm) * m.map_stride;
    m.coords = m.f32 ? static_cast<const void*>(static_cast<const float*>(m.coords) + o)
                     : static_cast<const void*>(static_cast<const double*>(m.coords) + o);
}

__device__ __forceinline__ bool no_point(const MapPoint& q) { return q.r != q.r || q.c != q.c; }

// the WarpGeo the shared bodies read (S, output size, low pads, pad mode; no matrix, no rectangle offsets).  Low pads the caller
// left to the map come from its first entry: a uniform load, no host round trip for a device-resident map.
__device__ __forceinline__ WarpGeo remap_warp_geo(const RemapGeo& m, int H, int W) {
    WarpGeo g;
    g.S = m.S; g.oH = m.oH; g.oW = m.oW;
#pragma unroll
    for (int k = 0; k < 9; ++k) g.minv[k] = 0.0;
    g.pad_r_lo = m.pad_r_lo; g.pad_c_lo = m.pad_c_lo;
    if (m.pad_r_lo < 0 || m.pad_c_lo < 0) {
        const MapPoint q0 = remap_entry(m, 0, 0);
        if (m.pad_r_lo < 0) g.pad_r_lo = remap_pad_lo(q0.r, H, m.S);
        if (m.pad_c_lo < 0) g.pad_c_lo = remap_pad_lo(q0.c, W, m.S);
    }
    g.pad_r_hi = 0; g.pad_c_hi = 0;
    g.pad_mode = m.pad_mode;
    g.oy0 = 0; g.ox0 = 0;
    return g;
}

__device__ __forceinline__ WarpPixel remap_pixel(const WarpGeo& g, const MapPoint& q, int H, int W) {
    return remap_pixel(q.r, q.c, g.S, g.pad_r_lo, g.pad_c_lo, H, W);
}

// lerf_remap_geo_t -> RemapGeo; what can be checked on the host is (the map's values cannot, and need not be: lerf_remap.hip)
inline int remap_geo(const lerf_remap_geo_t* geo, RemapGeo& m) {
    if (!geo || !geo->coords || geo->out_h < 1 || geo->out_w < 1) return LERF_EINVAL;
    if (geo->coords_dtype != LERF_F32 && geo->coords_dtype != LERF_F64) return LERF_EINVAL;
    const size_t entry = geo->coords_dtype == LERF_F32 ? 8 : 16;               // one aligned load per entry
    if ((size_t)(uintptr_t)geo->coords % entry != 0 || (geo->row_stride & 1) || geo->row_stride < 2 * (int64_t)geo->out_w) return LERF_EINVAL;
    if (geo->pad_mode < LERF_PAD_CONSTANT || geo->pad_mode > LERF_PAD_WRAP) return LERF_EINVAL;
    // explicit low pads: what calc_pad_sz can yield for a clipped point, 0 .. ceil(S / 2) (the field of view starts at >= -S/2)
    for (int p : {geo->pad_r_lo, geo->pad_c_lo})
        if (p != LERF_REMAP_PADS_FROM_MAP && (p < 0 || p > LERF_MAX_SUPPORT)) return LERF_EINVAL;
    m.S = geo->S; m.oH = geo->out_h; m.oW = geo->out_w;
    m.coords = geo->coords; m.f32 = geo->coords_dtype == LERF_F32; m.stride = geo->row_stride;
    m.pad_r_lo = geo->pad_r_lo; m.pad_c_lo = geo->pad_c_lo; m.pad_mode = geo->pad_mode;
    m.map_stride = 0; m.ppm = 1;
    return LERF_OK;
}

// the same for `n_maps` maps, `map_stride` elements apart, geo describing map 0 (the *_batched entry points): `count` planes or
// frames, `ppm` of them per map.  An even stride keeps every map's entries aligned like map 0's (an entry is two elements); maps
// may not overlap.  One map: the stride is checked and then not used -- the call is the plain entry point's
inline int remap_geo_batched(const lerf_remap_geo_t* geo, int n_maps, int64_t map_stride, int count, int ppm, RemapGeo& m) {
    const int rc = remap_geo(geo, m);
    if (rc != LERF_OK) return rc;
    if (n_maps < 1 || ppm < 1 || count < 1 || count % n_maps != 0 || (int64_t)n_maps * ppm != count) return LERF_EINVAL;
    const size_t elem = geo->coords_dtype == LERF_F32 ? 4 : 8;
    if (map_stride < 0 || (map_stride & 1) || ((size_t)map_stride * elem) % (2 * elem) != 0) return LERF_EINVAL;
    if (n_maps > 1) {
        if (map_stride < (int64_t)(geo->out_h - 1) * geo->row_stride + 2 * (int64_t)geo->out_w) return LERF_EINVAL;
        m.map_stride = map_stride; m.ppm = ppm;
    }
    return LERF_OK;
}

}  // namespace lerf
