// Host-side geometry of the LeRF path, free of any HIP dependency: what lerf_api.hip exports as lerf_sr_axis_tables(_f32),
// lerf_out_size, lerf_invert3x3, lerf_warp_pads, lerf_mode_offsets, and the helpers the kernels share with it (pattern
// offsets, image pad rule, homography projection, support boundary, the one source-index rule of every resampler's taps,
// source_tap, and the homographic warp's tap geometry built on it: warp_pixel + axis_tap, which every warp kernel, its tie
// guard and the tile-fused warp's ownership key derive their taps from).  One source for both builds: liblerf_hip.so (hipcc)
// and the AddressSanitizer / UBSan host build of the same functions (csrc/lerf_host_sanitize.cpp, `make asan`), which the
// CPU suite runs against the product library (tests/test_sanitizers_cpu.py).
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "lerf_hip.h"

#ifdef __HIPCC__
#define LERF_HD __host__ __device__
#else
#define LERF_HD
#endif

namespace lerf {

constexpr float kEps32 = 1.1920928955078125e-07f;  // np.finfo(np.float32).eps

LERF_HD inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Sampling patterns of resample/eval_lut_sr.py:30-81, (dy, dx) of pixels a,b,c,d.
LERF_HD constexpr bool mode_pattern(char mode, int8_t dy[4], int8_t dx[4]) {
    dy[0] = 0; dx[0] = 0;
    switch (mode) {
        case 's': dy[1] = 0; dx[1] = 1; dy[2] = 1; dx[2] = 0; dy[3] = 1; dx[3] = 1; return true;
        case 'd': dy[1] = 0; dx[1] = 2; dy[2] = 2; dx[2] = 0; dy[3] = 2; dx[3] = 2; return true;
        case 'y': dy[1] = 1; dx[1] = 1; dy[2] = 1; dx[2] = 2; dy[3] = 2; dx[3] = 1; return true;
        case 'c': dy[1] = 0; dx[1] = 1; dy[2] = 0; dx[2] = 2; dy[3] = 0; dx[3] = 3; return true;
        case 't': dy[1] = 1; dx[1] = 1; dy[2] = 2; dx[2] = 2; dy[3] = 3; dx[3] = 3; return true;
        default: return false;
    }
}

// np.rot90(img, r) + bottom/right edge pad + pattern + rot90 back
// == offsets rotated r times by (dy,dx)->(dx,-dy) with clamped coordinates.
LERF_HD constexpr bool mode_offsets(char mode, int rot, int8_t dy[4], int8_t dx[4]) {
    if (!mode_pattern(mode, dy, dx)) return false;
    rot &= 3;
    for (int k = 0; k < 4; ++k)
        for (int r = 0; r < rot; ++r) {
            int8_t t = dy[k];
            dy[k] = dx[k];
            dx[k] = (int8_t)(-t);
        }
    return true;
}

// Homography projection of output pixel (row i, col j) in float64, operation
// order of resize_right/resize_right2d_numpy.py:321-339 (no FMA contraction).
// project_unclipped: the products, sums and two divisions (:327-335), the one copy of them -- the warp kernels clip the
// result (project_point), the coordinate-map builders store it as it is (lerf_coords_models.h).
LERF_HD inline void project_unclipped(const double* m, int i, int j, double* row, double* col) {
#pragma clang fp contract(off)
    double x = (double)j, y = (double)i;
    double X = m[0] * x + m[1] * y + m[2];
    double Y = m[3] * x + m[4] * y + m[5];
    double Wh = m[6] * x + m[7] * y + m[8];
    X = X / Wh;
    Y = Y / Wh;
    *row = Y;
    *col = X;
}

LERF_HD inline void project_point(const double* m, int i, int j, int H, int W, double* gr, double* gc) {
    double r, c;
    project_unclipped(m, i, j, &r, &c);
    r = r < 0.0 ? 0.0 : (r > (double)H ? (double)H : r);
    c = c < 0.0 ? 0.0 : (c > (double)W ? (double)W : c);
    *gr = r;
    *gc = c;
}

LERF_HD inline int left_boundary(double g, int S) {
#pragma clang fp contract(off)
    return (int)ceil(g - (double)S / 2 - (double)kEps32);
}


// Exact x2 SR geometry (scale 2.0, n_out = 2 n_in) in closed form: what sr_axis_tables (below) computes for that case, without
// a table.  g = i / 2 - 1 / 4 exactly, so output i has first tap (i + 1) / 2 - S / 2 and tap k lies at distance
// S / 2 - k - 1 / 4 (even i) or S / 2 - k - 3 / 4 (odd i): exact binary fractions, the same bits in float32 and float64.  The
// X2 flavour of the tile-fused kernels (lerf_fused_impl.h) takes its geometry from here; host::sr_x2_exact checks a pair of
// tables against it and tests/test_x2_geometry_cpu.py pins the two against each other.
LERF_HD inline int x2_left(int i, int S) { return ((i + 1) >> 1) - S / 2; }
LERF_HD inline double x2_dis(int i, int k, int S) { return (double)(S / 2 - k) - ((i & 1) ? 0.75 : 0.25); }
// outputs [o0, o1) owned by tile ti of tn along one axis (LR pixels [t0, t0 + tpx) of the whole frame): those whose first
// tap lies in [t0 - S / 2, t0 + tpx - S / 2), the first and the last tile taking what lies beyond the frame's borders --
// the lower bounds the table kernels search for
LERF_HD inline void x2_owned(int ti, int tn, int t0, int tpx, int n_out, int* o0, int* o1) {
    *o0 = ti == 0 ? 0 : 2 * t0 - 1;
    *o1 = ti == tn - 1 ? n_out : 2 * (t0 + tpx) - 1;
}

// Source index of padded position i (unpadded coordinates, may lie outside [0, n)) under the padding rule of the IMAGE
// operand: np.pad(input, pad_vec, mode=self.pad_mode) (resize_right/resize_right2d_numpy.py:208, :560) /
// F.pad(input, pad_vec, mode=self.pad_mode) (resize_right2d_torch.py:189, :362).  *zero: the value is 0 (constant).
// reflect / symmetric / wrap follow numpy for any pad width (periodic extension).
LERF_HD inline int pad_index(int i, int n, int mode, bool* zero) {
    *zero = false;
    if (i >= 0 && i < n) return i;
    if (mode == 1) return i < 0 ? 0 : n - 1;                          // edge / replicate
    if (mode == 2) {                                                  // reflect (no edge repeat)
        const int p = 2 * (n - 1);
        if (p == 0) return 0;
        const int m = ((i % p) + p) % p;
        return m < n ? m : p - m;
    }
    if (mode == 3) {                                                  // symmetric (edge repeated)
        const int p = 2 * n;
        const int m = ((i % p) + p) % p;
        return m < n ? m : p - 1 - m;
    }
    if (mode == 4) return ((i % n) + n) % n;                          // wrap / circular
    *zero = true;                                                     // constant (0)
    return i < 0 ? 0 : n - 1;
}

// Warp2dNumpy.set_shape / get_distance (resize_right2d_numpy.py:321-407): output pixel (i, j) of the homographic warp in
// padded coordinates.  The projected point is clipped to [0, in] and shifted by the low pads (calc_pad_sz, :366-367); lr, lc
// are the support's left boundary.
struct WarpPixel {
    double gr, gc;      // projected point (padded coordinates)
    int lr, lc;         // left boundary of the support (padded coordinates)
};

// ... of a point (gr, gc) already clipped to [0, H] x [0, W]: the one place where a source position becomes a WarpPixel,
// whatever produced it (a homography: warp_pixel; a dense coordinate map: remap_pixel).
LERF_HD inline WarpPixel pixel_of_point(double gr, double gc, int S, int pad_r_lo, int pad_c_lo) {
    WarpPixel p;
    p.gr = gr;
    p.gc = gc;
    p.lr = left_boundary(p.gr, S) + pad_r_lo;
    p.lc = left_boundary(p.gc, S) + pad_c_lo;
    p.gr += (double)pad_r_lo;
    p.gc += (double)pad_c_lo;
    return p;
}

LERF_HD inline WarpPixel warp_pixel(const double minv[9], int S, int pad_r_lo, int pad_c_lo, int i, int j, int H, int W) {
    double gr, gc;
    project_point(minv, i, j, H, W, &gr, &gc);
    return pixel_of_point(gr, gc, S, pad_r_lo, pad_c_lo);
}

// Remap: the projected grid is read from a dense coordinate map instead of being projected -- entry (i, j) = (row, col) of the
// source position of output pixel (i, j), in the coordinates get_projected_grid2d holds BEFORE its clip (:335).  clip_coord is
// that clip (:338-339) in a form no value can escape: -inf -> 0, +inf -> n, and NaN -> 0 (a NaN entry is never resampled --
// the kernels write 0 / NaN for it -- but nothing downstream of this line can see a value outside [0, n]).
LERF_HD inline double clip_coord(double v, int n) { return !(v >= 0.0) ? 0.0 : (v > (double)n ? (double)n : v); }

LERF_HD inline WarpPixel remap_pixel(double row, double col, int S, int pad_r_lo, int pad_c_lo, int H, int W) {
    return pixel_of_point(clip_coord(row, H), clip_coord(col, W), S, pad_r_lo, pad_c_lo);
}

// calc_pad_sz's low pad (:365) of one axis from the map's FIRST entry: max(-left_boundary(clip(map[0, 0])), 0)
LERF_HD inline int remap_pad_lo(double v0, int n, int S) {
    const int l = left_boundary(clip_coord(v0, n), S);
    return -l > 0 ? -l : 0;
}

// Unpadded source coordinate s of a tap along one axis of n pixels (may lie outside [0, n)): where the replicate-padded
// hyper-parameter maps are read (:172-174) and where the image is read under its pad rule (:208, :560).  The one source-index
// rule of every resampler: the SR taps (SrTap, lerf_taps.h) and, through axis_tap, the warp's.
struct SourceTap {
    int cl;             // clamped source index: where the replicate-padded hyper-parameter maps are read
    bool inside;        // the tap lies inside the frame (the packed warps take the image as 0 outside it)
    int s;              // image index under the image's pad rule
    bool z;             // the image value is the constant pad (0)
};

LERF_HD inline SourceTap source_tap(int s, int n, int pad_mode) {
    SourceTap t;
    t.cl = clampi(s, 0, n - 1);
    t.inside = s == t.cl;
    t.s = pad_index(s, n, pad_mode, &t.z);
    return t;
}

// Tap k of the warp's support along one axis (rows: g = gr, l = lr, n = H, the row pads; columns likewise).  The taps are
// separable: a row tap depends on the row offset alone, a column tap on the column offset alone.
struct AxisTap : SourceTap {
    double d;           // float64 distance of the projected point from the tap
};

LERF_HD inline AxisTap axis_tap(double g, int l, int k, int n, int pad_lo, int pad_mode) {
    AxisTap t;
    const int p = clampi(l + k, 0, n - 1);      // field of view clipped to [0, in-1] while indexing the PADDED arrays (:396-398)
    t.d = g - (double)p;
    const SourceTap s = source_tap(p - pad_lo, n, pad_mode);
    t.cl = s.cl;
    t.inside = s.inside;
    t.s = s.s;
    t.z = s.z;
    return t;
}


namespace host {

// float32 rounding of a float64 distance that keeps its class for the
// amplified-linear kernel's hard masks (resize_right2d_numpy.py:233-235)
inline int dclass(double x) { return (x >= -1.0 && x < 0.0) ? 1 : ((x >= 0.0 && x <= 1.0) ? 2 : 0); }
inline int fclass(float x) { return (x >= -1.0f && x < 0.0f) ? 1 : ((x >= 0.0f && x <= 1.0f) ? 2 : 0); }

inline float class_preserving_f32(double d) {
    float f = (float)d;
    int want = dclass(d);
    if (fclass(f) == want) return f;
    float up = nextafterf(f, INFINITY), dn = nextafterf(f, -INFINITY);
    if (fclass(up) == want) return up;
    if (fclass(dn) == want) return dn;
    return f;
}


inline int out_size(int n_in, double scale) { return (int)ceil(scale * (double)n_in); }

inline int sr_axis_tables(int n_in, int n_out, double scale, int S, int32_t* left, double* dis64, float* dis32,
                        int32_t* pads) {
#pragma clang fp contract(off)
    if (n_in < 1 || n_out < 1 || !(scale > 0.0) || S < 1 || S > LERF_MAX_SUPPORT || !left || !dis64) return LERF_EINVAL;
    // g = i/s + (n_in-1)/2 - (n_out-1)/(2s)            resize_right2d_numpy.py:70-79
    const double a = (double)(n_in - 1) / 2;
    const double b = (double)(n_out - 1) / (2 * scale);
    int pad_lo = 0;
    for (int i = 0; i < n_out; ++i) {
        double g = (double)i / scale + a - b;
        int l = left_boundary(g, S);                    // :85-90
        if (i == 0) pad_lo = -l;                        // :101
        left[i] = l;
        double gp = g + (double)pad_lo;                 // :103
        for (int k = 0; k < S; ++k) {
            double d = gp - (double)(l + pad_lo + k);   // :131-134
            dis64[i * S + k] = d;
            if (dis32) dis32[i * S + k] = class_preserving_f32(d);
        }
    }
    if (pads) {
        pads[0] = pad_lo;
        pads[1] = left[n_out - 1] + S - 1 - n_in + 1;   // :101
    }
    return LERF_OK;
}

inline int sr_axis_tables_f32(int n_in, int n_out, double scale, int S, int32_t* left, float* dis32, int32_t* pads) {
#pragma clang fp contract(off)
    if (n_in < 1 || n_out < 1 || !(scale > 0.0) || S < 1 || S > LERF_MAX_SUPPORT || !left || !dis32) return LERF_EINVAL;
    // Resize2dTorch.get_projected_grid2d / get_field_of_view2d / cal_pad_sz / get_distance
    // (resize_right/resize_right2d_torch.py:48-103): every tensor op is float32, the python scalars are float64
    // expressions rounded to float32 when they meet the tensor.
    const float sf = (float)scale;
    const float a = (float)((double)(n_in - 1) / 2);
    const float b = (float)((double)(n_out - 1) / (2 * scale));
    const float half = (float)((double)S / 2);
    int pad_lo = 0;
    for (int i = 0; i < n_out; ++i) {
        float g = (float)i / sf;                        // :60
        g = g + a;
        g = g - b;
        float t = g - half;                             // :69
        t = t - kEps32;
        const int l = (int)ceilf(t);
        if (i == 0) pad_lo = -l;                        // :81
        left[i] = l;
        const float gp = g + (float)pad_lo;             // :83
        for (int k = 0; k < S; ++k) dis32[i * S + k] = gp - (float)(l + pad_lo + k);      // :98
    }
    if (pads) {
        pads[0] = pad_lo;
        pads[1] = left[n_out - 1] + S - 1 - n_in + 1;   // :81
    }
    return LERF_OK;
}

// the closed form as tables (any of the three may be NULL)
inline int sr_x2_tables(int n_out, int S, int32_t* left, double* dis64, float* dis32) {
    if (n_out < 1 || S < 1 || S > LERF_MAX_SUPPORT || (S & 1)) return LERF_EINVAL;
    for (int i = 0; i < n_out; ++i) {
        if (left) left[i] = x2_left(i, S);
        for (int k = 0; k < S; ++k) {
            if (dis64) dis64[i * S + k] = x2_dis(i, k, S);
            if (dis32) dis32[i * S + k] = (float)x2_dis(i, k, S);
        }
    }
    return LERF_OK;
}

// 1: the tables of one axis ARE the exact x2 tables -- scale 2.0, n_out = 2 n_in, every entry the closed form bit for bit
inline int sr_x2_exact(int n_in, int n_out, double scale, int S, const int32_t* left, const double* dis64, const float* dis32) {
    if (n_in < 1 || S < 1 || S > LERF_MAX_SUPPORT || (S & 1) || !left || !dis64 || !dis32) return 0;
    if (scale != 2.0 || (int64_t)n_out != 2 * (int64_t)n_in) return 0;
    for (int i = 0; i < n_out; ++i) {
        if (left[i] != x2_left(i, S)) return 0;
        for (int k = 0; k < S; ++k) {
            const double d = x2_dis(i, k, S);
            const float f = (float)d;
            if (memcmp(&dis64[i * S + k], &d, sizeof d) != 0 || memcmp(&dis32[i * S + k], &f, sizeof f) != 0) return 0;
        }
    }
    return 1;
}

// the owned output ranges of every tile of `tile` LR pixels along one axis: ranges[2 t] .. ranges[2 t + 1] (half open)
inline int sr_x2_owned(int n_in, int tile, int32_t* ranges) {
    if (n_in < 1 || tile < 1 || !ranges) return LERF_EINVAL;
    const int tn = (n_in + tile - 1) / tile;
    for (int t = 0; t < tn; ++t) x2_owned(t, tn, t * tile, tile, 2 * n_in, &ranges[2 * t], &ranges[2 * t + 1]);
    return LERF_OK;
}

// the builder's verdict on the tables of both axes: LERF_GEO_EXACT_X2 or 0
inline int sr_geometry_flags(int H, int W, int out_h, int out_w, double scale_h, double scale_w, int S, const int32_t* left_r,
                             const double* dis_r64, const float* dis_r32, const int32_t* left_c, const double* dis_c64,
                             const float* dis_c32) {
    return sr_x2_exact(H, out_h, scale_h, S, left_r, dis_r64, dis_r32) && sr_x2_exact(W, out_w, scale_w, S, left_c, dis_c64, dis_c32)
               ? LERF_GEO_EXACT_X2 : 0;
}

inline int invert3x3(const double m[9], double out[9]) {
    if (!m || !out) return LERF_EINVAL;
    double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
    if (det == 0.0) return LERF_EINVAL;
    out[0] = c00 / det;
    out[1] = (m[2] * m[7] - m[1] * m[8]) / det;
    out[2] = (m[1] * m[5] - m[2] * m[4]) / det;
    out[3] = c01 / det;
    out[4] = (m[0] * m[8] - m[2] * m[6]) / det;
    out[5] = (m[2] * m[3] - m[0] * m[5]) / det;
    out[6] = c02 / det;
    out[7] = (m[1] * m[6] - m[0] * m[7]) / det;
    out[8] = (m[0] * m[4] - m[1] * m[3]) / det;
    return LERF_OK;
}

inline int warp_pads(const double minv[9], int in_h, int in_w, int out_h, int out_w, int S, int32_t pads[4]) {
    if (!minv || !pads || in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1 || S < 1) return LERF_EINVAL;
    double gr, gc;
    project_point(minv, 0, 0, in_h, in_w, &gr, &gc);
    int l0r = left_boundary(gr, S), l0c = left_boundary(gc, S);
    project_point(minv, out_h - 1, out_w - 1, in_h, in_w, &gr, &gc);
    int l1r = left_boundary(gr, S), l1c = left_boundary(gc, S);
    // calc_pad_sz: (max(-fov[0,0],0), max(fov[-1,-1]-in+1,0)), fov[-1,-1] = left + S-1   (:363-366)
    pads[0] = -l0r > 0 ? -l0r : 0;
    pads[1] = (l1r + S - 1 - in_h + 1) > 0 ? (l1r + S - 1 - in_h + 1) : 0;
    pads[2] = -l0c > 0 ? -l0c : 0;
    pads[3] = (l1c + S - 1 - in_w + 1) > 0 ? (l1c + S - 1 - in_w + 1) : 0;
    return LERF_OK;
}

// Host mirror of what the remap kernels derive from a coordinate map in HOST memory (lerf_remap_host_geometry): the low pads
// (geo->pad_*_lo, or remap_pad_lo of the map's first entry) and, per output pixel, remap_pixel's gr, gc, lr, lc.
inline int remap_geometry(const lerf_remap_geo_t* geo, int H, int W, double* gr, double* gc, int32_t* lr, int32_t* lc, int32_t pads[2]) {
    if (!geo || !geo->coords || H < 1 || W < 1 || geo->out_h < 1 || geo->out_w < 1 || geo->S < 1 || geo->S > LERF_MAX_SUPPORT) return LERF_EINVAL;
    if ((geo->coords_dtype != LERF_F32 && geo->coords_dtype != LERF_F64) || geo->row_stride < 2 * (int64_t)geo->out_w) return LERF_EINVAL;
    auto entry = [&](int i, int j, int k) -> double {
        const int64_t o = (int64_t)i * geo->row_stride + 2 * (int64_t)j + k;
        return geo->coords_dtype == LERF_F32 ? (double)((const float*)geo->coords)[o] : ((const double*)geo->coords)[o];
    };
    const int pr = geo->pad_r_lo < 0 ? remap_pad_lo(entry(0, 0, 0), H, geo->S) : geo->pad_r_lo;
    const int pc = geo->pad_c_lo < 0 ? remap_pad_lo(entry(0, 0, 1), W, geo->S) : geo->pad_c_lo;
    if (pads) { pads[0] = pr; pads[1] = pc; }
    for (int i = 0; i < geo->out_h; ++i)
        for (int j = 0; j < geo->out_w; ++j) {
            const WarpPixel p = remap_pixel(entry(i, j, 0), entry(i, j, 1), geo->S, pr, pc, H, W);
            const int64_t o = (int64_t)i * geo->out_w + j;
            if (gr) gr[o] = p.gr;
            if (gc) gc[o] = p.gc;
            if (lr) lr[o] = p.lr;
            if (lc) lc[o] = p.lc;
        }
    return LERF_OK;
}

// Tile-fused warp (lerf_warp_fused_u8): a source tile of 64 x 64 pixels OWNS the output pixels whose support (2 x 2 taps,
// clamped into the frame like the reference clips its field of view, resize_right2d_numpy.py:396-398) has its LAST tap row /
// column inside the tile: key = min(first tap + 1, n - 1).  Both taps then lie in the tile or in the ring of one pixel above /
// left of it, which the tile's stage-2 region holds.  (Pixels projected outside the frame are clipped onto its border and belong
// to the border tiles.)
LERF_HD inline void warp_owner_key(const double minv[9], int pad_r_lo, int pad_c_lo, int i, int j, int H, int W, int* key_r, int* key_c) {
    const WarpPixel p = warp_pixel(minv, 2, pad_r_lo, pad_c_lo, i, j, H, W);
    const int r0 = axis_tap(p.gr, p.lr, 0, H, pad_r_lo, LERF_PAD_CONSTANT).cl, c0 = axis_tap(p.gc, p.lc, 0, W, pad_c_lo, LERF_PAD_CONSTANT).cl;
    *key_r = r0 + 1 < H - 1 ? r0 + 1 : H - 1;
    *key_c = c0 + 1 < W - 1 ? c0 + 1 : W - 1;
}

// boxes[t] = {i0, i1, j0, j1}: output rows [i0, i1) x columns [j0, j1) that contain every pixel tile t (row-major tiles of
// `tile` x `tile` source pixels) owns, widened by 2 pixels (the kernel decides ownership itself, pixel by pixel, with the
// same formula; the boxes only bound its search).  One pass over the output on the host, once per homography.
inline int warp_tile_boxes(const double minv[9], int pad_r_lo, int pad_c_lo, int H, int W, int oH, int oW, int tile, int32_t* boxes) {
    if (!minv || !boxes || H < 1 || W < 1 || oH < 1 || oW < 1 || tile < 1) return LERF_EINVAL;
    const int ty = (H + tile - 1) / tile, tx = (W + tile - 1) / tile;
    for (int t = 0; t < ty * tx; ++t) { boxes[4 * t] = oH; boxes[4 * t + 1] = -1; boxes[4 * t + 2] = oW; boxes[4 * t + 3] = -1; }
    for (int i = 0; i < oH; ++i)
        for (int j = 0; j < oW; ++j) {
            int kr, kc;
            warp_owner_key(minv, pad_r_lo, pad_c_lo, i, j, H, W, &kr, &kc);
            int32_t* b = boxes + 4 * ((kr / tile) * tx + kc / tile);
            if (i < b[0]) b[0] = i;
            if (i > b[1]) b[1] = i;
            if (j < b[2]) b[2] = j;
            if (j > b[3]) b[3] = j;
        }
    for (int t = 0; t < ty * tx; ++t) {
        int32_t* b = boxes + 4 * t;
        if (b[1] < 0) { b[0] = b[1] = b[2] = b[3] = 0; continue; }
        b[0] = b[0] - 2 > 0 ? b[0] - 2 : 0;
        b[1] = b[1] + 3 < oH ? b[1] + 3 : oH;
        b[2] = b[2] - 2 > 0 ? b[2] - 2 : 0;
        b[3] = b[3] + 3 < oW ? b[3] + 3 : oW;
    }
    return LERF_OK;
}

// Adjoint table of one axis pass of the separable resize (lerf_rr_axis): for every source index s of the n_in inputs the
// outputs j that read it and their weights, CSR: row_ptr[n_in + 1], idx[nnz] = j, wt[nnz] = w[j][k], entries of one source
// in (j, k) order.  A padded tap of a non-constant pad mode folds onto the source index the pad rule names (source_tap);
// a tap in a constant pad has no source and is dropped.  w / wt: float32 or float64 (w_dtype), idx and wt sized for
// n_out * taps entries.  Returns nnz, or a negative LERF_E* code.
inline int rr_adjoint_csr(int n_in, int n_out, int taps, const int32_t* left, const void* w, int w_dtype, int pad_mode,
                          int32_t* row_ptr, int32_t* idx, void* wt) {
    if (n_in < 1 || n_out < 1 || taps < 1 || !left || !w || !row_ptr || !idx || !wt) return LERF_EINVAL;
    if (w_dtype != LERF_F32 && w_dtype != LERF_F64) return LERF_EINVAL;
    if (pad_mode < LERF_PAD_CONSTANT || pad_mode > LERF_PAD_WRAP) return LERF_EINVAL;
    if ((int64_t)n_out * taps > 0x7fffffff) return LERF_EUNSUPPORTED;
    for (int s = 0; s <= n_in; ++s) row_ptr[s] = 0;
    for (int j = 0; j < n_out; ++j)
        for (int k = 0; k < taps; ++k) {
            const SourceTap t = source_tap(left[j] + k, n_in, pad_mode);
            if (!t.z) ++row_ptr[t.s + 1];
        }
    for (int s = 0; s < n_in; ++s) row_ptr[s + 1] += row_ptr[s];
    const int nnz = row_ptr[n_in];
    for (int j = 0; j < n_out; ++j)                     // row_ptr[s] serves as the cursor of source s ...
        for (int k = 0; k < taps; ++k) {
            const SourceTap t = source_tap(left[j] + k, n_in, pad_mode);
            if (t.z) continue;
            const int e = row_ptr[t.s]++;
            idx[e] = j;
            if (w_dtype == LERF_F64) ((double*)wt)[e] = ((const double*)w)[(int64_t)j * taps + k];
            else ((float*)wt)[e] = ((const float*)w)[(int64_t)j * taps + k];
        }
    for (int s = n_in; s > 0; --s) row_ptr[s] = row_ptr[s - 1];      // ... and now holds the start of s + 1: shift back
    row_ptr[0] = 0;
    return nnz;
}

}  // namespace host
}  // namespace lerf
