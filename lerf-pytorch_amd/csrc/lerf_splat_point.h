// Arithmetic of the forward warp by summation splatting (lerf_splat / lerf_splat_bwd in lerf_coords.hip), HIP-free on the host side:
// one source for the kernels and for the host twins, like lerf_coords_models.h.  Float64, only + - * /, floor, comparisons and
// selects, FMA contraction off.  A float32 operand is promoted exactly; a value is rounded to the image dtype T ONCE, where it is
// added (forward) or stored (backward).
//
// The operands of one source pixel (i, j) of set s: its values x_k (k < C), its weight m (1.0 when no weight plane is given) and its
// entry (r, c) of the forward map F -- the position in the [oH][oW] output frame at which it lands (invert_raster reads F the same way).
//
//   axis (splat_axis; rows: v = r, n = oH.  v is finite: the caller has tested it)
//                 f = floor(v),  t = v - f,  w[0] = 1 - t,  w[1] = t                      (0 <= t <= 1; t == 1 only by rounding)
//                 in[a] = (f + a >= 0 and f + a <= (double)(n - 1)), a = 0, 1       -- the frame test, in floating point
//                 i0 = (int)f if in[0] or in[1] (then -1 <= f <= n - 1), else 0     -- the ONLY conversion to int, after the test:
//                 1e300 forms no address and overflows nothing (clip_coord's rule)
//   forward (splat_point)
//                 r or c not finite (v - v != 0: NaN, +-inf): nothing is read, nothing is added, no address is formed ("no target",
//                 the mirror of remap's "no source")
//                 R = splat_axis(r, oH),  Cx = splat_axis(c, oW)
//                 taps t = 2a + b in the order (0,0) (0,1) (1,0) (1,1), pixel q = (R.i0 + a, Cx.i0 + b):
//                   on[t] = R.w[a] != 0 and Cx.w[b] != 0 and R.in[a] and Cx.in[b]
//                   a tap with a zero weight is SKIPPED (an integer position touches one pixel, r = oH - 1 is inside the frame);
//                   a tap outside [0, oH) x [0, oW) is DROPPED, NOT CLIPPED: mass that leaves the frame is lost (compose_axis clamps;
//                   this does not)
//                   wm[t] = (R.w[a] * Cx.w[b]) * m
//                 for k = 0 .. C - 1:  xk = x_k;  for every tap that is on, in tap order:  acc[k][q] += round_T(wm[t] * xk)
//                 with the norm plane:           for every tap that is on, in tap order:  acc[C][q] += round_T(wm[t])
//                 The add itself is in T.  acc is ACCUMULATED INTO (the caller zeroes it; several frames may be splatted into one
//                 canvas by consecutive calls).  Host: source pixels in row-major order, a plain add.  Device: one no-return atomic
//                 add per tap and plane -- equal up to the rounding of a reordered sum in T.
//   backward (splat_bwd_point)   upstream G [C (+ 1)][oH][oW] of dtype T, promoted exactly.  ONE writer per source pixel, every sum starts at
//                 +0.0 and adds its terms in the stated order, a term that is skipped is not added: pure gather, no atomics, so the
//                 device equals the host bit for bit and from run to run.  The three results are STORED (not accumulated), rounded
//                 once to their dtype at the store.
//                 r or c not finite: grad_X[k] = 0 for every k, grad_M = 0, grad_F = (0, 0), whatever G holds (a select; nothing of G is
//                 read) -- the non-finite rule of compose_bwd_point and model_point_bwd
//                 R, Cx, on[t], w[t] = R.w[a] * Cx.w[b] as in the forward;  inside[t] = R.in[a] and Cx.in[b]
//                 G is read at a corner t when inside[t] and (on[t] or grad_F is wanted); any other corner reads as 0 and forms no address
//                 for k = 0 .. C - 1:  g[t] = G[k][q_t]
//                   grad_X[k] = m * (sum over the taps that are on, in tap order, of w[t] * g[t])
//                   S[t] = S[t] + x_k * g[t]                                                       (when grad_M or grad_F is wanted)
//                 with the norm plane:  S[t] = S[t] + G[C][q_t]
//                 grad_M   = sum over the taps that are on, in tap order, of w[t] * S[t]
//                 grad_F.r = m * (sum over b = 0, 1 with Cx.w[b] != 0 of Cx.w[b] * (S[(1,b)] - S[(0,b)]))
//                 grad_F.c = m * (sum over a = 0, 1 with R.w[a] != 0 of R.w[a] * (S[(a,1)] - S[(a,0)]))
//                 grad_F is the derivative of the bilinear cell that floor picked, with S = 0 outside the frame: at an integer position
//                 it is ONE-SIDED, the derivative of the cell [f, f + 1] (towards +), and it reads S at f + 1 although the forward
//                 skipped that tap.  Across the frame's edge the forward is not continuous (mass is dropped); the formula is the
//                 derivative of the side the position is on.
#pragma once

#include "lerf_coords_models.h"

namespace lerf {
namespace coords {

struct SplatAxis {
    int i0;
    double w[2];
    bool in[2];
};

// v finite
LERF_HD inline SplatAxis splat_axis(double v, int n) {
#pragma clang fp contract(off)
    SplatAxis x;
    const double f = floor(v), last = (double)(n - 1);
    const double t = v - f;
    x.w[0] = 1.0 - t;
    x.w[1] = t;
    x.in[0] = f >= 0.0 && f <= last;
    x.in[1] = f + 1.0 >= 0.0 && f + 1.0 <= last;
    x.i0 = (x.in[0] || x.in[1]) ? (int)f : 0;
    return x;
}

// the four taps of one source pixel: which count, their weights and their pixels q = row * oW + col
struct SplatTaps {
    bool on[4], inside[4];
    double w[4];
    int64_t q[4];
    bool any_on, any_inside;
};

LERF_HD inline SplatTaps splat_taps(const SplatAxis& R, const SplatAxis& Cx, int oW) {
#pragma clang fp contract(off)
    SplatTaps T;
    T.any_on = T.any_inside = false;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int t = 2 * a + b;
            T.inside[t] = R.in[a] && Cx.in[b];
            T.on[t] = T.inside[t] && R.w[a] != 0.0 && Cx.w[b] != 0.0;
            T.w[t] = R.w[a] * Cx.w[b];
            T.q[t] = T.inside[t] ? (int64_t)(R.i0 + a) * oW + (Cx.i0 + b) : 0;
            T.any_on = T.any_on || T.on[t];
            T.any_inside = T.any_inside || T.inside[t];
        }
    return T;
}

// XLOAD(k) -> double: x_k of this source pixel; ADD(k, q, v): acc[k][q] += round_T(v), called only for taps that are on
template <typename XLOAD, typename ADD>
LERF_HD inline void splat_point(Point p, double m, int C, bool norm, int oH, int oW, XLOAD x, ADD add) {
#pragma clang fp contract(off)
    if (!finite_value(p.r) || !finite_value(p.c)) return;
    const SplatTaps T = splat_taps(splat_axis(p.r, oH), splat_axis(p.c, oW), oW);
    if (!T.any_on) return;
    double wm[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) wm[t] = T.w[t] * m;
    for (int k = 0; k < C; ++k) {
        const double xk = x(k);
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (T.on[t]) add(k, T.q[t], wm[t] * xk);
    }
    if (norm) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (T.on[t]) add(C, T.q[t], wm[t]);
    }
}

struct SplatGrad {
    double m;      // grad_M
    Point f;       // grad_F
};

// XLOAD(k) -> double; GLOAD(k, q) -> double: G[k][q]; GX(k, v): grad_X[k] = round_T(v), called for every k when want_x
template <typename XLOAD, typename GLOAD, typename GX>
LERF_HD inline SplatGrad splat_bwd_point(Point p, double m, int C, bool norm, int oH, int oW, bool want_x, bool want_m, bool want_f, XLOAD x,
                                         GLOAD g, GX gx) {
#pragma clang fp contract(off)
    SplatGrad out{0.0, {0.0, 0.0}};
    if (!finite_value(p.r) || !finite_value(p.c)) {
        if (want_x)
            for (int k = 0; k < C; ++k) gx(k, 0.0);
        return out;
    }
    const SplatAxis R = splat_axis(p.r, oH), Cx = splat_axis(p.c, oW);
    const SplatTaps T = splat_taps(R, Cx, oW);
    const bool want_s = want_m || want_f;
    bool read[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) read[t] = T.inside[t] && (T.on[t] || want_f);
    double S[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < C; ++k) {
        double gk[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) gk[t] = read[t] ? g(k, T.q[t]) : 0.0;
        if (want_x) {
            double s = 0.0;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (T.on[t]) s = s + T.w[t] * gk[t];
            gx(k, m * s);
        }
        if (want_s) {
            const double xk = x(k);
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (read[t]) S[t] = S[t] + xk * gk[t];
        }
    }
    if (!want_s) return out;
    if (norm) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (read[t]) S[t] = S[t] + g(C, T.q[t]);
    }
    double sm = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (T.on[t]) sm = sm + T.w[t] * S[t];
    out.m = sm;
    double dr = 0.0, dc = 0.0;
#pragma unroll
    for (int b = 0; b < 2; ++b)
        if (Cx.w[b] != 0.0) dr = dr + Cx.w[b] * (S[2 + b] - S[b]);
#pragma unroll
    for (int a = 0; a < 2; ++a)
        if (R.w[a] != 0.0) dc = dc + R.w[a] * (S[2 * a + 1] - S[2 * a]);
    out.f = {m * dr, m * dc};
    return out;
}

}  // namespace coords
}  // namespace lerf
