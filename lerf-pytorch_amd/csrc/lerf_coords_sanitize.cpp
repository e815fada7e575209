// Stand-alone sanitizer driver of the HOST twins of the coordinate maps (`make asan-coords`): lerf_coords.hip is compiled with
// AddressSanitizer + UndefinedBehaviorSanitizer on its host side and linked with this main, which calls lerf_coords_build_host,
// lerf_coords_build_bwd_host and lerf_coords_math_host (the fisheye and equirect models, the special arguments of the helpers) and
// lerf_coords_{mesh,compose,invert,compose_bwd,invert_bwd}_host on exactly-sized heap buffers -- strided tiles with an origin, both
// dtypes of every operand, a batch of sets, init and the gradient halves null and given, the refusals -- and lerf_coords_invert_raster_host
// on a folded map with NaN, +-inf and 1e300 entries, tiles at a non-zero origin, max_span 1 and 64.  The host twins of the six
// run the very functors the device runs (OnHost, ScatterOnHost in lerf_coords.hip), so this pass checks the addressing of the shared code.
// It needs no GPU and is never loaded into another process.  Exit status 0 and "ok" on the last line: no report.
#include "lerf_hip.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

static int fails = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { ++fails; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } \
    } while (0)

// a map [h][w][2] of one dtype in a heap buffer of exactly the bytes a tile of row stride 2 * (w + pad) spans
struct Map {
    int dt, h, w;
    int64_t stride;
    std::vector<double> d;
    std::vector<float> f;
    Map(int dt_, int h_, int w_, int pad = 3) : dt(dt_), h(h_), w(w_), stride(2 * (int64_t)(w_ + pad)) {
        const size_t n = (size_t)((h - 1) * stride + 2 * w);
        if (dt == LERF_F64) d.assign(n, -7.0);
        else f.assign(n, -7.0f);
    }
    void* p() { return dt == LERF_F64 ? (void*)d.data() : (void*)f.data(); }
    void set(int i, int j, double r, double c) {
        const size_t e = (size_t)(i * stride + 2 * j);
        if (dt == LERF_F64) { d[e] = r; d[e + 1] = c; }
        else { f[e] = (float)r; f[e + 1] = (float)c; }
    }
    bool same(const Map& o) const {
        return d.size() == o.d.size() && f.size() == o.f.size() && (d.empty() || !std::memcmp(d.data(), o.d.data(), d.size() * sizeof(double))) &&
               (f.empty() || !std::memcmp(f.data(), o.f.data(), f.size() * sizeof(float)));
    }
};

static bool same(const std::vector<double>& a, const std::vector<double>& b) {
    return a.size() == b.size() && !std::memcmp(a.data(), b.data(), a.size() * sizeof(double));
}

// mesh, compose, invert and the two adjoints on tiles [oH][oW] at origin (3, 7): every dtype mix, then the refusals
static void entry_ops(int oH, int oW) {
    const int DT[2] = {LERF_F32, LERF_F64};
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int gh = 3, gw = 4, aH = 4, aW = 6, fH = oH + 8, fW = oW + 12;
    for (int ta : DT)
        for (int tb : DT)
            for (int to : DT) {
                Map out(to, oH, oW), keep(to, oH, oW);
                // mesh: ctrl dense [gh][gw][2] of dtype ta (tb unused: once)
                if (tb == LERF_F32) {
                    Map ctrl(ta, gh, gw, 0);
                    for (int a = 0; a < gh; ++a)
                        for (int b = 0; b < gw; ++b) ctrl.set(a, b, 10.0 * a + 0.25 * b, 7.0 * b - 0.5 * a);
                    for (int interp : {LERF_MESH_BILINEAR, LERF_MESH_BICUBIC}) {
                        EXPECT(lerf_coords_mesh_host(ctrl.p(), ta, gh, gw, interp, oH + 5, oW + 8, out.p(), to, out.stride, oH, oW, 3, 7) == LERF_OK);
                        EXPECT(lerf_coords_mesh_host(ctrl.p(), ta, gh, gw, interp, oH + 2, oW + 8, keep.p(), to, keep.stride, oH, oW, 3, 7) == LERF_EINVAL);
                        EXPECT(lerf_coords_mesh_host(ctrl.p(), ta, 1, gw, interp, oH + 5, oW + 8, keep.p(), to, keep.stride, oH, oW, 3, 7) == LERF_EINVAL);
                    }
                    EXPECT(lerf_coords_mesh_host(ctrl.p(), ta, gh, gw, 2, oH + 5, oW + 8, keep.p(), to, keep.stride, oH, oW, 3, 7) == LERF_EINVAL);
                }
                // compose: A [aH][aW] (and a 1 x 1 A) of dtype ta sampled at B of dtype tb -- inside, on the border, outside, inf, NaN
                Map A(ta, aH, aW), A1(ta, 1, 1), B(tb, oH, oW);
                for (int i = 0; i < aH; ++i)
                    for (int j = 0; j < aW; ++j) A.set(i, j, 3.0 * i + 0.5 * j, 2.0 * j - 0.25 * i);
                A1.set(0, 0, 1.5, -2.5);
                for (int i = 0; i < oH; ++i)
                    for (int j = 0; j < oW; ++j) {
                        const int k = i * oW + j;
                        B.set(i, j, k % 11 == 3 ? nan : k % 13 == 5 ? -inf : k % 7 == 2 ? (double)(aH - 1) : 0.9 * i - 0.5,
                              k % 17 == 4 ? inf : k % 5 == 1 ? (double)(aW - 1) : 0.11 * j - 0.75);
                    }
                EXPECT(lerf_coords_compose_host(A.p(), ta, A.stride, aH, aW, B.p(), tb, B.stride, out.p(), to, out.stride, oH, oW) == LERF_OK);
                EXPECT(lerf_coords_compose_host(A1.p(), ta, A1.stride, 1, 1, B.p(), tb, B.stride, out.p(), to, out.stride, oH, oW) == LERF_OK);
                EXPECT(lerf_coords_compose_host(A.p(), ta, A.stride + 1, aH, aW, B.p(), tb, B.stride, keep.p(), to, keep.stride, oH, oW) == LERF_EINVAL);
                EXPECT(lerf_coords_compose_host(A.p(), ta, A.stride, aH, aW, B.p(), tb, 2 * (int64_t)oW - 2, keep.p(), to, keep.stride, oH, oW) == LERF_EINVAL);
                // invert: F of dtype ta, a sheared grid that covers the tile's targets; init of dtype tb, null and given
                Map F(ta, fH, fW), init(tb, oH, oW);
                for (int i = 0; i < fH; ++i)
                    for (int j = 0; j < fW; ++j) F.set(i, j, 0.9 * i + 0.05 * j - 1.0, 1.1 * j + 0.1 * i - 2.0);
                if (oH > 1) F.set(fH / 2, fW / 2, nan, 1.0);
                for (int i = 0; i < oH; ++i)
                    for (int j = 0; j < oW; ++j) init.set(i, j, (i * oW + j) % 19 == 6 ? nan : 4.0 + i, (i * oW + j) % 23 == 7 ? 1e300 : 8.0 + 0.9 * j);
                EXPECT(lerf_coords_invert_host(F.p(), ta, F.stride, fH, fW, nullptr, 0, 0, out.p(), to, out.stride, oH, oW, 3, 7, 16, 1e-9) == LERF_OK);
                EXPECT(lerf_coords_invert_host(F.p(), ta, F.stride, fH, fW, init.p(), tb, init.stride, out.p(), to, out.stride, oH, oW, 3, 7, 3, 0.0) == LERF_OK);
                EXPECT(lerf_coords_invert_host(F.p(), ta, F.stride, fH, fW, init.p(), tb, init.stride, keep.p(), to, keep.stride, oH, oW, 3, 7, 0, 1e-9) == LERF_EINVAL);
                EXPECT(lerf_coords_invert_host(F.p(), ta, F.stride, fH, 1, nullptr, 0, 0, keep.p(), to, keep.stride, oH, oW, 3, 7, 16, 1e-9) == LERF_EINVAL);
                if (tb == to) EXPECT(lerf_coords_invert_host(F.p(), ta, F.stride, fH, fW, keep.p(), tb, keep.stride, keep.p(), to, keep.stride, oH, oW, 3, 7, 16, 1e-9) == LERF_EINVAL);
                EXPECT(keep.same(Map(to, oH, oW)));
                if (to == LERF_F32) continue;
                // the adjoints: dense float64 gradients, exactly sized; B holds the inner map of compose and the inverse of invert
                std::vector<double> g((size_t)oH * oW * 2), gA((size_t)aH * aW * 2, 0.5), gB(g.size(), -0.5), gF((size_t)fH * fW * 2, 0.25);
                for (size_t k = 0; k < g.size(); ++k) g[k] = k % 29 == 9 ? nan : std::sin(0.37 * (double)k);
                const std::vector<double> gA0 = gA, gB0 = gB, gF0 = gF;
                EXPECT(lerf_coords_compose_bwd_host(A.p(), ta, A.stride, aH, aW, B.p(), tb, B.stride, g.data(), oH, oW, gA.data(), gB.data()) == LERF_OK);
                EXPECT(lerf_coords_compose_bwd_host(A.p(), ta, A.stride, aH, aW, B.p(), tb, B.stride, g.data(), oH, oW, nullptr, gB.data()) == LERF_OK);
                EXPECT(lerf_coords_compose_bwd_host(A.p(), ta, A.stride, aH, aW, B.p(), tb, B.stride, g.data(), oH, oW, gA.data(), nullptr) == LERF_OK);
                EXPECT(!same(gA, gA0) && (oH == 1 || !same(gB, gB0)));          // the 1 x 1 tile sits outside A: its inner gradient is blocked
                EXPECT(lerf_coords_invert_bwd_host(F.p(), ta, F.stride, fH, fW, B.p(), tb, B.stride, g.data(), oH, oW, gF.data()) == LERF_OK);
                gA = gA0; gB = gB0; gF = gF0;
                EXPECT(lerf_coords_compose_bwd_host(A.p(), ta, A.stride, aH, aW, B.p(), tb, B.stride, g.data(), oH, oW, nullptr, nullptr) == LERF_EINVAL);
                EXPECT(lerf_coords_compose_bwd_host(A.p(), ta, A.stride, 1, aW, B.p(), tb, B.stride, g.data(), oH, oW, gA.data(), gB.data()) == LERF_EINVAL);
                EXPECT(lerf_coords_compose_bwd_host(A.p(), ta, A.stride, aH, aW, B.p(), tb, B.stride, g.data(), oH, oW, gA.data(), g.data()) == LERF_EINVAL);
                EXPECT(lerf_coords_invert_bwd_host(F.p(), ta, F.stride, fH, fW, B.p(), tb, B.stride, g.data(), oH, oW, nullptr) == LERF_EINVAL);
                EXPECT(lerf_coords_invert_bwd_host(F.p(), ta, F.stride, 1, fW, B.p(), tb, B.stride, g.data(), oH, oW, gF.data()) == LERF_EINVAL);
                EXPECT(lerf_coords_invert_bwd_host(F.p(), ta, F.stride, fH, fW, B.p(), tb, B.stride, gF.data(), oH, oW, gF.data()) == LERF_EINVAL);
                EXPECT(same(gA, gA0) && same(gB, gB0) && same(gF, gF0));
            }
}

// the rasterising inverse: a folded map with NaN, +-inf and 1e300 entries drawn into tiles [oH][oW] at origin (3, 7) of exactly-sized
// buffers (F, depth, out, keys), every dtype mix, with and without depth, max_span 1 and 64, every orient, then the refusals
static void raster_ops(int oH, int oW) {
    const int DT[2] = {LERF_F32, LERF_F64};
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int fH = 9, fW = 70;
    for (int tf : DT)
        for (int to : DT) {
            Map F(tf, fH, fW), out(to, oH, oW), keep(to, oH, oW);
            for (int i = 0; i < fH; ++i)
                for (int j = 0; j < fW; ++j) F.set(i, j, 1.3 * i + 0.5 * std::sin(0.7 * j), 1.1 * j + 4.0 * std::sin(j / 2.5) + 0.25 * i);      // folds
            F.set(2, 5, nan, 3.0); F.set(4, 9, inf, 1.0); F.set(5, 20, 2.0, -inf); F.set(6, 30, 1e300, 1e300); F.set(1, 40, -1e300, 5.0);
            F.set(0, 0, 1e300, -1e300); F.set(fH - 1, fW - 1, nan, nan);
            std::vector<float> depth((size_t)fH * fW);
            for (size_t k = 0; k < depth.size(); ++k) depth[k] = k % 31 == 7 ? (float)nan : k % 37 == 9 ? (float)inf : 2.0f + std::sin(0.3f * (float)k);
            std::vector<uint64_t> keys((size_t)oH * oW, 5), keys0 = keys;
            for (const float* d : {(const float*)nullptr, (const float*)depth.data()})
                for (int span : {1, 4, 64})
                    for (int orient : {-1, 0, 1}) {
                        EXPECT(lerf_coords_invert_raster_host(F.p(), tf, F.stride, fH, fW, d, out.p(), to, out.stride, oH, oW, 3, 7, span, orient, keys.data()) == LERF_OK);
                        EXPECT(keys != keys0);
                    }
            // a far tile, and one that a 1e300 entry would reach if anything unclipped became an int
            EXPECT(lerf_coords_invert_raster_host(F.p(), tf, F.stride, fH, fW, depth.data(), out.p(), to, out.stride, oH, oW, 0x7fffffff - oH, 0x7fffffff - oW, 64, 0, keys.data()) == LERF_OK);
            EXPECT(keys[0] == ~(uint64_t)0);
            keys = keys0;
            const int64_t s = out.stride;
            EXPECT(lerf_coords_invert_raster_host(F.p(), tf, F.stride, fH, fW, nullptr, keep.p(), to, s, oH, oW, 3, 7, 0, 0, keys.data()) == LERF_EINVAL);
            EXPECT(lerf_coords_invert_raster_host(F.p(), tf, F.stride, fH, fW, nullptr, keep.p(), to, s, oH, oW, 3, 7, 65, 0, keys.data()) == LERF_EINVAL);
            EXPECT(lerf_coords_invert_raster_host(F.p(), tf, F.stride, fH, fW, nullptr, keep.p(), to, s, oH, oW, 3, 7, 16, 2, keys.data()) == LERF_EINVAL);
            EXPECT(lerf_coords_invert_raster_host(F.p(), tf, F.stride, fH, fW, nullptr, keep.p(), to, s, oH, oW, 3, 7, 16, 0, nullptr) == LERF_EINVAL);
            EXPECT(lerf_coords_invert_raster_host(F.p(), tf, F.stride, fH, fW, nullptr, keep.p(), to, s, oH, oW, -1, 7, 16, 0, keys.data()) == LERF_EINVAL);
            EXPECT(lerf_coords_invert_raster_host(F.p(), tf, F.stride, 1, fW, nullptr, keep.p(), to, s, oH, oW, 3, 7, 16, 0, keys.data()) == LERF_EINVAL);
            EXPECT(lerf_coords_invert_raster_host(F.p(), tf, F.stride, fH, fW, nullptr, keep.p(), to, s, oH, oW, 3, 7, 16, 0, (uint64_t*)((char*)keys.data() + 4)) == LERF_EINVAL);
            EXPECT(lerf_coords_invert_raster_host(F.p(), tf, F.stride, fH, fW, nullptr, keep.p(), to, s, oH, oW, 3, 7, 16, 0, (uint64_t*)F.p()) == LERF_EINVAL);
            EXPECT(lerf_coords_invert_raster_host(F.p(), tf, F.stride, fH, fW, (const float*)keep.p(), keep.p(), to, s, oH, oW, 3, 7, 16, 0, keys.data()) == LERF_EINVAL);
            EXPECT(keep.same(Map(to, oH, oW)) && keys == keys0);
        }
}

int main() {
    const double pi = 3.14159265358979323846;
    const double fish[17] = {1.0 / 35, 0, -27.5 / 35, 0, 1.0 / 33, -16.0 / 33, 0.001, -0.0005, 1, 61.5, 58.75, 25.25, 17.5, 0.05, -0.012, 0.004, -0.0009};
    const double view[13] = {1.0 / 64, 0, -26.0 / 64, 0, 0, -1, 0, 1.0 / 64, -18.0 / 64, 192 / (2 * pi), 96 / pi, 95.5, 47.5};      // through a pole
    const double behind[17] = {1.0 / 64, 0, -4.0 / 64, 0, 1.0 / 32, -3.0 / 32, -1.0 / 8, 0, 1, 64, 32, 4, 3, 0.05, -0.012, 0.004, -0.0009};
    struct Case { int model; const double* p; int n; };
    const Case cases[3] = {{LERF_COORDS_FISHEYE, fish, 17}, {LERF_COORDS_EQUIRECT, view, 13}, {LERF_COORDS_FISHEYE, behind, 17}};
    const int shapes[4][2] = {{1, 1}, {5, 65}, {37, 53}, {67, 257}};
    for (const Case& c : cases)
        for (const auto& hw : shapes) {
            const int oH = hw[0], oW = hw[1];
            const int64_t stride = 2 * (int64_t)(oW + 3);                                   // a tile inside a wider buffer, exactly sized
            std::vector<double> m64((size_t)((oH - 1) * stride + 2 * oW));
            std::vector<float> m32(m64.size());
            EXPECT(lerf_coords_build_host(c.model, c.p, c.n, m64.data(), LERF_F64, stride, oH, oW, 3, 7) == LERF_OK);
            EXPECT(lerf_coords_build_host(c.model, c.p, c.n, m32.data(), LERF_F32, stride, oH, oW, 3, 7) == LERF_OK);
            EXPECT(m32[0] == (float)m64[0] || (m32[0] != m32[0] && m64[0] != m64[0]));
            std::vector<double> g((size_t)2 * oH * oW * 2), ps, gp((size_t)2 * c.n, 0.0);
            for (size_t k = 0; k < g.size(); ++k) g[k] = c.p == behind && k % 97 == 5 ? std::numeric_limits<double>::quiet_NaN() : std::sin(0.37 * (double)k);
            for (int s = 0; s < 2; ++s) ps.insert(ps.end(), c.p, c.p + c.n);
            EXPECT(lerf_coords_build_bwd_host(c.model, ps.data(), 2, c.n, g.data(), oH, oW, 3, 7, gp.data()) == LERF_OK);
            EXPECT(lerf_coords_build_bwd_host(c.model, ps.data(), 1, c.n - 1, g.data(), oH, oW, 3, 7, gp.data()) == LERF_EINVAL);
            EXPECT(lerf_coords_build_host(c.model, c.p, c.n + 4, m64.data(), LERF_F64, stride, oH, oW, 0, 0) == LERF_EINVAL);
        }
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> x = {0.0, -0.0, 4.0, 4.9e-324, 1e-310, 2.2250738585072014e-308, 1.7976931348623157e308, inf, -1.0, -inf, nan,
                             0.4375, 0.6875, 1.1875, 2.4375, 1e-10, -1e-10, 1e300, -1e300, 3.0, -3.0};
    std::vector<double> y(x.rbegin(), x.rend()), out(x.size());
    for (int op = 0; op < 3; ++op) EXPECT(lerf_coords_math_host(op, x.data(), y.data(), (int64_t)x.size(), out.data()) == LERF_OK);
    EXPECT(lerf_coords_math_host(LERF_MATH_SQRT, x.data(), nullptr, (int64_t)x.size(), out.data()) == LERF_OK && out[2] == 2.0 && out[0] == 0.0);
    EXPECT(out[7] == inf && out[8] != out[8] && out[10] != out[10] && out[3] > 0.0);
    EXPECT(lerf_coords_math_host(LERF_MATH_ATAN, x.data(), nullptr, (int64_t)x.size(), x.data()) == LERF_OK);                        // in place
    EXPECT(lerf_coords_math_host(3, x.data(), y.data(), 4, out.data()) == LERF_EINVAL && lerf_coords_math_host(2, x.data(), nullptr, 4, out.data()) == LERF_EINVAL);
    EXPECT(lerf_coords_math_host(0, x.data(), nullptr, -1, out.data()) == LERF_EINVAL && lerf_coords_math_host(0, x.data(), nullptr, 0, out.data()) == LERF_OK);
    entry_ops(1, 1);
    entry_ops(2, 2);
    entry_ops(5, 67);
    raster_ops(1, 1);
    raster_ops(2, 2);
    raster_ops(5, 67);
    std::printf(fails ? "%d check(s) failed\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
