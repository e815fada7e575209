// Stand-alone sanitizer driver of the HOST twins of the coordinate maps (`make asan-coords`): lerf_coords.hip is compiled with
// AddressSanitizer + UndefinedBehaviorSanitizer on its host side and linked with this main, which calls lerf_coords_build_host,
// lerf_coords_build_bwd_host and lerf_coords_math_host (the fisheye and equirect models, the special arguments of the helpers) and
// lerf_coords_{mesh,compose,invert,compose_bwd,invert_bwd}_host on exactly-sized heap buffers -- strided tiles with an origin, both
// dtypes of every operand, a batch of sets, init and the gradient halves null and given, the refusals -- and lerf_coords_invert_raster_host
// on a folded map with NaN, +-inf and 1e300 entries, tiles at a non-zero origin, max_span 1 and 64.  The host twins of the six
// run the very functors the device runs (OnHost, ScatterOnHost in lerf_coords.hip), so this pass checks the addressing of the shared code.
// The batched twins (lerf_coords_*_batched_host) run three sets with padded set strides, a folded set with NaN / +-inf / 1e300 entries,
// non-zero origins and shared operands, and must equal the single-map twins set by set (batched_ops).
// lerf_coords_reproject_host and lerf_coords_reproject_bwd_host (reproject_ops) run three sets of both kinds and both depth dtypes into a
// strided out at a non-zero origin, depth_out and each gradient half null and given, special depths, and their refusals.
// lerf_splat_host and lerf_splat_bwd_host (splat_ops) run one and three sets of both image dtypes and both map dtypes, C = 1 and 3, with and
// without the norm plane and the weight, a shared and a per-set strided map with NaN, +-inf, 1e300 and frame-edge entries, each gradient
// half null and given, and their refusals.
// The ordered twins (ordered_ops: lerf_splat_ordered_host, lerf_coords_compose_bwd_batched_ordered_host, lerf_coords_invert_bwd_batched_ordered_host
// and lerf_scan_exclusive_u32_host) run their four passes over a workspace of exactly lerf_scatter_ordered_workspace_bytes bytes, two sets,
// pre-filled targets, entries beyond every edge and NaN entries, with a generous cap (the result must be the plain twin's bytes) and with
// a cap of 1 (the NaN branch), and a workspace one byte short is refused.
// The triangle-mesh rasteriser's host twins (trimesh_ops: lerf_coords_trimesh_host, lerf_coords_trimesh_batched_host) draw a fan wider than
// the tile, with indices -1, V and 2^31 - 1, NaN, +-inf and 1e300 vertices and w <= 0 among its faces, into a strided out at a non-zero
// origin, every dtype mix, two sets with shared faces; a workspace one byte short is refused.
// Its adjoint's host twins (lerf_coords_trimesh_bwd_host, lerf_coords_trimesh_bwd_batched_host) run inside trimesh_ops at the keys of every one of
// those forwards: upstream NaN in every hole, exactly-sized gradients and workspace, every NULL combination, a cap of 64 and of 1, two sets.
// It needs no GPU and is never loaded into another process.  Exit status 0 and "ok" on the last line: no report.
#include "lerf_hip.h"

#include <cmath>
#include <cstdint>
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

// The batched host twins (lerf_coords_*_batched_host) on THREE sets in exactly-sized heap buffers: the set stride of every operand is
// larger than a set (the gap holds the sentinel -7), the maps are strided tiles at origin (3, 7), set 1 holds a folded map with NaN,
// +-inf and 1e300 entries.  Set s must equal the single-map twin on the same operands, byte for byte, and no gap may change.
struct Batch {
    int dt, n, h, w;
    int64_t stride, set;
    std::vector<double> d;
    std::vector<float> f;
    Batch(int dt_, int n_, int h_, int w_, int pad = 3, int gap = 4)
        : dt(dt_), n(n_), h(h_), w(w_), stride(2 * (int64_t)(w_ + pad)), set((h_ - 1) * 2 * (int64_t)(w_ + pad) + 2 * w_ + gap) {
        const size_t len = (size_t)((n - 1) * set + (h - 1) * stride + 2 * w);
        if (dt == LERF_F64) d.assign(len, -7.0);
        else f.assign(len, -7.0f);
    }
    void* p(int s = 0) { return dt == LERF_F64 ? (void*)(d.data() + s * set) : (void*)(f.data() + s * set); }
    void set_entry(int s, int i, int j, double r, double c) {
        const size_t e = (size_t)(s * set + i * stride + 2 * j);
        if (dt == LERF_F64) { d[e] = r; d[e + 1] = c; }
        else { f[e] = (float)r; f[e + 1] = (float)c; }
    }
    // the entries of set s equal those of the single map m, and everything between the entries is the sentinel
    bool set_is(int s, Map& m) {
        for (int i = 0; i < h; ++i)
            for (int k = 0; k < 2 * w; ++k) {
                const size_t e = (size_t)(s * set + i * stride + k), q = (size_t)(i * m.stride + k);
                if (dt == LERF_F64 ? std::memcmp(&d[e], &m.d[q], 8) : std::memcmp(&f[e], &m.f[q], 4)) return false;
            }
        return true;
    }
    bool gaps_kept() const {
        const size_t len = d.size() + f.size();
        for (size_t e = 0; e < len; ++e) {
            const size_t in_set = e % (size_t)set, row = in_set / (size_t)stride, col = in_set % (size_t)stride;
            if ((int)row < h && (int)col < 2 * w) continue;
            if (dt == LERF_F64 ? d[e] != -7.0 : f[e] != -7.0f) return false;
        }
        return true;
    }
};

static void batched_ops(int oH, int oW) {
    const int DT[2] = {LERF_F32, LERF_F64}, N = 3;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int gh = 3, gw = 4, fH = 9, fW = 12;
    for (int ta : DT)
        for (int to : DT) {
            // F: set 0 a sheared grid, set 1 a FOLDED map with NaN, +-inf and 1e300 entries, set 2 a stretched grid
            Batch F(ta, N, fH, fW), B(ta, N, oH, oW), out(to, N, oH, oW);
            for (int s = 0; s < N; ++s) {
                for (int i = 0; i < fH; ++i)
                    for (int j = 0; j < fW; ++j)
                        F.set_entry(s, i, j, s == 1 ? 1.3 * i + 0.5 * std::sin(0.7 * j) : (0.9 + 0.3 * s) * i + 0.05 * j,
                                    s == 1 ? 1.1 * j + 4.0 * std::sin(j / 2.5) + 0.25 * i : (1.1 + 0.2 * s) * j + 0.1 * i);
                for (int i = 0; i < oH; ++i)
                    for (int j = 0; j < oW; ++j) {
                        const int k = i * oW + j + s;
                        B.set_entry(s, i, j, s == 1 && k % 11 == 3 ? nan : s == 1 && k % 13 == 5 ? -inf : 0.9 * (i % fH) - 0.5,
                                    s == 1 && k % 17 == 4 ? inf : s == 1 && k % 7 == 2 ? 1e300 : 0.11 * j - 0.75);
                    }
            }
            F.set_entry(1, 2, 5, nan, 3.0); F.set_entry(1, 4, 9, inf, 1.0); F.set_entry(1, 5, 3, 2.0, -inf); F.set_entry(1, 6, 7, 1e300, 1e300);
            F.set_entry(1, 0, 0, 1e300, -1e300);
            auto single_map = [&](Batch& b, int s) {
                Map m(b.dt, b.h, b.w);
                for (int i = 0; i < b.h; ++i)
                    for (int k = 0; k < 2 * b.w; ++k) {
                        if (b.dt == LERF_F64) m.d[(size_t)(i * m.stride + k)] = b.d[(size_t)(s * b.set + i * b.stride + k)];
                        else m.f[(size_t)(i * m.stride + k)] = b.f[(size_t)(s * b.set + i * b.stride + k)];
                    }
                return m;
            };
            // mesh: dense control meshes per set with a gap between them
            {
                const int64_t cset = 2 * gh * gw + 6;
                std::vector<double> c64((size_t)((N - 1) * cset + 2 * gh * gw), -7.0);
                std::vector<float> c32(c64.size(), -7.0f);
                for (int s = 0; s < N; ++s)
                    for (int k = 0; k < 2 * gh * gw; ++k) {
                        const double v = s == 1 && k == 5 ? nan : s == 1 && k == 8 ? 1e300 : s == 1 && k == 11 ? -inf : 3.0 * (k / 2) + 0.25 * s - (s == 1 ? 9.0 * (k % 4) : 0.0);
                        c64[(size_t)(s * cset + k)] = v;
                        c32[(size_t)(s * cset + k)] = (float)v;
                    }
                void* c = ta == LERF_F64 ? (void*)c64.data() : (void*)c32.data();
                const size_t el = ta == LERF_F64 ? 8 : 4;
                for (int interp : {LERF_MESH_BILINEAR, LERF_MESH_BICUBIC}) {
                    EXPECT(lerf_coords_mesh_batched_host(c, ta, gh, gw, interp, oH + 5, oW + 8, out.p(), to, out.stride, oH, oW, 3, 7, N, cset, out.set) == LERF_OK);
                    for (int s = 0; s < N; ++s) {
                        Map one(to, oH, oW);
                        EXPECT(lerf_coords_mesh_host((char*)c + (size_t)(s * cset) * el, ta, gh, gw, interp, oH + 5, oW + 8, one.p(), to, one.stride, oH, oW, 3, 7) == LERF_OK);
                        EXPECT(out.set_is(s, one));
                    }
                    EXPECT(out.gaps_kept());
                }
                EXPECT(lerf_coords_mesh_batched_host(c, ta, gh, gw, 0, oH + 5, oW + 8, out.p(), to, out.stride, oH, oW, 3, 7, N, cset, out.set + 1) == LERF_EINVAL);
                EXPECT(lerf_coords_mesh_batched_host(c, ta, gh, gw, 0, oH + 5, oW + 8, out.p(), to, out.stride, oH, oW, 3, 7, N, cset, 0) == LERF_EINVAL);
            }
            // compose: per-set outer maps, then ONE shared outer map
            for (int64_t a_set : {F.set, (int64_t)0}) {
                EXPECT(lerf_coords_compose_batched_host(F.p(), ta, F.stride, fH, fW, B.p(), ta, B.stride, out.p(), to, out.stride, oH, oW, N, a_set, B.set, out.set) == LERF_OK);
                for (int s = 0; s < N; ++s) {
                    Map one(to, oH, oW), a1 = single_map(F, a_set ? s : 0), b1 = single_map(B, s);
                    EXPECT(lerf_coords_compose_host(a1.p(), ta, a1.stride, fH, fW, b1.p(), ta, b1.stride, one.p(), to, one.stride, oH, oW) == LERF_OK);
                    EXPECT(out.set_is(s, one));
                }
                EXPECT(out.gaps_kept());
            }
            EXPECT(lerf_coords_compose_batched_host(F.p(), ta, F.stride, fH, fW, B.p(), ta, B.stride, out.p(), to, out.stride, oH, oW, N, F.set, 0, out.set) == LERF_EINVAL);
            EXPECT(lerf_coords_compose_batched_host(F.p(), ta, F.stride, fH, fW, B.p(), ta, B.stride, out.p(), to, out.stride, oH, oW, 65536, F.set, B.set, out.set) == LERF_EUNSUPPORTED);
            // invert at origin (3, 7): the affine start, then a start per set (B: NaN, inf and 1e300 in set 1)
            for (int with_init : {0, 1}) {
                EXPECT(lerf_coords_invert_batched_host(F.p(), ta, F.stride, fH, fW, with_init ? B.p() : nullptr, ta, B.stride, out.p(), to, out.stride, oH, oW, 3, 7,
                                                       5, 1e-9, N, F.set, B.set, out.set) == LERF_OK);
                for (int s = 0; s < N; ++s) {
                    Map one(to, oH, oW), f1 = single_map(F, s), b1 = single_map(B, s);
                    EXPECT(lerf_coords_invert_host(f1.p(), ta, f1.stride, fH, fW, with_init ? b1.p() : nullptr, ta, b1.stride, one.p(), to, one.stride, oH, oW, 3, 7,
                                                   5, 1e-9) == LERF_OK);
                    EXPECT(out.set_is(s, one));
                }
                EXPECT(out.gaps_kept());
            }
            // the rasterising inverse at origin (3, 7): keys and depth per set with gaps, then a shared depth
            {
                const int64_t kset = (int64_t)oH * oW + 3, dset = (int64_t)fH * fW + 5;
                std::vector<uint64_t> keys((size_t)((N - 1) * kset + oH * oW), 5), one_keys((size_t)oH * oW);
                std::vector<float> depth((size_t)((N - 1) * dset + fH * fW), -7.0f);
                for (int s = 0; s < N; ++s)
                    for (int k = 0; k < fH * fW; ++k) depth[(size_t)(s * dset + k)] = s == 1 && k % 31 == 7 ? (float)nan : 2.0f + std::sin(0.3f * (float)(k + s));
                for (int64_t d_set : {dset, (int64_t)0}) {
                    EXPECT(lerf_coords_invert_raster_batched_host(F.p(), ta, F.stride, fH, fW, depth.data(), out.p(), to, out.stride, oH, oW, 3, 7, 16, 0, keys.data(),
                                                                  N, F.set, d_set, out.set, kset) == LERF_OK);
                    for (int s = 0; s < N; ++s) {
                        Map one(to, oH, oW), f1 = single_map(F, s);
                        EXPECT(lerf_coords_invert_raster_host(f1.p(), ta, f1.stride, fH, fW, depth.data() + s * d_set, one.p(), to, one.stride, oH, oW, 3, 7, 16, 0,
                                                              one_keys.data()) == LERF_OK);
                        EXPECT(out.set_is(s, one) && !std::memcmp(one_keys.data(), keys.data() + s * kset, one_keys.size() * 8));
                    }
                    EXPECT(out.gaps_kept());
                    for (int s = 0; s + 1 < N; ++s)
                        for (int k = oH * oW; k < kset; ++k) EXPECT(keys[(size_t)(s * kset + k)] == 5);
                }
                EXPECT(lerf_coords_invert_raster_batched_host(F.p(), ta, F.stride, fH, fW, depth.data(), out.p(), to, out.stride, oH, oW, 3, 7, 16, 0, keys.data(), N,
                                                              F.set, dset, out.set, 0) == LERF_EINVAL);
            }
            if (to == LERF_F32) continue;
            // the adjoints: dense float64 gradients per set with gaps; a shared outer map with ONE grad_a
            const int64_t gset = 2 * (int64_t)oH * oW + 4, fset = 2 * (int64_t)fH * fW + 6;
            std::vector<double> g((size_t)((N - 1) * gset + 2 * oH * oW), -7.0), gB(g.size(), -7.0), gA((size_t)((N - 1) * fset + 2 * fH * fW), -7.0), gF(gA.size(), -7.0);
            for (int s = 0; s < N; ++s) {
                for (int k = 0; k < 2 * oH * oW; ++k) { g[(size_t)(s * gset + k)] = s == 1 && k % 29 == 9 ? nan : std::sin(0.37 * (double)(k + s)); gB[(size_t)(s * gset + k)] = 0.0; }
                for (int k = 0; k < 2 * fH * fW; ++k) gA[(size_t)(s * fset + k)] = gF[(size_t)(s * fset + k)] = 0.0;
            }
            EXPECT(lerf_coords_compose_bwd_batched_host(F.p(), ta, F.stride, fH, fW, B.p(), ta, B.stride, g.data(), oH, oW, gA.data(), gB.data(), N, F.set, B.set, gset,
                                                        fset, gset) == LERF_OK);
            EXPECT(lerf_coords_invert_bwd_batched_host(F.p(), ta, F.stride, fH, fW, B.p(), ta, B.stride, g.data(), oH, oW, gF.data(), N, F.set, B.set, gset, fset) == LERF_OK);
            std::vector<double> shared((size_t)2 * fH * fW, 0.0), acc(shared.size(), 0.0);
            EXPECT(lerf_coords_compose_bwd_batched_host(F.p(), ta, F.stride, fH, fW, B.p(), ta, B.stride, g.data(), oH, oW, shared.data(), nullptr, N, 0, B.set, gset, 0,
                                                        0) == LERF_OK);
            for (int s = 0; s < N; ++s) {
                Map f1 = single_map(F, s), f0 = single_map(F, 0), b1 = single_map(B, s);
                std::vector<double> a1((size_t)2 * fH * fW, 0.0), b_1((size_t)2 * oH * oW, 0.0), fg((size_t)2 * fH * fW, 0.0);
                EXPECT(lerf_coords_compose_bwd_host(f1.p(), ta, f1.stride, fH, fW, b1.p(), ta, b1.stride, g.data() + s * gset, oH, oW, a1.data(), b_1.data()) == LERF_OK);
                EXPECT(!std::memcmp(a1.data(), gA.data() + s * fset, a1.size() * 8) && !std::memcmp(b_1.data(), gB.data() + s * gset, b_1.size() * 8));
                EXPECT(lerf_coords_invert_bwd_host(f1.p(), ta, f1.stride, fH, fW, b1.p(), ta, b1.stride, g.data() + s * gset, oH, oW, fg.data()) == LERF_OK);
                EXPECT(!std::memcmp(fg.data(), gF.data() + s * fset, fg.size() * 8));
                EXPECT(lerf_coords_compose_bwd_host(f0.p(), ta, f0.stride, fH, fW, b1.p(), ta, b1.stride, g.data() + s * gset, oH, oW, acc.data(), nullptr) == LERF_OK);
            }
            EXPECT(!std::memcmp(acc.data(), shared.data(), acc.size() * 8));               // the sum over the sets, in set order
            for (int s = 0; s + 1 < N; ++s) {
                for (int64_t k = 2 * oH * oW; k < gset; ++k) EXPECT(gB[(size_t)(s * gset + k)] == -7.0);
                for (int64_t k = 2 * fH * fW; k < fset; ++k) EXPECT(gA[(size_t)(s * fset + k)] == -7.0 && gF[(size_t)(s * fset + k)] == -7.0);
            }
            const std::vector<double> keepA = gA, keepF = gF;
            EXPECT(lerf_coords_compose_bwd_batched_host(F.p(), ta, F.stride, fH, fW, B.p(), ta, B.stride, g.data(), oH, oW, gA.data(), gB.data(), N, F.set, B.set, gset, 0,
                                                        gset) == LERF_EINVAL);              // one grad_a for three different outer maps
            EXPECT(lerf_coords_compose_bwd_batched_host(F.p(), ta, F.stride, fH, fW, B.p(), ta, B.stride, g.data(), oH, oW, gA.data(), gB.data(), N, F.set, B.set, 0, fset,
                                                        gset) == LERF_EINVAL);
            EXPECT(lerf_coords_invert_bwd_batched_host(F.p(), ta, F.stride, fH, fW, B.p(), ta, B.stride, g.data(), oH, oW, gF.data(), N, F.set, B.set, gset, 0) == LERF_EINVAL);
            EXPECT(lerf_coords_invert_bwd_batched_host(F.p(), ta, F.stride, fH, fW, B.p(), ta, B.stride, g.data(), oH, oW, gF.data(), 0, F.set, B.set, gset, fset) == LERF_EINVAL);
            EXPECT(same(keepA, gA) && same(keepF, gF));
        }
}

// reproject and its adjoint on tiles [oH][oW] at origin (3, 7): three sets, both kinds, both depth dtypes, a strided out of both dtypes,
// depth_out and each gradient half null and given, special depths (0, negative, NaN, inf, 1e-300, 1e300, W <= 0), then the refusals
template <typename TD>
static void reproject_ops_of(int oH, int oW, int ddt) {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int B = 3;
    const size_t n = (size_t)oH * oW;
    // m = K_dst . R . inv(K_src) of nearby cameras; set 2: W = depth - 3, so depths below 3 lie behind the second view
    const double P[B * LERF_REPROJECT_PARAMS] = {1.25,   0.02,  -4.5, -0.03, 1.125, -2.0, 0.001, -0.002, 1.0, 8.0,  -3.6,  0.3,
                                                 0.8,    -0.01, 3.2,  0.02,  0.9,   1.9,  -0.0005, 0.001, 1.0, -9.6, 8.0,   0.1,
                                                 1.25,   0.0,   -4.5, 0.0,   1.125, -2.0, 0.0,   0.0,    1.0, 4.0,  7.2,   -3.0};
    const double special[10] = {0.0, -1.5, nan, inf, 1e-300, 1e300, 3.0, 2.5, -0.0, -inf};
    std::vector<TD> depth(B * n);
    for (size_t k = 0; k < depth.size(); ++k) depth[k] = k % 3 == 0 && k / 3 < 10 ? (TD)special[k / 3] : (TD)(0.5 + 0.37 * (double)(k % 13));
    std::vector<double> g(B * n * 2), gz(B * n);
    for (size_t k = 0; k < g.size(); ++k) g[k] = k % 29 == 9 ? nan : std::sin(0.37 * (double)k);
    for (size_t k = 0; k < gz.size(); ++k) gz[k] = k % 31 == 4 ? inf : std::cos(0.21 * (double)k);
    for (int kind : {LERF_DEPTH_Z, LERF_DEPTH_INVERSE}) {
        for (int to : {LERF_F32, LERF_F64}) {
            const int64_t stride = 2 * (int64_t)(oW + 3), span = (oH - 1) * stride + 2 * oW, set = span + 6;      // padded rows and sets
            std::vector<double> o64(to == LERF_F64 ? (size_t)((B - 1) * set + span) : 0, -7.0);
            std::vector<float> o32(to == LERF_F32 ? (size_t)((B - 1) * set + span) : 0, -7.0f);
            void* out = to == LERF_F64 ? (void*)o64.data() : (void*)o32.data();
            std::vector<float> zo(B * n, -7.0f);
            EXPECT(lerf_coords_reproject_host(kind, P, B, depth.data(), ddt, (int64_t)n, out, to, set, stride, zo.data(), (int64_t)n, oH, oW, 3, 7) == LERF_OK);
            EXPECT(lerf_coords_reproject_host(kind, P, B, depth.data(), ddt, (int64_t)n, out, to, set, stride, nullptr, 0, oH, oW, 3, 7) == LERF_OK);
            EXPECT(lerf_coords_reproject_host(kind, P, B, depth.data(), ddt, 0, out, to, set, stride, zo.data(), (int64_t)n, oH, oW, 3, 7) == LERF_OK);       // a shared plane
            EXPECT(lerf_coords_reproject_host(kind, P, 1, depth.data(), ddt, 0, out, to, 0, stride, zo.data(), 0, oH, oW, 0, 0) == LERF_OK);
            if (oW > 1) EXPECT(to == LERF_F64 ? o64[2 * oW] == -7.0 : o32[2 * oW] == -7.0f);                       // the padding of row 0
            // the refusals write nothing
            std::vector<float> keep = zo;
            EXPECT(lerf_coords_reproject_host(2, P, B, depth.data(), ddt, (int64_t)n, out, to, set, stride, zo.data(), (int64_t)n, oH, oW, 3, 7) == LERF_EINVAL);
            EXPECT(lerf_coords_reproject_host(kind, nullptr, B, depth.data(), ddt, (int64_t)n, out, to, set, stride, zo.data(), (int64_t)n, oH, oW, 3, 7) == LERF_EINVAL);
            EXPECT(lerf_coords_reproject_host(kind, P, B, nullptr, ddt, (int64_t)n, out, to, set, stride, zo.data(), (int64_t)n, oH, oW, 3, 7) == LERF_EINVAL);
            EXPECT(lerf_coords_reproject_host(kind, P, B, depth.data(), 0, (int64_t)n, out, to, set, stride, zo.data(), (int64_t)n, oH, oW, 3, 7) == LERF_EINVAL);
            EXPECT(lerf_coords_reproject_host(kind, P, B, depth.data(), ddt, (int64_t)n, out, 3, set, stride, zo.data(), (int64_t)n, oH, oW, 3, 7) == LERF_EINVAL);
            EXPECT(lerf_coords_reproject_host(kind, P, 0, depth.data(), ddt, (int64_t)n, out, to, set, stride, zo.data(), (int64_t)n, oH, oW, 3, 7) == LERF_EINVAL);
            EXPECT(lerf_coords_reproject_host(kind, P, 65536, depth.data(), ddt, (int64_t)n, out, to, set, stride, zo.data(), (int64_t)n, oH, oW, 3, 7) == LERF_EINVAL);
            EXPECT(lerf_coords_reproject_host(kind, P, B, depth.data(), ddt, (int64_t)n, out, to, set, stride + 1, zo.data(), (int64_t)n, oH, oW, 3, 7) == LERF_EINVAL);
            EXPECT(lerf_coords_reproject_host(kind, P, B, depth.data(), ddt, (int64_t)n, out, to, set, 2 * (int64_t)oW - 2, zo.data(), (int64_t)n, oH, oW, 3, 7) == LERF_EINVAL);
            EXPECT(lerf_coords_reproject_host(kind, P, B, depth.data(), ddt, (int64_t)n, out, to, span - 2, stride, zo.data(), (int64_t)n, oH, oW, 3, 7) == LERF_EINVAL);
            if (n > 1)                                          // a short set stride; on 1 x 1 it would be 0, the shared plane
                EXPECT(lerf_coords_reproject_host(kind, P, B, depth.data(), ddt, (int64_t)n - 1, out, to, set, stride, zo.data(), (int64_t)n, oH, oW, 3, 7) == LERF_EINVAL);
            EXPECT(lerf_coords_reproject_host(kind, P, B, depth.data(), ddt, (int64_t)n, out, to, set, stride, zo.data(), (int64_t)n - 1, oH, oW, 3, 7) == LERF_EINVAL);
            EXPECT(lerf_coords_reproject_host(kind, P, B, depth.data(), ddt, (int64_t)n, out, to, set, stride, zo.data(), (int64_t)n, 0, oW, 3, 7) == LERF_EINVAL);
            EXPECT(lerf_coords_reproject_host(kind, P, B, depth.data(), ddt, (int64_t)n, out, to, set, stride, zo.data(), (int64_t)n, oH, oW, -1, 7) == LERF_EINVAL);
            EXPECT(lerf_coords_reproject_host(kind, P, B, depth.data(), ddt, (int64_t)n, out, to, set, stride, (float*)depth.data(), (int64_t)n, oH, oW, 3, 7) == LERF_EINVAL);
            EXPECT(lerf_coords_reproject_host(kind, P, B, zo.data(), LERF_F32, 0, out, to, set, stride, zo.data(), (int64_t)n, oH, oW, 3, 7) == LERF_EINVAL);
            EXPECT(keep == zo || std::memcmp(keep.data(), zo.data(), keep.size() * sizeof(float)) == 0);
        }
        // the adjoint: each half null and given, with and without the upstream of zo; gradients exactly sized
        std::vector<double> gd(B * n, 0.5), gp(B * LERF_REPROJECT_PARAMS, -0.5);
        const std::vector<double> gd0 = gd, gp0 = gp;
        EXPECT(lerf_coords_reproject_bwd_host(kind, P, B, depth.data(), ddt, (int64_t)n, g.data(), gz.data(), oH, oW, 3, 7, gd.data(), gp.data()) == LERF_OK);
        EXPECT(!same(gd, gd0) && !same(gp, gp0));
        EXPECT(lerf_coords_reproject_bwd_host(kind, P, B, depth.data(), ddt, (int64_t)n, g.data(), nullptr, oH, oW, 3, 7, gd.data(), gp.data()) == LERF_OK);
        EXPECT(lerf_coords_reproject_bwd_host(kind, P, B, depth.data(), ddt, (int64_t)n, g.data(), gz.data(), oH, oW, 3, 7, nullptr, gp.data()) == LERF_OK);
        EXPECT(lerf_coords_reproject_bwd_host(kind, P, B, depth.data(), ddt, (int64_t)n, g.data(), gz.data(), oH, oW, 3, 7, gd.data(), nullptr) == LERF_OK);
        EXPECT(lerf_coords_reproject_bwd_host(kind, P, B, depth.data(), ddt, 0, g.data(), gz.data(), oH, oW, 3, 7, gd.data(), gp.data()) == LERF_OK);
        gd = gd0; gp = gp0;
        EXPECT(lerf_coords_reproject_bwd_host(kind, P, B, depth.data(), ddt, (int64_t)n, g.data(), gz.data(), oH, oW, 3, 7, nullptr, nullptr) == LERF_EINVAL);
        EXPECT(lerf_coords_reproject_bwd_host(5, P, B, depth.data(), ddt, (int64_t)n, g.data(), gz.data(), oH, oW, 3, 7, gd.data(), gp.data()) == LERF_EINVAL);
        EXPECT(lerf_coords_reproject_bwd_host(kind, P, B, depth.data(), ddt, (int64_t)n, nullptr, gz.data(), oH, oW, 3, 7, gd.data(), gp.data()) == LERF_EINVAL);
        EXPECT(lerf_coords_reproject_bwd_host(kind, P, B, depth.data(), ddt, (int64_t)n, g.data(), gz.data(), oH, oW, 3, 7, g.data(), gp.data()) == LERF_EINVAL);
        EXPECT(lerf_coords_reproject_bwd_host(kind, P, B, depth.data(), ddt, (int64_t)n, g.data(), gz.data(), oH, oW, 3, 7, gz.data(), gp.data()) == LERF_EINVAL);
        EXPECT(lerf_coords_reproject_bwd_host(kind, P, B, depth.data(), ddt, (int64_t)n, g.data(), gz.data(), oH, oW, 3, 7, gd.data(), gd.data()) == LERF_EINVAL);
        EXPECT(lerf_coords_reproject_bwd_host(kind, P, B, depth.data(), ddt, (int64_t)n, g.data(), gz.data(), oH, oW, 3, 7, gd.data(), (double*)P) == LERF_EINVAL);
        EXPECT(lerf_coords_reproject_bwd_host(kind, P, B, depth.data(), ddt, (int64_t)n, g.data(), gz.data(), oH, 0, 3, 7, gd.data(), gp.data()) == LERF_EINVAL);
        EXPECT(lerf_coords_reproject_bwd_host(kind, P, B, depth.data(), ddt, (int64_t)n, g.data(), gz.data(), oH, oW, 3, -7, gd.data(), gp.data()) == LERF_EINVAL);
        EXPECT(same(gd, gd0) && same(gp, gp0));
    }
}

static void reproject_ops(int oH, int oW) {
    reproject_ops_of<float>(oH, oW, LERF_F32);
    reproject_ops_of<double>(oH, oW, LERF_F64);
}

// the forward warp by splatting and its adjoint (lerf_splat_host, lerf_splat_bwd_host): sources [H][W] into a frame [oH][oW] unequal to
// it, C = 1 and 3, with and without the norm plane and the weight, both image dtypes and both map dtypes, one set and three sets with a
// per-set and a shared strided map, exactly-sized heap buffers; the map holds NaN, +-inf, 1e300, -0.5, oH - 1 exactly, oH - 0.5 and
// positions beyond every edge of the frame; each null half of the backward; then the refusals
template <typename T>
static void splat_ops_of(int H, int W, int oH, int oW, int dt) {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int N = 3;
    const size_t n = (size_t)H * W, on = (size_t)oH * oW;
    const double special[12][2] = {{nan, 3.0}, {2.0, nan}, {inf, 1.0}, {1.0, -inf}, {1e300, 2.0}, {2.0, -1e300}, {-0.5, 1.25}, {oH - 1.0, 0.5},
                                   {oH - 0.5, 2.0}, {1.5, oW - 0.5}, {oH - 1.0, oW - 1.0}, {-1.0, (double)oW}};
    for (int tf : {LERF_F32, LERF_F64})
        for (int C : {1, 3})
            for (int norm : {0, 1}) {
                Batch F(tf, N, H, W);
                for (int s = 0; s < N; ++s)
                    for (int i = 0; i < H; ++i)
                        for (int j = 0; j < W; ++j) {
                            const int k = i * W + j + s;
                            if (k % 5 == 0 && (k / 5) % 16 < 12) F.set_entry(s, i, j, special[(k / 5) % 16][0], special[(k / 5) % 16][1]);
                            else F.set_entry(s, i, j, (i + 0.37) * (oH + 2.0) / H - 1.5 + 0.7 * std::sin(0.31 * j + s), (j + 0.61) * (oW + 3.0) / W - 2.0);
                        }
                const int P = C + norm;
                std::vector<T> x(N * C * n), m(N * n), acc(N * P * on, (T)0), g(N * P * on), gx(N * C * n, (T)-7), gm(N * n, (T)-7);
                std::vector<double> gf(N * 2 * n, -7.0);
                for (size_t k = 0; k < x.size(); ++k) x[k] = (T)std::sin(0.37 * (double)k);
                for (size_t k = 0; k < m.size(); ++k) m[k] = (T)(1.0 + 0.5 * std::cos(0.21 * (double)k));
                for (size_t k = 0; k < g.size(); ++k) g[k] = k % 29 == 9 ? (T)nan : (T)std::cos(0.13 * (double)k);
                const int64_t xs = (int64_t)(C * n), ms = (int64_t)n, as = (int64_t)(P * on), gfs = (int64_t)(2 * n);
                for (const T* mp : {(const T*)nullptr, (const T*)m.data()})
                    for (int64_t fset : {F.set, (int64_t)0}) {
                        EXPECT(lerf_splat_host(x.data(), dt, C, H, W, xs, F.p(), tf, F.stride, fset, mp, ms, acc.data(), norm, oH, oW, as, N) == LERF_OK);
                        EXPECT(lerf_splat_host(x.data(), dt, C, H, W, 0, F.p(1), tf, F.stride, 0, mp, 0, acc.data(), norm, oH, oW, 0, 1) == LERF_OK);
                        EXPECT(lerf_splat_bwd_host(x.data(), dt, C, H, W, xs, F.p(), tf, F.stride, fset, mp, ms, g.data(), norm, oH, oW, as, gx.data(), xs,
                                                   gm.data(), ms, gf.data(), gfs, N) == LERF_OK);
                        EXPECT(lerf_splat_bwd_host(x.data(), dt, C, H, W, xs, F.p(), tf, F.stride, fset, mp, ms, g.data(), norm, oH, oW, as, nullptr, 0,
                                                   gm.data(), ms, gf.data(), gfs, N) == LERF_OK);
                        EXPECT(lerf_splat_bwd_host(x.data(), dt, C, H, W, xs, F.p(), tf, F.stride, fset, mp, ms, g.data(), norm, oH, oW, as, gx.data(), xs,
                                                   nullptr, 0, gf.data(), gfs, N) == LERF_OK);
                        EXPECT(lerf_splat_bwd_host(x.data(), dt, C, H, W, xs, F.p(), tf, F.stride, fset, mp, ms, g.data(), norm, oH, oW, as, gx.data(), xs,
                                                   gm.data(), ms, nullptr, 0, N) == LERF_OK);
                        EXPECT(lerf_splat_bwd_host(x.data(), dt, C, H, W, 0, F.p(2), tf, F.stride, 0, mp, 0, g.data(), norm, oH, oW, 0, gx.data(), 0, nullptr, 0,
                                                   nullptr, 0, 1) == LERF_OK);
                    }
                EXPECT(F.gaps_kept());
                EXPECT(gx[0] != (T)-7 && gm[0] == (T)0 && gf[0] == 0.0 && gf[1] == 0.0);      // entry (0, 0) of set 0 is (NaN, 3): exact zeros under a g with NaNs
                // the refusals write nothing
                const std::vector<T> acc0 = acc, gx0 = gx, gm0 = gm;
                const std::vector<double> gf0 = gf;
                EXPECT(lerf_splat_host(nullptr, dt, C, H, W, xs, F.p(), tf, F.stride, F.set, m.data(), ms, acc.data(), norm, oH, oW, as, N) == LERF_EINVAL);
                EXPECT(lerf_splat_host(x.data(), 0, C, H, W, xs, F.p(), tf, F.stride, F.set, m.data(), ms, acc.data(), norm, oH, oW, as, N) == LERF_EINVAL);
                EXPECT(lerf_splat_host(x.data(), dt, 0, H, W, xs, F.p(), tf, F.stride, F.set, m.data(), ms, acc.data(), norm, oH, oW, as, N) == LERF_EINVAL);
                EXPECT(lerf_splat_host(x.data(), dt, C, H, W, xs, F.p(), tf, F.stride + 1, F.set, m.data(), ms, acc.data(), norm, oH, oW, as, N) == LERF_EINVAL);
                EXPECT(lerf_splat_host(x.data(), dt, C, H, W, xs, F.p(), tf, F.stride, F.set, m.data(), ms, acc.data(), norm, 0, oW, as, N) == LERF_EINVAL);
                EXPECT(lerf_splat_host(x.data(), dt, C, H, W, xs, F.p(), tf, F.stride, F.set, m.data(), ms, acc.data(), norm, oH, oW, as - 1, N) == LERF_EINVAL);
                EXPECT(lerf_splat_host(x.data(), dt, C, H, W, xs, F.p(), tf, F.stride, F.set, m.data(), ms, (void*)x.data(), norm, oH, oW, as, N) == LERF_EINVAL);
                EXPECT(lerf_splat_host(x.data(), dt, C, H, W, xs, F.p(), tf, F.stride, F.set, m.data(), ms, acc.data(), norm, oH, oW, as, 0) == LERF_EINVAL);
                EXPECT(lerf_splat_bwd_host(x.data(), dt, C, H, W, xs, F.p(), tf, F.stride, F.set, m.data(), ms, g.data(), norm, oH, oW, as, nullptr, 0, nullptr, 0,
                                           nullptr, 0, N) == LERF_EINVAL);
                EXPECT(lerf_splat_bwd_host(x.data(), dt, C, H, W, xs, F.p(), tf, F.stride, F.set, m.data(), ms, nullptr, norm, oH, oW, as, gx.data(), xs, gm.data(),
                                           ms, gf.data(), gfs, N) == LERF_EINVAL);
                EXPECT(lerf_splat_bwd_host(x.data(), dt, C, H, W, xs, F.p(), tf, F.stride, F.set, m.data(), ms, g.data(), norm, oH, oW, as, (void*)x.data(), xs,
                                           gm.data(), ms, gf.data(), gfs, N) == LERF_EINVAL);
                EXPECT(lerf_splat_bwd_host(x.data(), dt, C, H, W, xs, F.p(), tf, F.stride, F.set, m.data(), ms, g.data(), norm, oH, oW, as, gx.data(), xs,
                                           (void*)m.data(), ms, gf.data(), gfs, N) == LERF_EINVAL);
                EXPECT(lerf_splat_bwd_host(x.data(), dt, C, H, W, xs, F.p(), tf, F.stride, F.set, m.data(), ms, g.data(), norm, oH, oW, as, gx.data(), xs,
                                           gm.data(), ms, gf.data(), gfs - 2, N) == LERF_EINVAL);
                EXPECT(!std::memcmp(acc.data(), acc0.data(), acc.size() * sizeof(T)) && !std::memcmp(gx.data(), gx0.data(), gx.size() * sizeof(T)) &&
                       !std::memcmp(gm.data(), gm0.data(), gm.size() * sizeof(T)) && same(gf, gf0));
            }
}

static void splat_ops(int H, int W, int oH, int oW) {
    splat_ops_of<float>(H, W, oH, oW, LERF_F32);
    splat_ops_of<double>(H, W, oH, oW, LERF_F64);
}

// the ordered scatter's host twins against the plain ones, byte for byte, on exactly-sized heap buffers
template <typename T>
static void ordered_splat_of(int H, int W, int oH, int oW, int dt) {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int N = 2, C = 3, P = C + 1;
    const size_t n = (size_t)H * W, on = (size_t)oH * oW;
    const double special[8][2] = {{nan, 3.0}, {inf, 1.0}, {1e300, 2.0}, {-0.5, 1.25}, {oH - 1.0, 0.5}, {oH - 0.5, 2.0}, {oH - 1.0, oW - 1.0}, {-1.0, (double)oW}};
    std::vector<double> F(N * 2 * n);
    for (int s = 0; s < N; ++s)
        for (size_t e = 0; e < n; ++e) {
            const int i = (int)(e / W), j = (int)(e % W);
            const bool sp = (e + s) % 5 == 0 && ((e + s) / 5) % 16 < 8;
            F[2 * (s * n + e)] = sp ? special[((e + s) / 5) % 16][0] : (i + 0.37) * (oH + 2.0) / H - 1.5 + 0.7 * std::sin(0.31 * j + s);
            F[2 * (s * n + e) + 1] = sp ? special[((e + s) / 5) % 16][1] : (j + 0.61) * (oW + 3.0) / W - 2.0;
        }
    std::vector<T> x(N * C * n), m(N * n), acc(N * P * on), got, capped;
    for (size_t k = 0; k < x.size(); ++k) x[k] = (T)std::sin(0.37 * (double)k);
    for (size_t k = 0; k < m.size(); ++k) m[k] = (T)(1.0 + 0.5 * std::cos(0.21 * (double)k));
    for (size_t k = 0; k < acc.size(); ++k) acc[k] = (T)std::cos(0.11 * (double)k);
    got = capped = acc;
    const size_t bytes = lerf_scatter_ordered_workspace_bytes((int64_t)n, (int64_t)on, N);
    EXPECT(bytes >= 16 + 4 * N * (on + 4 * n));
    std::vector<uint32_t> ws(bytes / 4, 0xa5a5a5a5u);
    const int64_t xs = (int64_t)(C * n), fs = (int64_t)(2 * n), ms = (int64_t)n, as = (int64_t)(P * on);
    EXPECT(lerf_splat_host(x.data(), dt, C, H, W, xs, F.data(), LERF_F64, 2 * W, fs, m.data(), ms, acc.data(), 1, oH, oW, as, N) == LERF_OK);
    EXPECT(lerf_splat_ordered_host(x.data(), dt, C, H, W, xs, F.data(), LERF_F64, 2 * W, fs, m.data(), ms, got.data(), 1, oH, oW, as, N, ws.data(),
                                   bytes, 1 << 20) == LERF_OK);
    EXPECT(!std::memcmp(acc.data(), got.data(), acc.size() * sizeof(T)));
    const uint32_t most = ws[1];
    EXPECT(ws[0] == 0 && most >= 1 && most <= 4 * n);
    EXPECT(lerf_splat_ordered_host(x.data(), dt, C, H, W, xs, F.data(), LERF_F64, 2 * W, fs, m.data(), ms, capped.data(), 1, oH, oW, as, N, ws.data(),
                                   bytes, 1) == LERF_OK);
    EXPECT(ws[1] == most);
    const std::vector<T> before = capped;
    EXPECT(lerf_splat_ordered_host(x.data(), dt, C, H, W, xs, F.data(), LERF_F64, 2 * W, fs, m.data(), ms, capped.data(), 1, oH, oW, as, N, ws.data(),
                                   bytes - 1, 4) == LERF_EINVAL);
    EXPECT(lerf_splat_ordered_host(x.data(), dt, C, H, W, xs, F.data(), LERF_F64, 2 * W, fs, m.data(), ms, capped.data(), 1, oH, oW, as, N, ws.data(),
                                   bytes, 0) == LERF_EINVAL);
    EXPECT(lerf_splat_ordered_host(x.data(), dt, C, H, W, xs, F.data(), LERF_F64, 2 * W, fs, m.data(), ms, capped.data(), 1, oH, oW, as, N, capped.data(),
                                   bytes, 4) == LERF_EINVAL);
    EXPECT(!std::memcmp(capped.data(), before.data(), capped.size() * sizeof(T)));
}

static void ordered_adjoints(int aH, int aW, int oH, int oW) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int N = 2;
    const size_t na = (size_t)2 * aH * aW, nb = (size_t)2 * oH * oW;
    std::vector<double> A(N * na), B(N * nb), g(N * nb), ga(N * na), gb(N * nb), gf(N * na);
    for (int s = 0; s < N; ++s)
        for (int i = 0; i < aH; ++i)
            for (int j = 0; j < aW; ++j) {
                A[s * na + 2 * (i * aW + j)] = 1.1 * i + 0.2 * std::sin(0.9 * j + s) + 0.05 * i * j;
                A[s * na + 2 * (i * aW + j) + 1] = 0.9 * j + 0.3 * std::cos(0.7 * i + s) - 0.03 * i * j;
            }
    for (size_t e = 0; e < N * nb / 2; ++e) {
        B[2 * e] = e % 11 == 3 ? nan : -2.5 + std::fmod(0.731 * (double)e, aH + 4.0);      // beyond every edge: the taps clamp onto the border cells
        B[2 * e + 1] = e % 13 == 5 ? 1e300 : -2.5 + std::fmod(1.137 * (double)e, aW + 4.0);
    }
    for (size_t k = 0; k < g.size(); ++k) g[k] = std::sin(0.37 * (double)k);
    for (size_t k = 0; k < ga.size(); ++k) ga[k] = gf[k] = std::cos(0.19 * (double)k);
    for (size_t k = 0; k < gb.size(); ++k) gb[k] = std::cos(0.23 * (double)k);
    std::vector<double> ga2 = ga, gb2 = gb, gf2 = gf;
    const size_t bytes = lerf_scatter_ordered_workspace_bytes((int64_t)oH * oW, (int64_t)aH * aW, N);
    std::vector<uint32_t> ws(bytes / 4, 0x5a5a5a5au);
    const int64_t sa = (int64_t)na, sb = (int64_t)nb;
    EXPECT(lerf_coords_compose_bwd_batched_host(A.data(), LERF_F64, 2 * aW, aH, aW, B.data(), LERF_F64, 2 * oW, g.data(), oH, oW, ga.data(), gb.data(), N, sa,
                                                sb, sb, sa, sb) == LERF_OK);
    EXPECT(lerf_coords_compose_bwd_batched_ordered_host(A.data(), LERF_F64, 2 * aW, aH, aW, B.data(), LERF_F64, 2 * oW, g.data(), oH, oW, ga2.data(),
                                                        gb2.data(), N, sa, sb, sb, sa, sb, ws.data(), bytes, 1 << 20) == LERF_OK);
    EXPECT(same(ga, ga2) && same(gb, gb2) && ws[1] >= 1);
    EXPECT(lerf_coords_invert_bwd_batched_host(A.data(), LERF_F64, 2 * aW, aH, aW, B.data(), LERF_F64, 2 * oW, g.data(), oH, oW, gf.data(), N, sa, sb, sb,
                                               sa) == LERF_OK);
    EXPECT(lerf_coords_invert_bwd_batched_ordered_host(A.data(), LERF_F64, 2 * aW, aH, aW, B.data(), LERF_F64, 2 * oW, g.data(), oH, oW, gf2.data(), N, sa,
                                                       sb, sb, sa, ws.data(), bytes, 1 << 20) == LERF_OK);
    EXPECT(same(gf, gf2));
    // the cap of 1 (NaN in every target with two adders), each half alone, the single-map forms, a short workspace
    EXPECT(lerf_coords_compose_bwd_batched_ordered_host(A.data(), LERF_F64, 2 * aW, aH, aW, B.data(), LERF_F64, 2 * oW, g.data(), oH, oW, ga2.data(),
                                                        nullptr, N, sa, sb, sb, sa, 0, ws.data(), bytes, 1) == LERF_OK);
    EXPECT(lerf_coords_compose_bwd_ordered_host(A.data(), LERF_F64, 2 * aW, aH, aW, B.data(), LERF_F64, 2 * oW, g.data(), oH, oW, nullptr, gb2.data(),
                                                ws.data(), bytes, 4) == LERF_OK);
    EXPECT(lerf_coords_invert_bwd_ordered_host(A.data(), LERF_F64, 2 * aW, aH, aW, B.data(), LERF_F64, 2 * oW, g.data(), oH, oW, gf2.data(), ws.data(),
                                               bytes, 1) == LERF_OK);
    const std::vector<double> keep = gf2;
    EXPECT(lerf_coords_invert_bwd_batched_ordered_host(A.data(), LERF_F64, 2 * aW, aH, aW, B.data(), LERF_F64, 2 * oW, g.data(), oH, oW, gf2.data(), N, sa,
                                                       sb, sb, sa, ws.data(), bytes - 1, 4) == LERF_EINVAL);
    EXPECT(lerf_coords_compose_bwd_batched_ordered_host(A.data(), LERF_F64, 2 * aW, aH, aW, B.data(), LERF_F64, 2 * oW, g.data(), oH, oW, gf2.data(),
                                                        nullptr, N, sa, sb, sb, 0, 0, ws.data(), bytes, 4) == LERF_EINVAL);
    EXPECT(same(gf2, keep));
}

// the triangle-mesh rasteriser (lerf_coords_trimesh_host / _batched_host) on exactly-sized heap buffers: a fan wider than the tile with
// skipped faces among the drawn ones -- indices -1, V and 2^31 - 1, NaN, +-inf and 1e300 vertices, NaN depth, w <= 0 -- drawn into a
// strided out at origin (3, 7), every dtype mix, with and without depth, w (both dtypes), attr_faces and depth_out, every orient, max_span
// 0, 1 and 300; two sets that share their faces; a far tile; a workspace one byte short and the other refusals
static void trimesh_ops(int oH, int oW) {
    const int DT[2] = {LERF_F32, LERF_F64};
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int V = 14, Va = 16, F = 20;
    const double P[V][2] = {{14.3, 18.6}, {-150.0, 20.0}, {-20.0, 210.0}, {160.0, 150.0}, {170.0, -90.0}, {10.0, -160.0}, {5.5, 9.25}, {8.0, 40.0},
                            {nan, 4.0}, {3.0, inf}, {-inf, 2.0}, {1e300, 1e300}, {-1e300, 1e300}, {1e300, 6.0}};
    const int32_t faces[F][3] = {{-1, 1, 2}, {0, 1, 2}, {0, V, 3}, {0, 2, 3}, {0, 3, 0x7fffffff}, {0, 3, 4}, {0, 8, 1}, {0, 4, 5}, {9, 0, 1}, {0, 5, 1},
                                 {10, 2, 3}, {11, 12, 0}, {6, 7, 13}, {6, 6, 7}, {6, 7, 0}, {0, 7, 6}, {12, 0, 11}, {1, 3, 5}, {INT32_MIN, 0, 1}, {7, 6, 13}};
    int32_t afaces[F][3];
    for (int f = 0; f < F; ++f)
        for (int k = 0; k < 3; ++k) afaces[f][k] = f == 7 ? Va : faces[f][k] < 0 || faces[f][k] >= V ? faces[f][k] : faces[f][k] + (f & 1) * 2;
    std::vector<int32_t> fc(&faces[0][0], &faces[0][0] + 3 * F), af(&afaces[0][0], &afaces[0][0] + 3 * F);
    std::vector<float> depth(V), w32(V), zo((size_t)oH * oW, -7.0f);
    std::vector<double> w64(V);
    for (int v = 0; v < V; ++v) {
        depth[v] = v == 5 ? (float)nan : 1.0f + 0.125f * (float)(v % 4);
        w64[v] = v == 4 ? 0.0 : v == 2 ? -0.75 : v == 7 ? inf : 1.0 + 0.0625 * v;
        w32[v] = (float)w64[v];
    }
    const size_t need = lerf_coords_trimesh_workspace_bytes(F, 1), need2 = lerf_coords_trimesh_workspace_bytes(F, 2);
    EXPECT(need == 4 * (size_t)(F + 1) && need2 == 2 * need && lerf_coords_trimesh_workspace_bytes(0, 1) == 0);
    std::vector<unsigned char> ws(need, 0x55), ws2(need2, 0x55);
    for (int tp : DT)
        for (int ta : DT)
            for (int to : DT) {
                Map pos(tp, V, 1, 0), attr(ta, Va, 1, 0), out(to, oH, oW), keep(to, oH, oW);
                for (int v = 0; v < V; ++v) pos.set(v, 0, P[v][0], P[v][1]);
                for (int v = 0; v < Va; ++v) attr.set(v, 0, 1.25 * v, 50.0 - 0.5 * v);
                std::vector<uint64_t> keys((size_t)oH * oW, 5), keys0 = keys;
                int drawn = 0;
                for (int with = 0; with < 8; ++with)
                    for (int span : {0, 1, 300})
                        for (int orient : {-1, 0, 1}) {
                            const float* d = (with & 1) ? depth.data() : nullptr;
                            const void* w = (with & 2) ? ((with & 4) ? (const void*)w64.data() : (const void*)w32.data()) : nullptr;
                            EXPECT(lerf_coords_trimesh_host(pos.p(), tp, V, attr.p(), ta, Va, fc.data(), (with & 4) ? af.data() : nullptr, F, d, w,
                                                            (with & 4) ? LERF_F64 : LERF_F32, out.p(), to, out.stride, oH, oW, 3, 7, span, orient, keys.data(),
                                                            d ? zo.data() : nullptr, ws.data(), need) == LERF_OK);
                            EXPECT(keys != keys0);
                            for (uint64_t k : keys) drawn += k != ~(uint64_t)0;
                            // the adjoint at these keys (lerf_coords_trimesh_bwd_host) on exactly-sized heap buffers: NaN upstream in every hole, a
                            // generous cap (every gradient finite) and a cap of 1 (the NaN branch), every NULL combination, one byte short
                            std::vector<double> go((size_t)oH * oW * 2), ga((size_t)2 * Va), gp((size_t)2 * V), gw((size_t)V);
                            for (size_t k = 0; k < go.size(); ++k) go[k] = keys[k / 2] == ~(uint64_t)0 ? nan : std::sin(0.37 * (double)k);
                            const size_t nb = lerf_coords_trimesh_bwd_workspace_bytes(F, V, Va, 1);
                            EXPECT(nb == 16 + 8 * 15 * (size_t)F + 4 * ((size_t)Va + 3 * (size_t)F));
                            std::vector<unsigned char> bws(nb, 0x55);
                            for (int cap : {64, 1})
                                for (int mask = 1; mask < 8; ++mask) {
                                    if ((mask & 4) && !w) continue;
                                    std::fill(ga.begin(), ga.end(), 0.0); std::fill(gp.begin(), gp.end(), 0.0); std::fill(gw.begin(), gw.end(), 0.0);
                                    EXPECT(lerf_coords_trimesh_bwd_host(pos.p(), tp, V, attr.p(), ta, Va, fc.data(), (with & 4) ? af.data() : nullptr, F, d, w,
                                                                        (with & 4) ? LERF_F64 : LERF_F32, oH, oW, 3, 7, span, orient, keys.data(), go.data(),
                                                                        (mask & 1) ? ga.data() : nullptr, (mask & 2) ? gp.data() : nullptr,
                                                                        (mask & 4) ? gw.data() : nullptr, bws.data(), nb, cap) == LERF_OK);
                                    if (cap == 64)
                                        for (const std::vector<double>* g : {&ga, &gp, &gw})
                                            for (double v : *g) EXPECT(v - v == 0.0);
                                }
                            EXPECT(lerf_coords_trimesh_bwd_host(pos.p(), tp, V, attr.p(), ta, Va, fc.data(), nullptr, F, d, w, (with & 4) ? LERF_F64 : LERF_F32, oH, oW, 3,
                                                                7, span, orient, keys.data(), go.data(), ga.data(), gp.data(), nullptr, bws.data(), nb - 1, 64) ==
                                   LERF_EINVAL);
                            EXPECT(lerf_coords_trimesh_bwd_host(pos.p(), tp, V, attr.p(), ta, Va, fc.data(), nullptr, F, d, w, (with & 4) ? LERF_F64 : LERF_F32, oH, oW, 3,
                                                                7, span, orient, keys.data(), go.data(), nullptr, nullptr, nullptr, bws.data(), nb, 64) == LERF_EINVAL);
                        }
                EXPECT(drawn > 0);
                // a far tile: nothing unclipped may become an int
                EXPECT(lerf_coords_trimesh_host(pos.p(), tp, V, attr.p(), ta, Va, fc.data(), nullptr, F, depth.data(), nullptr, LERF_F32, out.p(), to, out.stride,
                                                oH, oW, 0x7fffffff - oH, 0x7fffffff - oW, 0, 0, keys.data(), nullptr, ws.data(), need) == LERF_OK);
                EXPECT(keys[0] == ~(uint64_t)0);
                // two sets: their own positions and outputs, shared faces, attributes, depth and w
                {
                    Map pos2(tp, 2 * V, 1, 0), out2(to, 2 * oH, oW);
                    for (int v = 0; v < 2 * V; ++v) pos2.set(v, 0, P[v % V][0] + (v / V) * 0.5, P[v % V][1]);
                    std::vector<uint64_t> keys2((size_t)2 * oH * oW, 5);
                    std::vector<float> zo2((size_t)2 * oH * oW, -7.0f);
                    EXPECT(lerf_coords_trimesh_batched_host(pos2.p(), tp, V, attr.p(), ta, Va, fc.data(), af.data(), F, depth.data(), w32.data(), LERF_F32, out2.p(), to,
                                                            out2.stride, oH, oW, 3, 7, 0, 0, keys2.data(), zo2.data(), ws2.data(), need2, 2, 2 * V, 0, 0, 0, 0, 0,
                                                            oH * out2.stride, (int64_t)oH * oW, (int64_t)oH * oW) == LERF_OK);
                    EXPECT(lerf_coords_trimesh_host(pos.p(), tp, V, attr.p(), ta, Va, fc.data(), af.data(), F, depth.data(), w32.data(), LERF_F32, out.p(), to,
                                                    out.stride, oH, oW, 3, 7, 0, 0, keys.data(), zo.data(), ws.data(), need) == LERF_OK);
                    EXPECT(!std::memcmp(keys.data(), keys2.data(), keys.size() * sizeof(uint64_t)) && !std::memcmp(zo.data(), zo2.data(), zo.size() * sizeof(float)));
                    // the adjoint of the two sets in one call: per-set gradients, exactly sized; set 0 equals the single call
                    {
                        const size_t nb2 = lerf_coords_trimesh_bwd_workspace_bytes(F, V, Va, 2), nb1 = lerf_coords_trimesh_bwd_workspace_bytes(F, V, Va, 1);
                        std::vector<unsigned char> bws2(nb2, 0x55);
                        std::vector<double> go2((size_t)2 * oH * oW * 2), ga2((size_t)4 * Va, 0.0), gp2((size_t)4 * V, 0.0), gw2((size_t)2 * V, 0.0);
                        std::vector<double> ga1((size_t)2 * Va, 0.0), gp1((size_t)2 * V, 0.0), gw1((size_t)V, 0.0);
                        for (size_t k = 0; k < go2.size(); ++k) go2[k] = keys2[k / 2] == ~(uint64_t)0 ? nan : std::cos(0.21 * (double)k);
                        EXPECT(lerf_coords_trimesh_bwd_batched_host(pos2.p(), tp, V, attr.p(), ta, Va, fc.data(), af.data(), F, depth.data(), w32.data(), LERF_F32, oH,
                                                                    oW, 3, 7, 0, 0, keys2.data(), go2.data(), ga2.data(), gp2.data(), gw2.data(), bws2.data(), nb2, 64, 2,
                                                                    2 * V, 0, 0, 0, 0, 0, (int64_t)oH * oW, 2 * (int64_t)oH * oW, 2 * Va, 2 * V, V) == LERF_OK);
                        EXPECT(lerf_coords_trimesh_bwd_host(pos.p(), tp, V, attr.p(), ta, Va, fc.data(), af.data(), F, depth.data(), w32.data(), LERF_F32, oH, oW, 3, 7, 0,
                                                            0, keys.data(), go2.data(), ga1.data(), gp1.data(), gw1.data(), bws2.data(), nb1, 64) == LERF_OK);
                        EXPECT(!std::memcmp(ga1.data(), ga2.data(), ga1.size() * 8) && !std::memcmp(gp1.data(), gp2.data(), gp1.size() * 8) &&
                               !std::memcmp(gw1.data(), gw2.data(), gw1.size() * 8));
                        // a gradient shared between the sets, and the workspace of one set for two
                        EXPECT(lerf_coords_trimesh_bwd_batched_host(pos2.p(), tp, V, attr.p(), ta, Va, fc.data(), af.data(), F, depth.data(), w32.data(), LERF_F32, oH,
                                                                    oW, 3, 7, 0, 0, keys2.data(), go2.data(), ga2.data(), gp2.data(), gw2.data(), bws2.data(), nb2, 64, 2,
                                                                    2 * V, 0, 0, 0, 0, 0, (int64_t)oH * oW, 2 * (int64_t)oH * oW, 0, 2 * V, V) == LERF_EINVAL);
                        EXPECT(lerf_coords_trimesh_bwd_batched_host(pos2.p(), tp, V, attr.p(), ta, Va, fc.data(), af.data(), F, depth.data(), w32.data(), LERF_F32, oH,
                                                                    oW, 3, 7, 0, 0, keys2.data(), go2.data(), ga2.data(), gp2.data(), gw2.data(), bws2.data(), nb1, 64, 2,
                                                                    2 * V, 0, 0, 0, 0, 0, (int64_t)oH * oW, 2 * (int64_t)oH * oW, 2 * Va, 2 * V, V) == LERF_EINVAL);
                    }
                    // the sets' outputs must not be shared; the workspace of one set is short for two
                    EXPECT(lerf_coords_trimesh_batched_host(pos2.p(), tp, V, attr.p(), ta, Va, fc.data(), af.data(), F, depth.data(), w32.data(), LERF_F32, keep.p(), to,
                                                            keep.stride, oH, oW, 3, 7, 0, 0, keys2.data(), nullptr, ws2.data(), need2, 2, 2 * V, 0, 0, 0, 0, 0, 0,
                                                            (int64_t)oH * oW, 0) == LERF_EINVAL);
                    EXPECT(lerf_coords_trimesh_batched_host(pos2.p(), tp, V, attr.p(), ta, Va, fc.data(), af.data(), F, depth.data(), w32.data(), LERF_F32, out2.p(), to,
                                                            out2.stride, oH, oW, 3, 7, 0, 0, keys2.data(), nullptr, ws.data(), need, 2, 2 * V, 0, 0, 0, 0, 0,
                                                            oH * out2.stride, (int64_t)oH * oW, 0) == LERF_EINVAL);
                }
                keys = keys0;
                const int64_t s = keep.stride;
                auto call = [&](const void* pp, int v, const int32_t* ff, int nf, const float* d, float* z, int span, int orient, int i0, uint64_t* k, void* wsp,
                                size_t wb) {
                    return lerf_coords_trimesh_host(pp, tp, v, attr.p(), ta, Va, ff, nullptr, nf, d, nullptr, LERF_F32, keep.p(), to, s, oH, oW, i0, 7, span, orient, k,
                                                    z, wsp, wb);
                };
                EXPECT(call(pos.p(), V, fc.data(), F, nullptr, nullptr, 0, 0, 3, keys.data(), ws.data(), need - 1) == LERF_EINVAL);      // one byte short
                EXPECT(call(pos.p(), V, fc.data(), F, nullptr, nullptr, 0, 0, 3, keys.data(), ws.data() + 1, need - 1) == LERF_EINVAL);
                EXPECT(call(pos.p(), V, fc.data(), F, nullptr, nullptr, 0, 0, 3, keys.data(), nullptr, need) == LERF_EINVAL);
                EXPECT(call(nullptr, V, fc.data(), F, nullptr, nullptr, 0, 0, 3, keys.data(), ws.data(), need) == LERF_EINVAL);
                EXPECT(call(pos.p(), 0, fc.data(), F, nullptr, nullptr, 0, 0, 3, keys.data(), ws.data(), need) == LERF_EINVAL);
                EXPECT(call(pos.p(), V, nullptr, F, nullptr, nullptr, 0, 0, 3, keys.data(), ws.data(), need) == LERF_EINVAL);
                EXPECT(call(pos.p(), V, fc.data(), 0, nullptr, nullptr, 0, 0, 3, keys.data(), ws.data(), need) == LERF_EINVAL);
                EXPECT(call(pos.p(), V, fc.data(), F, nullptr, zo.data(), 0, 0, 3, keys.data(), ws.data(), need) == LERF_EINVAL);      // depth_out without depth
                EXPECT(call(pos.p(), V, fc.data(), F, nullptr, nullptr, -1, 0, 3, keys.data(), ws.data(), need) == LERF_EINVAL);
                EXPECT(call(pos.p(), V, fc.data(), F, nullptr, nullptr, 65537, 0, 3, keys.data(), ws.data(), need) == LERF_EINVAL);
                EXPECT(call(pos.p(), V, fc.data(), F, nullptr, nullptr, 0, 2, 3, keys.data(), ws.data(), need) == LERF_EINVAL);
                EXPECT(call(pos.p(), V, fc.data(), F, nullptr, nullptr, 0, 0, -1, keys.data(), ws.data(), need) == LERF_EINVAL);
                EXPECT(call(pos.p(), V, fc.data(), F, nullptr, nullptr, 0, 0, 3, nullptr, ws.data(), need) == LERF_EINVAL);
                EXPECT(call(pos.p(), V, fc.data(), F, nullptr, nullptr, 0, 0, 3, (uint64_t*)ws.data(), ws.data(), need) == LERF_EINVAL);      // keys IS the workspace
                EXPECT(call(pos.p(), V, fc.data(), F, nullptr, nullptr, 0, 0, 3, keys.data(), fc.data(), need) == LERF_EINVAL);               // the workspace IS faces
                EXPECT(call(keep.p(), 1, fc.data(), F, nullptr, nullptr, 0, 0, 3, keys.data(), ws.data(), need) == LERF_EINVAL);              // out IS pos
                EXPECT(lerf_coords_trimesh_host(nullptr, tp, 3, nullptr, ta, 3, nullptr, nullptr, 40000, nullptr, nullptr, LERF_F32, nullptr, to, 2 * 3840, 2160, 3840, 0, 0,
                                                0, 0, nullptr, nullptr, nullptr, 0) == LERF_EUNSUPPORTED);                               // the size rule, before any pointer
                EXPECT(keep.same(Map(to, oH, oW)) && keys == keys0);
                for (unsigned char b : ws) EXPECT(b == 0x55);
            }
}

static void ordered_ops() {
    ordered_splat_of<float>(1, 1, 1, 1, LERF_F32);
    ordered_splat_of<float>(23, 31, 29, 37, LERF_F32);
    ordered_splat_of<double>(5, 67, 7, 61, LERF_F64);
    ordered_splat_of<float>(35, 65, 8, 8, LERF_F32);            // several hundred adders per target: the heap sort
    ordered_splat_of<double>(35, 65, 3, 2, LERF_F64);
    ordered_adjoints(2, 2, 1, 1);
    ordered_adjoints(7, 9, 11, 13);
    ordered_adjoints(3, 4, 40, 33);                             // segments beyond the insertion sort
    std::vector<uint32_t> v(1024 * 3 + 5, 3u);
    EXPECT(lerf_scan_exclusive_u32_host(v.data(), (int64_t)v.size()) == LERF_OK && v[0] == 0 && v.back() == 3u * (uint32_t)(v.size() - 1));
    EXPECT(lerf_scan_exclusive_u32_host(v.data(), 0) == LERF_EINVAL && lerf_scan_exclusive_u32_host(nullptr, 4) == LERF_EINVAL);
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
    batched_ops(1, 1);
    batched_ops(2, 2);
    batched_ops(5, 67);
    reproject_ops(1, 1);
    reproject_ops(2, 2);
    reproject_ops(5, 67);
    reproject_ops(70, 130);                                     // two bands x three column blocks of the adjoint's sums
    splat_ops(1, 1, 1, 1);
    splat_ops(1, 1, 5, 9);
    splat_ops(5, 67, 7, 61);
    splat_ops(23, 31, 29, 37);
    ordered_ops();
    trimesh_ops(1, 1);
    trimesh_ops(2, 2);
    trimesh_ops(5, 67);
    trimesh_ops(29, 37);
    std::printf(fails ? "%d check(s) failed\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
