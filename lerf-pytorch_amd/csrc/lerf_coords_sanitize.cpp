// Stand-alone sanitizer driver of the HOST twins of the fisheye and equirect models (`make asan-coords`): lerf_coords.hip is compiled
// with AddressSanitizer + UndefinedBehaviorSanitizer on its host side and linked with this main, which calls lerf_coords_build_host,
// lerf_coords_build_bwd_host and lerf_coords_math_host on exactly-sized heap buffers -- strided tiles with an origin, both dtypes, a
// batch of sets, the special arguments of the helpers, the refusals.  It needs no GPU and is never loaded into another process.
// Exit status 0 and "ok" on the last line: no report.
#include "lerf_hip.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

static int fails = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { ++fails; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } \
    } while (0)

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
    std::printf(fails ? "%d check(s) failed\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
