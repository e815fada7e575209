// Host-side dispatch shared by the stage-3 launches (SR resize, homographic warp, remap; forward, packed, batched, backward):
// run-time kind / flag -> compile-time template argument, the operand types and arithmetic of warp and remap, and the C ABI's
// warp geometry as the kernels take it.  Host code only.
#pragma once

#include <string.h>

#include <type_traits>

#include "lerf_kernels.h"

namespace lerf {

// One convention for every dispatcher here: f is a generic lambda that takes the compile-time tag and returns a LERF_* code
// (LERF_OK after a launch), and the dispatcher returns that code, or LERF_EUNSUPPORTED for a value outside its set.
//
// with_*_kind: the tag is std::integral_constant<int, LERF_KIND_*>.  A call site instantiates its kernel for every kind of the
// set it names, so a site that serves the two kinds with hyper-parameter maps only takes with_hyper_kind, not with_kind.
template <int K>
using kind_c = std::integral_constant<int, K>;

template <typename F>
inline int with_hyper_kind(int kind, F&& f) {
    switch (kind) {
        case LERF_KIND_GAUSS: return f(kind_c<LERF_KIND_GAUSS>{});
        case LERF_KIND_LINEAR: return f(kind_c<LERF_KIND_LINEAR>{});
    }
    return LERF_EUNSUPPORTED;
}

template <typename F>
inline int with_fixed_kind(int kind, F&& f) {
    switch (kind) {
        case LERF_KIND_NEAREST: return f(kind_c<LERF_KIND_NEAREST>{});
        case LERF_KIND_CUBIC: return f(kind_c<LERF_KIND_CUBIC>{});
        case LERF_KIND_BILINEAR: return f(kind_c<LERF_KIND_BILINEAR>{});
        case LERF_KIND_LANCZOS2: return f(kind_c<LERF_KIND_LANCZOS2>{});
        case LERF_KIND_LANCZOS3: return f(kind_c<LERF_KIND_LANCZOS3>{});
    }
    return LERF_EUNSUPPORTED;
}

template <typename F>
inline int with_kind(int kind, F&& f) {
    return kind == LERF_KIND_GAUSS || kind == LERF_KIND_LINEAR ? with_hyper_kind(kind, f) : with_fixed_kind(kind, f);
}

template <typename F>
inline int with_bool(bool flag, F&& f) {
    return flag ? f(std::true_type{}) : f(std::false_type{});
}

// Operand types of the strided stage-3 warps (lerf_warp, lerf_remap): image, hyper-parameter maps, output, arithmetic.
// `fixed`: a kind without hyper-parameter maps, whose h_dtype is not read.
template <typename TI_, typename TH_, typename TO_, typename A_>
struct Stage3Types {
    using TI = TI_; using TH = TH_; using TO = TO_; using A = A_;
};

template <typename F>
inline int with_stage3_types(int in_dtype, int h_dtype, int out_dtype, bool fixed, F&& f) {
    if (in_dtype == LERF_U8 && (h_dtype == LERF_U8 || fixed)) {
        if (out_dtype == LERF_U8) return f(Stage3Types<uint8_t, uint8_t, uint8_t, float>{});
        if (out_dtype == LERF_F32) return f(Stage3Types<uint8_t, uint8_t, float, double>{});     // float64 arithmetic, rounded once
        if (out_dtype == LERF_F64) return f(Stage3Types<uint8_t, uint8_t, double, double>{});
    } else if (in_dtype == LERF_F32 && (h_dtype == LERF_F32 || fixed)) {
        if (out_dtype == LERF_F32) return f(Stage3Types<float, float, float, double>{});
        if (out_dtype == LERF_F64) return f(Stage3Types<float, float, double, double>{});
    }
    return LERF_EUNSUPPORTED;
}

inline WarpGeo to_warp_geo(const lerf_warp_geo_t& geo) {
    WarpGeo g{};
    g.S = geo.S; g.oH = geo.out_h; g.oW = geo.out_w;
    memcpy(g.minv, geo.minv, sizeof(g.minv));
    g.pad_r_lo = geo.pad_r_lo; g.pad_r_hi = geo.pad_r_hi; g.pad_c_lo = geo.pad_c_lo; g.pad_c_hi = geo.pad_c_hi;
    g.pad_mode = geo.pad_mode;
    g.oy0 = geo.out_y0; g.ox0 = geo.out_x0;
    return g;
}

}  // namespace lerf
