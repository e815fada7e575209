// One axis pass of the separable, anti-aliased resize (resize_right/resize_right.py:221-252, apply_weights) and its adjoint:
//   out[o, j, i] = sum_k w[j][k] * in[o, src(left[j] + k), i]          tensor viewed as [outer][n][inner], contiguous
// src() is the image pad rule (source_tap, lerf_host_geometry.h); a tap in a constant pad contributes w * 0.  The tables
// (left, w) are built by the host, O(n_out * taps); the number of taps is a run-time value (x1/8 cubic: 32, Lanczos-3: 48).
// The sum runs over the taps in tap order, every product and every sum rounded on its own (no FMA contraction): numpy adds
// the reference's tap slices in that order, and at x1/3 byte equality near rounding ties depends on it.
// The adjoint is the same gather over a CSR table (for each source index its outputs and weights, built by
// host::rr_adjoint_csr with padded taps folded onto their source index): no atomics, fixed order.
//
// Two lane mappings:
//   wide   (inner >= 64): lanes along `inner`, four elements per lane 256 apart (coalesced); j and the outer index are
//          uniform per workgroup, so left[j], the weights and the source indices are scalar loads and live in SGPRs.
//   narrow (inner < 64, the last-dim pass at inner = 1): a workgroup owns 256 / inner consecutive outputs of one outer
//          slice; lanes run along (j, i).  Neighbouring lanes read overlapping taps, so the source segment
//          [left[j0], left[j1] + taps) is staged once in LDS, converted to the accumulator type and with the pad rule
//          applied; a segment that does not fit (or any CSR pass) reads global memory instead.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lerf_common.h"

namespace lerf {
namespace rr {

constexpr int kThreads = 256;
constexpr int kVec = 4;                // wide: elements per lane
constexpr int kWin = 4096;             // narrow: LDS segment, in accumulator elements (32 KB of float64)

template <typename T>
__device__ __forceinline__ T rr_store(double v);
template <>
__device__ __forceinline__ double rr_store<double>(double v) { return v; }
template <>
__device__ __forceinline__ float rr_store<float>(double v) { return (float)v; }
// np.round(np.clip(x, 0, 255)).astype(np.uint8): round half to even (v_rndne_f64)
template <>
__device__ __forceinline__ uint8_t rr_store<uint8_t>(double v) {
    v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
    return (uint8_t)(int)rint(v);
}

template <typename TA, typename TO>
__device__ __forceinline__ TO rr_out(TA v) {
    if constexpr (sizeof(TO) == 1) return rr_store<uint8_t>((double)v);
    else return (TO)v;
}

struct Axis {
    int n_in, n_out, taps, pad_mode;
    const int32_t* left;       // forward form
    const int32_t* row_ptr;    // CSR form (taps == 0)
    const int32_t* idx;
};

template <typename TI, typename TA, typename TO, bool CSR>
__global__ void __launch_bounds__(kThreads)
rr_wide_kernel(const TI* __restrict__ in, TO* __restrict__ out, const TA* __restrict__ w, Axis ax, int64_t outer, int64_t inner) {
#pragma clang fp contract(off)
    const int64_t i0 = (int64_t)blockIdx.x * (kThreads * kVec) + threadIdx.x;
    for (int64_t o = blockIdx.z; o < outer; o += gridDim.z) {
        const TI* __restrict__ src = in + o * ax.n_in * inner;
        for (int j = blockIdx.y; j < ax.n_out; j += gridDim.y) {
            int e0, cnt, l = 0;
            if (CSR) {
                e0 = ax.row_ptr[j];
                cnt = ax.row_ptr[j + 1] - e0;
            } else {
                e0 = j * ax.taps;
                cnt = ax.taps;
                l = ax.left[j];
            }
            TA acc[kVec];
#pragma unroll
            for (int v = 0; v < kVec; ++v) acc[v] = (TA)0;
            for (int k = 0; k < cnt; ++k) {
                const TA wk = w[e0 + k];
                int s;
                bool z = false;
                if (CSR) {
                    s = ax.idx[e0 + k];
                } else {
                    const SourceTap t = source_tap(l + k, ax.n_in, ax.pad_mode);
                    s = t.s;
                    z = t.z;
                }
                const TI* __restrict__ row = src + (int64_t)s * inner;
#pragma unroll
                for (int v = 0; v < kVec; ++v) {
                    const int64_t i = i0 + v * kThreads;
                    const TA x = (z || i >= inner) ? (TA)0 : (TA)row[i];
                    const TA p = wk * x;
                    acc[v] = acc[v] + p;
                }
            }
            TO* __restrict__ dst = out + (o * ax.n_out + j) * inner;
#pragma unroll
            for (int v = 0; v < kVec; ++v) {
                const int64_t i = i0 + v * kThreads;
                if (i < inner) dst[i] = rr_out<TA, TO>(acc[v]);
            }
        }
    }
}

template <typename TI, typename TA, typename TO, bool CSR>
__global__ void __launch_bounds__(kThreads)
rr_narrow_kernel(const TI* __restrict__ in, TO* __restrict__ out, const TA* __restrict__ w, Axis ax, int64_t outer, int inner, int jt) {
#pragma clang fp contract(off)
    __shared__ TA win[CSR ? 1 : kWin];
    const int tid = threadIdx.x;
    const int j0 = blockIdx.x * jt;
    const int j1 = min(j0 + jt, ax.n_out) - 1;
    const int jl = tid / inner, i = tid - jl * inner, j = j0 + jl;
    const bool active = jl < jt && j <= j1;
    int lo = 0, span = 0;
    bool lds = false;
    if (!CSR) {
        lo = ax.left[j0];
        const int64_t sp = (int64_t)ax.left[j1] + ax.taps - lo;       // exact for a monotone grid; any other order: taps outside it read global
        lds = sp > 0 && sp * inner <= kWin;
        span = lds ? (int)sp : 0;
    }
    for (int64_t o = blockIdx.y; o < outer; o += gridDim.y) {
        const TI* __restrict__ src = in + o * ax.n_in * inner;
        if (lds) {
            __syncthreads();                                          // the previous slice's readers are done
            for (int e = tid; e < span * inner; e += kThreads) {
                const int p = e / inner, c = e - p * inner;
                const SourceTap t = source_tap(lo + p, ax.n_in, ax.pad_mode);
                win[e] = t.z ? (TA)0 : (TA)src[(int64_t)t.s * inner + c];
            }
            __syncthreads();
        }
        if (!active) continue;
        int e0, cnt, l = 0;
        if (CSR) {
            e0 = ax.row_ptr[j];
            cnt = ax.row_ptr[j + 1] - e0;
        } else {
            e0 = j * ax.taps;
            cnt = ax.taps;
            l = ax.left[j];
        }
        TA acc = (TA)0;
        for (int k = 0; k < cnt; ++k) {
            const TA wk = w[e0 + k];
            TA x;
            const int p = l + k - lo;
            if (!CSR && lds && p >= 0 && p < span) {
                x = win[p * inner + i];
            } else if (CSR) {
                x = (TA)src[(int64_t)ax.idx[e0 + k] * inner + i];
            } else {
                const SourceTap t = source_tap(l + k, ax.n_in, ax.pad_mode);
                x = t.z ? (TA)0 : (TA)src[(int64_t)t.s * inner + i];
            }
            const TA pr = wk * x;
            acc = acc + pr;
        }
        out[(o * ax.n_out + j) * inner + i] = rr_out<TA, TO>(acc);
    }
}

template <typename TI, typename TA, typename TO>
static int launch(const void* in, void* out, const void* w, const Axis& ax, int64_t outer, int64_t inner, hipStream_t st) {
    const bool csr = ax.taps == 0;
    if (inner >= 64) {
        const int64_t gx = (inner + kThreads * kVec - 1) / (kThreads * kVec);
        if (gx > 0x7fffffff) return LERF_EUNSUPPORTED;
        dim3 grid((unsigned)gx, (unsigned)min(ax.n_out, 65535), (unsigned)(outer < 65535 ? outer : 65535));
        if (csr) hipLaunchKernelGGL((rr_wide_kernel<TI, TA, TO, true>), grid, dim3(kThreads), 0, st, (const TI*)in, (TO*)out, (const TA*)w, ax, outer, inner);
        else hipLaunchKernelGGL((rr_wide_kernel<TI, TA, TO, false>), grid, dim3(kThreads), 0, st, (const TI*)in, (TO*)out, (const TA*)w, ax, outer, inner);
    } else {
        const int jt = kThreads / (int)inner;
        dim3 grid((unsigned)((ax.n_out + jt - 1) / jt), (unsigned)(outer < 65535 ? outer : 65535));
        if (csr) hipLaunchKernelGGL((rr_narrow_kernel<TI, TA, TO, true>), grid, dim3(kThreads), 0, st, (const TI*)in, (TO*)out, (const TA*)w, ax, outer, (int)inner, jt);
        else hipLaunchKernelGGL((rr_narrow_kernel<TI, TA, TO, false>), grid, dim3(kThreads), 0, st, (const TI*)in, (TO*)out, (const TA*)w, ax, outer, (int)inner, jt);
    }
    return LERF_OK;
}

template <typename TA>
static int launch_acc(const void* in, int in_dtype, void* out, int out_dtype, const void* w, const Axis& ax, int64_t outer, int64_t inner,
                      hipStream_t st) {
    constexpr int acc_dtype = sizeof(TA) == 8 ? LERF_F64 : LERF_F32;
    if (out_dtype == LERF_U8) {
        // the LR-making epilogue: uint8 from the float64 result of the last pass
        if (acc_dtype != LERF_F64) return LERF_EUNSUPPORTED;
        switch (in_dtype) {
            case LERF_U8: return launch<uint8_t, double, uint8_t>(in, out, w, ax, outer, inner, st);
            case LERF_F32: return launch<float, double, uint8_t>(in, out, w, ax, outer, inner, st);
            case LERF_F64: return launch<double, double, uint8_t>(in, out, w, ax, outer, inner, st);
        }
        return LERF_EINVAL;
    }
    if (out_dtype != acc_dtype) return LERF_EUNSUPPORTED;
    switch (in_dtype) {
        case LERF_U8: return launch<uint8_t, TA, TA>(in, out, w, ax, outer, inner, st);
        case LERF_F32: return launch<float, TA, TA>(in, out, w, ax, outer, inner, st);
        case LERF_F64: return launch<double, TA, TA>(in, out, w, ax, outer, inner, st);
    }
    return LERF_EINVAL;
}

}  // namespace rr
}  // namespace lerf

using namespace lerf;

extern "C" {

int lerf_rr_adjoint_csr(int n_in, int n_out, int taps, const int32_t* left, const void* w, int w_dtype, int pad_mode,
                        int32_t* row_ptr, int32_t* idx, void* wt) {
    return host::rr_adjoint_csr(n_in, n_out, taps, left, w, w_dtype, pad_mode, row_ptr, idx, wt);
}

int lerf_rr_axis(const void* in, int in_dtype, int64_t outer, int64_t inner, const lerf_rr_axis_t* axis, int acc_dtype,
                 void* out, int out_dtype, void* stream) {
    if (!in || !out || !axis || !axis->w || outer < 1 || inner < 1 || axis->n_in < 1 || axis->n_out < 1) return LERF_EINVAL;
    if (axis->taps < 0 || (axis->taps > 0 && !axis->left) || (axis->taps == 0 && (!axis->row_ptr || !axis->idx))) return LERF_EINVAL;
    if (axis->pad_mode < LERF_PAD_CONSTANT || axis->pad_mode > LERF_PAD_WRAP) return LERF_EINVAL;
    if (axis->taps > 0 && (int64_t)axis->n_out * axis->taps > 0x7fffffff) return LERF_EUNSUPPORTED;
    rr::Axis ax;
    ax.n_in = axis->n_in;
    ax.n_out = axis->n_out;
    ax.taps = axis->taps;
    ax.pad_mode = axis->pad_mode;
    ax.left = axis->left;
    ax.row_ptr = axis->row_ptr;
    ax.idx = axis->idx;
    clear_stale_error();
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (acc_dtype == LERF_F64) rc = rr::launch_acc<double>(in, in_dtype, out, out_dtype, axis->w, ax, outer, inner, st);
    else if (acc_dtype == LERF_F32) rc = rr::launch_acc<float>(in, in_dtype, out, out_dtype, axis->w, ax, outer, inner, st);
    else return LERF_EINVAL;
    if (rc != LERF_OK) return rc;
    return launch_status();
}

}  // extern "C"
