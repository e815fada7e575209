// Fine-tuning path: the float32 LUT pass of the reference's trainable twin
// SWF2LUT.InterpTorchBatch (resample/model.py:172-385) and its backward.
//
// Forward: LUTq = clamp(rne(127 * weight), -127, 127); out = sum_n w_n * LUTq[idx_n] / q, the 4-simplex walk taking
// its MSBs from the mode's pattern pixels and its LSBs from `lsb` pattern pixels -- for modes c and t the reference
// reads the LSBs at the 'y' pattern positions (:229-232, :240-243); that is reproduced, not repaired.  All products and
// sums are integers below 2^24, so float32 is exact and the result equals the reference bit for bit.
//
// Backward (what torch autograd derives for the reference code):
//   d out / d weight[idx_n][oc] = 127 * w_n / q   where -127 <= rne(127 weight) <= 127 (round = BPDA identity, clamp gate)
//   d out / d img[LSB pixel of sorted axis n] = (P_{n+1} - P_n) / q      (torch.remainder passes the gradient through,
//   floor_divide does not).  Ties between LSBs: the reference's case chain puts the LATER axis first (fab = fa > fb ...),
//   so the sort key carries the axis number below the LSB.
// The backward of the SR resamplers that follow the LUT pass (train_model.py:431-441) is lerf_resize_bwd.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lerf_common.h"

namespace lerf {
namespace train {

struct Pattern { int dy[4], dx[4], ldy[4], ldx[4]; };

static bool make_pattern(char mode, Pattern* p) {
    int8_t dy[4], dx[4], ly[4], lx[4];
    if (!mode_pattern(mode, dy, dx)) return false;
    // LSB source pixels: own pattern for s, d, y; the 'y' pattern for c and t (model.py:229-232, 240-243)
    mode_pattern((mode == 'c' || mode == 't') ? 'y' : mode, ly, lx);
    for (int k = 0; k < 4; ++k) { p->dy[k] = dy[k]; p->dx[k] = dx[k]; p->ldy[k] = ly[k]; p->ldx[k] = lx[k]; }
    return true;
}

__device__ __forceinline__ float lutq(float w) { return fminf(fmaxf(rintf(w * 127.0f), -127.0f), 127.0f); }

struct Walk {
    int idx[5];     // LUT rows of the 5 corners
    int w[5];       // integer weights, sum = q
    int axis[4];    // axis (0..3 = a..d) stepped at sorted position n
};

// keys: (LSB << 4 | axis) << 16 | stride, sorted descending -> later axis first among equal LSBs
__device__ __forceinline__ Walk walk(const int m[4], const int f[4]) {
    unsigned k0 = ((unsigned)(f[0] << 4 | 0) << 16) | (unsigned)kStrideA;
    unsigned k1 = ((unsigned)(f[1] << 4 | 1) << 16) | (unsigned)kStrideB;
    unsigned k2 = ((unsigned)(f[2] << 4 | 2) << 16) | (unsigned)kStrideC;
    unsigned k3 = ((unsigned)(f[3] << 4 | 3) << 16) | (unsigned)kStrideD;
    ce_desc(k0, k1);
    ce_desc(k2, k3);
    ce_desc(k0, k2);
    ce_desc(k1, k3);
    ce_desc(k1, k2);
    const unsigned k[4] = {k0, k1, k2, k3};
    Walk r;
    r.idx[0] = m[0] * kStrideA + m[1] * kStrideB + m[2] * kStrideC + m[3];
    int fs[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        r.idx[n + 1] = r.idx[n] + (int)(k[n] & 0xffffu);
        fs[n] = (int)(k[n] >> 20);
        r.axis[n] = (int)((k[n] >> 16) & 3u);
    }
    r.w[0] = kQ - fs[0];
    r.w[1] = fs[0] - fs[1];
    r.w[2] = fs[1] - fs[2];
    r.w[3] = fs[2] - fs[3];
    r.w[4] = fs[3];
    return r;
}

__device__ __forceinline__ Walk walk_at(const float* __restrict__ plane, int wp, int y, int x, const Pattern& pt) {
    int m[4], f[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int vm = (int)plane[(y + pt.dy[k]) * wp + x + pt.dx[k]];
        const int vl = (int)plane[(y + pt.ldy[k]) * wp + x + pt.ldx[k]];
        m[k] = vm >> 4;          // floor_divide(img, q)
        f[k] = vl & 15;          // img % q
    }
    return walk(m, f);
}

template <int OC>
__global__ void __launch_bounds__(256)
interp_fwd_kernel(const float* __restrict__ weight, const float* __restrict__ img, int n_planes, int h, int w, int bd,
                  Pattern pt, float* __restrict__ out) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, p = blockIdx.z;
    if (x >= w) return;
    const int wp = w + bd;
    const Walk r = walk_at(img + (int64_t)p * (h + bd) * wp, wp, y, x, pt);
#pragma unroll
    for (int oc = 0; oc < OC; ++oc) {
        float acc = 0.0f;
#pragma unroll
        for (int n = 0; n < 5; ++n) acc += (float)r.w[n] * lutq(weight[(int64_t)r.idx[n] * OC + oc]);
        out[(((int64_t)p * OC + oc) * h + y) * w + x] = acc / (float)kQ;
    }
}

// Backward.  One workgroup owns a band of rows of one plane (about 4096 pixels).  Photo-like patches hit very few LUT
// rows (every pixel of a smooth region lands in the same 16-corner cell), and float atomics to one address serialise at
// the memory side of the 8 XCDs, so the LUT-row contributions are first summed in an LDS table keyed by the row
// (open slot claimed with an LDS compare-and-swap, ds_add_f32 into it; a key that finds its slot taken by another row
// goes to global memory directly) and flushed with one global atomic per occupied entry.  Worst case (uniform noise:
// more distinct rows than slots) costs what the direct version cost; a smooth batch needs ~20x fewer global atomics.
constexpr int BWD_NT = 1024;     // 16 waves per workgroup: the per-pixel chain (image reads -> LUT reads -> LDS CAS) is latency-bound
template <int OC, int LOG_TS>
__global__ void __launch_bounds__(1024)
interp_bwd_kernel(const float* __restrict__ weight, const float* __restrict__ img, const float* __restrict__ gout, int n_planes,
                  int h, int w, int bd, int rows_per_band, int bands, int gim_lds, Pattern pt, float* __restrict__ gweight,
                  float* __restrict__ gimg) {
    constexpr int TS = 1 << LOG_TS;
    __shared__ int tag[TS];
    __shared__ float val[TS * OC];
    extern __shared__ float gim[];          // image-gradient rows of the band (+ bd rows of pattern reach), when it fits
    const int tid = threadIdx.x;
    const int p = blockIdx.x / bands, band = blockIdx.x - p * bands;
    const int y0 = band * rows_per_band, y1 = min(h, y0 + rows_per_band);
    const int wp = w + bd;
    const int gim_n = gim_lds ? (y1 - y0 + bd) * wp : 0;
    for (int i = tid; i < TS; i += BWD_NT) tag[i] = -1;
    for (int i = tid; i < TS * OC; i += BWD_NT) val[i] = 0.0f;
    for (int i = tid; i < gim_n; i += BWD_NT) gim[i] = 0.0f;
    __syncthreads();
    const int64_t poff = (int64_t)p * (h + bd) * wp;
    for (int i = tid; i < (y1 - y0) * w; i += BWD_NT) {
        const int y = y0 + i / w, x = i % w;
        const Walk r = walk_at(img + poff, wp, y, x, pt);
        float g[OC], gf[4] = {0.0f, 0.0f, 0.0f, 0.0f};       // gf: d loss / d f at sorted position n
#pragma unroll
        for (int oc = 0; oc < OC; ++oc) g[oc] = gout[(((int64_t)p * OC + oc) * h + y) * w + x] / (float)kQ;
        float Pprev[OC];
#pragma unroll
        for (int n = 0; n < 5; ++n) {
            const int row = r.idx[n];
            int slot = -1;
            if (gweight && r.w[n] != 0) {
                const int s = (int)(((unsigned)row * 2654435761u) >> (32 - LOG_TS));
                const int old = atomicCAS(&tag[s], -1, row);
                slot = (old == -1 || old == row) ? s : -2;      // -2: table slot belongs to another row
            }
#pragma unroll
            for (int oc = 0; oc < OC; ++oc) {
                const float rq = rintf(weight[(int64_t)row * OC + oc] * 127.0f);
                const float Pn = fminf(fmaxf(rq, -127.0f), 127.0f);
                if (slot != -1 && rq >= -127.0f && rq <= 127.0f) {
                    const float c = g[oc] * (float)r.w[n] * 127.0f;
                    if (slot >= 0) atomicAdd(&val[slot * OC + oc], c);
                    else atomicAdd(gweight + (int64_t)row * OC + oc, c);
                }
                if (n > 0) gf[n - 1] += g[oc] * (Pn - Pprev[oc]);
                Pprev[oc] = Pn;
            }
        }
        if (gimg) {
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int a = r.axis[n];
                if (gim_lds) atomicAdd(&gim[(y - y0 + pt.ldy[a]) * wp + x + pt.ldx[a]], gf[n]);
                else atomicAdd(gimg + poff + (y + pt.ldy[a]) * wp + x + pt.ldx[a], gf[n]);
            }
        }
    }
    __syncthreads();
    if (gimg && gim_lds) {
        // the band's rows of the plane: exclusive when the plane is one band, shared halo rows otherwise
        float* dst = gimg + poff + (int64_t)y0 * wp;
        for (int i = tid; i < gim_n; i += BWD_NT) {
            const float v = gim[i];
            if (v != 0.0f) {
                if (bands == 1) dst[i] += v;
                else atomicAdd(dst + i, v);
            }
        }
    }
    if (gweight)
        for (int s = tid; s < TS; s += BWD_NT) {
            const int row = tag[s];
            if (row >= 0) {
#pragma unroll
                for (int oc = 0; oc < OC; ++oc) {
                    const float v = val[s * OC + oc];
                    if (v != 0.0f) atomicAdd(gweight + (int64_t)row * OC + oc, v);
                }
            }
        }
}

}  // namespace train
}  // namespace lerf

using namespace lerf::train;

extern "C" {

int lerf_swf2lut_interp_f32(const float* weight, int oC, char mode, const float* img, int n_planes, int h, int w, int bd,
                            float* out, void* stream) {
    Pattern pt;
    if (!weight || !img || !out || n_planes < 1 || h < 1 || w < 1 || bd < 0) return LERF_EINVAL;
    if (!make_pattern(mode, &pt)) return LERF_EINVAL;
    for (int k = 0; k < 4; ++k)
        if (pt.dy[k] > bd || pt.dx[k] > bd || pt.ldy[k] > bd || pt.ldx[k] > bd) return LERF_EINVAL;
    dim3 block(256), grid((w + 255) / 256, h, n_planes);
    hipStream_t st = (hipStream_t)stream;
    if (oC == 1) hipLaunchKernelGGL(interp_fwd_kernel<1>, grid, block, 0, st, weight, img, n_planes, h, w, bd, pt, out);
    else if (oC == 3) hipLaunchKernelGGL(interp_fwd_kernel<3>, grid, block, 0, st, weight, img, n_planes, h, w, bd, pt, out);
    else return LERF_EUNSUPPORTED;
    return lerf::launch_status();
}

int lerf_swf2lut_interp_bwd_f32(const float* weight, int oC, char mode, const float* img, const float* grad_out, int n_planes,
                                int h, int w, int bd, float* grad_weight, float* grad_img, void* stream) {
    Pattern pt;
    if (!weight || !img || !grad_out || n_planes < 1 || h < 1 || w < 1 || bd < 0) return LERF_EINVAL;
    if (!make_pattern(mode, &pt)) return LERF_EINVAL;
    for (int k = 0; k < 4; ++k)
        if (pt.dy[k] > bd || pt.dx[k] > bd || pt.ldy[k] > bd || pt.ldx[k] > bd) return LERF_EINVAL;
    // bands of about 4096 pixels per workgroup
    int rows_per_band = 4096 / w;
    if (rows_per_band < 1) rows_per_band = 1;
    if (rows_per_band > h) rows_per_band = h;
    const int bands = (h + rows_per_band - 1) / rows_per_band;
    dim3 block(BWD_NT), grid((unsigned)(n_planes * bands));
    hipStream_t st = (hipStream_t)stream;
    size_t gim_bytes = grad_img ? (size_t)(rows_per_band + bd) * (size_t)(w + bd) * sizeof(float) : 0;
    const int gim_lds = gim_bytes > 0 && gim_bytes <= 40 * 1024;
    if (!gim_lds) gim_bytes = 0;
    if (oC == 1)
        hipLaunchKernelGGL((interp_bwd_kernel<1, 12>), grid, block, gim_bytes, st, weight, img, grad_out, n_planes, h, w, bd, rows_per_band,
                           bands, gim_lds, pt, grad_weight, grad_img);
    else if (oC == 3)
        hipLaunchKernelGGL((interp_bwd_kernel<3, 12>), grid, block, gim_bytes, st, weight, img, grad_out, n_planes, h, w, bd, rows_per_band,
                           bands, gim_lds, pt, grad_weight, grad_img);
    else
        return LERF_EUNSUPPORTED;
    return lerf::launch_status();
}

}  // extern "C"
