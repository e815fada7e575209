// LeRF-Net on MI355X (gfx950): the forward of one IMDN_RTC net (the reference's resample/model.py:434-537 at upscale 1,
// one stage of IMDN2), the dense-convolution hyper-parameter predictor of LeRF-Net / LeRF-Net++.
//
// Reference being replaced: nn.Sequential(fea_conv, ShortcutBlock(5 x IMDModule_speed + LR_conv), upsampler conv) run as
// stock cuDNN convolutions with zero padding (k-1)/2.  Here every convolution is one launch of imdn_conv_kernel, an
// implicit GEMM on the float32-input MFMA (v_mfma_f32_16x16x4_f32: exact float32 products, float32 sums): rows are output
// pixels, columns output channels, and K runs over (tap, input channel); each tap's neighbour is zero outside the image,
// so every layer pads its own input.  A workgroup owns 128 consecutive pixels of the flattened [B][H][W] grid (a wave
// 32 of them, two 16-row blocks) and all output channels (up to four 16-column blocks), so any B, H, W tiles without a
// border case beyond the per-tap bounds check, and image b never reads image b' (batch independence).
//
// The epilogue is fused: bias, LeakyReLU(0.05) for c1..c3, the residual add (module input after c5, fea after LR_conv)
// and, on the last conv, the `predict` clamp and affine.  Split and concat are addressing: channels below `split` go to
// one NHWC destination (c1..c4 write their distilled channels straight into the 4d-channel buffer c5 reads), the rest
// to another (the remaining channels the next conv reads).  The 1x1 convolutions run in place (a pixel's inputs are read
// by the wave that writes it, before it writes).  No atomics, a fixed summation order: the output is deterministic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lerf_imdn_conv.h"
#include "lerf_imdn_layout.h"
#include "lerf_kernels.h"

namespace lerf {
namespace imdn {

constexpr int NT = 256;              // 4 waves
constexpr int PIX = 128;             // output pixels per workgroup (32 per wave)
typedef float floatx4 __attribute__((ext_vector_type(4)));

__device__ inline floatx4 mfma4(float a, float b, floatx4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

template <int NB, int KK>
__global__ void __launch_bounds__(NT) imdn_conv_kernel(ConvArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    const int64_t base = (int64_t)blockIdx.x * PIX + wave * 32;
    const int64_t HW = (int64_t)a.H * a.W;
    // 16x16x4 operands: A[i][k] from lane i + 16 k, B[k][j] from lane j + 16 k; D[4 (lane/16) + reg][lane % 16]
    int pb[2], py[2], px[2];
    bool pv[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int64_t p = base + q * 16 + li;
        pv[q] = p < a.n_pix;
        const int64_t b = pv[q] ? p / HW : 0, yx = pv[q] ? p - b * HW : 0;
        pb[q] = (int)b;
        py[q] = (int)(yx / a.W);
        px[q] = (int)(yx - (int64_t)py[q] * a.W);
    }
    floatx4 acc[2][NB];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[q][nb] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
    const float* __restrict__ w = a.w;
#pragma unroll 1
    for (int tap = 0; tap < KK; ++tap) {
        const int dy = KK == 9 ? tap / 3 - 1 : 0, dx = KK == 9 ? tap % 3 - 1 : 0;
        const float* ap[2];
        bool av[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int yy = py[q] + dy, xx = px[q] + dx;
            av[q] = pv[q] && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
            ap[q] = a.in.p + (int64_t)pb[q] * a.in.sb + ((int64_t)yy * a.W + xx) * a.in.sp;
        }
#pragma unroll 2
        for (int c0 = 0; c0 < a.cin; c0 += 4) {
            const int c = c0 + lk;
            const bool cv = c < a.cin;
            const float a0 = av[0] && cv ? ap[0][c * a.in.sc] : 0.0f;
            const float a1 = av[1] && cv ? ap[1][c * a.in.sc] : 0.0f;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int n = nb * 16 + li;
                const float bv = cv && n < a.cout ? w[((int64_t)n * a.cin + c) * KK + tap] : 0.0f;
                acc[0][nb] = mfma4(a0, bv, acc[0][nb]);
                acc[1][nb] = mfma4(a1, bv, acc[1][nb]);
            }
        }
    }
    const float* bias = w + (int64_t)a.cout * a.cin * KK;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int n = nb * 16 + li;
        if (n >= a.cout) continue;
        const float bn = bias[n];
        const View& o = n < a.split ? a.lo : a.hi;
        const int no = n < a.split ? n : n - a.split;
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t p = base + q * 16 + 4 * lk + r;
                if (p >= a.n_pix) continue;
                const int64_t b = p / HW, yx = p - b * HW;
                float v = __fadd_rn(acc[q][nb][r], bn);
                if (a.act) v = v > 0.0f ? v : __fmul_rn(v, 0.05f);
                if (a.res) v = __fadd_rn(v, a.res[b * a.lo.sb + yx * a.lo.sp + (int64_t)n * a.lo.sc]);
                if (a.post) {
                    v = fminf(fmaxf(v, -1.0f), 1.0f);
                    v = a.post == 1 ? __fadd_rn(__fmul_rn(v, 127.0f), 127.0f) : __fadd_rn(__fmul_rn(v, 0.5f), 0.5f);
                }
                o.p[b * o.sb + yx * o.sp + (int64_t)no * o.sc] = v;
            }
    }
}

template <int KK>
void launch_conv(const ConvArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)((a.n_pix + PIX - 1) / PIX));
    switch ((a.cout + 15) / 16) {
    case 1: hipLaunchKernelGGL((imdn_conv_kernel<1, KK>), grid, dim3(NT), 0, st, a); break;
    case 2: hipLaunchKernelGGL((imdn_conv_kernel<2, KK>), grid, dim3(NT), 0, st, a); break;
    case 3: hipLaunchKernelGGL((imdn_conv_kernel<3, KK>), grid, dim3(NT), 0, st, a); break;
    default: hipLaunchKernelGGL((imdn_conv_kernel<4, KK>), grid, dim3(NT), 0, st, a); break;
    }
}

void launch_conv(const ConvArgs& a, bool k3, hipStream_t st) {
    if (k3) launch_conv<9>(a, st);
    else launch_conv<1>(a, st);
}

}  // namespace imdn

size_t imdn_weight_floats(int nf, int in_nc, int out_nc) { return (size_t)imdn::weight_floats(nf, in_nc, out_nc); }

size_t imdn_workspace_bytes(int nf, int B, int H, int W) {
    return (size_t)B * H * W * imdn::ws_floats_per_pixel(nf) * sizeof(float);
}

int launch_imdn_fwd(const float* weights, int nf, int in_nc, int out_nc, const float* x, int B, int H, int W, int post,
                    void* workspace, float* out, hipStream_t st) {
    using namespace imdn;
    const int d = nf / 4, r = nf - d;
    const int64_t P = (int64_t)B * H * W, HW = (int64_t)H * W;
    float* fea = static_cast<float*>(workspace);
    float* h = fea + P * nf;
    float* cat = h + P * nf;
    float* r1 = cat + P * nf;
    float* r2 = r1 + P * r;
    auto nhwc = [&](float* p, int pitch) { return View{p, HW * pitch, pitch, 1}; };
    auto conv = [&](int off, int cin, int cout, int split, View in, View lo, View hi, const float* res, int act, int pst,
                    bool k3) {
        ConvArgs a{weights + off, cin, cout, split, in, lo, hi, res, act, pst, H, W, P};
        launch_conv(a, k3, st);
    };
    const View none{nullptr, 0, 0, 0};
    // fea_conv, reading the NCHW input
    conv(0, in_nc, nf, nf, View{const_cast<float*>(x), (int64_t)in_nc * HW, 1, HW}, nhwc(fea, nf), none, nullptr, 0, 0, true);
    for (int m = 0; m < MODULES; ++m) {
        float* hin = m == 0 ? fea : h;
        conv(off_conv(nf, in_nc, m, 1), nf, nf, d, nhwc(hin, nf), nhwc(cat, nf), nhwc(r1, r), nullptr, 1, 0, true);
        conv(off_conv(nf, in_nc, m, 2), r, nf, d, nhwc(r1, r), nhwc(cat + d, nf), nhwc(r2, r), nullptr, 1, 0, true);
        conv(off_conv(nf, in_nc, m, 3), r, nf, d, nhwc(r2, r), nhwc(cat + 2 * d, nf), nhwc(r1, r), nullptr, 1, 0, true);
        conv(off_conv(nf, in_nc, m, 4), r, d, d, nhwc(r1, r), nhwc(cat + 3 * d, nf), none, nullptr, 0, 0, true);
        conv(off_conv(nf, in_nc, m, 5), nf, nf, nf, nhwc(cat, nf), nhwc(h, nf), none, hin, 0, 0, false);
    }
    conv(off_lr(nf, in_nc), nf, nf, nf, nhwc(h, nf), nhwc(h, nf), none, fea, 0, 0, false);       // LR_conv + fea (in place)
    conv(off_up(nf, in_nc), nf, out_nc, out_nc, nhwc(h, nf), View{out, (int64_t)out_nc * HW, 1, HW}, none, nullptr, 0, post,
         true);
    return LERF_OK;
}

}  // namespace lerf
