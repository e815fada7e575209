// Packed weight layout of one IMDN_RTC net (the reference's resample/model.py:434-537, upscale 1: one stage of IMDN2),
// shared by lerf_imdn.hip and the host entry points: the state_dict tensors in state_dict order, each flattened in
// PyTorch's [out][in][kh][kw] order,
//   model.0       W[nf][in_nc][3][3] b[nf]                               fea_conv
//   model.1.sub.m (m = 0..4, IMDModule_speed, d = nf/4, r = nf - d)
//                 c1 W[nf][nf][3][3] b[nf]  c2 W[nf][r][3][3] b[nf]  c3 W[nf][r][3][3] b[nf]
//                 c4 W[d][r][3][3] b[d]     c5 W[nf][4d][1][1] b[nf]
//   model.1.sub.5 W[nf][nf][1][1] b[nf]                                  LR_conv
//   model.2       W[out_nc][nf][3][3] b[out_nc]                          upsampler conv (PixelShuffle(1) = identity)
#pragma once

namespace lerf {
namespace imdn {

constexpr int MODULES = 5;

__host__ __device__ constexpr int conv_floats(int cout, int cin, int kk) { return cout * cin * kk + cout; }

// floats of one IMDModule_speed
__host__ __device__ constexpr int module_floats(int nf) {
    return conv_floats(nf, nf, 9) + 2 * conv_floats(nf, nf - nf / 4, 9) + conv_floats(nf / 4, nf - nf / 4, 9) +
           conv_floats(nf, nf, 1);
}

__host__ __device__ constexpr int off_module(int nf, int in_nc, int m) { return conv_floats(nf, in_nc, 9) + m * module_floats(nf); }

// offset of conv j (1..5 = c1..c5) inside module m
__host__ __device__ constexpr int off_conv(int nf, int in_nc, int m, int j) {
    const int d = nf / 4, r = nf - d;
    int o = off_module(nf, in_nc, m);
    if (j > 1) o += conv_floats(nf, nf, 9);
    if (j > 2) o += conv_floats(nf, r, 9);
    if (j > 3) o += conv_floats(nf, r, 9);
    if (j > 4) o += conv_floats(d, r, 9);
    return o;
}

__host__ __device__ constexpr int off_lr(int nf, int in_nc) { return off_module(nf, in_nc, MODULES); }
__host__ __device__ constexpr int off_up(int nf, int in_nc) { return off_lr(nf, in_nc) + conv_floats(nf, nf, 1); }
__host__ __device__ constexpr int weight_floats(int nf, int in_nc, int out_nc) { return off_up(nf, in_nc) + conv_floats(out_nc, nf, 9); }

// floats per pixel of the NHWC workspace: fea, h, the concatenated distilled channels (4d = nf), two remaining planes (r)
__host__ __device__ constexpr int ws_floats_per_pixel(int nf) { return 3 * nf + 2 * (nf - nf / 4); }

}  // namespace imdn
}  // namespace lerf
