// The convolution launch of the LeRF-Net forward (lerf_imdn.hip), shared with the training entry points (lerf_imdn_bwd.hip):
// strided tensor views, the arguments of one imdn_conv_kernel launch, and the launcher.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lerf {
namespace imdn {

// a [B][C][H][W] tensor in any channel order: element (b, y, x, c) at p + b sb + (y W + x) sp + c sc
struct View {
    float* p;
    int64_t sb, sp, sc;
};

struct ConvArgs {
    const float* w;                  // [cout][cin][KK] (PyTorch order), then bias[cout]
    int cin, cout, split;            // channels n < split go to lo (channel n), the others to hi (channel n - split)
    View in, lo, hi;
    const float* res;                // nullable: added after the activation, laid out like lo
    int act, post;                   // act: LeakyReLU(0.05); post: 0 raw, 1 clamp * 127 + 127, 2 clamp / 2 + 1/2
    int H, W;
    int64_t n_pix;                   // B H W
};

// one launch of imdn_conv_kernel: a 3x3 (k3) or 1x1 convolution with its fused epilogue
void launch_conv(const ConvArgs& a, bool k3, hipStream_t st);

}  // namespace imdn
}  // namespace lerf
