// Packed weight layout of one SRNet hyper-network (common/network.py:40-163: SRUnit conv1 + ReLU, four dense 1x1 layers
// with concatenation, conv6 + tanh), shared by the net -> LUT transfer (lerf_transfer.hip) and the trainable net
// (lerf_srnet.hip): the state_dict tensors of one SRNet flattened in module order,
//   W1[64][4] b1[64] W2[64][64] b2[64] W3[64][128] b3[64] W4[64][192] b4[64] W5[64][256] b5[64] W6[outC][320] b6[outC].
// A weight gradient in the same layout is what lerf_srnet_bwd_f32 accumulates.
#pragma once

namespace lerf {
namespace srnet {

constexpr int NF = 64;               // hidden width (option.py: --nf 64)
constexpr int ACT = 5 * NF;          // 320 concatenated activations feeding conv6

// input width of layer 1..6: 4 sampled pixels, then 64, 128, 192, 256 concatenated activations, then 320
__host__ __device__ constexpr int layer_in(int layer) { return layer == 1 ? 4 : (layer - 1) * NF; }

__host__ __device__ constexpr int off_w(int layer) {      // layer 1..6 -> offset of W_layer; b_layer follows W_layer
    int o = 0;
    for (int l = 1; l < layer; ++l) o += NF * layer_in(l) + NF;
    return o;
}

__host__ __device__ constexpr int off_b(int layer, int outC) { return off_w(layer) + (layer == 6 ? outC : NF) * layer_in(layer); }

__host__ __device__ constexpr int weight_floats(int outC) { return off_w(6) + outC * ACT + outC; }

}  // namespace srnet
}  // namespace lerf
