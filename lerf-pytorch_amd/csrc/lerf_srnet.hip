// The trainable SRNet hyper-network on MI355X (gfx950): forward and backward of one SRNet of the reference's SRNetsSWF2
// (resample/model.py:69-129) on image planes, the network that train_model.py -e ... --twoStage trains.
//
// Reference being replaced: SRNet.forward (common/network.py:127-163: unfold the K x K receptive field, pick the mode's
// four pixels, SRUnit, fold back) and SRUnit (:40-71: conv1 4 -> 64 + ReLU, four dense 1x1 layers 64 -> 64, 128 -> 64,
// 192 -> 64, 256 -> 64 whose outputs are concatenated to their inputs, conv6 320 -> outC + tanh), and what autograd
// derives for it.  Per output position the four pattern pixels of lerf_host_geometry.h's mode_pattern are one row of a
// dense MLP; 32 rows form a tile whose concatenated activations stay in LDS.  The hidden layers run on the matrix cores
// with the float32-input MFMA (v_mfma_f32_16x16x4_f32: exact float32 products, float32 sums, as the reference trains).
//
// Backward: the forward of the tile is recomputed (nothing is stored between the two launches), then the layers run in
// reverse.  Each layer's output gradient dz overwrites that layer's activations in LDS (they are dead once the mask
// [out > 0] has been applied), the gradient of the concatenated input accumulates in a second LDS array dact.
// Weight gradients are deterministic: workgroup g owns slab g of the workspace (packed layout) and walks tiles g, g + G,
// g + 2G, ... in order, adding each tile's contribution with plain loads and stores; srnet_reduce_kernel then sums the G
// slabs in slab order into grad_weights.  The input gradient of each position (4 floats) goes to a buffer that
// srnet_gather_kernel sums per image pixel in fixed tap order.  No float atomics, no waiting between workgroups.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lerf_host_geometry.h"
#include "lerf_kernels.h"
#include "lerf_srnet_layout.h"

namespace lerf {
namespace srnet {

constexpr int ROWS = 32;             // positions per tile
constexpr int NT = 256;              // 4 waves
constexpr int PA = ACT + 4;          // act row pitch (floats)
constexpr int PD = 4 * NF + 4;       // dact row pitch: gradients of act[:, 0:256] (act[:, 256:320] feeds conv6 only)
constexpr int MAX_SLABS = 512;       // workgroups of the backward = weight-gradient slabs (2 per CU resident)
typedef float floatx4 __attribute__((ext_vector_type(4)));

struct Geo {
    const float* img;                // [n_planes][h+bd][w+bd]
    int h, w, bd;
    int n_pos;                       // n_planes * h * w
    int8_t dy[4], dx[4];
};

__device__ inline floatx4 mfma4(float a, float b, floatx4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// the four pattern pixels of tile row r (0 for rows past the end)
__device__ inline void load_inputs(const Geo& g, int tile, float (*xin)[4]) {
    const int t = threadIdx.x;
    if (t < ROWS * 4) {
        const int r = t >> 2, k = t & 3;
        const int p = tile * ROWS + r;
        float v = 0.0f;
        if (p < g.n_pos) {
            const int hw = g.h * g.w, plane = p / hw, rem = p - plane * hw, y = rem / g.w, x = rem - y * g.w;
            const int wp = g.w + g.bd;
            v = g.img[((int64_t)plane * (g.h + g.bd) + y + g.dy[k]) * wp + x + g.dx[k]];
        }
        xin[r][k] = v;
    }
}

// act[:, 0:320] of the tile from xin: conv1 + ReLU, then the dense layers 2..5 on the matrix cores.  Ends synchronised.
__device__ void tile_forward(const float* __restrict__ W, const float (*xin)[4], float* act) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    {   // conv1 (4 -> 64) + ReLU: thread = (row, 8 neurons)
        const int r = t >> 3, n0 = (t & 7) * 8;
        const float* w1 = W + off_w(1);
        const float* b1 = W + off_b(1, 0);
#pragma unroll
        for (int n = n0; n < n0 + 8; ++n) {
            float s = b1[n];
#pragma unroll
            for (int k = 0; k < 4; ++k) s = __builtin_fmaf(w1[n * 4 + k], xin[r][k], s);
            act[r * PA + n] = s > 0.0f ? s : 0.0f;
        }
    }
    __syncthreads();
    // out[r][n] = relu(act[r, :K] . W[n, :K] + b[n]); wave = 16 rows x 32 neurons, two 16x16 blocks.
    // 16x16x4 operands: A[i][k] from lane i + 16 k, B[k][j] from lane j + 16 k; D[4 (lane/16) + reg][lane % 16]
    const int rb = (wave & 1) * 16, nb = (wave >> 1) * 32, li = lane & 15, lk = lane >> 4;
#pragma unroll 1
    for (int layer = 2; layer <= 5; ++layer) {
        const int K = layer_in(layer);
        const float* w = W + off_w(layer);
        const float* b = W + off_b(layer, 0);
        floatx4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = acc0;
        const float* ap = act + (rb + li) * PA + lk;
        const float* bp0 = w + (nb + li) * K + lk;
        const float* bp1 = bp0 + 16 * K;
#pragma unroll 4
        for (int k0 = 0; k0 < K; k0 += 4) {
            const float a = ap[k0];
            acc0 = mfma4(a, bp0[k0], acc0);
            acc1 = mfma4(a, bp1[k0], acc1);
        }
        const float bias0 = b[nb + li], bias1 = b[nb + 16 + li];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float* o = act + (rb + 4 * lk + r) * PA + K + nb + li;
            const float s0 = acc0[r] + bias0, s1 = acc1[r] + bias1;
            o[0] = s0 > 0.0f ? s0 : 0.0f;
            o[16] = s1 > 0.0f ? s1 : 0.0f;
        }
        __syncthreads();
    }
}

// conv6 pre-activation of (row r, channel c)
__device__ inline float conv6(const float* __restrict__ W, int outC, const float* act, int r, int c) {
    const float* w6 = W + off_w(6) + c * ACT;
    float s = W[off_b(6, outC) + c];
    const float* a = act + r * PA;
#pragma unroll 8
    for (int k = 0; k < ACT; ++k) s = __builtin_fmaf(w6[k], a[k], s);
    return s;
}

__device__ inline int64_t out_index(const Geo& g, int outC, int p, int c) {      // [n_planes][outC][h][w]
    const int hw = g.h * g.w, plane = p / hw, rem = p - plane * hw;
    return ((int64_t)plane * outC + c) * hw + rem;
}

__global__ void __launch_bounds__(NT) srnet_fwd_kernel(const float* __restrict__ W, int outC, Geo g, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float act[ROWS * PA];
    __shared__ float xin[ROWS][4];
    const int tile = blockIdx.x;
    load_inputs(g, tile, xin);
    __syncthreads();
    tile_forward(W, xin, act);
    const int t = threadIdx.x;
    if (t < ROWS * outC) {
        const int r = t / outC, c = t - r * outC, p = tile * ROWS + r;
        const float y = tanhf(conv6(W, outC, act, r, c));
        if (p < g.n_pos) out[out_index(g, outC, p, c)] = y;
    }
}

// slab[i] (+)= v: the first tile of a workgroup initialises its slab, the later ones accumulate
__device__ inline void slab_put(float* slab, int i, float v, bool first) { slab[i] = first ? v : slab[i] + v; }

// dW_l[n][k] (+)= sum_r dz[r][n] act[r][k] (k < K) and dact[r][k] += sum_n dz[r][n] W_l[n][k], dz = act[:, K:K+64]
__device__ void layer_backward(const float* __restrict__ W, int layer, float* act, float* dact, float* slab, bool first) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, lk = lane >> 4;
    const int K = layer_in(layer);
    const float* w = W + off_w(layer);
    float* sw = slab + off_w(layer);
    {   // weight gradient: wave = neurons 16 w .. 16 w + 15, two 16-column blocks of k at a time; the sum runs over rows
        const int nb = wave * 16;
#pragma unroll 1
        for (int kb = 0; kb < K; kb += 32) {
            floatx4 acc0, acc1;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = (nb + 4 * lk + r) * K + kb + li;
                acc0[r] = first ? 0.0f : sw[i];
                acc1[r] = first ? 0.0f : sw[i + 16];
            }
#pragma unroll
            for (int r0 = 0; r0 < ROWS; r0 += 4) {
                const float* row = act + (r0 + lk) * PA;
                const float a = row[K + nb + li];               // A[n][r] = dz[r][n]
                acc0 = mfma4(a, row[kb + li], acc0);            // B[r][k] = act[r][k]
                acc1 = mfma4(a, row[kb + 16 + li], acc1);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = (nb + 4 * lk + r) * K + kb + li;
                sw[i] = acc0[r];
                sw[i + 16] = acc1[r];
            }
        }
    }
    if (t < NF) {   // bias gradient
        float s = 0.0f;
        for (int r = 0; r < ROWS; ++r) s += act[r * PA + K + t];
        slab_put(slab, off_b(layer, 0) + t, s, first);
    }
    {   // input gradient: wave = rows 16 (w & 1).., k blocks (w >> 1) + 2 i; the sum runs over the 64 neurons
        const int rb = (wave & 1) * 16;
#pragma unroll 1
        for (int kb = (wave >> 1) * 16; kb < K; kb += 64) {
            floatx4 acc0, acc1;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* d = dact + (rb + 4 * lk + r) * PD + kb + li;
                acc0[r] = d[0];
                acc1[r] = d[32];
            }
            const float* ap = act + (rb + li) * PA + K + lk;    // A[r][n] = dz[r][n]
            const float* bp = w + lk * K + kb + li;             // B[n][k] = W_l[n][k]
#pragma unroll 4
            for (int n0 = 0; n0 < NF; n0 += 4) {
                const float a = ap[n0];
                acc0 = mfma4(a, bp[n0 * K], acc0);
                acc1 = mfma4(a, bp[n0 * K + 32], acc1);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float* d = dact + (rb + 4 * lk + r) * PD + kb + li;
                d[0] = acc0[r];
                d[32] = acc1[r];
            }
        }
    }
    __syncthreads();
    // dz of the layer below (overwrites its activations): dact gated by ReLU, [out > 0] == [act > 0]
    const int Kb = K - NF;
    for (int i = t; i < ROWS * NF; i += NT) {
        const int r = i >> 6, n = i & 63;
        float* a = act + r * PA + Kb + n;
        *a = *a > 0.0f ? dact[r * PD + Kb + n] : 0.0f;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(NT, 2)
srnet_bwd_kernel(const float* __restrict__ W, int outC, Geo g, const float* __restrict__ grad_out, int n_tiles,
                 float* __restrict__ slabs, int slab_stride, float* __restrict__ dxbuf) {
    __shared__ __attribute__((aligned(16))) float act[ROWS * PA];
    __shared__ __attribute__((aligned(16))) float dact[ROWS * PD];
    __shared__ float xin[ROWS][4];
    __shared__ float dz6[ROWS][4];
    const int t = threadIdx.x;
    float* slab = slabs + (int64_t)blockIdx.x * slab_stride;
#pragma unroll 1
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const bool first = tile == (int)blockIdx.x;
        load_inputs(g, tile, xin);
        __syncthreads();
        tile_forward(W, xin, act);
        // conv6 + tanh: dz6 = g (1 - y^2); rows past the end get 0 and so contribute nothing anywhere
        if (t < ROWS * outC) {
            const int r = t / outC, c = t - r * outC, p = tile * ROWS + r;
            const float y = tanhf(conv6(W, outC, act, r, c));
            const float go = p < g.n_pos ? grad_out[out_index(g, outC, p, c)] : 0.0f;
            dz6[r][c] = go * (1.0f - y * y);
        }
        __syncthreads();
        const float* w6 = W + off_w(6);
        for (int i = t; i < outC * ACT; i += NT) {          // dW6[c][k] = sum_r dz6[r][c] act[r][k]
            const int c = i / ACT, k = i - c * ACT;
            float s = 0.0f;
            for (int r = 0; r < ROWS; ++r) s = __builtin_fmaf(dz6[r][c], act[r * PA + k], s);
            slab_put(slab, off_w(6) + i, s, first);
        }
        if (t < outC) {
            float s = 0.0f;
            for (int r = 0; r < ROWS; ++r) s += dz6[r][t];
            slab_put(slab, off_b(6, outC) + t, s, first);
        }
        for (int i = t; i < ROWS * 4 * NF; i += NT) {       // dact[r][k] = sum_c dz6[r][c] W6[c][k], k < 256
            const int r = i >> 8, k = i & 255;
            float s = 0.0f;
            for (int c = 0; c < outC; ++c) s = __builtin_fmaf(dz6[r][c], w6[c * ACT + k], s);
            dact[r * PD + k] = s;
        }
        __syncthreads();
        for (int i = t; i < ROWS * NF; i += NT) {           // dz5 = (dz6 . W6[:, 256:320]) [act > 0]
            const int r = i >> 6, n = i & 63;
            float s = 0.0f;
            for (int c = 0; c < outC; ++c) s = __builtin_fmaf(dz6[r][c], w6[c * ACT + 4 * NF + n], s);
            float* a = act + r * PA + 4 * NF + n;
            *a = *a > 0.0f ? s : 0.0f;
        }
        __syncthreads();
#pragma unroll 1
        for (int layer = 5; layer >= 2; --layer) layer_backward(W, layer, act, dact, slab, first);
        // layer 1: dz1 = act[:, 0:64]
        const float* w1 = W + off_w(1);
        {   // dW1[n][k] = sum_r dz1[r][n] x[r][k]
            const int n = t >> 2, k = t & 3;
            float s = 0.0f;
            for (int r = 0; r < ROWS; ++r) s = __builtin_fmaf(act[r * PA + n], xin[r][k], s);
            slab_put(slab, off_w(1) + t, s, first);
        }
        if (t < NF) {
            float s = 0.0f;
            for (int r = 0; r < ROWS; ++r) s += act[r * PA + t];
            slab_put(slab, off_b(1, 0) + t, s, first);
        }
        if (dxbuf && t < ROWS * 4) {                         // dx[r][k] = sum_n dz1[r][n] W1[n][k]
            const int r = t >> 2, k = t & 3, p = tile * ROWS + r;
            float s = 0.0f;
            for (int n = 0; n < NF; ++n) s = __builtin_fmaf(act[r * PA + n], w1[n * 4 + k], s);
            if (p < g.n_pos) dxbuf[(int64_t)p * 4 + k] = s;
        }
        __syncthreads();
    }
}

// grad_weights[i] += sum_g slabs[g][i], g = 0, 1, ..., n_slabs - 1
__global__ void __launch_bounds__(256)
srnet_reduce_kernel(const float* __restrict__ slabs, int slab_stride, int n_slabs, int n, float* __restrict__ grad_weights) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.0f;
    for (int k = 0; k < n_slabs; ++k) s += slabs[(int64_t)k * slab_stride + i];
    grad_weights[i] += s;
}

// grad_img[plane][yy][xx] += sum over taps k = 0..3 of dx[position (yy - dy[k], xx - dx[k])][k]
__global__ void __launch_bounds__(256)
srnet_gather_kernel(const float* __restrict__ dxbuf, Geo g, int n_planes, float* __restrict__ grad_img) {
    const int wp = g.w + g.bd, hp = g.h + g.bd;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)n_planes * hp * wp) return;
    const int plane = (int)(i / ((int64_t)hp * wp)), rem = (int)(i - (int64_t)plane * hp * wp), yy = rem / wp, xx = rem - yy * wp;
    float s = 0.0f;
    bool any = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int y = yy - g.dy[k], x = xx - g.dx[k];
        if (y >= 0 && y < g.h && x >= 0 && x < g.w) {
            s += dxbuf[((int64_t)plane * g.h * g.w + (int64_t)y * g.w + x) * 4 + k];
            any = true;
        }
    }
    if (any) grad_img[i] += s;
}

inline int n_tiles_of(int64_t n_pos) { return (int)((n_pos + ROWS - 1) / ROWS); }
inline int n_slabs_of(int64_t n_pos) { return n_tiles_of(n_pos) < MAX_SLABS ? n_tiles_of(n_pos) : MAX_SLABS; }
inline int slab_stride_of(int outC) { return (weight_floats(outC) + 63) & ~63; }   // 256-byte aligned slabs

bool make_geo(char mode, const float* img, int n_planes, int h, int w, int bd, Geo* g) {
    if (!mode_pattern(mode, g->dy, g->dx)) return false;
    for (int k = 0; k < 4; ++k)
        if (g->dy[k] > bd || g->dx[k] > bd) return false;
    g->img = img;
    g->h = h;
    g->w = w;
    g->bd = bd;
    g->n_pos = n_planes * h * w;
    return true;
}

}  // namespace srnet

size_t srnet_bwd_workspace_bytes(int outC, int n_planes, int h, int w) {
    using namespace srnet;
    const int64_t n_pos = (int64_t)n_planes * h * w;
    return (size_t)n_slabs_of(n_pos) * slab_stride_of(outC) * sizeof(float) + (size_t)n_pos * 4 * sizeof(float);
}

int launch_srnet_fwd(const float* weights, int outC, char mode, const float* img, int n_planes, int h, int w, int bd,
                     float* out, hipStream_t st) {
    using namespace srnet;
    Geo g;
    if (!make_geo(mode, img, n_planes, h, w, bd, &g)) return LERF_EINVAL;
    hipLaunchKernelGGL(srnet_fwd_kernel, dim3(n_tiles_of(g.n_pos)), dim3(NT), 0, st, weights, outC, g, out);
    return LERF_OK;
}

int launch_srnet_bwd(const float* weights, int outC, char mode, const float* img, const float* grad_out, int n_planes, int h,
                     int w, int bd, float* grad_weights, float* grad_img, void* workspace, size_t workspace_bytes,
                     hipStream_t st) {
    using namespace srnet;
    Geo g;
    if (!make_geo(mode, img, n_planes, h, w, bd, &g)) return LERF_EINVAL;
    if (workspace_bytes < srnet_bwd_workspace_bytes(outC, n_planes, h, w)) return LERF_EINVAL;
    const int n_tiles = n_tiles_of(g.n_pos), n_slabs = n_slabs_of(g.n_pos), stride = slab_stride_of(outC);
    float* slabs = static_cast<float*>(workspace);
    float* dxbuf = grad_img ? slabs + (size_t)n_slabs * stride : nullptr;
    hipLaunchKernelGGL(srnet_bwd_kernel, dim3(n_slabs), dim3(NT), 0, st, weights, outC, g, grad_out, n_tiles, slabs, stride, dxbuf);
    const int nw = weight_floats(outC);
    hipLaunchKernelGGL(srnet_reduce_kernel, dim3((nw + 255) / 256), dim3(256), 0, st, slabs, stride, n_slabs, nw, grad_weights);
    if (grad_img) {
        const int64_t n_img = (int64_t)n_planes * (h + bd) * (w + bd);
        hipLaunchKernelGGL(srnet_gather_kernel, dim3((unsigned)((n_img + 255) / 256)), dim3(256), 0, st, dxbuf, g, n_planes, grad_img);
    }
    return LERF_OK;
}

}  // namespace lerf
