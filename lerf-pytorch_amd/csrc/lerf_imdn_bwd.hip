// Training LeRF-Net on MI355X (gfx950): the saving forward and the backward of one IMDN_RTC net (the reference's
// resample/model.py:434-537 at upscale 1, one stage of IMDN2), float32, in the packed layout of lerf_imdn_layout.h.
//
// Reference being replaced: what autograd derives for nn.Sequential(fea_conv, ShortcutBlock(5 x IMDModule_speed + LR_conv),
// upsampler conv) run as stock convolutions, and for IMDN2.predict's clamp and affine on top of it.
//
// Saving forward: the launches of lerf_imdn.hip's imdn_conv_kernel with every activation the backward needs in a buffer
// of its own (lerf_imdn.hip reuses h, cat, r1, r2 across modules): fea, the five module outputs, per module the
// concatenated distilled channels and the three remaining-channel planes, the upsampler's input, and with post != 0 the
// raw output y (it decides the clamp mask); imdn_post_kernel then applies the inference epilogue's clamp and affine to y.
//
// Backward, per convolution from the last to the first, on v_mfma_f32_16x16x4_f32 (exact float32 products, float32 sums):
//   imdn_dgrad_kernel  gin[y][x][c] = sum over (tap, n) of g[y - dy][x - dx][n] W[n][c][tap]: an implicit GEMM, rows
//                      pixels, columns input channels, K over (tap, output channel), the weight read transposed;
//   imdn_wgrad_kernel  dW[n][c][tap] = sum over pixels of g[p][n] in[p + tap][c], db[n] = sum over pixels of g[p][n]:
//                      rows output channels, columns input channels, K over pixels, one product per tap.
// A workgroup owns an 8 x 16 pixel tile of one image (so image b never reads image b').  Every MFMA operand comes from
// LDS: the tile of gradients (dgrad: with its one-pixel halo) and the tile of activations (wgrad: with halo) are staged
// once, the tap's weight slice (dgrad) once per tap from a [tap][n][c] copy made once per conv; the LDS row pitches
// make the operand reads conflict-free.
// Split and concat stay addressing, as in the forward: the gradient of a conv output is gathered from two NHWC views
// (GradSrc: the distilled channels from c5's dgrad, the remaining channels from the next conv's dgrad).  Fused: the
// LeakyReLU(0.05) derivative from the sign of the saved activation and the residual fan-in in the dgrad epilogue, the
// clamp mask and post factor of the last conv in the gradient gather.
// Weight gradients are deterministic: workgroup g owns slab g of the workspace and walks tiles g, g + G, ... in order,
// imdn_wreduce_kernel sums the G slabs in slab order and writes (not accumulates) the packed gradient.  No float atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lerf_imdn_conv.h"
#include "lerf_imdn_layout.h"
#include "lerf_kernels.h"

namespace lerf {
namespace imdn {

constexpr int NT = 256;              // 4 waves
constexpr int TH = 8, TW = 16;       // pixel tile of a workgroup: a wave owns two rows of 16
constexpr int TP = TH * TW;
constexpr int MAX_SLABS = 256;       // workgroups of a wgrad launch = weight-gradient slabs (one per CU)
typedef float floatx4 __attribute__((ext_vector_type(4)));

__device__ inline floatx4 mfma4(float a, float b, floatx4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// LDS row pitch of nb 16-channel blocks with pitch % 32 == 16: rows k and k + 1 land on opposite bank halves
__host__ __device__ constexpr int pitch16(int nb) { return nb * 16 + ((nb & 1) ? 0 : 16); }

// the gradient of a conv output: channel n < split from lo (channel n), the others from hi (channel n - split); with
// post != 0 (the last conv) times predict's derivative, post 1: 127 [-1 <= y <= 1], post 2: 1/2 [-1 <= y <= 1]
struct GradSrc {
    View lo, hi;
    int cout, split;
    View y;                          // the raw output, laid out like lo (post != 0 only)
    int post;
};

__device__ inline float load_grad(const GradSrc& g, int b, int64_t yx, int n) {
    const View& v = n < g.split ? g.lo : g.hi;
    const int no = n < g.split ? n : n - g.split;
    float val = v.p[b * v.sb + yx * v.sp + no * v.sc];
    if (g.post) {
        const float y = g.y.p[b * g.y.sb + yx * g.y.sp + n * g.y.sc];
        val = y >= -1.0f && y <= 1.0f ? val * (g.post == 1 ? 127.0f : 0.5f) : 0.0f;
    }
    return val;
}

struct TileGeo {
    int H, W, tiles_x, tiles_y, n_tiles;
};

__device__ inline void tile_origin(const TileGeo& t, int tile, int* b, int* y0, int* x0) {
    const int tx = tile % t.tiles_x, r = tile / t.tiles_x, ty = r % t.tiles_y;
    *b = r / t.tiles_y;
    *y0 = ty * TH;
    *x0 = tx * TW;
}

struct DgradArgs {
    const float* wt;                 // the weights transposed to [KK][cout][cin] (imdn_wtranspose_kernel): coalesced tap slices
    int cin;                         // channels of the result
    GradSrc g;
    View out;
    const float* res;                // nullable: residual fan-in, laid out like out
    const float* res2;
    View sgn;                        // saved activation of result channel c: c < n_act is scaled by 0.05 where it is <= 0
    int n_act;
    TileGeo t;
};

template <int NB, int KK>
__global__ void __launch_bounds__(NT) imdn_dgrad_kernel(DgradArgs a) {
    constexpr int HALO = KK == 9 ? 1 : 0, HW = TW + 2 * HALO, HH = TH + 2 * HALO, WP = pitch16(NB);
    // gradient tile [halo pixel][n], pitch % 4 == 2: the 16 pixels x 2 channels of a half-wave read hit 32 banks
    __shared__ float gt[HH * HW * 66];
    __shared__ float wl[64 * WP];    // the tap's weights [n][c]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, lk = lane >> 4;
    const int N = a.g.cout, Np = (N + 3) & ~3, PG = Np + 2;
    int b, y0, x0;
    tile_origin(a.t, blockIdx.x, &b, &y0, &x0);
    for (int i = t; i < HH * HW * Np; i += NT) {
        const int hp = i / Np, n = i - hp * Np, hy = hp / HW, hx = hp - hy * HW;
        const int y = y0 + hy - HALO, x = x0 + hx - HALO;
        float v = 0.0f;
        if (n < N && y >= 0 && y < a.t.H && x >= 0 && x < a.t.W) v = load_grad(a.g, b, (int64_t)y * a.t.W + x, n);
        gt[hp * PG + n] = v;
    }
    floatx4 acc[2][NB];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[q][nb] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
    // 16x16x4 operands: A[i][k] from lane i + 16 k, B[k][j] from lane j + 16 k; D[4 (lane/16) + reg][lane % 16]
#pragma unroll 1
    for (int tap = 0; tap < KK; ++tap) {
        const int dy = KK == 9 ? tap / 3 - 1 : 0, dx = KK == 9 ? tap % 3 - 1 : 0;
        __syncthreads();                                       // the previous tap's reads of wl
        for (int i = t; i < Np * NB * 16; i += NT) {
            const int n = i / (NB * 16), c = i - n * (NB * 16);
            wl[n * WP + c] = n < N && c < a.cin ? a.wt[(tap * N + n) * a.cin + c] : 0.0f;
        }
        __syncthreads();
        const float* ap = gt + ((2 * wave + HALO - dy) * HW + li + HALO - dx) * PG + lk;
        const float* bp = wl + lk * WP + li;
#pragma unroll 2
        for (int n0 = 0; n0 < Np; n0 += 4) {
            const float a0 = ap[n0], a1 = ap[HW * PG + n0];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const float bv = bp[n0 * WP + nb * 16];
                acc[0][nb] = mfma4(a0, bv, acc[0][nb]);
                acc[1][nb] = mfma4(a1, bv, acc[1][nb]);
            }
        }
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int c = nb * 16 + li;
        if (c >= a.cin) continue;
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int y = y0 + 2 * wave + q, x = x0 + 4 * lk + r;
                if (y >= a.t.H || x >= a.t.W) continue;
                const int64_t yx = (int64_t)y * a.t.W + x, o = b * a.out.sb + yx * a.out.sp + c * a.out.sc;
                float v = acc[q][nb][r];
                if (a.res) v += a.res[o];
                if (a.res2) v += a.res2[o];
                if (c < a.n_act && !(a.sgn.p[b * a.sgn.sb + yx * a.sgn.sp + c * a.sgn.sc] > 0.0f)) v *= 0.05f;
                a.out.p[o] = v;
            }
    }
}

struct WgradArgs {
    GradSrc g;
    View in;                         // the conv's input, cin channels
    int cin;
    TileGeo t;
    float* slabs;                    // slab g: [KK][cout][cin] then bias[cout]
    int slab_stride;
};

// slab[i] (+)= v: the first tile of a workgroup initialises its slab, the later ones accumulate
__device__ inline void slab_put(float* slab, int i, float v, bool first) { slab[i] = first ? v : slab[i] + v; }

template <int NBC, int KK>
__global__ void __launch_bounds__(NT) imdn_wgrad_kernel(WgradArgs a) {
    constexpr int HALO = KK == 9 ? 1 : 0, HW = TW + 2 * HALO, HH = TH + 2 * HALO, PI = pitch16(NBC);
    __shared__ float gt[TP * pitch16(4)];        // gradient tile [pixel][n]
    __shared__ float it[HH * HW * PI];           // activation tile [halo pixel][c]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, lk = lane >> 4;
    const int N = a.g.cout, NBN = (N + 15) / 16, PG = pitch16(NBN);
    float* slab = a.slabs + (int64_t)blockIdx.x * a.slab_stride;
#pragma unroll 1
    for (int tile = blockIdx.x; tile < a.t.n_tiles; tile += gridDim.x) {
        const bool first = tile == (int)blockIdx.x;
        int b, y0, x0;
        tile_origin(a.t, tile, &b, &y0, &x0);
        __syncthreads();                                       // the previous tile's reads
        for (int i = t; i < TP * NBN * 16; i += NT) {
            const int p = i / (NBN * 16), n = i - p * (NBN * 16);
            const int y = y0 + (p >> 4), x = x0 + (p & 15);
            float v = 0.0f;
            if (n < N && y < a.t.H && x < a.t.W) v = load_grad(a.g, b, (int64_t)y * a.t.W + x, n);
            gt[p * PG + n] = v;
        }
        for (int i = t; i < HH * HW * NBC * 16; i += NT) {
            const int hp = i / (NBC * 16), c = i - hp * (NBC * 16), hy = hp / HW, hx = hp - hy * HW;
            const int y = y0 + hy - HALO, x = x0 + hx - HALO;
            float v = 0.0f;
            if (c < a.cin && y >= 0 && y < a.t.H && x >= 0 && x < a.t.W)
                v = a.in.p[b * a.in.sb + ((int64_t)y * a.t.W + x) * a.in.sp + c * a.in.sc];
            it[hp * PI + c] = v;
        }
        __syncthreads();
        // a job = (tap, 16 output channels): A[n][p] = g[p][n], B[p][c] = in[p + tap][c], the sum runs over the tile
#pragma unroll 1
        for (int job = wave; job < KK * NBN; job += 4) {
            const int tap = job / NBN, nb = job - tap * NBN;
            const int dy = KK == 9 ? tap / 3 - 1 : 0, dx = KK == 9 ? tap % 3 - 1 : 0;
            floatx4 acc[NBC];
#pragma unroll
            for (int cb = 0; cb < NBC; ++cb) acc[cb] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
            const float* ap = gt + lk * PG + nb * 16 + li;
            const float* bp = it + ((HALO + dy) * HW + lk + HALO + dx) * PI + li;
#pragma unroll 4
            for (int k0 = 0; k0 < TP; k0 += 4) {
                const float av = ap[k0 * PG];
                const float* br = bp + ((k0 >> 4) * HW + (k0 & 15)) * PI;
#pragma unroll
                for (int cb = 0; cb < NBC; ++cb) acc[cb] = mfma4(av, br[cb * 16], acc[cb]);
            }
#pragma unroll
            for (int cb = 0; cb < NBC; ++cb) {
                const int c = cb * 16 + li;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = nb * 16 + 4 * lk + r;
                    if (n < N && c < a.cin) slab_put(slab, (tap * N + n) * a.cin + c, acc[cb][r], first);
                }
            }
        }
        if (t < N) {
            float s = 0.0f;
            for (int p = 0; p < TP; ++p) s += gt[p * PG + t];
            slab_put(slab, KK * N * a.cin + t, s, first);
        }
    }
}

// wt[tap][n][c] = w[n][c][tap]: once per conv, so that every dgrad workgroup stages a tap's slice with coalesced loads
__global__ void __launch_bounds__(256) imdn_wtranspose_kernel(const float* __restrict__ w, int NC, int KK, float* __restrict__ wt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NC * KK) return;
    const int tap = i / NC, nc = i - tap * NC;
    wt[i] = w[nc * KK + tap];
}

// dst (PyTorch order W[n][c][KK] then bias[n]) = sum over slabs g = 0, 1, ..., n_slabs - 1 of slab g ([KK][n][c], bias)
__global__ void __launch_bounds__(256)
imdn_wreduce_kernel(const float* __restrict__ slabs, int slab_stride, int n_slabs, int N, int C, int KK, float* __restrict__ dst) {
    const int i = blockIdx.x * 256 + threadIdx.x, nw = KK * N * C;
    if (i >= nw + N) return;
    float s = 0.0f;
    for (int g = 0; g < n_slabs; ++g) s += slabs[(int64_t)g * slab_stride + i];
    if (i < nw) {
        const int tap = i / (N * C), nc = i - tap * (N * C);
        dst[nc * KK + tap] = s;
    } else {
        dst[i] = s;
    }
}

// the inference epilogue's clamp and affine (imdn_conv_kernel with post), on the saved raw output
__global__ void __launch_bounds__(256) imdn_post_kernel(const float* __restrict__ y, int64_t n, int post, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = fminf(fmaxf(y[i], -1.0f), 1.0f);
    out[i] = post == 1 ? __fadd_rn(__fmul_rn(v, 127.0f), 127.0f) : __fadd_rn(__fmul_rn(v, 0.5f), 0.5f);
}

template <int KK>
void launch_dgrad(const DgradArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)a.t.n_tiles);
    switch ((a.cin + 15) / 16) {
    case 1: hipLaunchKernelGGL((imdn_dgrad_kernel<1, KK>), grid, dim3(NT), 0, st, a); break;
    case 2: hipLaunchKernelGGL((imdn_dgrad_kernel<2, KK>), grid, dim3(NT), 0, st, a); break;
    case 3: hipLaunchKernelGGL((imdn_dgrad_kernel<3, KK>), grid, dim3(NT), 0, st, a); break;
    default: hipLaunchKernelGGL((imdn_dgrad_kernel<4, KK>), grid, dim3(NT), 0, st, a); break;
    }
}

template <int KK>
void launch_wgrad(const WgradArgs& a, int n_slabs, hipStream_t st) {
    const dim3 grid((unsigned)n_slabs);
    switch ((a.cin + 15) / 16) {
    case 1: hipLaunchKernelGGL((imdn_wgrad_kernel<1, KK>), grid, dim3(NT), 0, st, a); break;
    case 2: hipLaunchKernelGGL((imdn_wgrad_kernel<2, KK>), grid, dim3(NT), 0, st, a); break;
    case 3: hipLaunchKernelGGL((imdn_wgrad_kernel<3, KK>), grid, dim3(NT), 0, st, a); break;
    default: hipLaunchKernelGGL((imdn_wgrad_kernel<4, KK>), grid, dim3(NT), 0, st, a); break;
    }
}

inline TileGeo tile_geo(int B, int H, int W) {
    TileGeo t;
    t.H = H;
    t.W = W;
    t.tiles_x = (W + TW - 1) / TW;
    t.tiles_y = (H + TH - 1) / TH;
    t.n_tiles = B * t.tiles_y * t.tiles_x;
    return t;
}
inline int n_slabs_of(const TileGeo& t) { return t.n_tiles < MAX_SLABS ? t.n_tiles : MAX_SLABS; }
inline int slab_stride_of(int nf) { return (conv_floats(nf, nf, 9) + 63) & ~63; }     // the largest conv; 256-byte aligned slabs

// floats per pixel of `saved`: fea, the five module outputs, the upsampler's input, per module cat and r1..r3, y
inline int saved_floats_per_pixel(int nf, int out_nc) { return 7 * nf + MODULES * (nf + 3 * (nf - nf / 4)) + out_nc; }
// floats per pixel of the backward's gradient planes: gu, two module gradients, gcat, two remaining-channel gradients
inline int grad_floats_per_pixel(int nf) { return 4 * nf + 2 * (nf - nf / 4); }

struct Saved {
    float* h[MODULES + 1];           // h[0] = fea, h[m + 1] = output of module m
    float* u;                        // LR_conv(h[5]) + fea
    float* cat[MODULES];
    float* r[MODULES][3];
    float* y;                        // [B][out_nc][H][W], written with post != 0 only
};

inline Saved carve_saved(float* p, int nf, int64_t P) {
    const int r = nf - nf / 4;
    Saved s;
    for (int m = 0; m <= MODULES; ++m, p += P * nf) s.h[m] = p;
    s.u = p;
    p += P * nf;
    for (int m = 0; m < MODULES; ++m) {
        s.cat[m] = p;
        p += P * nf;
        for (int j = 0; j < 3; ++j, p += P * r) s.r[m][j] = p;
    }
    s.y = p;
    return s;
}

}  // namespace imdn

size_t imdn_saved_bytes(int nf, int out_nc, int B, int H, int W) {
    return (size_t)B * H * W * imdn::saved_floats_per_pixel(nf, out_nc) * sizeof(float);
}

size_t imdn_bwd_workspace_bytes(int nf, int B, int H, int W) {
    using namespace imdn;
    // gradient planes, one conv's transposed weights, the slabs
    return ((size_t)B * H * W * grad_floats_per_pixel(nf) + (size_t)(n_slabs_of(tile_geo(B, H, W)) + 1) * slab_stride_of(nf)) * sizeof(float);
}

int launch_imdn_fwd_train(const float* weights, int nf, int in_nc, int out_nc, const float* x, int B, int H, int W, int post,
                          void* saved, float* out, hipStream_t st) {
    using namespace imdn;
    const int d = nf / 4, r = nf - d;
    const int64_t P = (int64_t)B * H * W, HW = (int64_t)H * W;
    const Saved s = carve_saved(static_cast<float*>(saved), nf, P);
    auto nhwc = [&](float* p, int pitch) { return View{p, HW * pitch, pitch, 1}; };
    auto conv = [&](int off, int cin, int cout, int split, View in, View lo, View hi, const float* res, int act, bool k3) {
        launch_conv(ConvArgs{weights + off, cin, cout, split, in, lo, hi, res, act, 0, H, W, P}, k3, st);
    };
    const View none{nullptr, 0, 0, 0};
    conv(0, in_nc, nf, nf, View{const_cast<float*>(x), (int64_t)in_nc * HW, 1, HW}, nhwc(s.h[0], nf), none, nullptr, 0, true);
    for (int m = 0; m < MODULES; ++m) {
        float* cat = s.cat[m];
        conv(off_conv(nf, in_nc, m, 1), nf, nf, d, nhwc(s.h[m], nf), nhwc(cat, nf), nhwc(s.r[m][0], r), nullptr, 1, true);
        conv(off_conv(nf, in_nc, m, 2), r, nf, d, nhwc(s.r[m][0], r), nhwc(cat + d, nf), nhwc(s.r[m][1], r), nullptr, 1, true);
        conv(off_conv(nf, in_nc, m, 3), r, nf, d, nhwc(s.r[m][1], r), nhwc(cat + 2 * d, nf), nhwc(s.r[m][2], r), nullptr, 1, true);
        conv(off_conv(nf, in_nc, m, 4), r, d, d, nhwc(s.r[m][2], r), nhwc(cat + 3 * d, nf), none, nullptr, 0, true);
        conv(off_conv(nf, in_nc, m, 5), nf, nf, nf, nhwc(cat, nf), nhwc(s.h[m + 1], nf), none, s.h[m], 0, false);
    }
    conv(off_lr(nf, in_nc), nf, nf, nf, nhwc(s.h[MODULES], nf), nhwc(s.u, nf), none, s.h[0], 0, false);
    float* y = post ? s.y : out;
    conv(off_up(nf, in_nc), nf, out_nc, out_nc, nhwc(s.u, nf), View{y, (int64_t)out_nc * HW, 1, HW}, none, nullptr, 0, true);
    if (post) {
        const int64_t n = P * out_nc;
        hipLaunchKernelGGL(imdn_post_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, y, n, post, out);
    }
    return LERF_OK;
}

int launch_imdn_bwd(const float* weights, int nf, int in_nc, int out_nc, const float* x, int B, int H, int W, int post,
                    void* saved, const float* grad_out, float* grad_weights, float* grad_x, void* workspace, hipStream_t st) {
    using namespace imdn;
    const int d = nf / 4, r = nf - d;
    const int64_t P = (int64_t)B * H * W, HW = (int64_t)H * W;
    const Saved s = carve_saved(static_cast<float*>(saved), nf, P);
    const TileGeo tg = tile_geo(B, H, W);
    const int n_slabs = n_slabs_of(tg), stride = slab_stride_of(nf);
    float* gu = static_cast<float*>(workspace);
    float* gh[2] = {gu + P * nf, gu + 2 * P * nf};
    float* gcat = gu + 3 * P * nf;
    float* gr[2] = {gcat + P * nf, gcat + P * nf + P * r};
    float* wt = gr[1] + P * r;
    float* slabs = wt + stride;
    auto nhwc = [&](float* p, int pitch) { return View{p, HW * pitch, pitch, 1}; };
    const View none{nullptr, 0, 0, 0};
    auto src = [&](View lo, View hi, int cout, int split) { return GradSrc{lo, hi, cout, split, none, 0}; };
    // one convolution: its weight and bias gradient, then (out.p != nullptr) the gradient of its input
    auto conv = [&](int off, int cin, bool k3, const GradSrc& g, View in, View out, const float* res, const float* res2,
                    View sgn, int n_act) {
        const WgradArgs wa{g, in, cin, tg, slabs, stride};
        if (k3) launch_wgrad<9>(wa, n_slabs, st);
        else launch_wgrad<1>(wa, n_slabs, st);
        const int KK = k3 ? 9 : 1, nw = conv_floats(g.cout, cin, KK);
        hipLaunchKernelGGL(imdn_wreduce_kernel, dim3((nw + 255) / 256), dim3(256), 0, st, slabs, stride, n_slabs, g.cout, cin, KK,
                           grad_weights + off);
        if (!out.p) return;
        const int nc = g.cout * cin;
        hipLaunchKernelGGL(imdn_wtranspose_kernel, dim3((nc * KK + 255) / 256), dim3(256), 0, st, weights + off, nc, KK, wt);
        const DgradArgs da{wt, cin, g, out, res, res2, sgn, n_act, tg};
        if (k3) launch_dgrad<9>(da, st);
        else launch_dgrad<1>(da, st);
    };
    // upsampler conv: the gradient of y is grad_out times predict's derivative
    const View go{const_cast<float*>(grad_out), (int64_t)out_nc * HW, 1, HW};
    conv(off_up(nf, in_nc), nf, true, GradSrc{go, none, out_nc, out_nc, View{s.y, (int64_t)out_nc * HW, 1, HW}, post}, nhwc(s.u, nf),
         nhwc(gu, nf), nullptr, nullptr, none, 0);
    // LR_conv; gu also reaches fea directly (added where fea's gradient is completed, below)
    int cur = 0;
    conv(off_lr(nf, in_nc), nf, false, src(nhwc(gu, nf), none, nf, nf), nhwc(s.h[MODULES], nf), nhwc(gh[cur], nf), nullptr, nullptr,
         none, 0);
    for (int m = MODULES - 1; m >= 0; --m) {
        // c5: the gradient of cat; its first 3d channels are LeakyReLU outputs
        conv(off_conv(nf, in_nc, m, 5), nf, false, src(nhwc(gh[cur], nf), none, nf, nf), nhwc(s.cat[m], nf), nhwc(gcat, nf), nullptr,
             nullptr, nhwc(s.cat[m], nf), 3 * d);
        conv(off_conv(nf, in_nc, m, 4), r, true, src(nhwc(gcat + 3 * d, nf), none, d, d), nhwc(s.r[m][2], r), nhwc(gr[0], r), nullptr,
             nullptr, nhwc(s.r[m][2], r), r);
        conv(off_conv(nf, in_nc, m, 3), r, true, src(nhwc(gcat + 2 * d, nf), nhwc(gr[0], r), nf, d), nhwc(s.r[m][1], r), nhwc(gr[1], r),
             nullptr, nullptr, nhwc(s.r[m][1], r), r);
        conv(off_conv(nf, in_nc, m, 2), r, true, src(nhwc(gcat + d, nf), nhwc(gr[1], r), nf, d), nhwc(s.r[m][0], r), nhwc(gr[0], r),
             nullptr, nullptr, nhwc(s.r[m][0], r), r);
        // c1: + the module's residual; module 0's input is fea, which LR_conv's residual also reads
        conv(off_conv(nf, in_nc, m, 1), nf, true, src(nhwc(gcat, nf), nhwc(gr[0], r), nf, d), nhwc(s.h[m], nf), nhwc(gh[cur ^ 1], nf),
             gh[cur], m == 0 ? gu : nullptr, none, 0);
        cur ^= 1;
    }
    conv(0, in_nc, true, src(nhwc(gh[cur], nf), none, nf, nf), View{const_cast<float*>(x), (int64_t)in_nc * HW, 1, HW},
         grad_x ? View{grad_x, (int64_t)in_nc * HW, 1, HW} : none, nullptr, nullptr, none, 0);
    return LERF_OK;
}

}  // namespace lerf
