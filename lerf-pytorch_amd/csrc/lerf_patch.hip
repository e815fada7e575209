// The training batch of the reference's DIV2K provider (resample/data.py:107-165) in one launch: for every sample the LR
// patch `im` and the HR patch `lb` are cut from uint8 HWC RGB images that live in one device pool,
//     crop -> channel -> np.fliplr -> np.flipud -> np.rot90(., k) -> float32(u8) / 255.0f (+ noise on im)
// and written as float32 [B][C][n][n].  The five index steps are one affine map from an output pixel (y, x) to a source
// pixel (source_of below); the division is IEEE (v_div_scale / v_div_fmas / v_div_fixup), never a multiply by 1/255.
//
// Lane mapping: a workgroup owns one 32 x 32 output tile of one sample, all C channels; lanes run along the output x, so a
// wave stores two 128-byte row segments per instruction.  For odd k the matching source walk runs down a column of the HWC
// image (one byte per row pitch of several KB), so the source rectangle of the tile is staged in LDS first: it is read row
// by row (contiguous 3 * 32 bytes per row, coalesced) whatever k is, and the transposed / mirrored walk happens on the LDS
// copy.  LDS rows are 100 bytes apart = 25 banks, so a column walk of 32 lanes touches 32 different banks.
// Every index is checked: tiles are clipped to n, and a descriptor that would read outside its image or outside the pool
// makes the kernel write zeros for that sample instead of reading (desc_ok).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lerf_common.h"

namespace lerf {
namespace patch {

constexpr int kTile = 32;
constexpr int kThreads = 256;
constexpr int kRows = kThreads / kTile;          // output rows per pass of the workgroup
constexpr int kLdsPitch = kTile * 3 + 4;         // bytes; 25 dwords: odd, so a column walk is conflict-free

struct Image {
    int64_t off;
    int h, w, pitch, i, j;                       // i, j: the crop origin
};

__host__ __device__ inline bool image_ok(int64_t off, int h, int w, int pitch, int i, int j, int n, int64_t pool_bytes) {
    if (off < 0 || h <= 0 || w <= 0 || pitch < 3 * (int64_t)w) return false;
    if (off > pool_bytes || (int64_t)h * pitch > pool_bytes - off) return false;
    return i >= 0 && j >= 0 && (int64_t)i + n <= h && (int64_t)j + n <= w;
}

__host__ __device__ inline bool desc_ok(const lerf_patch_desc_t& d, int C, int sz, int hsz, int64_t pool_bytes) {
    if (C == 1 && (d.chan < 0 || d.chan > 2)) return false;
    if (d.k < 0 || d.k > 3) return false;
    return image_ok(d.lr_off, d.lr_h, d.lr_w, d.lr_pitch, d.li, d.lj, sz, pool_bytes) &&
           image_ok(d.hr_off, d.hr_h, d.hr_w, d.hr_pitch, d.hi, d.hj, hsz, pool_bytes);
}

// (row, column) of the crop that output pixel (y, x) of an n x n patch shows: rot90 undone first, then flipud, then fliplr
__device__ __forceinline__ void source_of(int y, int x, int n, int k, bool fl, bool fu, int& sy, int& sx) {
    switch (k) {
        case 0: sy = y; sx = x; break;
        case 1: sy = x; sx = n - 1 - y; break;
        case 2: sy = n - 1 - y; sx = n - 1 - x; break;
        default: sy = n - 1 - x; sx = y; break;
    }
    if (fu) sy = n - 1 - sy;
    if (fl) sx = n - 1 - sx;
}

__global__ void __launch_bounds__(kThreads)
patch_batch_kernel(const uint8_t* __restrict__ pool, int64_t pool_bytes, const lerf_patch_desc_t* __restrict__ desc, int C, int sz,
                   int hsz, int tiles_lr, const float* __restrict__ noise, float* __restrict__ im, float* __restrict__ lb) {
    __shared__ uint8_t tile[kTile * kLdsPitch];
    const int b = blockIdx.y;
    const lerf_patch_desc_t d = desc[b];
    const bool hr = (int)blockIdx.x >= tiles_lr * tiles_lr;
    const int n = hr ? hsz : sz;
    const int per_row = hr ? (hsz + kTile - 1) / kTile : tiles_lr;
    const int t = hr ? (int)blockIdx.x - tiles_lr * tiles_lr : (int)blockIdx.x;
    const int y0 = (t / per_row) * kTile, x0 = (t % per_row) * kTile;
    const int th = min(kTile, n - y0), tw = min(kTile, n - x0);          // the tile clipped to the patch
    float* __restrict__ out = (hr ? lb : im) + (int64_t)b * C * n * n;
    const float* __restrict__ nz = (!hr && noise) ? noise + (int64_t)b * C * n * n : nullptr;
    const int lx = threadIdx.x % kTile, ly = threadIdx.x / kTile;

    if (!desc_ok(d, C, sz, hsz, pool_bytes)) {                           // uniform per workgroup: zeros, and no read
        if (lx < tw)
            for (int c = 0; c < C; ++c)
                for (int y = ly; y < th; y += kRows) out[((int64_t)c * n + y0 + y) * n + x0 + lx] = 0.0f;
        return;
    }
    const Image I = hr ? Image{d.hr_off, d.hr_h, d.hr_w, d.hr_pitch, d.hi, d.hj} : Image{d.lr_off, d.lr_h, d.lr_w, d.lr_pitch, d.li, d.lj};
    const bool fl = d.fliplr != 0, fu = d.flipud != 0;
    // the source rectangle of the tile: the images of two opposite corners bound it (the map is a signed permutation)
    int ay, ax, by, bx;
    source_of(y0, x0, n, d.k, fl, fu, ay, ax);
    source_of(y0 + th - 1, x0 + tw - 1, n, d.k, fl, fu, by, bx);
    const int sy0 = min(ay, by), sx0 = min(ax, bx);
    const int sh = (d.k & 1) ? tw : th, sw = (d.k & 1) ? th : tw;        // <= kTile each
    const int row_bytes = sw * 3;
    const uint8_t* __restrict__ src = pool + I.off + (int64_t)(I.i + sy0) * I.pitch + (int64_t)(I.j + sx0) * 3;
    for (int e = threadIdx.x; e < sh * row_bytes; e += kThreads) {
        const int r = e / row_bytes, q = e - r * row_bytes;
        tile[r * kLdsPitch + q] = src[(int64_t)r * I.pitch + q];
    }
    __syncthreads();
    if (lx >= tw) return;
    for (int y = ly; y < th; y += kRows) {
        int sy, sx;
        source_of(y0 + y, x0 + lx, n, d.k, fl, fu, sy, sx);
        const uint8_t* __restrict__ px = tile + (sy - sy0) * kLdsPitch + (sx - sx0) * 3;
        for (int c = 0; c < C; ++c) {
            const int64_t o = ((int64_t)c * n + y0 + y) * n + x0 + lx;
            float v = __fdiv_rn((float)px[C == 1 ? d.chan : c], 255.0f);
            if (nz) v = v + nz[o];
            out[o] = v;
        }
    }
}

}  // namespace patch
}  // namespace lerf

using namespace lerf;

extern "C" {

int lerf_patch_batch_u8(const uint8_t* pool, int64_t pool_bytes, const lerf_patch_desc_t* desc, const lerf_patch_desc_t* desc_host,
                        int B, int C, int sz, int hsz, const float* noise, float* im, float* lb, void* stream) {
    if (!pool || !desc || !im || !lb || pool_bytes <= 0 || B <= 0 || (C != 1 && C != 3) || sz <= 0 || hsz <= 0) return LERF_EINVAL;
    if (B > 65535) return LERF_EUNSUPPORTED;
    if (desc_host)
        for (int b = 0; b < B; ++b)
            if (!patch::desc_ok(desc_host[b], C, sz, hsz, pool_bytes)) return LERF_EINVAL;
    const int64_t tl = (sz + patch::kTile - 1) / patch::kTile, th = (hsz + patch::kTile - 1) / patch::kTile;
    if (tl * tl + th * th > 0x7fffffff) return LERF_EUNSUPPORTED;
    clear_stale_error();
    hipLaunchKernelGGL(patch::patch_batch_kernel, dim3((unsigned)(tl * tl + th * th), (unsigned)B), dim3(patch::kThreads), 0,
                       (hipStream_t)stream, pool, pool_bytes, desc, C, sz, hsz, (int)tl, noise, im, lb);
    return launch_status();
}

}  // extern "C"
