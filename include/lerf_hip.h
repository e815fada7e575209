/*
 * lerf_hip.h -- C ABI of liblerf_hip.so: the MI355X (gfx950) implementation of
 * the LeRF LUT resampling hot path.
 *
 * The reference (ddlee-cn/LeRF-PyTorch) is pure Python and has no FFI; the
 * boundary a replacement has to offer is its Python class/function API
 * (SURVEY.md section 8b).  This header is what the Python mirror of that API
 * (the lerf-pytorch_amd Python package) binds through ctypes.  Every entry point cites the
 * reference code it replaces (paths relative to the upstream repository).
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / HIP types in the signatures
 *     (`stream` is a hipStream_t passed as void*; NULL = default stream);
 *   - every function returns 0 on success or a negative LERF_E* code -- no
 *     exceptions cross the ABI, nothing is allocated, there is no mutable
 *     global state (per-device "kernel attribute set" flags apart); the caller
 *     owns every buffer, LUT buffers are borrowed read-only;
 *   - device entry points only enqueue work on `stream`; they never
 *     synchronise with the host;
 *   - re-entrant: concurrency = different streams.
 *   - image operands are described by a base pointer plus ELEMENT strides
 *     (sy, sx, sc) so that HWC-interleaved uint8 frames and planar CHW float
 *     tensors go through the same kernels.
 */
#ifndef LERF_HIP_H
#define LERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LERF_ABI_VERSION 7
#define LERF_MAX_MODES 5          /* s, c, t, d, y  (resample/eval_lut_sr.py:12-18) */
#define LERF_LUT_ENTRIES 83521    /* 17^4, interval = 4 (resample/eval_lut_sr.py:27-28) */
#define LERF_MAX_SUPPORT 8

enum {
    LERF_OK = 0,
    LERF_EINVAL = -1,        /* bad argument (null pointer, size <= 0, unknown mode ...) */
    LERF_EUNSUPPORTED = -2,  /* valid request this build has no kernel for */
    LERF_ELAUNCH = -3,       /* HIP reported a launch error */
    LERF_ENODEVICE = -4      /* no usable gfx950 device */
};

enum { LERF_U8 = 0, LERF_F32 = 1, LERF_F64 = 2, LERF_I16 = 3 };
enum {
    LERF_KIND_GAUSS = 0,     /* steering Gaussian, 3 hyper maps  (LeRF-G) */
    LERF_KIND_LINEAR = 1,    /* amplified linear, 1 hyper map    (LeRF-L) */
    LERF_KIND_NEAREST = 2,   /* box2d                              (resize_right/interp_methods.py:67-70, 83-85) */
    LERF_KIND_CUBIC = 3,     /* cubic2d   (:35-43, 73-75)   -- fixed kernels: lerf_warp only, no hyper maps */
    LERF_KIND_BILINEAR = 4,  /* linear2d  (:60-64, 78-80) */
    LERF_KIND_LANCZOS2 = 5,  /* lanczos2d (:46-50, 88-90) */
    LERF_KIND_LANCZOS3 = 6   /* lanczos3d (:53-57, 93-95) */
};

/* Padding rule of the IMAGE operand of stage 3 (the hyper maps are always edge-padded, :172-174): the `pad_mode` argument of
 * the reference's resampler classes, np.pad / F.pad names in brackets (resize_right2d_numpy.py:143,208; _torch.py:189). */
enum {
    LERF_PAD_CONSTANT = 0,   /* zeros ["constant"] -- the default of every class and the only mode of the uint8 paths */
    LERF_PAD_EDGE = 1,       /* ["edge" / "replicate"] */
    LERF_PAD_REFLECT = 2,    /* ["reflect"] */
    LERF_PAD_SYMMETRIC = 3,  /* ["symmetric"] (numpy only) */
    LERF_PAD_WRAP = 4        /* ["wrap" / "circular"] */
};

typedef struct {
    const void* ptr;      /* device pointer */
    int dtype;            /* LERF_U8 / LERF_F32 / LERF_F64 */
    int64_t sy, sx, sc;   /* element strides of row, column, channel */
} lerf_plane_t;

typedef struct {
    void* ptr;
    int dtype;
    int64_t sy, sx, sc;
} lerf_mplane_t;

/* The LUT set of one model, as the reference loads it
 * (resample/eval_lut_sr.py:750-775): int8, C order [17^4][oC]. */
typedef struct {
    int n_modes1;                               /* len(opt.modes)  */
    int n_modes2;                               /* len(opt.modes2) */
    char modes1[LERF_MAX_MODES];                /* e.g. 's','c','t' */
    char modes2[LERF_MAX_MODES];
    int oC;                                     /* 3 = LeRF-G (rho, sigma_x, sigma_y), 1 = LeRF-L (alpha) */
    const int8_t* s1[LERF_MAX_MODES];           /* device, [17^4]      LUT_s1_<mode>r0 */
    const int8_t* s2[LERF_MAX_MODES][2];        /* device, [17^4][oC]  LUT_s2_<mode>r{0,1} */
    const void* fused_pack;                     /* optional (may be NULL): lerf_fused_lutpack_build output */
} lerf_luts_t;

/* Separable SR geometry: the 1-D content of Resize2dNumpy.get_distance's dense
 * maps (resize_right/resize_right2d_numpy.py:106-140); build with
 * lerf_sr_axis_tables and upload. */
typedef struct {
    int S;                   /* support size (2 in every published result, 4 = class default) */
    int out_h, out_w;
    const int32_t* left_r;   /* device [out_h]    first source row of the support (unpadded coords) */
    const float* dis_r;      /* device [out_h*S]  row distances: uint8 outputs (float32 production arithmetic) */
    const int32_t* left_c;   /* device [out_w] */
    const float* dis_c;      /* device [out_w*S] */
    const double* dis_r64;   /* device [out_h*S]: REQUIRED for LERF_F32 and LERF_F64 outputs of lerf_resize (both are evaluated */
    const double* dis_c64;   /* in float64, LERF_EINVAL without them); optional for uint8 outputs, where they arm the tie guard */
    int pad_mode;            /* LERF_PAD_* of the image operand; non-constant modes: float outputs of lerf_resize only */
    /* ---- ABI 4 (zero = the behaviour of ABI 3) */
    int tie_queue_cap;       /* test hook of the tile-fused kernel: outputs within 1.5e-4 of a rounding tie are queued per tile and
                              * re-evaluated in float64 behind the tile's task loop; 0 = the default capacity (2048 per tile), n > 0 =
                              * n entries, < 0 = no queue (every tie is evaluated inside the loop).  Lets the parity tests drive the
                              * overflow path; carried per call, the library keeps no state */
    int roi_y, roi_x;        /* LR region the tiles of lerf_sr_fused_u8 are laid over (origin and extent in LR pixels); roi_h = 0 or */
    int roi_h, roi_w;        /* roi_w = 0: the whole frame.  A rank of a 2-D block partition passes its OWNED block here and the block
                              * plus halo as the frame: halo pixels then only ever serve as tile halos (255 instead of 288 tiles for a
                              * 1080x960 block of a 2160x3840 frame).  OWNERSHIP RULE (ABI 5, exact): the output tables must list
                              * exactly the outputs whose support CENTRE lies in the region, left + S/2 in [roi_y, roi_y + roi_h)
                              * for rows (columns alike) -- i.e. left in [roi_y - S/2, roi_y + roi_h - S/2); outputs beyond a TRUE
                              * frame border (left + S/2 < 0 or >= H) belong to the region that touches that border.  This is the
                              * slicing rule of lerf-pytorch_amd/dist.py (BlockPlan / StripPlan, `check_support`).  A tile looks the
                              * hyper-parameters up on [tile - S/2, tile + T + S/2 - 1): an output whose support merely STARTS in
                              * the last row / column of the region (left = roi_y + roi_h - 1; accepted by ABI 4's wording) reads a
                              * position no tile of this launch fills.  The library cannot check device tables.  With a workspace
                              * the region takes the two-launch path too: stage 1 runs once per pixel over the region widened by
                              * 3 + S/2 pixels (ABI 5; ABI 4 recomputed stage 1 on every tile's halo for regions) */
    /* ---- ABI 5 (zero = the behaviour of ABI 4) */
    int flags;               /* LERF_GEO_* bits, per call (the library reads no environment variables and keeps no state) */
    int out_row_pitch;       /* lerf_sr_fused_u8: BYTES between output rows; 0 = dense rows of out_w * C bytes.  >= out_w * C.  A rank of
                              * a block partition owns 1919 or 1921 output columns at x2: with rows padded to a multiple of 16 bytes its
                              * tiles keep the aligned store paths (dense 5757-byte rows cost +13 % per launch) */
} lerf_sr_geo_t;
#define LERF_GEO_FORCE_GENERAL 1   /* diagnostic: take the general tile-fused kernels where the specialised ones would serve (A/B runs) */
#define LERF_GEO_SINGLE_LAUNCH 2   /* diagnostic: the single-launch kernel although a workspace is passed (the stamped build keeps its stamps there) */
#define LERF_GEO_X2_TABLES 16      /* the caller vouches that the tables are lerf_sr_axis_tables(scale = 2) on both axes (or row / column slices of
                                    * them).  Reserved: read only by the round-4 persistent-kernel experiment (experiments/r04_persist,
                                    * not in this library); ignored */
#define LERF_GEO_NO_PERSIST 32     /* reserved (same experiment); ignored */
#define LERF_GEO_TILE_ROWS_64 64    /* force the tile height of the RGB tile-fused kernels (default: 64 rows, 32 / 16 for launches too small to */
#define LERF_GEO_TILE_ROWS_32 128   /* fill the chip with 64-row tiles -- a 256 x 256 frame runs as 64 tiles of 16 rows); tests and A/B runs */
#define LERF_GEO_TILE_ROWS_16 256
#define LERF_GEO_INPUT_DEVICE 4    /* lerf_sr_fused_u8: the input frames are device memory / pinned host memory (read over PCIe from inside the */
#define LERF_GEO_INPUT_HOST 8      /* kernel, once per pixel); neither bit: the library asks the runtime (one hipPointerGetAttributes per call) */
#define LERF_GEO_EXACT_X2 512      /* the caller's promise that the tables are the x2 SR tables of the WHOLE frame (lerf_sr_axis_tables with scale
                                    * 2.0 and out = 2 x in on both axes, as lerf_sr_geometry_flags verifies): RGB launches of lerf_sr_fused_u8 then
                                    * run the X2 flavour of the tile-fused kernels, which takes the stage-3 geometry from the closed form
                                    * (lerf_sr_x2_tables) and never reads left_* / dis_* (they must still be passed; dis_*64 still arm the tie
                                    * guard).  Taken only with S = 2 (the 4 x 4 support keeps the tables: registers), 64-row tiles (launches small
                                    * enough for the 32- / 16-row tiles keep the tables), out_h = 2 H, out_w = 2 W and no region of interest,
                                    * never by ragged launches; a launch that sets the bit
                                    * with other sizes or a region runs the table path (a slice of x2 tables starts at an arbitrary origin).
                                    * LERF_GEO_FORCE_GENERAL wins.  Same bytes either way */
#define LERF_GEO_FORCE_TABLES 1024 /* diagnostic: the table path although LERF_GEO_EXACT_X2 is set (tests, A/B runs) */

/* Homography geometry (resize_right/resize_right2d_numpy.py:306-407): evaluated
 * per output pixel on the device in float64; pad_* come from lerf_warp_pads. */
typedef struct {
    int S;
    int out_h, out_w;
    double minv[9];          /* inverse of the 3x3 matrix, row major */
    int pad_r_lo, pad_r_hi, pad_c_lo, pad_c_hi;
    int pad_mode;            /* LERF_PAD_*; non-constant modes: float outputs of lerf_warp only */
    /* ---- ABI 7 (zero = the behaviour of ABI 6): one RECTANGLE of the output from a BAND of the source, for partitions of a warp over
     * ranks (lerf-pytorch_amd/dist.py WarpRowPlan).  out_h / out_w are then the rectangle's size, `out` its first pixel; the pixel
     * (i, j) of the rectangle is the output pixel (out_y0 + i, out_x0 + j) -- the offsets enter the projection as integers, so the
     * float64 arithmetic is the whole frame's, bit for bit -- and pad_* stay those of the WHOLE output (lerf_warp_pads).  The source
     * operands (feat / hyper planes, packed maps) hold the frame's rows from src_y0 on: row r of the frame is row r - src_y0 of the
     * operand; H, W stay the frame's.  The caller guarantees that every tap of the rectangle lies in the rows it passes.
     * lerf_warp_fused_u8 takes whole outputs only (offsets must be zero). */
    int out_y0, out_x0, src_y0;
} lerf_warp_geo_t;

/* Remap geometry: the homographic warp with its projected grid READ from a dense coordinate map instead of projected through a
 * matrix -- lens undistortion, rectification, optical-flow and mesh warps.  Entry (i, j) of the map is (row, col) of the source
 * position of output pixel (i, j) in the reference's convention: integers are pixel indices, the values are what
 * get_projected_grid2d (resize_right/resize_right2d_numpy.py:306-342) holds before its clip.  Everything after the point is the
 * warp's: clip to [0, H] x [0, W], support boundary, low pads, taps, arithmetic, tie guard.  A NaN row or column coordinate reads
 * no memory and yields 0 (uint8) / NaN (float); +-inf clip like any other out-of-range value; no map value can produce an
 * out-of-range address. */
#define LERF_REMAP_PADS_FROM_MAP (-1)
typedef struct {
    int S;
    int out_h, out_w;
    const void* coords;      /* device [out_h][row_stride] elements, (row, col) pairs: entry (i, j) at coords + i * row_stride + 2 * j.
                              * Aligned to one entry (16 bytes LERF_F64, 8 bytes LERF_F32): a kernel reads an entry with one load */
    int coords_dtype;        /* LERF_F64 or LERF_F32 (promoted exactly to float64) */
    int64_t row_stride;      /* ELEMENTS between rows of the map; even, >= 2 * out_w */
    int pad_mode;            /* LERF_PAD_*; non-constant modes: float outputs of lerf_remap only */
    int pad_r_lo, pad_c_lo;  /* low pads (calc_pad_sz, :363-369).  LERF_REMAP_PADS_FROM_MAP: the reference's, derived on the device
                              * from coords[0][0] -- max(-left_boundary(clip(.)), 0) -- which makes the map of a homography reproduce
                              * lerf_warp bit for bit.  A tile of a larger map (coords = the tile's first entry, out_h / out_w its
                              * size) passes the WHOLE map's pads explicitly, like lerf_warp_geo_t's rectangles keep the whole
                              * output's.  (Only the low pads reach a tap; the high pads are never needed.) */
} lerf_remap_geo_t;

/* ---------------------------------------------------------------- host side */
int lerf_abi_version(void);
const char* lerf_strerror(int code);

/* number of visible HIP devices (does not initialise a context); <0 on error */
int lerf_device_count(void);

/* Rotated sampling offsets of mode in {'s','c','t','d','y'} for rotation r,
 * expressed in the unrotated frame (resample/eval_lut_sr.py:30-81, 549-553, 468).
 * LERF_EINVAL for an unknown mode == the reference's ValueError (:84). */
int lerf_mode_offsets(char mode, int rot, int8_t dy[4], int8_t dx[4]);

/* 1-D SR tables, float64 arithmetic in the reference's exact operation order
 * (resize_right/resize_right2d_numpy.py:70-79, 85-90, 100-104, 131-134).
 * left[n_out], dis64[n_out*S], dis32[n_out*S] (class-preserving float32
 * rounding: the <0 / [0,1] / >1 classes of the linear kernel are kept),
 * pads[2] = {pad_lo, pad_hi}.  dis32 / pads may be NULL. */
int lerf_sr_axis_tables(int n_in, int n_out, double scale, int S,
                        int32_t* left, double* dis64, float* dis32, int32_t* pads);

/* The same tables with the float32 arithmetic of the reference's torch classes
 * (Resize2dTorch.get_distance, resize_right/resize_right2d_torch.py:48-103): bit-equal to the class's
 * field_of_view / dis tensors, including the scales where float32 and float64 put a support boundary on different
 * sides (x3, S=2).  pads may be NULL. */
int lerf_sr_axis_tables_f32(int n_in, int n_out, double scale, int S, int32_t* left, float* dis32, int32_t* pads);

/* Exact x2 (scale 2.0, n_out = 2 n_in, even S) in closed form: output i has first tap (i + 1) / 2 - S / 2 and tap k at
 * distance S / 2 - k - 1/4 (even i) or S / 2 - k - 3/4 (odd i) -- the same bits in float32 and float64.
 * lerf_sr_x2_tables writes the closed form as tables (any of left / dis64 / dis32 may be NULL).
 * lerf_sr_x2_owned writes, for every tile t of `tile` LR pixels along one axis of n_in pixels, the owned outputs
 * ranges[2 t] .. ranges[2 t + 1] (half open) -- what the X2 kernels compute instead of searching `left`.
 * lerf_sr_geometry_flags is the host geometry builder's verdict on a pair of axis tables it has just built (host memory):
 * LERF_GEO_EXACT_X2 when both scales are exactly 2.0, out = 2 x in on both axes and every entry equals the closed form
 * bit for bit, else 0 (also for bad arguments). */
int lerf_sr_x2_tables(int n_out, int S, int32_t* left, double* dis64, float* dis32);
int lerf_sr_x2_owned(int n_in, int tile, int32_t* ranges);
int lerf_sr_geometry_flags(int H, int W, int out_h, int out_w, double scale_h, double scale_w, int S,
                           const int32_t* left_r, const double* dis_r64, const float* dis_r32,
                           const int32_t* left_c, const double* dis_c64, const float* dis_c32);

/* ceil(scale * n_in) (resize_right/resize_right2d_numpy.py:41-45) */
int lerf_out_size(int n_in, double scale);

/* 3x3 inverse (adjugate).  Callers that need bit parity with the reference pass
 * np.linalg.inv's result instead (resize_right/resize_right2d_numpy.py:327). */
int lerf_invert3x3(const double m[9], double out[9]);

/* Pad sizes {r_lo, r_hi, c_lo, c_hi} of Warp2dNumpy.calc_pad_sz from the two
 * corner pixels (:363-369), for the INVERSE homography `minv`. */
int lerf_warp_pads(const double minv[9], int in_h, int in_w, int out_h, int out_w, int S,
                   int32_t pads[4]);

/* -------------------------------------------------------------- device side */

/* FourSimplexInterpFaster (resample/eval_lut_sr.py:24-470) without the final
 * rot90 and /q: integer numerators (value*16) of the 4-simplex interpolation
 * of `lut` ([17^4][oC] int8) over 4 pixels sampled at offsets (dy[k], dx[k])
 * from each of the h x w positions of the uint8 image `img` (coordinates are
 * clamped to [0,img_h-1] x [0,img_w-1]).  out: int16 [C][oC][h][w].
 * interval: the LUT's sampling interval (:27-28; q = 2^interval, L = 2^(8-interval) + 1 levels per axis, `lut` has
 * L^4 rows, numerators are value * q); 4 for every shipped LUT, 1..7 accepted. */
int lerf_lut_interp_i16(const lerf_plane_t* img, int img_h, int img_w, int C,
                        int h, int w, const int8_t dy[4], const int8_t dx[4],
                        const int8_t* lut, int oC, int interval, int16_t* out, void* stream);

/* ABI 6.  The same pass with the reference's epilogue inside the store: the image may be LERF_U8 or LERF_F32 (float32 arrays of
 * integer values are what the call sites hand over, resample/eval_lut_sr.py:549-553; other values are rounded half-to-even and
 * clipped to 0..255), `out` is LERF_I16 (numerators, value * q), LERF_F32 or LERF_F64 (VALUES, numerator / q: :469) with SIGNED
 * element strides sy / sx over the h x w positions and sc between the C * oC result planes -- a caller that points `ptr` at the
 * right corner and hands in the strides of a rotated view gets np.rot90(result, rot, [1, 2]) (:464-468) written in place. */
int lerf_lut_interp(const lerf_plane_t* img, int img_h, int img_w, int C, int h, int w, const int8_t dy[4], const int8_t dx[4],
                    const int8_t* lut, int oC, int interval, const lerf_mplane_t* out, void* stream);

/* ABI 7.  lerf_lut_interp with per-call flags (0 = lerf_lut_interp).  For the shipped interval (4) the pass runs in persistent
 * workgroups that keep one byte plane of the LUT in LDS (csrc/lerf_lut_interp.hip) when the launch is large enough to pay for it
 * (>= 65 536 positions), the pattern reaches no further than 3 pixels, C <= 4, the image strides are non-negative and one of the
 * output strides sy / sx is +-1; the direct kernel (LUT gathered from L1 / L2) serves everything else -- same values either way.
 *   LERF_INTERP_ACCUMULATE  out += result instead of out = result: the call sites' `pred += FourSimplexInterpFaster(...)`
 *                           (resample/eval_lut_sr.py:555, :564, :589, :601) without a second pass over the planes.  The planes
 *                           must hold valid numbers (the first call of a sum runs without the flag).
 *   LERF_INTERP_LDS / LERF_INTERP_DIRECT   tests and A/B runs: insist on one of the two kernels (LERF_EUNSUPPORTED when the LDS
 *                           kernel does not cover the call). */
#define LERF_INTERP_ACCUMULATE 1
#define LERF_INTERP_LDS 2
#define LERF_INTERP_DIRECT 4
#define LERF_INTERP_TILE64 8       /* A/B runs: force the larger (128 x 32) / smaller (128 x 16) tile of the LDS kernel (default: by the launch's tile count) */
#define LERF_INTERP_TILE32 16
#define LERF_INTERP_LUT_PLANAR 32  /* `lut` is oC planes of 83 584 bytes (17^4 entries + padding to 64), plane k = channel k of every entry: the
                                    * LDS kernel's own format (it copies one plane per workgroup; from the reference's [17^4][oC] layout it has to
                                    * read all oC).  Interval 4 only; LERF_EUNSUPPORTED when the LDS kernel does not cover the call (the caller
                                    * repeats it with the interleaved table) */
#define LERF_LUT_PLANE_BYTES 83584
int lerf_lut_interp_ex(const lerf_plane_t* img, int img_h, int img_w, int C, int h, int w, const int8_t dy[4], const int8_t dx[4],
                       const int8_t* lut, int oC, int interval, const lerf_mplane_t* out, int flags, void* stream);

/* ABI 7.  The call sites' epilogue of a LUT stage (resample/eval_lut_sr.py:573-577, 621-628, resample/eval_lut_warp.py:136-140,
 * 185-191), applied to the int16 NUMERATORS a chain of LERF_INTERP_ACCUMULATE passes has summed (value = numerator / 2^interval):
 *     np.round(np.clip(pred / avg_factor + bias, 0, norm)).astype(np.float32)
 * as a program of float64 steps in the caller's order -- each step is numpy's own float64 operation (IEEE division, addition,
 * minimum / maximum, round-half-even), the result is rounded once to float32: bit for bit what numpy returns for the float64
 * array acc / 2^interval.  acc: int16 [n]; out: float32 [n] (device, dense). */
enum { LERF_EPI_DIV = 0, LERF_EPI_MUL = 1, LERF_EPI_ADD = 2, LERF_EPI_CLIP = 3, LERF_EPI_ROUND = 4 };
#define LERF_EPI_MAX_OPS 8
typedef struct { int op; double a, b; } lerf_epi_op_t;   /* DIV / MUL / ADD: operand a; CLIP: [a, b]; ROUND: none */
int lerf_numer_epilogue_f32(const int16_t* acc, int64_t n, int interval, const lerf_epi_op_t* ops, int n_ops, float* out, void* stream);

/* LUT pack for the tile-fused kernel (1..4 modes per stage, any of "sdyct"; oC = 1 or 3): the stage-1
 * LUTs padded to 16-byte multiples, and the stage-2 LUTs as one uint32 per
 * entry holding the oC biased bytes, cut into the pieces the kernel stages (layout in DESIGN.md).  The caller owns
 * `buf` (lerf_fused_lutpack_bytes(luts) bytes of device memory; 0 = this LUT set has no fused kernel) and stores it in
 * lerf_luts_t.fused_pack. */
size_t lerf_fused_lutpack_bytes(const lerf_luts_t* luts);
int lerf_fused_lutpack_build(const lerf_luts_t* luts, void* buf, void* stream);

/* Stages 1+2 of eltr._worker (resample/eval_lut_sr.py:541-628,
 * resample/eval_lut_warp.py:104-191): uint8 image -> feat (uint8, same shape)
 * and hyper numerators hq (uint8, [H][W][C][oC] through `hyper` strides with
 * sc = stride of c and the oC values contiguous).  feat/hyper may alias
 * nothing.  Either output pointer may be NULL to skip writing it. */
int lerf_lut_stages_u8(const lerf_plane_t* img, int H, int W, int C,
                       const lerf_luts_t* luts,
                       const lerf_mplane_t* feat, const lerf_mplane_t* hyper,
                       void* stream);

/* Stage 3, SR: SteeringGaussianResize2dNumpy.resize (:162-223) /
 * AmplifiedLinearResize2dNumpy.resize (:243-282) and their Torch twins
 * (resize_right/resize_right2d_torch.py:154-197, 214-247).
 * feat: uint8 or float32.  hyper[k]: uint8 numerators (h = u8/255) or float32
 * maps in [0,1]; k = rho, sigma_x, sigma_y (gauss) or alpha (linear).
 * out: uint8 (clip(rne)), float32 or float64 (float64 arithmetic).
 * kind NEAREST / CUBIC / BILINEAR / LANCZOS2 / LANCZOS3: the fixed-kernel resize of Resize2dTorch.resize +
 * BicubicResize2dTorch (resize_right2d_torch.py:105-138, interp_methods.py:35-95) on the same geometry;
 * `hyper` is ignored (may be NULL). */
int lerf_resize(const lerf_plane_t* feat, const lerf_plane_t hyper[3],
                int H, int W, int C, const lerf_sr_geo_t* geo,
                int kind, double max_sigma, const lerf_mplane_t* out, void* stream);

/* Stage 3, homography: SteeringGaussianWarp2dNumpy.warp (:516-577),
 * AmplifiedLinearWarp2dNumpy.warp (:597-636), NearestWarp2dNumpy (:460-467,
 * 409-449), the fixed-kernel baselines Bicubic/Bilinear/Lanczos2/Lanczos3Warp2dNumpy
 * (:451-494) and the Torch twins (resize_right2d_torch.py:346-487).
 * Pixels whose weights all vanish are NaN in float outputs (the reference's
 * 0/0) and 0 in uint8 outputs.  There is no mask operand: the harness's validity
 * mask (eval_lut_warp.py:197-204) is a NEAREST warp (S = 1) of a white frame with
 * a black border, compared with 255 by the caller. */
int lerf_warp(const lerf_plane_t* feat, const lerf_plane_t hyper[3],
              int H, int W, int C, const lerf_warp_geo_t* geo,
              int kind, double max_sigma, const lerf_mplane_t* out, void* stream);

/* Stages 1+2 by the tile-fused kernel (luts->fused_pack set), `n` frames:
 * packed[(y*W + x)*C + c] = hq0 | hq1<<8 | hq2<<16 | feat<<24  (hq1, hq2 = 0 for LeRF-L).
 * Same values as lerf_lut_stages_u8, ~4x faster; feeds lerf_warp_packed / lerf_unpack_stages.
 * workspace: optional device scratch (NULL = none) of `workspace_bytes` bytes: with it stage 1 runs as its own launch
 * without recomputing tile halos, like lerf_sr_fused_u8.  LERF_EINVAL when it is non-NULL and smaller than
 * lerf_sr_fused_workspace_bytes(H, W, C, n). */
int lerf_stages_packed_u8(const uint8_t* img, int64_t in_sn, int n, int H, int W, int C,
                          const lerf_luts_t* luts, uint32_t* packed, int64_t packed_sn,
                          void* workspace, size_t workspace_bytes, void* stream);

/* packed dwords -> feat uint8 [n_pxch] and hq uint8 [n_pxch][oC] (either may be NULL) */
int lerf_unpack_stages(const uint32_t* packed, int64_t n_pxch, int oC, uint8_t* feat, uint8_t* hq, void* stream);

/* lerf_warp (gauss / linear) reading the packed stage outputs of `n` HWC frames that share one homography (frame
 * strides packed_sn in dwords, out_sn in elements of `out`; n = 1: one frame) in ONE launch; out: uint8 or float32 */
int lerf_warp_packed(const uint32_t* packed, int64_t packed_sn, int n, int H, int W, int C, const lerf_warp_geo_t* geo,
                     int kind, double max_sigma, const lerf_mplane_t* out, int64_t out_sn, void* stream);

/* Stage 3 by a dense coordinate map (lerf_remap_geo_t): lerf_warp / lerf_warp_packed with the point of every output pixel read from
 * the map.  Same operands, dtype table, kinds, supports, pad modes and arithmetic as their namesakes -- after the point is known the
 * kernels run the same code -- so the map of a homography (its unclipped projected grid) gives lerf_warp's bytes.  There is no
 * tile-fused remap (a dense map has no closed-form tile boxes); the backward is lerf_remap_bwd (at the end of this header).
 *   lerf_remap_host_geometry   host, no GPU: geo->coords is HOST memory; writes what the kernels derive from the map -- pads[2] =
 *                              the low pads (row, col) and, per output pixel, the clipped point gr / gc (padded coordinates) and the
 *                              support's first tap lr / lc ([out_h * out_w] each; any may be NULL). */
int lerf_remap(const lerf_plane_t* feat, const lerf_plane_t hyper[3],
               int H, int W, int C, const lerf_remap_geo_t* geo,
               int kind, double max_sigma, const lerf_mplane_t* out, void* stream);
int lerf_remap_packed(const uint32_t* packed, int64_t packed_sn, int n, int H, int W, int C, const lerf_remap_geo_t* geo,
                      int kind, double max_sigma, const lerf_mplane_t* out, int64_t out_sn, void* stream);
int lerf_remap_host_geometry(const lerf_remap_geo_t* geo, int H, int W, double* gr, double* gc, int32_t* lr, int32_t* lc,
                             int32_t pads[2]);

/* The same with ONE MAP PER SAMPLE: `n_maps` maps of geo's shape, dtype and row_stride, `map_stride` ELEMENTS apart; geo describes
 * map 0.  A call returns exactly what n_maps calls of the plain entry point return, one per map, in one launch:
 *   lerf_remap_batched          C == n_maps * planes_per_map planes; plane p reads map p / planes_per_map
 *   lerf_remap_packed_batched   n == n_maps frames; frame f reads map f (RGB S = 2 gauss / linear: one thread per pixel and frame)
 * LERF_REMAP_PADS_FROM_MAP is resolved per map, from that map's own first entry; explicit pads apply to every map of the call.
 * Refused with LERF_EINVAL before anything is launched: n_maps < 1; a plane or frame count other than n_maps * planes_per_map
 * (n_maps for the packed form); a negative or odd map_stride (an entry is two elements: an even stride keeps every map's entries
 * aligned like map 0's); for n_maps > 1 a map_stride below (out_h - 1) * row_stride + 2 * out_w (overlapping maps).  n_maps == 1
 * is the plain entry point.  lerf_coords_build_dev writes such a batch of model maps in one launch; the mesh builder, compose,
 * invert and their adjoints take a batch through lerf_coords_*_batched (the end of this header). */
int lerf_remap_batched(const lerf_plane_t* feat, const lerf_plane_t hyper[3], int H, int W, int C, const lerf_remap_geo_t* geo,
                       int n_maps, int64_t map_stride, int planes_per_map, int kind, double max_sigma, const lerf_mplane_t* out,
                       void* stream);
int lerf_remap_packed_batched(const uint32_t* packed, int64_t packed_sn, int n, int H, int W, int C, const lerf_remap_geo_t* geo,
                              int n_maps, int64_t map_stride, int kind, double max_sigma, const lerf_mplane_t* out, int64_t out_sn,
                              void* stream);

/* ABI 7.  The whole warp path of the harness (resample/eval_lut_warp.py:100-222: stage 1, stage 2, SteeringGaussianWarp2dNumpy /
 * AmplifiedLinearWarp2dNumpy.warp, resize_right/resize_right2d_numpy.py:516-636) for `n` RGB frames that share one homography,
 * TILE-FUSED: stage 1 runs once per pixel into the workspace (as in lerf_sr_fused_u8); the second launch runs stage 2 per 64 x 64
 * source tile and evaluates, from the tile's packed stage outputs in LDS, the output pixels that tile OWNS -- those whose 2 x 2
 * support (clamped into the frame) has its last tap row / column inside the tile; pixels projected outside the frame are clipped
 * onto its border like the reference clips its grid (:338-339) and belong to the border tiles.  No packed maps travel through
 * HBM (lerf_stages_packed_u8 + lerf_warp_packed write and re-read 12 bytes per source pixel); same bytes as that path.
 *   lerf_warp_tile_boxes   host: boxes[t] = {i0, i1, j0, j1}, the output rows x columns that bound what tile t (row-major,
 *                          ceil(H / 64) x ceil(W / 64) tiles) owns; one pass over the output per homography.  The caller uploads
 *                          them (int32 [tiles][4]) and passes the device pointer as `tile_boxes`.
 *   workspace              device scratch of at least lerf_sr_fused_workspace_bytes(H, W, C, n) bytes (required).
 * RGB frames, S = 2, the shipped pattern set "sct" / "sct", constant padding, max_sigma <= 13, out_h * out_w < 2^26:
 * lerf_warp_fused_supported says so; everything else: lerf_stages_packed_u8 + lerf_warp_packed. */
int lerf_warp_tile_boxes(const lerf_warp_geo_t* geo, int H, int W, int32_t* boxes);
int lerf_warp_fused_supported(int C, const lerf_luts_t* luts, const lerf_warp_geo_t* geo, int H, int W, int kind, double max_sigma);
int lerf_warp_fused_u8(const uint8_t* img, int64_t in_sn, int n, int H, int W, int C, const lerf_luts_t* luts, const lerf_warp_geo_t* geo,
                       const int32_t* tile_boxes, int kind, double max_sigma, uint8_t* out, int64_t out_sn, void* workspace,
                       size_t workspace_bytes, void* stream);

/* Whole SR path of eltr._worker (resample/eval_lut_sr.py:541-665) for a batch of `n` frames (batch strides
 * in_sn / out_sn in elements): uint8 HWC in -> uint8 HWC out.
 * workspace != NULL (`workspace_bytes` >= lerf_sr_fused_workspace_bytes(H, W, C, n) bytes of device memory, LERF_EINVAL
 * when shorter): TWO launches over the same grid of 64x64 LR tiles; stage 1 runs once per pixel and its
 * uint8 output (C bytes per LR pixel) waits in the workspace, the second launch runs stage 2, the finalisation and stage
 * 3 per tile; the hyper-parameters never leave the CU.
 * workspace == NULL: ONE launch; every tile recomputes stage 1 on its halo (about 4 % slower on a batch, the better
 * choice for a single frame or block that fills the chip once) and nothing but the input, the LUT pack and the output
 * touches HBM.  Configurations outside the tile-fused kernel (see lerf_sr_fused_supported) need the workspace and run
 * the three direct kernels through it. */
size_t lerf_sr_fused_workspace_bytes(int H, int W, int C, int n);
int lerf_sr_fused_u8(const uint8_t* img, int64_t in_sn, int n, int H, int W, int C,
                     const lerf_luts_t* luts, const lerf_sr_geo_t* geo,
                     int kind, double max_sigma,
                     uint8_t* out, int64_t out_sn, void* workspace, size_t workspace_bytes, void* stream);
/* 1 when lerf_sr_fused_u8 would take the tile-fused kernels for this configuration, 0 when it would fall back to the
 * direct kernels (host-side query, no device work) */
int lerf_sr_fused_supported(int C, const lerf_luts_t* luts, const lerf_sr_geo_t* geo, int H, int W, int kind, double max_sigma);

/* Frames of DIFFERENT sizes through ONE launch pair of the general tile-fused kernels (each workgroup finds its frame in a
 * descriptor table that travels in the kernel arguments: 16 frames per launch pair, more frames = more launch pairs): what
 * eltr.run does image by image over a benchmark folder (resample/eval_lut_sr.py:489-512).  Every item carries its own
 * geometry; the support S, pad_mode, tie_queue_cap and flags must be the same for all items (LERF_EINVAL otherwise), an
 * item with a region of interest sends the call item by item through lerf_sr_fused_u8, as does any configuration without
 * a tile-fused kernel.  All frames, tables and the workspace live on ONE device (the caller's current one).  `items` is a
 * HOST array.  workspace: device scratch of at least lerf_sr_ragged_workspace_bytes(items, n, C) bytes (required). */
typedef struct {
    const uint8_t* img;      /* device, dense uint8 [H][W][C] */
    uint8_t* out;            /* device, dense uint8 [geo.out_h][geo.out_w][C] */
    int H, W;
    lerf_sr_geo_t geo;
} lerf_sr_item_t;
size_t lerf_sr_ragged_workspace_bytes(const lerf_sr_item_t* items, int n, int C);
int lerf_sr_fused_ragged_u8(const lerf_sr_item_t* items, int n, int C, const lerf_luts_t* luts, int kind, double max_sigma,
                            void* workspace, size_t workspace_bytes, void* stream);
/* the same for stages 1+2 alone (packed dwords out, see lerf_stages_packed_u8): the warp harness' stage passes over a
 * folder of images (resample/eval_lut_warp.py:100-191) */
typedef struct {
    const uint8_t* img;      /* device, dense uint8 [H][W][C] */
    uint32_t* packed;        /* device, dense uint32 [H][W][C] */
    int H, W;
} lerf_stage_item_t;
size_t lerf_stages_ragged_workspace_bytes(const lerf_stage_item_t* items, int n, int C);
int lerf_stages_packed_ragged_u8(const lerf_stage_item_t* items, int n, int C, const lerf_luts_t* luts,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* Halo plumbing of the multi-GPU partitions (lerf-pytorch_amd/dist.py): copies up to LERF_MAX_RECTS rectangles between
 * a batch of dense uint8 frames [n][fh][fw][C] and one contiguous staging buffer, in ONE launch.
 * to_staging = 1: frame rectangles -> staging (pack before the sends); 0: staging -> frame rectangles (unpack after the
 * receives).  Rectangle r covers rows [y, y+h) x columns [x, x+w) of every frame and lives at staging + off (bytes) as a
 * dense [n][h][w][C] block. */
#define LERF_MAX_RECTS 8
typedef struct { int y, x, h, w; int64_t off; } lerf_rect_t;
int lerf_rect_copy_u8(uint8_t* frames, int n, int fh, int fw, int C, uint8_t* staging,
                      const lerf_rect_t* rects, int n_rects, int to_staging, void* stream);

/* ---- evaluation metrics of the reference harness, on the device (uint8 HWC RGB, row pitch in elements).
 * Each call leaves two doubles in `result` (device memory): a sum and a count; no host sync.
 *
 * lerf_metric_y_sse_u8: ingredients of PSNR(_rgb2ycbcr(gt)[:,:,0], _rgb2ycbcr(out)[:,:,0], shave)
 *   (resample/eval_lut_sr.py:741-742, common/utils.py:46-76, 138-151): result[0] = sum over the frame minus a
 *   `shave`-pixel border of (float32(Y_out) - float32(Y_gt))^2, result[1] = number of pixels summed.
 * lerf_metric_ssim_y_u8: cal_ssim(y_gt, y_out) (eval_lut_sr.py:743, common/utils.py:177-206; 11x11 Gaussian
 *   window sigma 1.5, 'valid', float64): result[0] = sum of the SSIM map, result[1] = (H-10)*(W-10).
 * lerf_metric_masked_sse_u8: ingredients of mPSNR(sr, hr, mask) (resample/eval_lut_warp.py:233,
 *   common/utils.py:168-175) over n = H*W*C elements: result[0] = sum (mask*(sr-hr)/255)^2 in float32 steps,
 *   result[1] = sum(mask); mask is 0 / non-zero bytes. */
int lerf_metric_y_sse_u8(const uint8_t* gt, int64_t gt_sy, const uint8_t* out, int64_t out_sy, int H, int W, int shave,
                         double* result, void* stream);
int lerf_metric_ssim_y_u8(const uint8_t* gt, int64_t gt_sy, const uint8_t* out, int64_t out_sy, int H, int W,
                          double* result, void* stream);
int lerf_metric_masked_sse_u8(const uint8_t* sr, const uint8_t* hr, const uint8_t* mask, int64_t n, double* result,
                              void* stream);

/* ---- fine-tuning path: the trainable float32 twin of the LUT pass, SWF2LUT.InterpTorchBatch
 * (resample/model.py:172-385), forward and backward.
 * weight: float32 [17^4][oC] LUT parameters (LUT value = clamp(rne(127 w), -127, 127), :177-179);
 * img: float32 [n_planes][h+bd][w+bd], integer-valued 0..255, already rotated and replicate-padded by the caller
 * (SWF2LUT.predict, :398-431), n_planes = B*C; out / grad_out: float32 [n_planes][oC][h][w]  (= [B][C*oC][h][w]).
 * mode: one of "sdyct"; modes c and t read their LSBs at the 'y' pattern pixels exactly like the reference
 * (:229-232, :240-243).  bd >= the pattern reach (mode_pad_dict: s 1, d 2, y 2, c 3, t 3).
 * Backward = what autograd derives for the reference code: grad_weight (accumulated with float atomics INTO the
 * caller's buffer, so zero it or pass the running .grad) and grad_img (same; through the LSB terms only).  Either
 * gradient pointer may be NULL. */
int lerf_swf2lut_interp_f32(const float* weight, int oC, char mode, const float* img, int n_planes, int h, int w, int bd,
                            float* out, void* stream);
int lerf_swf2lut_interp_bwd_f32(const float* weight, int oC, char mode, const float* img, const float* grad_out,
                                int n_planes, int h, int w, int bd, float* grad_weight, float* grad_img, void* stream);

/* Backward of lerf_resize on planar float32 maps, as autograd derives it for the reference's torch resizes
 * (SteeringGaussianResize2dTorch / AmplifiedLinearResize2dTorch.resize, Resize2dTorch.resize with BicubicResize2dTorch's
 * cubic and the bilinear / lanczos kinds on the same base class, resize_right2d_torch.py:105-247), on the float32 distance
 * tables of `geo`.
 * feat, h0..h2: float32 [N][H][W] (hyper maps in [0,1]; h0..h2 for GAUSS, h0 alone for LINEAR, none for the fixed kinds
 * NEAREST..LANCZOS3, where they may be NULL), grad_out: float32 [N][out_h][out_w].  grad_feat / grad_h*: float32 [N][H][W],
 * ACCUMULATED into with float atomics (zero them first); any of them may be NULL.  Kinds GAUSS and LINEAR give image and
 * hyper-map gradients, the fixed kinds the image gradient only (their weights are the forward's k(dx) k(dy) / (sr sc),
 * not normalised at S = 1).  The image gradient follows geo->pad_mode, LERF_PAD_CONSTANT..LERF_PAD_WRAP (else LERF_EINVAL):
 * constant: taps outside the frame get nothing; edge / reflect / symmetric / wrap: the pixel the pad names, F.pad's
 * backward.  Hyper gradients land on the clamped tap pixel (replicate). */
int lerf_resize_bwd_f32(const float* feat, const float* h0, const float* h1, const float* h2, int N, int H, int W,
                        const lerf_sr_geo_t* geo, int kind, double max_sigma, const float* grad_out, float* grad_feat,
                        float* grad_h0, float* grad_h1, float* grad_h2, void* stream);

/* Backward of lerf_warp on planar float32 maps, as autograd derives it for the reference's torch warps
 * (SteeringGaussianWarp2dTorch / AmplifiedLinearWarp2dTorch / NearestWarp2dTorch / BicubicWarp2dTorch.warp and the
 * bilinear / lanczos kinds on the same base class, resize_right2d_torch.py:249-487): float64 distances, weights and
 * normalisation; each tap's terms rounded to float32 and summed in float32.
 * feat, h0..h2: float32 [N][H][W] (hyper maps in [0,1]; h0 alone for LINEAR, none for the fixed kinds), grad_out: float64
 * [N][out_h][out_w] (the warps return float64).  grad_feat / grad_h*: float32 [N][H][W], ACCUMULATED into with float
 * atomics (zero them first); any of them may be NULL.  Kinds GAUSS and LINEAR give image and hyper-map gradients, the fixed
 * kinds the image gradient only.  geo: whole outputs only (out_y0 = out_x0 = src_y0 = 0, else LERF_EUNSUPPORTED); the image
 * gradient follows geo->pad_mode (constant: taps outside the frame get nothing; replicate / reflect / wrap: the pixel the pad
 * names, F.pad's backward), hyper gradients land on the clamped tap pixel (replicate).  Pixels whose weights all vanish are
 * NaN in the forward and hand their taps NaN, as autograd does. */
int lerf_warp_bwd(const float* feat, const float* h0, const float* h1, const float* h2, int N, int H, int W,
                  const lerf_warp_geo_t* geo, int kind, double max_sigma, const double* grad_out, float* grad_feat,
                  float* grad_h0, float* grad_h1, float* grad_h2, void* stream);

/* ---- net -> LUT transfer (resample/transfer_to_lut.py:12-170): one hyper-network of the reference's SRNetsSWF2
 * (resample/model.py:81-99; an SRNet = SRUnit MLP, common/network.py:40-163) evaluated on all L^4 sampled pixel
 * tuples (L = 2^(8-interval) + 1; get_input_tensor :12-42, first pixel = slowest axis) and quantised like :117-119:
 * lut[e][c] = int8(round_half_even(clamp(y, -1, 1) * 127)), C order [L^4][outC] -- the array the reference saves as
 * LUT_<key>.npy (there with two trailing singleton dims, scripts.sh:19-24).
 * weights: device, lerf_srnet_weight_floats(outC) floats: W1[64][4] b1[64] W2[64][64] b2[64] W3[64][128] b3[64]
 * W4[64][192] b4[64] W5[64][256] b5[64] W6[outC][320] b6[outC]  (the state_dict tensors of one SRNet, flattened in
 * module order).  y (optional, device float32 [L^4][outC]): the network outputs before quantisation.
 * The hidden layers run on the matrix cores (float32-input MFMA: exact float32 arithmetic). */
size_t lerf_srnet_weight_floats(int outC);
int lerf_srnet_to_lut(const float* weights, int outC, int interval, int8_t* lut, float* y, void* stream);

/* ---- training the hyper-networks (train_model.py -e ... --twoStage, model SRNetsSWF2, resample/model.py:69-129): one
 * SRNet on image planes, forward and backward, the trainable twin of lerf_srnet_to_lut.
 * weights: device, lerf_srnet_weight_floats(outC) floats in the packed layout above; outC 1..4 (else LERF_EUNSUPPORTED).
 * img: float32 [n_planes][h+bd][w+bd] (values in [0,1] as the reference feeds its nets), already rotated and
 * replicate-padded by the caller (SRNetsSWF2.predict); mode: one of "sdyct" with its own pattern pixels (lerf_mode_offsets,
 * rotation 0: no LSB quirk), bd >= the pattern reach (mode_pad_dict: s 1, d 2, y 2, c 3, t 3), else LERF_EINVAL.
 * out / grad_out: float32 [n_planes][outC][h][w] (= [B][C*outC][h][w]); out = tanh(net), SRNet.forward (common/network.py:
 * 127-163) -- the scale by norm//2, the straight-through round and the rotation stay with the caller.
 * Backward = what autograd derives for the reference module, the forward recomputed inside (nothing is kept between the
 * calls): grad_weights (packed layout, required) and grad_img (float32 [n_planes][h+bd][w+bd], may be NULL) are ACCUMULATED
 * into.  Deterministic: no float atomics, repeated calls give bitwise-identical gradients.  workspace: device memory of at
 * least lerf_srnet_bwd_workspace_bytes(outC, n_planes, h, w) bytes (else LERF_EINVAL), contents arbitrary, used by this
 * call only (per-workgroup weight-gradient slabs and a per-position input-gradient buffer); 0 for a bad outC or shape. */
int lerf_srnet_fwd_f32(const float* weights, int outC, char mode, const float* img, int n_planes, int h, int w, int bd,
                       float* out, void* stream);
size_t lerf_srnet_bwd_workspace_bytes(int outC, int n_planes, int h, int w);
int lerf_srnet_bwd_f32(const float* weights, int outC, char mode, const float* img, const float* grad_out, int n_planes, int h,
                       int w, int bd, float* grad_weights, float* grad_img, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ---- LeRF-Net (resample/model.py:434-537): the forward of one IMDN_RTC net at upscale 1, i.e. one stage of IMDN2
 * (stage1: in_nc -> in_nc channels, stage2: in_nc -> in_nc * outC).  fea_conv 3x3, five IMDModule_speed (c1..c3 3x3 +
 * LeakyReLU(0.05), distilled d = nf/4 channels split off each; c4 3x3 -> d; c5 1x1 over the 4d concatenated channels +
 * the module input), LR_conv 1x1 + fea, upsampler conv 3x3 -> out_nc; every conv zero-padded by (k-1)/2.
 * weights: device, lerf_imdn_weight_floats(nf, in_nc, out_nc) floats: the state_dict tensors of the IMDN_RTC in
 * state_dict order, each in PyTorch's [out][in][kh][kw] order (model.0, model.1.sub.{0..4}.c{1..5}, model.1.sub.5,
 * model.2; weight then bias; csrc/lerf_imdn_layout.h).  nf a multiple of 16 in [16, 64], in_nc 1 or 3, out_nc 1, 3 or 9
 * (else LERF_EUNSUPPORTED; 0 from the size queries).
 * x: float32 NCHW [B][in_nc][H][W]; out: float32 NCHW [B][out_nc][H][W]; B, H, W >= 1.
 * post: 0 the raw net output, 1 clamp(y, -1, 1) * 127 + 127 (IMDN2.predict stage 1 at norm 255), 2 clamp(y, -1, 1) / 2
 * + 1/2 (stage 2); each step rounded to float32 as the reference's torch ops are.
 * workspace: device memory of at least lerf_imdn_workspace_bytes(nf, B, H, W) bytes (18 nf bytes per pixel; NHWC
 * activations), contents arbitrary, used by this call only.  A short workspace, a null pointer or a bad shape or post is
 * LERF_EINVAL, and nothing is written.  Float32 products and sums on the matrix cores (v_mfma_f32_16x16x4_f32); no
 * atomics, so the output is deterministic and image b of a batch equals image b run alone.  Launches on `stream`, no
 * sync. */
size_t lerf_imdn_weight_floats(int nf, int in_nc, int out_nc);
size_t lerf_imdn_workspace_bytes(int nf, int B, int H, int W);
int lerf_imdn_fwd_f32(const float* weights, int nf, int in_nc, int out_nc, const float* x, int B, int H, int W, int post,
                      void* workspace, size_t workspace_bytes, float* out, void* stream);

/* ---- training LeRF-Net (train_model.py with model IMDN2): the saving forward and the backward of one IMDN_RTC net, the
 * trainable twin of lerf_imdn_fwd_f32.  weights, nf, in_nc, out_nc, x, B, H, W, post, out: as lerf_imdn_fwd_f32, the same
 * supported set (else LERF_EUNSUPPORTED; 0 from the size queries).
 * lerf_imdn_fwd_train_f32: out is bit-equal to lerf_imdn_fwd_f32's for the same arguments.  saved: device memory of at
 * least lerf_imdn_saved_bytes(nf, in_nc, out_nc, B, H, W) bytes ((23.25 nf + out_nc) floats per pixel: fea, every module's
 * output, concatenated distilled channels and three remaining-channel planes, the upsampler conv's input, the raw output
 * that decides the clamp mask); it needs no other workspace.  Hand saved, unchanged, with the same weights, x, shape and
 * post to lerf_imdn_bwd_f32.
 * lerf_imdn_bwd_f32: what autograd derives for the reference module and IMDN2.predict's clamp and affine (post 1: 127 where
 * -1 <= y <= 1, post 2: 1/2 there, 0 elsewhere; LeakyReLU(0.05)'s slope where the activation is <= 0).
 * grad_out: float32 NCHW [B][out_nc][H][W].  grad_weights: lerf_imdn_weight_floats floats in the packed layout; every float
 * is written exactly once: OVERWRITTEN, not accumulated into (no need to zero it).  grad_x: float32 NCHW [B][in_nc][H][W],
 * overwritten, or NULL to skip the input gradient.  workspace: device memory of at least
 * lerf_imdn_bwd_workspace_bytes(nf, in_nc, out_nc, B, H, W) bytes, contents arbitrary, used by this call only (gradient
 * planes, and per-workgroup weight-gradient slabs that a second pass sums in slab order).
 * A short saved or workspace, a null pointer (grad_x excepted) or a bad shape or post is LERF_EINVAL, and nothing is
 * written.  Float32 products and sums on the matrix cores (v_mfma_f32_16x16x4_f32), no float atomics: repeated calls give
 * bitwise-identical gradients, and grad_x of image b equals that of image b run alone.  Launches on `stream`, no sync,
 * no allocation, no global state. */
size_t lerf_imdn_saved_bytes(int nf, int in_nc, int out_nc, int B, int H, int W);
int lerf_imdn_fwd_train_f32(const float* weights, int nf, int in_nc, int out_nc, const float* x, int B, int H, int W, int post,
                            void* saved, size_t saved_bytes, float* out, void* stream);
size_t lerf_imdn_bwd_workspace_bytes(int nf, int in_nc, int out_nc, int B, int H, int W);
int lerf_imdn_bwd_f32(const float* weights, int nf, int in_nc, int out_nc, const float* x, int B, int H, int W, int post,
                      const void* saved, size_t saved_bytes, const float* grad_out, float* grad_weights, float* grad_x,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- resize_right.resize (resize_right/resize_right.py:36-127): one axis pass of the separable, anti-aliased, any-scale
 * resize, and its adjoint.  The tensor is viewed as [outer][n][inner], contiguous:
 *     out[o][j][i] = sum_k w[j][k] * in[o][src(left[j] + k)][i],   j < n_out, k < taps
 * src() is the image pad rule `pad_mode` (LERF_PAD_*; a tap in a constant pad contributes w * 0), left[j] the first source
 * index of output j in unpadded coordinates (get_field_of_view :145-154, may be negative), w the weights normalised per output
 * (get_weights :208-218); both tables are built by the caller (O(n_out * taps)) and live on the device.  taps is not bounded
 * by LERF_MAX_SUPPORT.  left needs no particular order: it may decrease, repeat or jump, and every tap still follows the
 * pad rule.  Products and sums are rounded separately and added in tap order, in the accumulator type.
 * taps == 0 selects the CSR form, used for the adjoint: row j sums w[e] * in[o][idx[e]][i] over e in
 * [row_ptr[j], row_ptr[j + 1]), every idx in [0, n_in); build it with lerf_rr_adjoint_csr and run it with n_in / n_out
 * exchanged: it then maps the output gradient [outer][n_out][inner] to the input gradient [outer][n_in][inner], without
 * atomics and in a fixed order. */
typedef struct {
    int n_in, n_out;
    int taps;                 /* > 0: forward form (left, w[n_out][taps]); 0: CSR form (row_ptr, idx, w[nnz]) */
    const int32_t* left;      /* device [n_out] */
    const int32_t* row_ptr;   /* device [n_out + 1] */
    const int32_t* idx;       /* device [nnz] */
    const void* w;            /* device, element type = acc_dtype */
    int pad_mode;             /* forward form only */
} lerf_rr_axis_t;

/* in: LERF_U8 / LERF_F32 / LERF_F64; acc_dtype: LERF_F32 / LERF_F64 (the type of w, of the products and of the sum);
 * out_dtype: acc_dtype, or LERF_U8 with a float64 accumulator: round-half-to-even of the sum clipped to [0, 255]
 * (np.round(np.clip(x, 0, 255)).astype(np.uint8)).  Other combinations: LERF_EUNSUPPORTED.  in and out must not overlap.
 * Launches on `stream`, no sync. */
int lerf_rr_axis(const void* in, int in_dtype, int64_t outer, int64_t inner, const lerf_rr_axis_t* axis, int acc_dtype,
                 void* out, int out_dtype, void* stream);

/* Host: the adjoint table of a forward axis (HOST pointers).  For every source index s < n_in the outputs that read it:
 * row_ptr[n_in + 1], idx[nnz] = j, wt[nnz] = w[j][k], in (j, k) order per source; padded taps of the non-constant pad
 * modes fold onto the source index the pad rule names, taps in a constant pad are dropped.  w / wt: w_dtype = LERF_F32 or
 * LERF_F64; idx and wt must hold n_out * taps entries.  Returns nnz >= 0, or a negative LERF_E* code. */
int lerf_rr_adjoint_csr(int n_in, int n_out, int taps, const int32_t* left, const void* w, int w_dtype, int pad_mode,
                        int32_t* row_ptr, int32_t* idx, void* wt);

/* ---- the training batch of the DIV2K provider (resample/data.py:107-165).  The decoded train images live once in a device
 * pool of uint8 HWC RGB images; a sample is a descriptor, and one launch fills the whole batch:
 *     im [B][C][sz][sz], lb [B][C][hsz][hsz] float32, dense
 * Output (b, c) is, in the reference's order: crop rows [i, i + n), columns [j, j + n) of the image (n = sz at (li, lj) of
 * the LR image, hsz at (hi, hj) of the HR image); channel `chan` for C == 1, channel c for C == 3; np.fliplr if `fliplr`;
 * np.flipud if `flipud`; np.rot90(., k); float32(u8) / 255.0f as an IEEE division.  `noise` (device float32 [B][C][sz][sz], or
 * NULL) is added to im after the division, in float32 (:163).
 * Descriptors are read by the kernel from DEVICE memory (`desc`, B entries).  `desc_host` is the same array in host memory,
 * or NULL: when given, every entry is checked before the launch and a crop that leaves its image, an image that leaves the
 * pool (off < 0, off + h * pitch > pool_bytes, pitch < 3 * w), chan outside 0..2 (C == 1) or k outside 0..3 is LERF_EINVAL
 * with nothing launched.  The kernel repeats the same check per sample and never reads outside [off, off + h * pitch): a
 * sample whose descriptor fails it gets im and lb filled with zeros.  Null pool / desc / im / lb, pool_bytes <= 0, B <= 0,
 * C not 1 or 3, sz <= 0 or hsz <= 0: LERF_EINVAL.  One launch on `stream`, no sync, no allocation. */
typedef struct {
    int64_t lr_off, hr_off;          /* byte offset of the image's first pixel in the pool */
    int32_t lr_h, lr_w, lr_pitch;    /* rows, columns, bytes between rows (>= 3 * w) */
    int32_t hr_h, hr_w, hr_pitch;
    int32_t li, lj, hi, hj;          /* crop origins (row, column) */
    int32_t chan;                    /* 0..2 for C == 1, ignored for C == 3 */
    int32_t fliplr, flipud;          /* 0 / 1 */
    int32_t k;                       /* np.rot90 quarter turns, 0..3 */
} lerf_patch_desc_t;

int lerf_patch_batch_u8(const uint8_t* pool, int64_t pool_bytes, const lerf_patch_desc_t* desc, const lerf_patch_desc_t* desc_host,
                        int B, int C, int sz, int hsz, const float* noise, float* im, float* lb, void* stream);

/* ---- calibration (bench.py roofline_lds): `workgroups` x 1024 threads, each wave issuing 10 x `iters` ds_read_b32 gathers
 * into a 134-KB LDS table -- pattern 0: random addresses (the rate a data-dependent LUT gather gets), pattern 1:
 * conflict-free.  The caller times the launch (one workgroup per CU: wave-gathers per CU = 160 x iters) and owns `sink`
 * (4 bytes of device memory, practically never written).  Not part of the reference's path: a ruler for it. */
int lerf_ubench_lds_gather(int pattern, int iters, int workgroups, uint32_t* sink, void* stream);

/* Backward of lerf_remap on planar float32 maps: lerf_warp_bwd with the point of every output pixel read from the coordinate map
 * (the same operands, kinds, supports, pad modes, formulas, NaN rule and float-atomic accumulation; see there), plus the gradient
 * with respect to the MAP, which a homography has no tensor for.
 * grad_coords: float64 [N][out_h][out_w][2], dense, 16-byte aligned, PER PLANE -- d loss / d (row, col) of entry (i, j) through
 * plane n; the caller sums over the planes that share the map.  The point enters through the distances alone; the tap set, the
 * pads and the amplified-linear classes are piecewise constant, so this is the gradient autograd gives with them held fixed, with
 * torch.clamp's backward for the clip to [0, H] x [0, W] (it passes at the borders, is 0 outside and for +-inf).  Float64
 * throughout; every element has one writer (a plain load-add-store: ACCUMULATED into like the other gradients, no atomics,
 * bit-equal from run to run).  Identically 0 for LERF_KIND_NEAREST.
 * A NaN entry is masked: the pixel contributes to no gradient and adds nothing to its own.  Any gradient pointer may be NULL and
 * is then skipped.  geo: as lerf_remap takes it (row_stride and explicit low pads included, so a row tile of a larger map works:
 * grad_out and grad_coords are then the tile's rows).  Refuses what lerf_warp_bwd and lerf_remap refuse. */
int lerf_remap_bwd(const float* feat, const float* h0, const float* h1, const float* h2, int N, int H, int W,
                   const lerf_remap_geo_t* geo, int kind, double max_sigma, const double* grad_out,
                   float* grad_feat, float* grad_h0, float* grad_h1, float* grad_h2, double* grad_coords, void* stream);
/* lerf_remap_bwd with one map per sample (see lerf_remap_batched): N == n_maps * planes_per_map planes, plane n reads map
 * n / planes_per_map.  grad_coords stays PER PLANE, float64 [N][out_h][out_w][2], one writer per element: the sum over a sample's
 * planes is the caller's.  Refuses what lerf_remap_bwd and lerf_remap_batched refuse. */
int lerf_remap_bwd_batched(const float* feat, const float* h0, const float* h1, const float* h2, int N, int H, int W,
                           const lerf_remap_geo_t* geo, int n_maps, int64_t map_stride, int planes_per_map, int kind,
                           double max_sigma, const double* grad_out, float* grad_feat, float* grad_h0, float* grad_h1,
                           float* grad_h2, double* grad_coords, void* stream);

/* ---- Coordinate maps on the device (csrc/lerf_coords.hip, arithmetic: csrc/lerf_coords_models.h).  A map is what
 * lerf_remap_geo_t.coords reads: [oH][row_stride] elements, (row, col) pairs, entry (i, j) at out + i * row_stride + 2 * j,
 * LERF_F64 or LERF_F32, row_stride even and >= 2 * oW, the base aligned to one entry (16 / 8 bytes).  Values are UNCLIPPED source
 * positions; the remap clips.  Everything is computed in float64 with + - * / only and no FMA contraction, so each device entry
 * point and its *_host twin (the same statements in a plain loop over HOST pointers; no GPU needed) agree bit for bit; a
 * float32 map is the float64 value rounded once at the store.  Device entry points: one launch on `stream` (two for
 * lerf_coords_mesh_bwd and lerf_coords_build_bwd), no sync, no allocation, no global state.  Refused (LERF_EINVAL, nothing is
 * launched or written): a null pointer, oH or oW < 1, gh or gw < 2, an odd or short row stride, a misaligned base pointer, an
 * unknown model, dtype or interp, a parameter count that is not the model's, a non-finite model parameter (where the parameters
 * are HOST memory: lerf_coords_build, lerf_coords_build_host), a negative origin or a tile outside the whole map, a short
 * workspace.  Operands must not overlap the output. */
enum { LERF_COORDS_HOMOGRAPHY = 0, LERF_COORDS_RADIAL = 1, LERF_COORDS_BROWN = 2, LERF_COORDS_FISHEYE = 16, LERF_COORDS_EQUIRECT = 17 };
enum { LERF_MESH_BILINEAR = 0, LERF_MESH_BICUBIC = 1 };
#define LERF_COORDS_MAX_PARAMS 21

/* Entry (i, j) of the tile = the model's point of output pixel (i0 + i, j0 + j): a tile of a larger map built in place (out = the
 * tile's first entry, row_stride the whole map's) equals those entries of the whole map bit for bit.  params: HOST doubles,
 *   LERF_COORDS_HOMOGRAPHY  9: the INVERSE matrix, row-major; the warp kernels' projection without its clip (lerf_remap on this
 *                              map = lerf_warp of the matrix, bit for bit)
 *   LERF_COORDS_RADIAL      8: cr, cc, no, ni, hr, hc, k1, k2 -- centre (row, col) in the source, half-diagonals of the output
 *                              and of the source, half-extents (oH - 1) / 2, (oW - 1) / 2 of the WHOLE output, coefficients:
 *                              ur = (i - hr) / no, uc = (j - hc) / no, r2 = ur ur + uc uc, f = 1 + k1 r2 + (k2 r2) r2,
 *                              row = cr + (ur f) ni, col = cc + (uc f) ni
 *   LERF_COORDS_BROWN      21: m[9] = inv(new_K . R) row-major, fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 -- the pinhole +
 *                              Brown-Conrady model of cv::initUndistortRectifyMap without skew: (x, y) = m (j, i, 1) divided
 *                              through, r2 = x x + y y, rad = (1 + r2 (k1 + r2 (k2 + r2 k3))) / (1 + r2 (k4 + r2 (k5 + r2 k6))),
 *                              x'' = x rad + 2 p1 x y + p2 (r2 + 2 x x), y'' = y rad + p1 (r2 + 2 y y) + 2 p2 x y,
 *                              col = fx x'' + cx, row = fy y'' + cy
 *   LERF_COORDS_FISHEYE    17: m[9] = inv(new_K . R), fx, fy, cx, cy, k1, k2, k3, k4 -- cv::fisheye::initUndistortRectifyMap's
 *                              equidistant model without skew: (x, y) = m (j, i, 1) divided through by Wh; Wh <= 0 (a ray behind the
 *                              camera): (NaN, NaN); r = sqrt(x x + y y), th = atan(r), th_d = th (1 + k1 th^2 + k2 th^4 + k3 th^6 +
 *                              k4 th^8), s = th_d / r (1 at r = 0), col = fx x s + cx, row = fy y s + cy
 *   LERF_COORDS_EQUIRECT   13: m[9] = inv(K_view . R), sx, sy, cxp, cyp -- a pinhole view of an equirectangular panorama:
 *                              d = m (j, i, 1), lon = atan2(d.x, d.z), lat = atan2(d.y, sqrt(d.x d.x + d.z d.z)),
 *                              col = cxp + sx lon, row = cyp + sy lat; for a panorama [Hp][Wp]: sx = Wp / (2 pi), sy = Hp / pi,
 *                              cxp = (Wp - 1) / 2, cyp = (Hp - 1) / 2.  The seam lon = +-pi is clipped like any border.
 * Codes 3 .. 15 are not models.  The models from 16 on take their square root and arc tangents from sqrt_pm / atan_pm / atan2_pm
 * of csrc/lerf_coords_models.h (float64 + - * /, selects and bit-casts; within 1 ulp (sqrt, atan) and 2 ulp (atan2) of the exact
 * value, NOT equal to a math library's), so they too agree bit for bit between a device entry point and its host twin.
 * (the rounding order of every statement: the top of csrc/lerf_coords_models.h). */
int lerf_coords_build(int model, const double* params, int n_params, void* out, int out_dtype, int64_t row_stride,
                      int oH, int oW, int i0, int j0, void* stream);
int lerf_coords_build_host(int model, const double* params, int n_params, void* out, int out_dtype, int64_t row_stride,
                           int oH, int oW, int i0, int j0);

/* Mesh upsample: ctrl [gh][gw][2] (LERF_F32 / LERF_F64, dense, entry-aligned) holds absolute source positions at control
 * vertices placed align-corners over the WHOLE output [full_h][full_w] (vertex a at output row a (full_h - 1) / (gh - 1)); the
 * tile [oH][oW] at origin (i0, j0) of it is written (i0 + oH <= full_h, j0 + oW <= full_w).  interp: LERF_MESH_BILINEAR, or
 * LERF_MESH_BICUBIC = Keys A = -0.75 with border taps clamped, torch's upsample_bicubic2d(align_corners=True) forms. */
int lerf_coords_mesh(const void* ctrl, int ctrl_dtype, int gh, int gw, int interp, int full_h, int full_w,
                     void* out, int out_dtype, int64_t row_stride, int oH, int oW, int i0, int j0, void* stream);
int lerf_coords_mesh_host(const void* ctrl, int ctrl_dtype, int gh, int gw, int interp, int full_h, int full_w,
                          void* out, int out_dtype, int64_t row_stride, int oH, int oW, int i0, int j0);

/* Adjoint of lerf_coords_mesh over a whole map (the exact transpose of its weights, clamped bicubic taps included):
 * grad_map float64 [oH][oW][2] dense, 16-byte aligned (what lerf_remap_bwd's grad_coords holds after the sum over planes);
 * grad_ctrl float64 [gh][gw][2] dense, 16-byte aligned, ACCUMULATED into (plain load-add-store, one writer per vertex).
 * Gather-shaped in two separable passes -- rows into the workspace ([gh][oW][2] doubles), then columns -- each sum in a fixed
 * order, no atomics: two runs are bit-equal.  workspace: device, >= lerf_coords_mesh_bwd_workspace_bytes(gh, gw, oH, oW) bytes
 * (0 from the query for refused sizes), 16-byte aligned, contents arbitrary, used by this call's two launches only. */
size_t lerf_coords_mesh_bwd_workspace_bytes(int gh, int gw, int oH, int oW);
int lerf_coords_mesh_bwd(const double* grad_map, int oH, int oW, int interp, int gh, int gw, double* grad_ctrl,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Composition C[i][j] = A(B[i][j]): the outer map a [aH][aW][2] sampled bilinearly at the position the inner map b [oH][oW][2]
 * holds, so that remapping by b the result of remapping by a describes the geometry of ONE remap by C.  Each of a, b, out obeys
 * the strided map contract with its own dtype.  Per axis the position is clipped onto [0, aH - 1] (-inf -> 0, +inf -> aH - 1),
 * i0 = min(floor(r), aH - 2) (0 when aH == 1), t = r - i0.  A NaN in either coordinate of b gives (NaN, NaN) and reads nothing
 * of a; a tap whose weight is exactly 0 is not read (a NaN in a reaches C only through a tap that counts); no value of b can
 * form an address outside a. */
int lerf_coords_compose(const void* a, int a_dtype, int64_t a_row_stride, int aH, int aW,
                        const void* b, int b_dtype, int64_t b_row_stride,
                        void* out, int out_dtype, int64_t out_row_stride, int oH, int oW, void* stream);
int lerf_coords_compose_host(const void* a, int a_dtype, int64_t a_row_stride, int aH, int aW,
                             const void* b, int b_dtype, int64_t b_row_stride,
                             void* out, int out_dtype, int64_t out_row_stride, int oH, int oW);

/* Inverse of a map: entry (i, j) of out [oH][oW][2] is the position u with F(u) = (i0 + i, j0 + j), where F(u) is the bilinear
 * interpolant of the map f [fH][fW][2] (fH, fW >= 2) under lerf_coords_compose's per-axis rule (the position clipped onto
 * [0, fH - 1], i = min(floor(r), fH - 2), t = r - i) -- so lerf_coords_compose(f, out) holds (i0 + i, j0 + j) within tol at every
 * entry of out that is not NaN.  out is shaped like the frame f points INTO; a tile of a larger inverse written in place (out =
 * the tile's first entry, the whole map's row stride, its origin) equals those entries of the whole inverse bit for bit.  Each
 * of f, init, out obeys the strided map contract with its own dtype; a float32 map is promoted exactly on load, the float64
 * result is rounded once at the store.
 * Newton's method per entry, at most max_iter passes (each reads ALL FOUR corners of the cell that holds the clipped iterate and
 * evaluates e = F(u) - target): max(|e.r|, |e.c|) <= tol ends it with the clipped iterate as the result; else the step solves
 * the patch's 2 x 2 Jacobian by Cramer's rule.  The start is entry (i, j) of init ([oH][oW][2], e.g. a model's analytic inverse or
 * the previous frame's inverse), or, with init NULL (init_dtype and init_row_stride are then ignored), the affine guess through
 * f[0][0], f[fH - 1][0] and f[0][fW - 1] (the middle of f when those three are degenerate), which does not depend on the tile.
 * (NaN, NaN) is written for: a NaN start, a NaN among the four corners read, a Jacobian determinant that is 0 or not finite (a
 * fold or a constant stretch of f), and an entry that has not met tol after max_iter passes -- the targets f does not reach.
 * lerf_remap treats such an entry as "no source" (mask false, output 0 / NaN).  No value of f, init or the target forms an
 * address outside f: the iterate is clipped in floating point before any conversion to int, +-inf in init is clipped like any
 * iterate.  One thread per entry, one store per entry, no atomics, no allocation; the rounding order of every statement: the
 * top of csrc/lerf_coords_models.h.  Refused in addition to the family's list: fH or fW < 2, max_iter outside 1..64, a tol that
 * is negative or not finite, a negative i0 / j0, a non-null init that violates the map contract, out's bytes (first entry to
 * last) intersecting f's or init's. */
int lerf_coords_invert(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW,
                       const void* init, int init_dtype, int64_t init_row_stride,
                       void* out, int out_dtype, int64_t out_row_stride, int oH, int oW, int i0, int j0,
                       int max_iter, double tol, void* stream);
int lerf_coords_invert_host(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW,
                            const void* init, int init_dtype, int64_t init_row_stride,
                            void* out, int out_dtype, int64_t out_row_stride, int oH, int oW, int i0, int j0,
                            int max_iter, double tol);

/* Rasterising inverse with a depth test, for maps that fold or tear: entry (i, j) of out [oH][oW][2] is the position
 * u with T(u) = (i0 + i, j0 + j), T the PIECEWISE-LINEAR interpolant of the map f [fH][fW][2] (fH, fW >= 2) over two triangles a
 * cell -- cell (i, j) gives triangle t = 2 (i (fW - 1) + j) with vertices A = (i, j), B = (i, j + 1), C = (i + 1, j) and triangle
 * t + 1 with A = (i + 1, j + 1), B = (i + 1, j), C = (i, j + 1) -- not lerf_coords_invert's bilinear patch; lerf_coords_invert with
 * init = out polishes to that one.  Every triangle is rasterised into the tile; where several cover a pixel the smallest key
 * (sortable(z) << 32) | t wins: z is the triangle's depth there (depth [fH][fW] float32 dense at the vertices, interpolated in
 * float64 and rounded once; NULL: z = 0 everywhere), sortable() the order-preserving map of float32 bits to uint32 (a NaN z sorts
 * last), so the NEAREST surface wins and ties go to the lowest triangle.  A pixel no triangle covers gets (NaN, NaN), which
 * lerf_remap treats as "no source".
 * A triangle is skipped -- it contributes nothing and forms no address -- when one of its six coordinates is not finite or one of
 * its three depths is NaN; when area2 = (B - A) x (C - A) is 0 or not finite; when orient = +1 and area2 < 0 or orient = -1 and
 * area2 > 0 (back-face culling: +1 keeps the identity's orientation, 0 keeps both); or when its box of integer pixels, ceil(min)
 * .. floor(max) per axis BEFORE the clip to the tile, holds more than max_span (1..64) pixels on either axis (the tear rule: a
 * cell stretched across a disocclusion does not fill it).  The box is clipped onto the tile in floating point before any
 * conversion to int: no value of f forms an address or overflows an int.  The inside test is closed and watertight: each edge
 * function is evaluated with its endpoints in ascending index i fW + j and negated for the triangle that runs the other way, so
 * the two triangles on an edge see one number; a pixel on a shared edge or vertex belongs to every triangle around it and the
 * key decides.  The statement order: the top of csrc/lerf_coords_models.h.
 * keys [oH][oW] uint64, 8-byte aligned, caller-owned (the library allocates nothing), contents arbitrary: workspace AND result.
 * On return entry (i, j) holds the winning key -- low 32 bits the triangle, high 32 sortable(z) -- or all ones for a hole.  Three
 * launches on the stream (fill keys; one thread per cell of f, one 64-bit integer atomic min per covered pixel; one thread per
 * entry resolves its key and is the entry's one writer), no sync.  A minimum over integers does not depend on the order: out and
 * keys are bit-equal from run to run and to the host twin, a row-major loop over the cells.  f and out obey the strided map
 * contract with their own dtypes; a tile of a larger inverse written in place (out = the tile's first entry, the whole map's row
 * stride, its origin; keys dense for the tile) equals those entries of the whole.
 * Refused in addition to the family's list: fH or fW < 2, 2 (fH - 1) (fW - 1) >= 2^32 or more than 262140 rows of cells,
 * max_span outside 1..64, orient outside -1..1, a null or misaligned keys, a misaligned depth, a negative i0 / j0, out's or keys'
 * bytes intersecting f's, depth's or each other.  A refused call writes nothing. */
int lerf_coords_invert_raster(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW,
                              const float* depth,
                              void* out, int out_dtype, int64_t out_row_stride, int oH, int oW, int i0, int j0,
                              int max_span, int orient, uint64_t* keys, void* stream);
int lerf_coords_invert_raster_host(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW,
                                   const float* depth,
                                   void* out, int out_dtype, int64_t out_row_stride, int oH, int oW, int i0, int j0,
                                   int max_span, int orient, uint64_t* keys);

/* Adjoints of lerf_coords_compose and lerf_coords_invert (the rounding order of every statement: the top of
 * csrc/lerf_coords_models.h).  a, b, f, g obey the strided map contract, LERF_F32 / LERF_F64 in any mix, promoted exactly on
 * load; aH, aW, fH, fW >= 2, so the four corners of a cell are inside the map.  grad_out [oH][oW][2], grad_a [aH][aW][2], grad_b
 * [oH][oW][2] and grad_f [fH][fW][2] are dense float64, 16-byte aligned, and the gradients are ACCUMULATED into (the contract of
 * lerf_remap_bwd's grad_coords and of lerf_coords_mesh_bwd: the caller zeroes them).
 *
 * Compose, one entry with inner point (row, col) = b[i][j] and upstream g = grad_out[i][j]: a NaN in row or col contributes
 * nothing, whatever g holds -- nothing of a is read, nothing is scattered, grad_b gains (0, 0).  Else, with the forward's cell
 * and weights (lerf_coords_compose's per-axis rule),
 *   grad_a[i0 + p][j0 + q] += (wr[p] wc[q]) g  for the taps with wr[p] != 0 and wc[q] != 0 (the forward's rule: a tap of weight
 *                             exactly 0 gets nothing and forms no address; a position clipped onto the border still scatters to
 *                             the border taps the forward read);
 *   grad_b[i][j] += (pass_r ? Jr . g : 0, pass_c ? Jc . g : 0), Jr = dC/drow and Jc = dC/dcol of the bilinear patch formed from
 *                             ALL FOUR corners of the cell, whatever their weights (lerf_coords_invert's Jacobian statements), and
 *                             pass_r = (0 <= row <= aH - 1), pass_c alike: torch.clamp's backward, a select -- the border passes,
 *                             outside and +-inf are blocked even when the sum behind is NaN.  This is the derivative of the
 *                             plain bilinear formula with the cell held constant: at an integer position it is that of cell
 *                             min(floor(r), n - 2), and a NaN corner gives a NaN entry of grad_b.
 * grad_a or grad_b may be NULL to skip that half (no atomics / no loads of a); both NULL is refused.
 *
 * Invert, one entry (r, c) = g[i][j] of the inverse (what lerf_coords_invert wrote for f) with upstream grad_out[i][j]: by the
 * implicit function theorem on F(G[q]) = q, grad_f gains the same bilinear scatter, at the cell of (r, c), of v = -J^-T g (J the
 * Jacobian above, solved by Cramer's rule).  A NaN in (r, c), a NaN among the four corners read, or a determinant that is 0 or
 * not finite contributes nothing.  init, max_iter and tol have no gradient.
 *
 * How the sums are formed: grad_b has ONE writer per entry, a plain 16-byte load-add-store -- bit-equal from run to run and to
 * the host twin.  grad_a and grad_f are data-dependent scatters: float64 atomic adds to global memory, so they are equal from run
 * to run (and to the host twin's row-major order) up to the rounding of a reordered float64 sum, not bit for bit -- like the image
 * and hyper gradients of lerf_remap_bwd.  The gradient buffers are ordinary (coarse-grained) device memory.  One launch, one
 * thread per entry, no sync, no allocation, no workspace, no global state.  Refused in addition to the family's list: aH, aW, fH
 * or fW < 2; grad_a and grad_b both NULL; a gradient buffer whose bytes intersect an operand's, grad_out's or the other gradient
 * buffer's. */
int lerf_coords_compose_bwd(const void* a, int a_dtype, int64_t a_row_stride, int aH, int aW,
                            const void* b, int b_dtype, int64_t b_row_stride,
                            const double* grad_out, int oH, int oW, double* grad_a, double* grad_b, void* stream);
int lerf_coords_compose_bwd_host(const void* a, int a_dtype, int64_t a_row_stride, int aH, int aW,
                                 const void* b, int b_dtype, int64_t b_row_stride,
                                 const double* grad_out, int oH, int oW, double* grad_a, double* grad_b);
int lerf_coords_invert_bwd(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW,
                           const void* g, int g_dtype, int64_t g_row_stride,
                           const double* grad_out, int oH, int oW, double* grad_f, void* stream);
int lerf_coords_invert_bwd_host(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW,
                                const void* g, int g_dtype, int64_t g_row_stride,
                                const double* grad_out, int oH, int oW, double* grad_f);

/* The model builders with their parameters in DEVICE memory, and their adjoint (the rounding order of every statement
 * and the ORDER OF THE SUMS: the top of csrc/lerf_coords_models.h).
 *
 * lerf_coords_build_dev is lerf_coords_build with two changes: params_dev is DEVICE memory, float64 [n_sets][n_params], dense, and
 * n_sets >= 1 maps are written in one launch, map s at out + s * set_stride ELEMENTS (each map under the strided contract with
 * row_stride; set_stride even and, for n_sets > 1, >= (oH - 1) * row_stride + 2 * oW).  Map s is bit-equal to lerf_coords_build
 * of the same 9 / 8 / 21 / 17 / 13 doubles; lerf_coords_build_host per set is the host twin.  No host round trip, no sync: the parameters
 * are not visible to the host, so NON-FINITE PARAMETERS ARE NOT REFUSED here (they give non-finite entries, which the remap
 * treats as it treats any map's).  Everything else on the family's list is refused, and n_sets outside 1 .. 65535, a misaligned
 * params_dev, params_dev's bytes intersecting the maps'.
 *
 * lerf_coords_build_bwd: grad_params[s][k] += sum over the entries (i, j) of map s of
 * d row / d p[k] * grad_map[s][i][j][0] + d col / d p[k] * grad_map[s][i][j][1], for EVERY entry of the parameter vector (radial's
 * geometry scalars included), by the hand-written reverse mode model_point_bwd.  grad_map: float64 [n_sets][oH][oW][2], dense,
 * 16-byte aligned (what lerf_remap_bwd_batched's grad_coords holds after the sum over a sample's planes); (i0, j0): the tile's
 * origin in the whole map, as in the forward.  grad_params: float64 [n_sets][n_params], ACCUMULATED into by a plain load-add-store
 * with one writer per value (the contract of lerf_remap_bwd and lerf_coords_mesh_bwd: the caller zeroes it).
 * An entry whose forward point is not finite in either coordinate (Wh == 0 and the like) contributes EXACTLY NOTHING, whatever
 * grad_map holds there -- a select, unlike autograd, which would return NaN; a NaN in grad_map at a finite point propagates.
 * Two passes, no atomics: every lane of pass 1 keeps n_params running sums over the entries it owns, a block (64 columns x a band
 * of 64 rows) combines them in a fixed order into ONE partial vector in the workspace; pass 2 sums the partials per (set, k) in
 * a fixed order.  The order is a function of (oH, oW, n_sets) only -- not of the CU count, the resident grid or timing -- so two
 * runs are bit-equal, and lerf_coords_build_bwd_host (host pointers, the same order) equals the device bit for bit.
 * workspace: device, >= lerf_coords_build_bwd_workspace_bytes(n_params, n_sets, oH, oW) bytes (n_sets * n_params *
 * ceil(oW / 64) * ceil(oH / 64) doubles; 0 from the query for refused sizes), 16-byte aligned, contents arbitrary, used by this
 * call's two launches only.  Two launches on `stream`, no sync, no allocation, no global state.  Refused in addition to the
 * family's list: n_sets outside 1 .. 65535, a short or misaligned workspace, grad_params' bytes intersecting params', grad_map's
 * or the workspace's. */
int lerf_coords_build_dev(int model, const double* params_dev, int n_sets, int n_params, void* out, int out_dtype,
                          int64_t set_stride, int64_t row_stride, int oH, int oW, int i0, int j0, void* stream);
size_t lerf_coords_build_bwd_workspace_bytes(int n_params, int n_sets, int oH, int oW);
int lerf_coords_build_bwd(int model, const double* params_dev, int n_sets, int n_params, const double* grad_map,
                          int oH, int oW, int i0, int j0, double* grad_params,
                          void* workspace, size_t workspace_bytes, void* stream);
int lerf_coords_build_bwd_host(int model, const double* params, int n_sets, int n_params, const double* grad_map,
                               int oH, int oW, int i0, int j0, double* grad_params);

/* The helpers of the fisheye and equirect models on their own, for tests: out[e] = sqrt_pm(x[e]) / atan_pm(x[e]) / atan2_pm(x[e], y[e])
 * for e < n, float64, dense.  y is ignored (and may be null) for the unary ops; out may be x or y.  lerf_coords_math takes DEVICE
 * pointers and runs one thread per element (one launch on `stream`, no sync); lerf_coords_math_host is its host twin, bit-equal.
 * Refused with LERF_EINVAL before anything is written: a null x or out, a null y for LERF_MATH_ATAN2, n < 0 or n > 2^31 - 1, an
 * unknown op.  n == 0 is a no-op. */
enum { LERF_MATH_SQRT = 0, LERF_MATH_ATAN = 1, LERF_MATH_ATAN2 = 2 };
int lerf_coords_math(int op, const double* x, const double* y, int64_t n, double* out, void* stream);
int lerf_coords_math_host(int op, const double* x, const double* y, int64_t n, double* out);

/* Reproject by depth (the rounding order of every statement and the order of the sums: the top of
 * csrc/lerf_coords_models.h): the map that carries view A, with a depth per pixel, into view B.  Entry (i, j) of set s is the
 * position (row, col) in view B of pixel (i0 + i, j0 + j) of view A, and depth_out its depth there:
 *     a = M (x, y, 1),  x = j0 + j, y = i0 + i
 *     LERF_DEPTH_Z       (depth = z):      (X, Y, W) = a z + q,    zo = W
 *     LERF_DEPTH_INVERSE (depth = d = 1/z): (X, Y, W) = a + q d,   zo = W / d   (d == 0, a point at infinity: a finite entry, zo = +inf)
 *     col = X / W,  row = Y / W
 * with M = K_dst . R . inv(K_src) and q = K_dst . t for X_dst = R X_src + t; the last row of K_dst must be (0, 0, 1) for zo to be
 * the depth in view B.  An entry is VALID when z > 0 (d >= 0), the depth is finite and W > 0; any other entry is (NaN, NaN) with
 * zo = NaN, which the remap treats as "no source" and the rasterising inverse skips.
 * params_dev: float64 [n_sets][LERF_REPROJECT_PARAMS] = m[9] row-major then q[3], dense, DEVICE memory for lerf_coords_reproject
 * (non-finite parameters are not refused, as for lerf_coords_build_dev) and host memory for the host twins.  depth: one dense plane
 * [oH][oW] of depth_dtype (LERF_F32, promoted exactly, or LERF_F64) per set -- the TILE's own plane -- set s at depth + s *
 * depth_set_stride elements (>= oH * oW, or 0 = one plane shared by all sets).  out: n_sets maps under the strided contract, map s at
 * out + s * out_set_stride elements (even, >= (oH - 1) * out_row_stride + 2 * oW for n_sets > 1).  depth_out: float [oH][oW] per
 * set, dense, set s at depth_out + s * depth_out_set_stride (>= oH * oW for n_sets > 1) -- the layout lerf_coords_invert_raster's
 * depth reads -- or NULL.  A float32 map or zo is the float64 value rounded once at the store.  One launch, one thread per entry, one
 * map store per entry and one zo store when depth_out is given; no atomics, no allocation, no sync.  The host twin is bit-equal.
 *
 * lerf_coords_reproject_bwd ACCUMULATES the adjoint: grad_map float64 [n_sets][oH][oW][2] dense (required), grad_depth_out float64
 * [n_sets][oH][oW] dense, the upstream of zo (NULL: none); grad_depth float64 [n_sets][oH][oW] gains d loss / d depth of every
 * entry by a plain load-add-store with one writer per entry (a shared depth plane still has one gradient plane per set);
 * grad_params float64 [n_sets][12] gains the sums over the entries of set s.  Either may be NULL to skip that half; both NULL is
 * refused.  An entry that is not valid contributes EXACTLY NOTHING to either, whatever the upstreams hold (lerf_coords_build_bwd's
 * rule); a zo that is not finite takes nothing from grad_depth_out.  grad_params is summed by lerf_coords_build_bwd's two passes
 * in its order -- a function of (oH, oW, n_sets) only, no atomics -- so two runs are bit-equal and lerf_coords_reproject_bwd_host
 * equals the device bit for bit.  workspace: device, >= lerf_coords_reproject_bwd_workspace_bytes(n_sets, oH, oW) bytes (n_sets * 12 *
 * ceil(oW / 64) * ceil(oH / 64) doubles; 0 from the query for refused sizes), 16-byte aligned, needed when grad_params is given
 * (else ignored: NULL will do).  One launch (two with grad_params) on `stream`, no sync, no allocation.
 * Refused with LERF_EINVAL, launching and writing nothing: the family's list (a null required pointer, misalignment, an odd or
 * short row stride, a bad dtype, oH or oW < 1, a bad tile origin), an unknown kind, n_sets outside 1 .. 65535, a set stride that is
 * negative, odd (out) or short, a short or misaligned workspace, and the bytes of any output (out, depth_out, grad_depth,
 * grad_params, the workspace) intersecting an operand's or another output's. */
enum { LERF_DEPTH_Z = 0, LERF_DEPTH_INVERSE = 1 };
#define LERF_REPROJECT_PARAMS 12
int lerf_coords_reproject(int kind, const double* params_dev, int n_sets, const void* depth, int depth_dtype,
                          int64_t depth_set_stride, void* out, int out_dtype, int64_t out_set_stride, int64_t out_row_stride,
                          float* depth_out, int64_t depth_out_set_stride, int oH, int oW, int i0, int j0, void* stream);
int lerf_coords_reproject_host(int kind, const double* params, int n_sets, const void* depth, int depth_dtype,
                               int64_t depth_set_stride, void* out, int out_dtype, int64_t out_set_stride, int64_t out_row_stride,
                               float* depth_out, int64_t depth_out_set_stride, int oH, int oW, int i0, int j0);
size_t lerf_coords_reproject_bwd_workspace_bytes(int n_sets, int oH, int oW);
int lerf_coords_reproject_bwd(int kind, const double* params_dev, int n_sets, const void* depth, int depth_dtype,
                              int64_t depth_set_stride, const double* grad_map, const double* grad_depth_out, int oH, int oW,
                              int i0, int j0, double* grad_depth, double* grad_params,
                              void* workspace, size_t workspace_bytes, void* stream);
int lerf_coords_reproject_bwd_host(int kind, const double* params, int n_sets, const void* depth, int depth_dtype,
                                   int64_t depth_set_stride, const double* grad_map, const double* grad_depth_out, int oH, int oW,
                                   int i0, int j0, double* grad_depth, double* grad_params);

/* The chained operations on a BATCH of n_sets maps in one launch: each entry point below is its single-map form with
 * n_sets and one SET STRIDE per operand appended; set s reads and writes operand base + s * set_stride ELEMENTS (of the operand's own
 * dtype: a map's floats or doubles, a float64 gradient's doubles, keys' uint64, depth's floats; the workspace of the mesh adjoint is
 * dense per set).  Every set has the shapes, dtypes, row strides and scalars of the single-map arguments, and set s of a batched call
 * is the single-map call on the same operands BIT FOR BIT (where the single-map form is bit-reproducible; the two atomic scatters
 * grad_a and grad_f stay equal up to the rounding of a reordered float64 sum).  The single-map entry points are the n_sets = 1 case
 * of the same kernels; with n_sets = 1 the set strides are not used (0 will do).
 * Set strides: non-negative; EVEN for maps and float64 gradients (pairs: every set's entries stay aligned like set 0's; keys and
 * depth hold scalars and take any stride); for n_sets > 1 at least the operand's extent, first element to one past the last --
 * (h - 1) * row_stride + 2 * w for a map, 2 * h * w for a gradient or a control mesh, h * w for keys and depth -- so sets do not
 * overlap, OR 0 = ONE operand shared by all sets, which is allowed for exactly these:
 *   read-only   a (the outer map of compose and of its adjoint), f, init, depth
 *   grad_a      the gradient of a shared outer map: every set scatters into the one buffer, which gains the SUM over the sets (device:
 *               the float64 atomic adds the scatter uses anyway; host twin: plain adds in set order, i.e. the single-map host twin
 *               called once per set on the same buffer, bit for bit).  grad_a_set_stride = 0 needs a_set_stride = 0.
 * Not shareable (0 refused for n_sets > 1): every single-writer output (out, grad_b, keys, grad_ctrl), the inner map b / the inverse g,
 * grad_out / grad_map, ctrl.  Where the single-map form refuses operands whose bytes intersect, the batched form refuses the same
 * pairs over the WHOLE batch: an operand's bytes run from its first element of set 0 to one past its last of set n_sets - 1.
 * lerf_coords_compose_batched with n_sets > 1 also refuses an out whose batch intersects a's, or b's unless it IS b (same base,
 * dtype, row and set stride: in place).  n_sets < 1: LERF_EINVAL; n_sets > 65535 (the grid's z limit): LERF_EUNSUPPORTED.  A
 * refused call launches and writes nothing; the device entry points refuse before they touch the device.
 * lerf_coords_invert_raster_batched: n_sets key planes (8 bytes per output pixel PER SET).  lerf_coords_mesh_bwd_batched: workspace
 * >= n_sets * lerf_coords_mesh_bwd_workspace_bytes(gh, gw, oH, oW) bytes, [n_sets][gh][oW][2] doubles. */
int lerf_coords_mesh_batched(const void* ctrl, int ctrl_dtype, int gh, int gw, int interp, int full_h, int full_w,
                             void* out, int out_dtype, int64_t row_stride, int oH, int oW, int i0, int j0,
                             int n_sets, int64_t ctrl_set_stride, int64_t out_set_stride, void* stream);
int lerf_coords_mesh_batched_host(const void* ctrl, int ctrl_dtype, int gh, int gw, int interp, int full_h, int full_w,
                                  void* out, int out_dtype, int64_t row_stride, int oH, int oW, int i0, int j0,
                                  int n_sets, int64_t ctrl_set_stride, int64_t out_set_stride);
int lerf_coords_mesh_bwd_batched(const double* grad_map, int oH, int oW, int interp, int gh, int gw, double* grad_ctrl,
                                 void* workspace, size_t workspace_bytes,
                                 int n_sets, int64_t grad_map_set_stride, int64_t grad_ctrl_set_stride, void* stream);
int lerf_coords_compose_batched(const void* a, int a_dtype, int64_t a_row_stride, int aH, int aW,
                                const void* b, int b_dtype, int64_t b_row_stride,
                                void* out, int out_dtype, int64_t out_row_stride, int oH, int oW,
                                int n_sets, int64_t a_set_stride, int64_t b_set_stride, int64_t out_set_stride, void* stream);
int lerf_coords_compose_batched_host(const void* a, int a_dtype, int64_t a_row_stride, int aH, int aW,
                                     const void* b, int b_dtype, int64_t b_row_stride,
                                     void* out, int out_dtype, int64_t out_row_stride, int oH, int oW,
                                     int n_sets, int64_t a_set_stride, int64_t b_set_stride, int64_t out_set_stride);
int lerf_coords_invert_batched(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW,
                               const void* init, int init_dtype, int64_t init_row_stride,
                               void* out, int out_dtype, int64_t out_row_stride, int oH, int oW, int i0, int j0,
                               int max_iter, double tol,
                               int n_sets, int64_t f_set_stride, int64_t init_set_stride, int64_t out_set_stride, void* stream);
int lerf_coords_invert_batched_host(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW,
                                    const void* init, int init_dtype, int64_t init_row_stride,
                                    void* out, int out_dtype, int64_t out_row_stride, int oH, int oW, int i0, int j0,
                                    int max_iter, double tol,
                                    int n_sets, int64_t f_set_stride, int64_t init_set_stride, int64_t out_set_stride);
int lerf_coords_invert_raster_batched(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW,
                                      const float* depth,
                                      void* out, int out_dtype, int64_t out_row_stride, int oH, int oW, int i0, int j0,
                                      int max_span, int orient, uint64_t* keys,
                                      int n_sets, int64_t f_set_stride, int64_t depth_set_stride, int64_t out_set_stride,
                                      int64_t keys_set_stride, void* stream);
int lerf_coords_invert_raster_batched_host(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW,
                                           const float* depth,
                                           void* out, int out_dtype, int64_t out_row_stride, int oH, int oW, int i0, int j0,
                                           int max_span, int orient, uint64_t* keys,
                                           int n_sets, int64_t f_set_stride, int64_t depth_set_stride, int64_t out_set_stride,
                                           int64_t keys_set_stride);
/* An indexed TRIANGLE MESH rasterised into a map: entry (i, j) of out [oH][oW][2] is the attribute -- the source
 * position -- the mesh holds at pixel (i0 + i, j0 + j) of the output frame, interpolated over the face that covers the pixel;
 * (NaN, NaN) where no face does, which lerf_remap treats as "no source".  The per-pixel arithmetic is lerf_coords_invert_raster's:
 * a closed, watertight inside test and a 64-bit key (sortable(z) << 32) | face under an integer minimum, so the nearest surface wins,
 * ties go to the lowest face, and out, keys and depth_out are bit-equal from run to run and to the host twin.
 *   pos        [V][2] (row, col) of pos_dtype (LERF_F32 promoted exactly / LERF_F64), dense, aligned to one entry: vertex positions in
 *              the output frame
 *   attr       [Va][2] (row, col) of attr_dtype, dense: what the map holds at a vertex
 *   faces      [F][3] int32, dense: indices into pos
 *   attr_faces [F][3] int32 indices into attr, or NULL = faces: welded positions may carry per-corner attributes (the OBJ v/vt model)
 *   depth      [V] float32 or NULL: per-vertex depth, interpolated affinely in the frame (float64, rounded once); NULL: z = +0
 *   w          [V] of w_dtype (LERF_F32 promoted exactly / LERF_F64) or NULL: per-vertex homogeneous w; attr is then interpolated perspective-correctly,
 *              u = (sum l_k a_k / w_k) / (sum l_k / w_k).  There is NO near-plane clipping: a face with a w that is not finite or <= 0 is skipped
 *   out        under the strided map contract, tile origin (i0, j0) >= 0 as in lerf_coords_invert_raster
 *   keys       [oH][oW] uint64, caller-owned, contents arbitrary: on return the winning key, low 32 bits the face, all ones = a hole
 *   depth_out  [oH][oW] float32 dense or NULL: the float of the winning key's high word (NaN in a hole); refused without depth
 *   max_span   0 = no tear rule, else 1..65536: a face whose box of integer pixels, before the clip, is wider than this on an axis is skipped
 *   orient     +1 / -1 keeps faces with area2 = (B - A) x (C - A) > 0 / < 0 only, 0 both
 *   workspace  device memory (the host twin: any memory; it is checked alike and not used), 4-byte aligned, at least
 *              lerf_coords_trimesh_workspace_bytes(F, n_sets) bytes: [n_sets][F + 1] uint32 counts and the partials of their scan
 * A face is skipped -- it contributes nothing and forms no address -- when one of its indices is outside [0, V) (attr_faces: [0, Va);
 * an unsigned compare before any vertex is read), a coordinate is not finite, a depth is NaN, a w is not finite or <= 0, area2 is 0 or
 * not finite (a repeated index), the cull, the tear rule, or a box that misses the tile.  Each edge function is evaluated with its
 * endpoints in ascending index of `faces`, so two faces that share an edge BY INDEX see one number with opposite signs; on the grid
 * triangulation (coords.grid_faces) the call returns lerf_coords_invert_raster's out and keys bit for bit.  The statement order: the
 * top of csrc/lerf_coords_models.h.
 * Device: fill keys; one thread per face counts the 4 x 16 pixel item tiles of its clipped box; an exclusive scan over all sets; a
 * fixed grid in which every wave draws one contiguous chunk of (face, tile) items, a pixel a lane, one 64-bit atomic min per
 * covered pixel; one thread per entry resolves its key.  Plain launches on the stream: no sync, no allocation, no read-back.
 * THE SIZE RULE, judged from the sizes before any pointer: n_sets * F * b <= 2^32 - 1 and n_sets * (F + 1) <= 2^32 - 1, b the most
 * item tiles one face can have = ceil(oH / 4) * ceil(oW / 16), or with max_span > 0 the fewer tiles a box max_span wide can touch,
 * else LERF_EUNSUPPORTED (2160 x 3840 with max_span = 0: about 33 000 faces; a finer mesh passes a max_span).
 * Batched: every operand takes a set stride in its own elements (pos / attr: floats or doubles, even; faces: int32;
 * depth / depth_out: floats; w: floats or doubles; keys: uint64); 0 shares a read-only operand (pos, attr, faces, attr_faces, depth, w) across the batch.
 * Refused with LERF_EINVAL, launching and writing nothing: the family's list, V, Va, F, oH or oW < 1, max_span outside 0..65536, orient
 * outside -1..1, depth_out without depth, a null, misaligned or short workspace, a negative i0 / j0, any of out, keys, depth_out and
 * the workspace intersecting an input or each other over the whole batch, an output shared between sets. */
size_t lerf_coords_trimesh_workspace_bytes(int64_t F, int n_sets);      /* 0: sizes that are not valid */
int lerf_coords_trimesh(const void* pos, int pos_dtype, int V, const void* attr, int attr_dtype, int Va,
                        const int32_t* faces, const int32_t* attr_faces, int F, const float* depth, const void* w, int w_dtype,
                        void* out, int out_dtype, int64_t out_row_stride, int oH, int oW, int i0, int j0,
                        int max_span, int orient, uint64_t* keys, float* depth_out,
                        void* workspace, size_t workspace_bytes, void* stream);
int lerf_coords_trimesh_host(const void* pos, int pos_dtype, int V, const void* attr, int attr_dtype, int Va,
                             const int32_t* faces, const int32_t* attr_faces, int F, const float* depth, const void* w, int w_dtype,
                             void* out, int out_dtype, int64_t out_row_stride, int oH, int oW, int i0, int j0,
                             int max_span, int orient, uint64_t* keys, float* depth_out,
                             void* workspace, size_t workspace_bytes);
int lerf_coords_trimesh_batched(const void* pos, int pos_dtype, int V, const void* attr, int attr_dtype, int Va,
                                const int32_t* faces, const int32_t* attr_faces, int F, const float* depth, const void* w, int w_dtype,
                                void* out, int out_dtype, int64_t out_row_stride, int oH, int oW, int i0, int j0,
                                int max_span, int orient, uint64_t* keys, float* depth_out,
                                void* workspace, size_t workspace_bytes,
                                int n_sets, int64_t pos_set_stride, int64_t attr_set_stride, int64_t faces_set_stride,
                                int64_t attr_faces_set_stride, int64_t depth_set_stride, int64_t w_set_stride,
                                int64_t out_set_stride, int64_t keys_set_stride, int64_t depth_out_set_stride, void* stream);
int lerf_coords_trimesh_batched_host(const void* pos, int pos_dtype, int V, const void* attr, int attr_dtype, int Va,
                                     const int32_t* faces, const int32_t* attr_faces, int F, const float* depth, const void* w, int w_dtype,
                                     void* out, int out_dtype, int64_t out_row_stride, int oH, int oW, int i0, int j0,
                                     int max_span, int orient, uint64_t* keys, float* depth_out,
                                     void* workspace, size_t workspace_bytes,
                                     int n_sets, int64_t pos_set_stride, int64_t attr_set_stride, int64_t faces_set_stride,
                                     int64_t attr_faces_set_stride, int64_t depth_set_stride, int64_t w_set_stride,
                                     int64_t out_set_stride, int64_t keys_set_stride, int64_t depth_out_set_stride);
/* The ADJOINT of lerf_coords_trimesh: the gradients of a loss on the map with respect to attr, pos and w at FIXED
 * VISIBILITY -- every pixel belongs to the face in the low word of its key; coverage, edges and the depth test are piecewise constant
 * and get no gradient, so depth gets none and depth_out is not differentiable.  The mesh operands, i0, j0, max_span and orient are
 * the forward's, and keys is the plane the forward wrote.
 *   grad_out   [oH][oW][2] float64, dense: the upstream gradient.  It is read ONLY at pixels a face won: a NaN at a hole reaches nothing
 *   grad_attr  [Va][2] float64, grad_pos [V][2] float64, grad_w [V] float64, dense: ACCUMULATED INTO (the caller zeroes); each may be
 *              NULL (that gradient is skipped), not all three; grad_w needs w
 *   workspace  8-byte aligned, lerf_coords_trimesh_bwd_workspace_bytes(F, V, Va, n_sets) bytes (the host twin uses it too): header [4]
 *              uint32, terms [n_sets][F][15] float64, cursor [n_sets][max(V, Va)], list [n_sets][3 F], the scan's partials
 *   max_adders >= 1: a vertex with more incident DRAWN faces (corners) than this is not summed: all its components become NaN.  After
 *              the call header word 1 (byte offset LERF_ORDERED_MAX_COUNT_OFFSET) holds the largest such count, as in the ordered scatter
 * Two passes whose sums have ONE order, stated at the top of csrc/lerf_coords_models.h, so the device equals the host twin BIT FOR BIT
 * and two runs agree exactly: a face pass (one workgroup of 4 waves per face reduces the face's 6 or 15 sums over the pixels it won by a
 * fixed tree) and a vertex pass (the ordered scatter's count, scan, fill, sort and sum with the faces as entries: one writer per element
 * adds its incident faces' terms in ascending (face, corner) order).  A face the forward's set-up skips adds nothing.  Plain launches on
 * the stream: no sync, no allocation, no read-back.
 * THE SIZE RULE, before any pointer: the forward's, and F <= 2^24 - 1, else LERF_EUNSUPPORTED.  Set strides as in the forward, the
 * gradients' in doubles; 0 shares a read-only mesh operand.  Refused with LERF_EINVAL, launching and writing nothing: the forward's
 * list, all three gradients NULL, grad_w without w, max_adders < 1, a null, misaligned or short workspace, a gradient or the workspace
 * intersecting an input or each other over the whole batch, a gradient shared between sets. */
size_t lerf_coords_trimesh_bwd_workspace_bytes(int64_t F, int64_t V, int64_t Va, int n_sets);      /* 0: sizes that are not valid */
int lerf_coords_trimesh_bwd(const void* pos, int pos_dtype, int V, const void* attr, int attr_dtype, int Va,
                            const int32_t* faces, const int32_t* attr_faces, int F, const float* depth, const void* w, int w_dtype,
                            int oH, int oW, int i0, int j0, int max_span, int orient, const uint64_t* keys,
                            const double* grad_out, double* grad_attr, double* grad_pos, double* grad_w,
                            void* workspace, size_t workspace_bytes, int max_adders, void* stream);
int lerf_coords_trimesh_bwd_host(const void* pos, int pos_dtype, int V, const void* attr, int attr_dtype, int Va,
                                 const int32_t* faces, const int32_t* attr_faces, int F, const float* depth, const void* w, int w_dtype,
                                 int oH, int oW, int i0, int j0, int max_span, int orient, const uint64_t* keys,
                                 const double* grad_out, double* grad_attr, double* grad_pos, double* grad_w,
                                 void* workspace, size_t workspace_bytes, int max_adders);
int lerf_coords_trimesh_bwd_batched(const void* pos, int pos_dtype, int V, const void* attr, int attr_dtype, int Va,
                                    const int32_t* faces, const int32_t* attr_faces, int F, const float* depth, const void* w, int w_dtype,
                                    int oH, int oW, int i0, int j0, int max_span, int orient, const uint64_t* keys,
                                    const double* grad_out, double* grad_attr, double* grad_pos, double* grad_w,
                                    void* workspace, size_t workspace_bytes, int max_adders,
                                    int n_sets, int64_t pos_set_stride, int64_t attr_set_stride, int64_t faces_set_stride,
                                    int64_t attr_faces_set_stride, int64_t depth_set_stride, int64_t w_set_stride, int64_t keys_set_stride,
                                    int64_t grad_out_set_stride, int64_t grad_attr_set_stride, int64_t grad_pos_set_stride,
                                    int64_t grad_w_set_stride, void* stream);
int lerf_coords_trimesh_bwd_batched_host(const void* pos, int pos_dtype, int V, const void* attr, int attr_dtype, int Va,
                                         const int32_t* faces, const int32_t* attr_faces, int F, const float* depth, const void* w, int w_dtype,
                                         int oH, int oW, int i0, int j0, int max_span, int orient, const uint64_t* keys,
                                         const double* grad_out, double* grad_attr, double* grad_pos, double* grad_w,
                                         void* workspace, size_t workspace_bytes, int max_adders,
                                         int n_sets, int64_t pos_set_stride, int64_t attr_set_stride, int64_t faces_set_stride,
                                         int64_t attr_faces_set_stride, int64_t depth_set_stride, int64_t w_set_stride, int64_t keys_set_stride,
                                         int64_t grad_out_set_stride, int64_t grad_attr_set_stride, int64_t grad_pos_set_stride,
                                         int64_t grad_w_set_stride);
int lerf_coords_compose_bwd_batched(const void* a, int a_dtype, int64_t a_row_stride, int aH, int aW,
                                    const void* b, int b_dtype, int64_t b_row_stride,
                                    const double* grad_out, int oH, int oW, double* grad_a, double* grad_b,
                                    int n_sets, int64_t a_set_stride, int64_t b_set_stride, int64_t grad_out_set_stride,
                                    int64_t grad_a_set_stride, int64_t grad_b_set_stride, void* stream);
int lerf_coords_compose_bwd_batched_host(const void* a, int a_dtype, int64_t a_row_stride, int aH, int aW,
                                         const void* b, int b_dtype, int64_t b_row_stride,
                                         const double* grad_out, int oH, int oW, double* grad_a, double* grad_b,
                                         int n_sets, int64_t a_set_stride, int64_t b_set_stride, int64_t grad_out_set_stride,
                                         int64_t grad_a_set_stride, int64_t grad_b_set_stride);
int lerf_coords_invert_bwd_batched(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW,
                                   const void* g, int g_dtype, int64_t g_row_stride,
                                   const double* grad_out, int oH, int oW, double* grad_f,
                                   int n_sets, int64_t f_set_stride, int64_t g_set_stride, int64_t grad_out_set_stride,
                                   int64_t grad_f_set_stride, void* stream);
int lerf_coords_invert_bwd_batched_host(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW,
                                        const void* g, int g_dtype, int64_t g_row_stride,
                                        const double* grad_out, int oH, int oW, double* grad_f,
                                        int n_sets, int64_t f_set_stride, int64_t g_set_stride, int64_t grad_out_set_stride,
                                        int64_t grad_f_set_stride);

/* Forward warp by summation splatting (the rounding order of every statement: the top of csrc/lerf_splat_point.h).
 * Every pixel of a source image is ADDED into an output frame at the position a forward map gives it -- the scatter that remap's
 * gather is the adjoint of, and the differentiable counterpart of lerf_coords_invert_raster's hard depth test.
 * Operands, for set s < n_sets (a single call is n_sets = 1, where the set strides are not used):
 *   x     [n_sets][C][H][W] of `dtype` T (LERF_F32 or LERF_F64), dense NCHW, set s at x + s * x_set_stride elements
 *   f     the forward map [H][W][2] of f_dtype (LERF_F32, promoted exactly, or LERF_F64) under the strided map contract (f_row_stride even,
 *         >= 2 * W, entry-aligned); f[i][j] = (r, c) is the position in the [oH][oW] output frame at which source pixel (i, j) lands
 *         (lerf_coords_invert_raster reads f the same way).  f_set_stride even; 0 = ONE map shared by every set
 *   m     [n_sets][H][W] of T, a weight per source pixel, or NULL: every weight is 1
 *   acc   [n_sets][C + with_norm][oH][oW] of T, dense; with_norm (0 / 1) adds the plane C that gathers the weights themselves
 * Forward, per source pixel, in float64:
 *   r or c not finite (NaN, +-inf): the pixel contributes nothing and forms no address -- "no target", the mirror of remap's "no source"
 *   i0 = floor(r), tr = r - i0, wr = {1 - tr, tr}; the columns alike.  Taps (i0 + a, j0 + b), a, b in {0, 1}, in the order (0,0) (0,1)
 *   (1,0) (1,1), each with w = wr[a] * wc[b]; a tap with wr[a] == 0 or wc[b] == 0 is skipped (an integer position touches ONE pixel,
 *   r = oH - 1 is inside the frame); a tap outside [0, oH) x [0, oW) is DROPPED, NOT CLIPPED: mass that leaves the frame is lost.  floor
 *   and the frame test run in floating point BEFORE any conversion to int: 1e300 forms no address and overflows nothing.
 *   acc[s][k][q] += round_T((w * m) * x_k) for k < C, and acc[s][C][q] += round_T(w * m) with the norm plane.
 *   acc is ACCUMULATED INTO (lerf_remap_bwd's contract): the caller zeroes it, and consecutive calls splat several frames into one
 *   canvas.  Device: one thread per source pixel, one no-return atomic add of T per tap and plane (a hardware float add for both
 *   dtypes on gfx950), so two runs are equal up to the rounding of a reordered sum in T; the host twin adds in row-major source order.
 * lerf_splat_bwd, the adjoint, takes g [n_sets][C + with_norm][oH][oW] of T (the upstream of acc).  S(q) = sum_k x_k g[k][q] + g[C][q]
 * (without the last term when with_norm == 0); S and g read as 0 at a dropped tap.  Per source pixel, ONE writer, a fixed tap order:
 *   grad_x[k][i][j] = m * sum_taps w g[k][q]                                     [n_sets][C][H][W] of T
 *   grad_m[i][j]    = sum_taps w S(q)                                            [n_sets][H][W] of T
 *   grad_f[i][j].r  = m * sum_b wc[b] (S(i0 + 1, j0 + b) - S(i0, j0 + b)),  .c the transposed statement      float64 [n_sets][H][W][2] dense
 * grad_f is the derivative of the cell that floor picked: ONE-SIDED (towards +) at an integer position.  A source pixel whose position
 * is not finite gets exact zeros in all three, whatever g holds.  The three are STORED, rounded once at the store (no accumulation, no
 * atomics: a pure gather), so the device equals lerf_splat_bwd_host bit for bit and two runs agree.  Each may be NULL to skip that half; all three
 * NULL is refused.  A map shared by the batch (f_set_stride 0) still has one grad_f per set: the caller sums them.
 * Both: caller-owned buffers, no allocation, no sync, one launch on `stream`.  Refused with LERF_EINVAL before anything is written: a null
 * required pointer, a pointer not aligned to its element (f: to its entry), a dtype code that is not LERF_F32 / LERF_F64, an odd or short
 * row stride, C < 1, H, W, oH or oW < 1, H > 262140 (the grid's y), with_norm not 0 / 1, n_sets outside 1 .. 65535, a set stride that is
 * negative, odd (f, grad_f) or, for n_sets > 1, shorter than a set's extent (f alone may be 0), acc intersecting x, m or f, and any
 * gradient intersecting x, f, m, g or another gradient (over the whole batch). */
int lerf_splat(const void* x, int dtype, int C, int H, int W, int64_t x_set_stride,
               const void* f, int f_dtype, int64_t f_row_stride, int64_t f_set_stride,
               const void* m, int64_t m_set_stride,
               void* acc, int with_norm, int oH, int oW, int64_t acc_set_stride, int n_sets, void* stream);
int lerf_splat_host(const void* x, int dtype, int C, int H, int W, int64_t x_set_stride,
                    const void* f, int f_dtype, int64_t f_row_stride, int64_t f_set_stride,
                    const void* m, int64_t m_set_stride,
                    void* acc, int with_norm, int oH, int oW, int64_t acc_set_stride, int n_sets);
int lerf_splat_bwd(const void* x, int dtype, int C, int H, int W, int64_t x_set_stride,
                   const void* f, int f_dtype, int64_t f_row_stride, int64_t f_set_stride,
                   const void* m, int64_t m_set_stride,
                   const void* g, int with_norm, int oH, int oW, int64_t g_set_stride,
                   void* grad_x, int64_t grad_x_set_stride, void* grad_m, int64_t grad_m_set_stride,
                   double* grad_f, int64_t grad_f_set_stride, int n_sets, void* stream);
int lerf_splat_bwd_host(const void* x, int dtype, int C, int H, int W, int64_t x_set_stride,
                        const void* f, int f_dtype, int64_t f_row_stride, int64_t f_set_stride,
                        const void* m, int64_t m_set_stride,
                        const void* g, int with_norm, int oH, int oW, int64_t g_set_stride,
                        void* grad_x, int64_t grad_x_set_stride, void* grad_m, int64_t grad_m_set_stride,
                        double* grad_f, int64_t grad_f_set_stride, int n_sets);

/* The ORDERED scatter: a deterministic form of the three float scatters -- lerf_splat, the outer gradient of
 * lerf_coords_compose_bwd, lerf_coords_invert_bwd.  Each _ordered entry point takes the arguments of its sibling plus a caller-owned
 * workspace and max_adders, computes the same sums in the order of the HOST twin (entries in row-major order, the taps of an entry in
 * the order (0,0) (0,1) (1,0) (1,1)) and so equals lerf_splat_host / lerf_coords_compose_bwd_host / lerf_coords_invert_bwd_host BIT
 * FOR BIT, from run to run and with a pre-filled acc / grad (accumulated into, as ever).  Four passes on `stream` over the workspace:
 * count the adders of every target element (integer atomics), an exclusive prefix sum of the counts, fill every target's list of
 * entries, then one thread per target sorts its list and adds its terms -- recomputed from the operands by the sibling's own
 * statements -- without atomics.  The inner gradient of compose (grad_b: one writer already) runs as in the sibling, in the same call.
 *   An "entry" is one call of the operation: source pixel (i, j) of the splat ([H][W]), entry (i, j) of grad_out ([oH][oW]) for the two
 *   adjoints; n_entries = their number per set.  A "target" is an element of the frame added into: [oH][oW] of acc, [aH][aW] of
 *   grad_a, [fH][fW] of grad_f; n_targets = their number per set.
 *   workspace   lerf_scatter_ordered_workspace_bytes(n_entries, n_targets, n_sets) bytes of device (host twin: host) memory, 4-byte
 *               aligned, contents arbitrary on entry; in uint32 words: header [4], cursor [n_sets][n_targets], list [n_sets][4 n_entries],
 *               scan partials [n_sets][P(n_targets)], P(n) = the sum of n_l = ceil(n_(l-1) / B) over the levels l >= 1 with
 *               n_(l-1) > B, n_0 = n, B = lerf_scan_exclusive_u32_block().  0 from the size query for a size it does not serve.
 *               After the call header word 1 (byte offset LERF_ORDERED_MAX_COUNT_OFFSET) holds the LARGEST number of adders any target
 *               of the call has (0 when nothing was scattered); words 0, 2 and 3 are 0.
 *   max_adders  the cap: a target with more adders than this is neither sorted nor summed -- every plane of it (both components of a
 *               gradient entry) becomes NaN, which bounds the run time of its thread; every other target is exact.  The caller reads
 *               the header word and refuses the result when it exceeds max_adders.
 * No allocation, no sync.  Refused before anything is launched or written, the workspace included: everything the sibling refuses,
 * and with LERF_EINVAL a null, misaligned or short workspace, a workspace intersecting any operand, max_adders < 1, and a target
 * operand shared between sets (n_sets > 1 with grad_a_set_stride 0: two sets would be two writers of one element; acc and grad_f can
 * never be shared).  4 * n_entries or n_targets beyond 2^32 - 1 is LERF_EUNSUPPORTED, judged before the pointers are looked at. */
#define LERF_ORDERED_MAX_COUNT_OFFSET 4
size_t lerf_scatter_ordered_workspace_bytes(int64_t n_entries, int64_t n_targets, int n_sets);
int lerf_splat_ordered(const void* x, int dtype, int C, int H, int W, int64_t x_set_stride,
                       const void* f, int f_dtype, int64_t f_row_stride, int64_t f_set_stride,
                       const void* m, int64_t m_set_stride,
                       void* acc, int with_norm, int oH, int oW, int64_t acc_set_stride, int n_sets,
                       void* workspace, size_t workspace_bytes, int max_adders, void* stream);
int lerf_splat_ordered_host(const void* x, int dtype, int C, int H, int W, int64_t x_set_stride,
                            const void* f, int f_dtype, int64_t f_row_stride, int64_t f_set_stride,
                            const void* m, int64_t m_set_stride,
                            void* acc, int with_norm, int oH, int oW, int64_t acc_set_stride, int n_sets,
                            void* workspace, size_t workspace_bytes, int max_adders);
int lerf_coords_compose_bwd_ordered(const void* a, int a_dtype, int64_t a_row_stride, int aH, int aW,
                                    const void* b, int b_dtype, int64_t b_row_stride,
                                    const double* grad_out, int oH, int oW, double* grad_a, double* grad_b,
                                    void* workspace, size_t workspace_bytes, int max_adders, void* stream);
int lerf_coords_compose_bwd_ordered_host(const void* a, int a_dtype, int64_t a_row_stride, int aH, int aW,
                                         const void* b, int b_dtype, int64_t b_row_stride,
                                         const double* grad_out, int oH, int oW, double* grad_a, double* grad_b,
                                         void* workspace, size_t workspace_bytes, int max_adders);
int lerf_coords_compose_bwd_batched_ordered(const void* a, int a_dtype, int64_t a_row_stride, int aH, int aW,
                                            const void* b, int b_dtype, int64_t b_row_stride,
                                            const double* grad_out, int oH, int oW, double* grad_a, double* grad_b,
                                            int n_sets, int64_t a_set_stride, int64_t b_set_stride, int64_t grad_out_set_stride,
                                            int64_t grad_a_set_stride, int64_t grad_b_set_stride,
                                            void* workspace, size_t workspace_bytes, int max_adders, void* stream);
int lerf_coords_compose_bwd_batched_ordered_host(const void* a, int a_dtype, int64_t a_row_stride, int aH, int aW,
                                                 const void* b, int b_dtype, int64_t b_row_stride,
                                                 const double* grad_out, int oH, int oW, double* grad_a, double* grad_b,
                                                 int n_sets, int64_t a_set_stride, int64_t b_set_stride, int64_t grad_out_set_stride,
                                                 int64_t grad_a_set_stride, int64_t grad_b_set_stride,
                                                 void* workspace, size_t workspace_bytes, int max_adders);
int lerf_coords_invert_bwd_ordered(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW,
                                   const void* g, int g_dtype, int64_t g_row_stride,
                                   const double* grad_out, int oH, int oW, double* grad_f,
                                   void* workspace, size_t workspace_bytes, int max_adders, void* stream);
int lerf_coords_invert_bwd_ordered_host(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW,
                                        const void* g, int g_dtype, int64_t g_row_stride,
                                        const double* grad_out, int oH, int oW, double* grad_f,
                                        void* workspace, size_t workspace_bytes, int max_adders);
int lerf_coords_invert_bwd_batched_ordered(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW,
                                           const void* g, int g_dtype, int64_t g_row_stride,
                                           const double* grad_out, int oH, int oW, double* grad_f,
                                           int n_sets, int64_t f_set_stride, int64_t g_set_stride, int64_t grad_out_set_stride,
                                           int64_t grad_f_set_stride,
                                           void* workspace, size_t workspace_bytes, int max_adders, void* stream);
int lerf_coords_invert_bwd_batched_ordered_host(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW,
                                                const void* g, int g_dtype, int64_t g_row_stride,
                                                const double* grad_out, int oH, int oW, double* grad_f,
                                                int n_sets, int64_t f_set_stride, int64_t g_set_stride, int64_t grad_out_set_stride,
                                                int64_t grad_f_set_stride,
                                                void* workspace, size_t workspace_bytes, int max_adders);

/* The scan of pass 2 on its own: data [n] uint32 -> its exclusive prefix sums, in place, modulo 2^32.  Device: blocks of
 * lerf_scan_exclusive_u32_block() elements scanned in LDS, the block sums scanned by the same kernels one level up, an add-back per
 * level -- plain launches in stream order, no workgroup waits for another; workspace: lerf_scan_exclusive_u32_workspace_bytes(n)
 * bytes of device memory (0, and then it may be NULL, when n fits one block).  No allocation, no sync.  LERF_EINVAL: a null or
 * misaligned data, n < 1 or > 2^32 - 1, a needed workspace that is null, misaligned, short or intersects data. */
int lerf_scan_exclusive_u32_block(void);
size_t lerf_scan_exclusive_u32_workspace_bytes(int64_t n);
int lerf_scan_exclusive_u32(uint32_t* data, int64_t n, void* workspace, size_t workspace_bytes, void* stream);
int lerf_scan_exclusive_u32_host(uint32_t* data, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* LERF_HIP_H */
