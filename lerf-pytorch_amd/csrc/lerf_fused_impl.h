// Implementation of the tile-fused kernels, included once per channel count: the including translation unit defines
//   LERF_FUSED_NS   namespace of this instance (fused = RGB, fused_c1 = single channel, fused_c4 = four channels)
//   LERF_FUSED_CH   channels per pixel; the LR tile is 64 rows x (192 / CH) pixels, 192 pixel-channels per tile row
//   LERF_FUSED_TH   tile rows (default 64)
// (a plain C++ namespace-parametrised include: everything in here is gfx950 code, there is no second platform).
//
// Tile-fused uint8 SR path for MI355X (gfx950): stage-1 LUTs -> stage-2 LUTs -> spatially-varying resampling per
// 64x64 LR tile (tiles handed to the XCDs in contiguous eighths: xcd_order).  With a caller workspace (the normal case)
// it is TWO launches: s1_kernel computes stage 1 once per pixel and parks its uint8 output in the workspace,
// sr_fused_kernel<.., FROM_FEAT> runs stage 2, the finalisation and stage 3 from it -- the hyper-parameters never leave
// the CU.  Without a workspace ONE launch does everything and recomputes stage 1 on each tile's halo.
//
// Reference path being replaced: eltr._worker, resample/eval_lut_sr.py:541-665
// (FourSimplexInterpFaster :24-470 x 24 passes, SteeringGaussianResize2dNumpy /
// AmplifiedLinearResize2dNumpy, resize_right/resize_right2d_numpy.py:142-282).
//
// Work decomposition
//   one 1024-thread workgroup (16 waves, 1 per CU: LDS-bound) per 64x64 LR tile
//   of one frame.  The tile owns the output pixels whose support starts inside
//   it.  Halo: 3 (stage 1) + 3 (stage 2) + S/2 (stage 3) LR pixels per side,
//   recomputed per tile; true image borders use the reference's rules (clamped
//   sampling for the LUT stages, zero image / edge hyper for stage 3).
//
// LDS plan (dynamic, one array; sizes for S=2 / S=4)
//   B    feat tile u8                   (72x72x3 = 15.5 KB / 74x74x3)     all stages
//   LUT  stage 1: one int8 LUT          83.5 KB
//        stage 2 (LeRF-G): a THIRD of one packed LUT = the 7 top-axis levels that pixels whose
//        centre level lies in the bin can touch, 7*4913 dwords = 134 KB
//   C    input tile u8 (78x78x3)        stage 1 only
//   ACC  int16 partial sums             stage 1 (and stage 2 of LeRF-L)
//   LST  pixel lists sorted by bin      stage 2 (LeRF-G), transient (under the piece, which waits in registers)
//   D    (hq0,hq1,hq2,feat) dwords      stage 3, overlays LUT (52 KB / 55 KB)
//   GEO  tile geometry tables           stage 3 (9 KB; staged at kernel start for S=2; the exact-x2 kernels leave it unused: GeoX2)
//   TQ   rounding-tie queue             stage 3 (8 KB, behind D)
//   OUT  the tile's output block        stage 3, block tasks (2 x 2 outputs that share their taps: integer x2 LeRF-G, LeRF-L):
//        assembled byte by byte (132 x 416 B behind TQ), ties patched in it, stored as whole 16-byte chunks
//   CGRP column-group table             stage 3, LeRF-L block tasks (behind OUT)
//
// Stage 2 of LeRF-G keeps the whole 3-channel LUT entry in one dword, so one
// simplex walk (index sort + 5 LDS gathers) serves all three hyper channels.
// The full packed LUT (326 KB) cannot live in LDS; pixels are therefore binned
// by the level of their centre value (which selects the slowest LUT axis
// for every mode and rotation), and each (LUT, bin) phase processes only the
// pixels of that bin with all 64 lanes busy.  Per-pixel accumulators stay in
// VGPRs across phases (two packed 16-bit fields + one).
#include <string.h>
#include <atomic>
#include <type_traits>

#include "lerf_kernels.h"
#include "lerf_simplex_lds.h"
#include "lerf_stage3.h"
#include "lerf_warp_px.h"

namespace lerf {
namespace LERF_FUSED_NS {

constexpr int NT = 1024;           // threads per workgroup (the binning of LeRF-G stage 2 is written for 16 waves)
constexpr int NW = NT / 64;        // waves
constexpr int CH = LERF_FUSED_CH;  // channels per pixel of this instance
static_assert(CH == 1 || CH == 3 || CH == 4, "192 pixel-channels per tile row");
#ifndef LERF_FUSED_TH
#define LERF_FUSED_TH 64           // tile rows: 64 = the throughput tile; the 32- and 16-row instances (lerf_fused_h32 / _h16.hip) serve launches
#endif                             // too small to fill the chip with 64-row tiles (a 256 x 256 frame: 16 / 32 / 64 workgroups)
constexpr int TH = LERF_FUSED_TH, TW = 192 / CH;   // LR tile: TH rows x 192 pixel-channels (64x64 RGB pixels, 64x192 grey, 64x48 RGBA):
                                   // the same number of stage-2 positions, registers and LDS bytes for every channel count
constexpr int R1 = 3, R2 = 3;      // stage radii: the reach of the widest sampling patterns (c, t: 3 px; s 1, d 2, y 2)
constexpr int MAXM = 4;            // modes per stage the 16-bit sums can hold (4 rotations x 4 modes x 16 x 255 < 2^16)
constexpr int LUT_PAD = 83584;     // padded entries per LUT in the pack (16-B multiple)
// Stage-2 bins: a pixel-channel goes by the top-axis level (high nibble) of its centre value, which selects the slowest
// LUT axis for every mode and rotation.  Bin b covers the levels [bin_lo(b), bin_lo(b + 1)); its piece of a packed LUT is
// those levels plus the one above (the simplex walk steps up once).
// Three bins of 6, 5 and 5 levels, 7-level pieces of 134 KiB that fill the LDS: 18 long phases per tile (the measured
// alternative, four bins of 4 levels with 5-level pieces of 96 KiB and 24 phases, lost).
constexpr int NBIN = 3;
__host__ __device__ constexpr int bin_lo(int b) { return b == 0 ? 0 : (b == 1 ? 6 : (b == 2 ? 11 : 16)); }
__device__ __forceinline__ uint32_t bin_of_level(uint32_t msb) { return (msb >= 6u ? 1u : 0u) + (msb >= 11u ? 1u : 0u); }
constexpr int PIECE_LEVELS = 7;                               // levels per piece
constexpr int PIECE_ENTRIES = PIECE_LEVELS * kStrideA;
constexpr int NSLAB = (PIECE_ENTRIES * 4 + 16 * NT - 1) / (16 * NT);   // 16 bytes per thread and slab
constexpr int PIECE_BYTES = NSLAB * 16 * NT;                  // one piece in the pack (144 KiB, 34391 dwords used)
constexpr int PIECE_BLOCKS = (PIECE_ENTRIES * 4 + 1023) / 1024;      // 1-KiB blocks of a piece that hold data
constexpr int PIECE_LDS = PIECE_BLOCKS * 1024;                // what a piece occupies in LDS

// BIG = false: geometry tables for scale factors up to 4.9, staged at kernel start for the 2x2 support of RGB frames (the
// headline layout).  BIG = true: up to x8.1, always staged late over the dead LUT area.
// NOHALO = true (the EMIT kernels): the hyper region is the tile itself -- the stage-3 ring of R3 pixels is looked up only by
// the kernels that run stage 3 (the packed maps a warp reads hold every pixel once); the feat region keeps its size, so the
// aligned-dword tile load stays.
template <int S, bool BIG = false, bool NOHALO = false>
struct Dims {
    static constexpr int R3 = S / 2;
    static constexpr int HR = NOHALO ? 0 : R3;                                             // ring of the hyper region around the tile
    static constexpr int HY = TH + 2 * HR, HX = TW + 2 * HR, HP = HX * CH, NH = HY * HP;   // hyper region
    static constexpr int FY = TH + 2 * R3 + 2 * R2, FX = TW + 2 * R3 + 2 * R2, FP = FX * CH, NF = FY * FP;   // feat region
    static constexpr int HO = R2 + R3 - HR;                                                // the hyper region's origin inside the feat region
    // input region; its LDS pitch is a dword multiple with room for a 0..3 byte phase, so that interior tiles can be
    // fetched as aligned dwords (row r of the tile = global bytes from the 4-byte boundary below its first pixel)
    static constexpr int IY = FY + 2 * R1, IX = FX + 2 * R1, IPB = IX * CH, IP = (IPB + 3 + 3) / 4 * 4, NI = IY * IP;
    static constexpr int up16(int x) { return (x + 15) / 16 * 16; }
    static constexpr int OFF_B = 0;
    static constexpr int OFF_X = up16(NF);                       // stage-dependent area starts here
    // stage 1 (and byte-LUT stage 2)
    static constexpr int OFF_LUT = OFF_X;
    static constexpr int OFF_C = OFF_LUT + LUT_PAD;
    static constexpr int OFF_ACC = OFF_C + up16(NI);
    static constexpr int END1 = OFF_ACC + up16(NF * 2);
    // stage 2, LeRF-G: one piece.  The position lists and the wave x bin count table only live between the binning and the
    // first piece store (the first piece waits in registers) and overlay the piece.
    // positions that are looked up: the hyper region without its last row and column (never read by an owned output, see the binning)
    static constexpr int NHL = HR > 0 ? (HY - 1) * (HX - 1) * CH : NH;
    static constexpr int MAXR = (NHL + NBIN * 63 + NT - 1) / NT;  // slot rounds: every bin padded to whole waves (13 for S = 2, 14 for S = 4)
    static constexpr int OFF_LST = OFF_X;
    static constexpr int OFF_TAB = OFF_LST + MAXR * NT * 2;       // [wave][4 bins] counts
    static_assert(OFF_TAB + NW * 4 * 4 <= OFF_X + PIECE_LDS, "binning scratch fits under the piece");
    static constexpr int END2 = OFF_X + PIECE_LDS;
    // stage 3
    static constexpr int OFF_D = OFF_X;
    // S = 2, RGB, scale <= 4.9: the tile geometry is staged at kernel start (its table look-ups overlap the input load) into
    // a region of its own; the other layouts have no room for that and stage it right before stage 3, over the dead LUT area
    static constexpr bool GEO_EARLY = (S == 2) && CH == 3 && !BIG;
    static constexpr int cmax0(int a, int b) { return a > b ? a : b; }
    static constexpr int OFF_GEO = GEO_EARLY ? cmax0(END1, END2) : OFF_D + up16(NH * 4);
    static constexpr int GEO_ROWS = BIG ? TH * 8 + 8 : TH * 5;    // max owned output rows per tile
    static constexpr int GEO_COLS = BIG ? TW * 8 + 8 : TW * 5;    // max owned output columns per tile
    static constexpr int SZ_GEO = (GEO_ROWS + GEO_COLS) * (4 + 4 * S) + (GEO_ROWS + 16) * 4;   // + row-group table
    static constexpr int END3 = OFF_GEO + SZ_GEO;
    // stage 3: queue of the outputs that sit on a rounding tie (re-evaluated in float64 after the task loop, all lanes
    // busy, instead of one lane at a time inside it); over the dead LUT piece, behind D (and behind the late geometry)
    static constexpr int TQ_CAP = 2048;                           // (lerf_sr_geo_t.tie_queue_cap lowers the part in use: tests)
    static constexpr int OFF_TQ = GEO_EARLY ? OFF_D + up16(NH * 4) : END3;
    static_assert(OFF_TQ + TQ_CAP * 4 <= OFF_X + PIECE_LDS, "tie queue fits under the piece");
    static_assert(GEO_EARLY || END3 <= OFF_X + PIECE_LDS, "late geometry fits under the piece");
    // stage 3, block tasks (integer x2 tiles: 2 x 2 outputs share their taps): the tile's output bytes are assembled in LDS
    // (behind the tie queue, over the dead LUT piece) and leave as whole 16-byte chunks; the rows sit at the phase of their
    // global address modulo 16
    static constexpr int OUT_ROWS = 2 * TH + 4, OUT_PITCH = up16(2 * TW * CH + 16 + 15);
    static constexpr int OFF_OUT = up16(OFF_TQ + TQ_CAP * 4);
    static constexpr int OFF_CGRP = OFF_OUT + OUT_ROWS * OUT_PITCH;          // column-group table of the LeRF-L block tasks
    static constexpr bool OUT_FITS = OFF_CGRP + (2 * TW + 16) * 4 <= OFF_X + PIECE_LDS;
    static constexpr int cmax(int a, int b) { return a > b ? a : b; }
    static constexpr int LDS_BYTES = cmax(END1, cmax(END2, GEO_EARLY ? END3 : 0)) + 512;  // + small control block
    static constexpr int OFF_CTL = LDS_BYTES - 512;
    static_assert(LDS_BYTES <= 160 * 1024, "one workgroup per CU: 160 KiB of LDS");
    static_assert(NT != 1024 || (MAXR <= 14 && (NH + NT - 1) / NT <= 15), "slot rounds / positions per thread the register budget was sized for");
};

// The int slots of the control block (Dims::OFF_CTL) that stage 3 uses: each is written by one wave and read by all of them
// behind a barrier.  A kernel runs one kind, so the two kinds' answers about the rows share a slot.
enum Ctl : int {
    CTL_I0 = 16,            // first owned output row (CTL_I0 + w = the result of search wave w: i0, i1, j0, j1)
    CTL_I1 = 17,            // one past the last owned output row
    CTL_J0 = 18,            // first owned output column
    CTL_J1 = 19,            // one past the last owned output column
    CTL_NGRP = 21,          // row groups of the tile
    CTL_GSAME = 22,         // rows per group when every group has as many, else 0
    CTL_TQ_COUNT = 23,      // tie queue: outputs pushed so far (runs past the capacity when the queue is full)
    CTL_CCODE = 24,         // LeRF-G: pair code of the columns (pair_census)
    CTL_NCGRP = 25,         // LeRF-L: column groups
    CTL_RCODE = 26,         // LeRF-G: pair code of the rows
    CTL_LIN_ROWS_OK = 26,   // LeRF-L: no row group has more than two rows
    CTL_LIN_COLS_OK = 27,   // LeRF-L: the column-group table holds every group
    CTL_CSTEP = 28,         // LeRF-G: column pair h + 1 starts exactly one tap right of pair h (x2)
    CTL_RSTEP = 29,         // LeRF-G: row pair h + 1 starts exactly one tap below pair h
};

// Frames of DIFFERENT sizes in one launch (general kernels only): the descriptors travel in the kernel-argument segment, so
// a workgroup finds its frame with scalar loads.  first_block = index of the frame's first tile in the launch.
constexpr int RAGGED_MAX = 16;
struct FrameDesc {
    const uint8_t* img; uint8_t* out; uint8_t* feat; uint32_t* emit;
    const int* left_r; const float* dis_r; const int* left_c; const float* dis_c;
    const double* dis_r64; const double* dis_c64;
    int H, W, oH, oW, tiles_x, tiles_y, first_block, pad_;
};
struct RaggedTable { int n; int pad_; FrameDesc d[RAGGED_MAX]; };
struct NoTable {};

struct Params {
    const uint8_t* img; int64_t in_sn;
    uint8_t* out; int64_t out_sn;
    int H, W, oH, oW, tiles_y, tiles_x;
    int ty_org, tx_org;              // LR origin of tile (0, 0): the region of interest of lerf_sr_geo_t (0, 0 = whole frame)
    const uint8_t* pack;             // fused LUT pack (see lerf_fused_lutpack_*)
    const int* left_r; const float* dis_r; const int* left_c; const float* dis_c;
    const double* dis_r64; const double* dis_c64;      // tie guard (may be NULL: guard off)
    float max_sigma;
    int n1, n2;                      // modes per stage (1..MAXM); the pack holds n1 stage-1 and 2 * n2 stage-2 LUTs
    int s2off[2 * MAXM][6];          // stage-2 LUT l: feat-tile byte offsets of pixels b,c,d for rotations par, par+2
    int s1off[MAXM][12];             // general kernels: stage-1 LUT m: input-tile byte offsets of b,c,d for rotations 0..3
    int s1dyx[MAXM][12];             // the same pixels as (dy << 16) | (dx & 0xFFFF) in the frame (vector-memory pixel path)
    int s2dyx[2 * MAXM][6];          // stage-2 LUT l, rotations par / par + 2
    uint32_t* emit; int64_t emit_sn;   // EMIT kernels: packed stage outputs, frame stride in dwords
    uint8_t* feat; int64_t feat_sn;    // two-launch path: stage-1 output [N][H][W][C] between s1_kernel and the FROM_FEAT kernel
    unsigned long long* stamps;      // diagnostic builds (-DLERF_STAMPS) only: [blocks][16] cycle stamps
    int tq_cap;                      // stage-3 tie queue entries in use (<= Dims::TQ_CAP; lerf_sr_geo_t.tie_queue_cap)
    int pad_mode;                    // LERF_PAD_* of the image operand of stage 3 at the true frame borders
    int host_input;                  // the input frames live in (pinned) HOST memory: read every pixel once (LDS tile), never 39 times
    int out_pitch;                   // bytes per output row (lerf_sr_geo_t.out_row_pitch; 0 = dense rows of oW * CH bytes)
    WarpGeo wgeo; const int32_t* wboxes;   // tile-fused warp (LERF_FUSED_WARP): homography + per-tile output boxes {i0, i1, j0, j1}
};

#ifdef LERF_STAMPS
#define LERF_STAMP(k) do { if (tid == 0) P.stamps[(size_t)blockIdx.x * 16 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#define LERF_STAMP_ADD(k, t0) do { if (tid == 0) P.stamps[(size_t)blockIdx.x * 16 + (k)] += __builtin_amdgcn_s_memtime() - (t0); } while (0)
#define LERF_NOW() __builtin_amdgcn_s_memtime()
// the constant 100 MHz counter beside the shader-clock one: (s_memtime ticks) / (s_memrealtime ticks) x 100 MHz = the clock
// the chip ran this tile at (tools/stamps.py prints it; slots 13 / 14 of a tile's stamps)
#define LERF_STAMP_RT(k) do { if (tid == 0) { unsigned long long t_; asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)); \
                                              P.stamps[(size_t)blockIdx.x * 16 + (k)] = t_; } } while (0)
#else
#define LERF_STAMP_RT(k) do {} while (0)
#define LERF_STAMP(k) do {} while (0)
#define LERF_STAMP_ADD(k, t0) do {} while (0)
#define LERF_NOW() 0ull
#endif

// (dy, dx) of the 3 non-centre pixels b, c, d of (mode, rot): mode_offsets (lerf_host_geometry.h), the one pattern table
struct DyDx { int dy[3], dx[3]; };
__host__ __device__ constexpr DyDx pattern_dydx(char mode, int rot) {
    int8_t dy[4] = {0, 0, 0, 0}, dx[4] = {0, 0, 0, 0};
    mode_offsets(mode, rot, dy, dx);
    return DyDx{{dy[1], dy[2], dy[3]}, {dx[1], dx[2], dx[3]}};
}
// their byte offsets in a u8 tile of pitch P
struct Off3 { int o[3]; };
__host__ __device__ constexpr Off3 tile_offsets(char mode, int rot, int pitch) {
    const DyDx q = pattern_dydx(mode, rot);
    return Off3{{q.dy[0] * pitch + q.dx[0] * CH, q.dy[1] * pitch + q.dx[1] * CH, q.dy[2] * pitch + q.dx[2] * CH}};
}
template <int P>
__host__ __device__ constexpr Off3 tile_offsets(char mode, int rot) { return tile_offsets(mode, rot, P); }
// The pattern tables of the general kernels (Params): rotations rot0 + h * rstep, h < nrot, of `mode` as byte offsets in an
// LDS tile of `pitch` bytes (off) and as (dy << 16) | (dx & 0xFFFF) in the frame (dyx)
inline void pattern_tables(char mode, int rot0, int rstep, int nrot, int pitch, int* off, int* dyx) {
    for (int h = 0; h < nrot; ++h) {
        const DyDx q = pattern_dydx(mode, rot0 + h * rstep);
        const Off3 o = tile_offsets(mode, rot0 + h * rstep, pitch);
        for (int i = 0; i < 3; ++i) {
            off[3 * h + i] = o.o[i];
            dyx[3 * h + i] = (q.dy[i] << 16) | (q.dx[i] & 0xFFFF);
        }
    }
}

// global -> LDS copy of `bytes` (rounded up to 16) by the whole workgroup; every load of a
// thread is issued before its first LDS write so the L2 latency is paid once per copy
template <int BYTES>
struct Stage16 {
    static constexpr int n = (BYTES + 15) >> 4;
    static constexpr int FULL = n / NT;       // iterations every thread takes part in
    static constexpr int TAIL = n - FULL * NT;
    uint4 r[FULL];
    uint4 rt;
    __device__ __forceinline__ void load(const uint8_t* __restrict__ src, int tid) {
        const uint4* s = reinterpret_cast<const uint4*>(src);
#pragma unroll
        for (int i = 0; i < FULL; ++i) r[i] = s[tid + i * NT];
        rt = make_uint4(0, 0, 0, 0);
        if (TAIL > 0 && tid < TAIL) rt = s[tid + FULL * NT];
    }
    __device__ __forceinline__ void store(uint8_t* dst, int tid) const {
        uint4* d = reinterpret_cast<uint4*>(dst);
#pragma unroll
        for (int i = 0; i < FULL; ++i) d[tid + i * NT] = r[i];
        if (TAIL > 0 && tid < TAIL) d[tid + FULL * NT] = rt;
    }
};

template <int BYTES>
__device__ __forceinline__ void copy16(uint8_t* dst, const uint8_t* __restrict__ src, int tid) {
    Stage16<BYTES> st;
    st.load(src, tid);
    st.store(dst, tid);
}

// ---------------------------------------------------------------------------
// The byte-LUT phase (stage 1, stage 2 of LeRF-L): one LUT, NROT (4 or 2) rotations of its sampling pattern, over a region
// of NDST px-ch positions (row pitch DPc).  A position is: read the centre pixel and the 3 pattern pixels of every rotation
// (a pixel SOURCE: issue, ready), walk the LUT (byte_walks), add the 16-bit partial sum and store or finalise it (a phase
// KIND: phase_finish).  Written once over sources x kinds:
//   sources   where the pixels come from      x   how the pattern is known
//     LdsStatic / LdsRt     the tile in LDS (pitch SP): byte_phase_lds walks the region, interior tiles without clamping
//     VmemStatic / VmemRt   the frame in HBM / L2 over the vector-memory path, interior regions only: stage 1 and these
//                           phases are bound by the LDS (the byte-LUT gathers keep its array 82 % busy, PMC) while the texture
//                           path idles, so byte_phase_vmem fetches a position's pixels (global_load_ubyte_d16_hi: the same
//                           "byte in bits 16..23" form the LDS reads deliver; L1 / L2 hits, the tile's rows are read 13
//                           times over) one position AHEAD of its lookups, and the LDS serves the LUT gathers and the
//                           partial sums only
//     *Static   MODE / ROT0 / NROT / RSTEP at compile time (the published "sct" kernels): the pattern offsets fold into
//               DS / global-load immediates
//     *Rt       the general kernels, any of the five patterns: wave-uniform offsets from the kernel arguments
//               (Params::s1off / s2off / s1dyx / s2dyx), one address add per pixel
//   kinds     PhaseIs<0 / 1 / 2>: first (store the sums) / add / add and finalise with (div, bias) into dst8, at compile
//             time; PhaseRt{first, last}: the same at run time, wave-uniform
// ---------------------------------------------------------------------------
// smallest (most negative) neighbour byte offset over the rotations of a phase: DS immediates are unsigned
template <int SP>
__host__ __device__ constexpr int min_tile_offset(char mode, int rot0, int nrot, int rstep) {
    int m = 0;
    for (int i = 0; i < nrot; ++i) {
        const Off3 o = tile_offsets<SP>(mode, rot0 + i * rstep);
        for (int k = 0; k < 3; ++k) m = o.o[k] < m ? o.o[k] : m;
    }
    return m;
}
// The four rotations of the 2x2 pattern 's' cover the 3x3 block around the centre; its edge neighbours E, S, W, N are pixel b of
// one rotation and pixel c of the previous one, its corners pixel d of one rotation: 8 reads serve the 12 operands (the
// static sources).  block3_offset: the eight neighbours, row by row (byte offsets in a tile of pitch SP); block3_slot: where
// neighbour i sits in a PixSet -- r = b[r], 4 + r = d[r] (pix_slot)
template <int SP>
__host__ __device__ constexpr int block3_offset(int i) {
    const int dy = i < 3 ? -1 : (i < 5 ? 0 : 1);
    const int dx = i < 3 ? i - 1 : (i < 5 ? (i == 3 ? -1 : 1) : i - 6);
    return dy * SP + dx * CH;
}
template <int SP>
__host__ __device__ constexpr int block3_slot(int i) {
    for (int r = 0; r < 4; ++r) {
        const Off3 o = tile_offsets<SP>('s', r);
        if (o.o[0] == block3_offset<SP>(i)) return r;
        if (o.o[2] == block3_offset<SP>(i)) return 4 + r;
    }
    return 0;
}
static_assert(pattern_dydx('s', 0).dy[1] == pattern_dydx('s', 1).dy[0] && pattern_dydx('s', 0).dx[1] == pattern_dydx('s', 1).dx[0],
              "pixel c of rotation r = pixel b of rotation r + 1");

// stages B-D of a byte-LUT position: NROT simplex walks around the centre pixel ra, all their gathers in flight together,
// and the numerator sum_rot sum_n w_n P_n (weights sum to 16 per lookup)
template <int NROT>
__device__ __forceinline__ int byte_walks(uint32_t lut_a, uint32_t ra, const uint32_t (&rb)[4], const uint32_t (&rc)[4],
                                          const uint32_t (&rd)[4]) {
    const unsigned sa = kStrideA, sb = kStrideB, sc = kStrideC, sd = kStrideD;
    const unsigned ka = key_of(ra, sa);
    const int basea = (int)(__umul24(msb_of(ra), kStrideA) + lut_a);      // LDS address of the base corner
    Walk<1> W[NROT];
    ByteCorners E[NROT];
    // the gathers of a walk are issued as soon as its indices exist and fly under the next walk (all 4 walks first, then all
    // 20 gathers: 0.8 % slower; groups of two: 0.2 % slower; A/B on one box): the LDS starts on a position's gathers ~100
    // instructions earlier.  The same split in the stage-2 slot LOST 0.25 %.
#pragma unroll
    for (int i = 0; i < NROT; ++i) {
        W[i] = simplex_walk<1>(ka, basea, rb[i], rc[i], rd[i], sb, sc, sd);
        E[i] = byte_gather(W[i]);
        __builtin_amdgcn_sched_barrier(0);
    }
    // stage D: the Abel sums of the walks (byte_abel) + 16 x the sum of their base corners
    int acc = 0, sum0 = 0;
#pragma unroll
    for (int i = 0; i < NROT; ++i) {
        sum0 += E[i].e0;
        acc = byte_abel(W[i], E[i], acc);
    }
    return acc + kQ * sum0;
}


// ---- phase kinds
template <int PHASE>
struct PhaseIs { static constexpr bool first = PHASE == 0, last = PHASE == 2; };
struct PhaseRt { bool first, last; };
// the epilogue of a position: v = the numerator of this phase's lookups
template <typename Kind>
__device__ __forceinline__ void phase_finish(Kind kind, int v, int16_t* acc16, uint8_t* dst8, int p, int div, int bias) {
    if (!kind.first) v += (int)acc16[p];
    if (kind.last)
        dst8[p] = (uint8_t)rne_div_clip255_fast(v + bias * div, div);
    else
        acc16[p] = (int16_t)v;
}

// ---- pixel sources.  The pixels of a position as the high-half byte loads deliver them (see lds_pixel_hi): the centre a and
// pixels b, c, d of rotation i.  A source has NROT, issue(PixSet&, address) = every read of a position, nothing waited for,
// and ready(PixSet&) = wait for them (wait_pixels: the counter of the source's memory path; the operand list pins every
// pixel register behind the wait).
struct PixSet { uint32_t a, b[4], c[4], d[4]; };
template <int S>
__device__ __forceinline__ uint32_t& pix_slot(PixSet& X) {
    if constexpr (S < 4) return X.b[S];
    else return X.d[S - 4];
}
enum class Wait { LDS, VMEM };
#define LERF_WAIT_PIXELS(...)                                                           \
    do {                                                                                \
        if constexpr (CNT == Wait::LDS) asm volatile("s_waitcnt lgkmcnt(0)" : __VA_ARGS__); \
        else asm volatile("s_waitcnt vmcnt(0)" : __VA_ARGS__);                          \
    } while (0)
template <Wait CNT, int NROT>
__device__ __forceinline__ void wait_pixels(PixSet& X) {
    static_assert(NROT == 2 || NROT == 4, "rotation pairs or all four");
    if constexpr (NROT == 4)
        LERF_WAIT_PIXELS("+v"(X.a), "+v"(X.b[0]), "+v"(X.c[0]), "+v"(X.d[0]), "+v"(X.b[1]), "+v"(X.c[1]), "+v"(X.d[1]), "+v"(X.b[2]),
                         "+v"(X.c[2]), "+v"(X.d[2]), "+v"(X.b[3]), "+v"(X.c[3]), "+v"(X.d[3]));
    else
        LERF_WAIT_PIXELS("+v"(X.a), "+v"(X.b[0]), "+v"(X.c[0]), "+v"(X.d[0]), "+v"(X.b[1]), "+v"(X.c[1]), "+v"(X.d[1]));
}
// the centre and the eight neighbours of the shared 3x3 block, in the order they were read; then pixel c of every rotation
template <Wait CNT>
__device__ __forceinline__ void wait_block3(PixSet& X, uint32_t& n0, uint32_t& n1, uint32_t& n2, uint32_t& n3, uint32_t& n4, uint32_t& n5,
                                            uint32_t& n6, uint32_t& n7) {
    LERF_WAIT_PIXELS("+v"(X.a), "+v"(n0), "+v"(n1), "+v"(n2), "+v"(n3), "+v"(n4), "+v"(n5), "+v"(n6), "+v"(n7));
    X.c[0] = X.b[1]; X.c[1] = X.b[2]; X.c[2] = X.b[3]; X.c[3] = X.b[0];
}
#undef LERF_WAIT_PIXELS
template <char MODE, int ROT0, int NROT, int RSTEP>
constexpr bool kShare3 = MODE == 's' && NROT == 4 && ROT0 == 0 && RSTEP == 1;

// pixels from a u8 tile in LDS of pitch SP_; address = LDS address of the centre pixel
template <int SP_, char MODE, int ROT0, int NROT_, int RSTEP>
struct LdsStatic {
    static constexpr int SP = SP_, NROT = NROT_;
    static constexpr bool STATIC = true;
    static constexpr int MINO = min_tile_offset<SP>(MODE, ROT0, NROT, RSTEP);
    template <int I>
    __device__ __forceinline__ static void rotation(PixSet& X, uint32_t base) {
        constexpr Off3 o = tile_offsets<SP>(MODE, ROT0 + I * RSTEP);
        X.b[I] = lds_pixel_hi_off<o.o[0] - MINO>(base);
        X.c[I] = lds_pixel_hi_off<o.o[1] - MINO>(base);
        X.d[I] = lds_pixel_hi_off<o.o[2] - MINO>(base);
    }
    template <int I>
    __device__ __forceinline__ static uint32_t& block3(PixSet& X) { return pix_slot<block3_slot<SP>(I)>(X); }
    template <int I>
    __device__ __forceinline__ static void read_block3(PixSet& X, uint32_t base) { block3<I>(X) = lds_pixel_hi_off<block3_offset<SP>(I) - MINO>(base); }
    __device__ __forceinline__ void issue(PixSet& X, uint32_t center) const {
        const uint32_t base = center + (uint32_t)MINO;
        X.a = lds_pixel_hi_off<-MINO>(base);
        if constexpr (kShare3<MODE, ROT0, NROT, RSTEP>) {
            read_block3<0>(X, base); read_block3<1>(X, base); read_block3<2>(X, base); read_block3<3>(X, base);
            read_block3<4>(X, base); read_block3<5>(X, base); read_block3<6>(X, base); read_block3<7>(X, base);
        } else {
            rotation<0>(X, base);
            rotation<1>(X, base);
            if constexpr (NROT == 4) {
                rotation<2>(X, base);
                rotation<3>(X, base);
            }
        }
    }
    __device__ __forceinline__ void ready(PixSet& X) const {
        if constexpr (kShare3<MODE, ROT0, NROT, RSTEP>)
            wait_block3<Wait::LDS>(X, block3<0>(X), block3<1>(X), block3<2>(X), block3<3>(X), block3<4>(X), block3<5>(X), block3<6>(X), block3<7>(X));
        else
            wait_pixels<Wait::LDS, NROT>(X);
    }
};
// o[3 i .. 3 i + 2] = byte offsets of pixels b, c, d of rotation i in the tile
template <int SP_, int NROT_>
struct LdsRt {
    static constexpr int SP = SP_, NROT = NROT_;
    static constexpr bool STATIC = false;
    const int* __restrict__ o;
    __device__ __forceinline__ void issue(PixSet& X, uint32_t center) const {
        X.a = lds_pixel_hi(center);
#pragma unroll
        for (int i = 0; i < NROT; ++i) {
            X.b[i] = lds_pixel_hi(center + (uint32_t)o[3 * i]);
            X.c[i] = lds_pixel_hi(center + (uint32_t)o[3 * i + 1]);
            X.d[i] = lds_pixel_hi(center + (uint32_t)o[3 * i + 2]);
        }
    }
    __device__ __forceinline__ void ready(PixSet& X) const { wait_pixels<Wait::LDS, NROT>(X); }
};

// pixels of an INTERIOR region from the frame (stage 1: the input, stage 2 of LeRF-L: the stage-1 output); origin = address of
// the region's first centre pixel, pitch = bytes per frame row, address = voff(row, byte in the row) of the position
template <int IMM>
__device__ __forceinline__ uint32_t gl_pixel_hi(uint32_t voff, uint64_t rowbase) {
    uint32_t r;
    asm volatile("global_load_ubyte_d16_hi %0, %1, %2 offset:%3" : "=v"(r) : "v"(voff), "s"(rowbase), "n"(IMM));
    return r;
}
__device__ __forceinline__ uint32_t gl_pixel_hi_rt(uint32_t voff, uint64_t origin) {
    uint32_t r;
    asm volatile("global_load_ubyte_d16_hi %0, %1, %2" : "=v"(r) : "v"(voff), "s"(origin));
    return r;
}
// addresses cost nothing: row base (one SGPR pair per dy in -3..3) + the position's byte offset (one VGPR) + dx * CH (immediate)
template <char MODE, int ROT0, int NROT_, int RSTEP>
struct VmemStatic {
    static constexpr int NROT = NROT_;
    uint64_t rows[7];             // rows[dy + 3] = address of the region's first centre pixel, dy rows away
    int pitch;
    __device__ __forceinline__ VmemStatic(const uint8_t* __restrict__ origin, int pitch_) : pitch(pitch_) {
#pragma unroll
        for (int dy = -3; dy <= 3; ++dy) rows[dy + 3] = (uint64_t)reinterpret_cast<uintptr_t>(origin + (int64_t)dy * pitch);
    }
    __device__ __forceinline__ uint32_t voff(int ry, int rb) const { return (uint32_t)(ry * pitch + rb); }
    template <int I, int K>       // pixel K (0..2 = b, c, d) of rotation I
    __device__ __forceinline__ uint32_t pixel(uint32_t at) const {
        constexpr DyDx q = pattern_dydx(MODE, ROT0 + I * RSTEP);
        return gl_pixel_hi<q.dx[K] * CH>(at, rows[q.dy[K] + 3]);
    }
    template <int I>
    __device__ __forceinline__ void rotation(PixSet& X, uint32_t at) const {
        X.b[I] = pixel<I, 0>(at); X.c[I] = pixel<I, 1>(at); X.d[I] = pixel<I, 2>(at);
    }
    __device__ __forceinline__ void issue(PixSet& X, uint32_t at) const {
        X.a = gl_pixel_hi<0>(at, rows[3]);
        if constexpr (kShare3<MODE, ROT0, NROT, RSTEP>) {
            X.b[0] = pixel<0, 0>(at); X.b[1] = pixel<1, 0>(at); X.b[2] = pixel<2, 0>(at); X.b[3] = pixel<3, 0>(at);
            X.d[0] = pixel<0, 2>(at); X.d[1] = pixel<1, 2>(at); X.d[2] = pixel<2, 2>(at); X.d[3] = pixel<3, 2>(at);
        } else {
            rotation<0>(X, at);
            rotation<1>(X, at);
            if constexpr (NROT == 4) {
                rotation<2>(X, at);
                rotation<3>(X, at);
            }
        }
    }
    __device__ __forceinline__ void ready(PixSet& X) const {
        if constexpr (kShare3<MODE, ROT0, NROT, RSTEP>)
            wait_block3<Wait::VMEM>(X, X.b[0], X.b[1], X.b[2], X.b[3], X.d[0], X.d[1], X.d[2], X.d[3]);
        else
            wait_pixels<Wait::VMEM, NROT>(X);
    }
};
// dyx[3 i + k] = (dy << 16) | (dx & 0xFFFF) of pixel k + 1 of rotation i (frame coordinates); a pixel's address = base +
// (position offset + dy * pitch + dx * CH)
template <int NROT_>
struct VmemRt {
    static constexpr int NROT = NROT_;
    // the VGPR offset of a global load is UNSIGNED: the base is moved up-left by the largest pattern reach (3 rows, 3 pixels;
    // inside the frame for an interior region) so that every pixel offset is non-negative
    int pitch, reach;
    uint64_t org;
    int off[NROT * 3];
    __device__ __forceinline__ VmemRt(const uint8_t* __restrict__ origin, int pitch_, const int* __restrict__ dyx)
        : pitch(pitch_), reach(3 * pitch_ + 3 * CH), org((uint64_t)reinterpret_cast<uintptr_t>(origin - (3 * pitch_ + 3 * CH))) {
#pragma unroll
        for (int i = 0; i < NROT * 3; ++i) off[i] = (dyx[i] >> 16) * pitch + (int)(int16_t)(dyx[i] & 0xFFFF) * CH;
    }
    __device__ __forceinline__ uint32_t voff(int ry, int rb) const { return (uint32_t)(ry * pitch + rb + reach); }
    __device__ __forceinline__ void issue(PixSet& X, uint32_t at) const {
        X.a = gl_pixel_hi_rt(at, org);
#pragma unroll
        for (int i = 0; i < NROT; ++i) {
            X.b[i] = gl_pixel_hi_rt(at + (uint32_t)off[3 * i], org);
            X.c[i] = gl_pixel_hi_rt(at + (uint32_t)off[3 * i + 1], org);
            X.d[i] = gl_pixel_hi_rt(at + (uint32_t)off[3 * i + 2], org);
        }
    }
    __device__ __forceinline__ void ready(PixSet& X) const { wait_pixels<Wait::VMEM, NROT>(X); }
};

// the lookups of one position, all its pixels read and waited for at once; lut_a = LDS address of the LUT
template <typename Src>
__device__ __forceinline__ int byte_lookups(const Src& src, uint32_t lut_a, uint32_t center) {
    PixSet X;
    src.issue(X, center);
    src.ready(X);
    return byte_walks<Src::NROT>(lut_a, X.a, X.b, X.c, X.d);
}

// position p of a region (pitch DPc px-ch per row, origin (y0g,x0g) in the frame) ->
// byte address of its clamped centre in the source tile (pitch SP, origin (sy0g,sx0g))
template <int DPc, int SP>
__device__ __forceinline__ int center_addr(int p, int y0g, int x0g, int sy0g, int sx0g, int H, int W, bool* inside) {
    int ry = p / DPc;
    int r3 = p - ry * DPc;
    if (H < 0) {                      // interior tile (caller passes H = -1): nothing to clamp
        if (inside) *inside = true;
        return (ry + (y0g - sy0g)) * SP + r3 + (x0g - sx0g) * CH;
    }
    int rx = r3 / CH;
    int c = r3 - rx * CH;
    int gy = y0g + ry, gx = x0g + rx;
    int cy = clampi(gy, 0, H - 1), cx = clampi(gx, 0, W - 1);
    if (inside) *inside = (cy == gy) && (cx == gx);
    return (cy - sy0g) * SP + (cx - sx0g) * CH + c;
}

template <typename Src, typename Kind>
__device__ __forceinline__ void byte_position(const Src& src, Kind kind, uint32_t lut_a, uint32_t center, int16_t* acc16, uint8_t* dst8, int p,
                                              int div, int bias) {
    phase_finish(kind, byte_lookups(src, lut_a, center), acc16, dst8, p, div, bias);
}
// One phase over a region (origin (y0g, x0g) in the frame) whose centres lie in the LDS tile `tile` (pitch Src::SP, origin
// (sy0g, sx0g)).  SKIP_OUTSIDE: positions outside the frame are not evaluated (callers that never read them: s1_kernel).
// Interior tiles (H < 0, a workgroup-uniform fact) take a loop of their own: no clamping or frame tests, instead of a
// per-position interior branch and an inside-the-frame mask; with a static source also a scalar trip count (whole rounds + a
// masked tail) instead of a vector loop condition -- the loop shape each kind of kernel has been measured with.
template <int NDST, int DPc, bool SKIP_OUTSIDE = false, typename Src, typename Kind>
__device__ __forceinline__ void byte_phase_lds(const Src& src, Kind kind, const int8_t* lut, const uint8_t* tile, int16_t* acc16, uint8_t* dst8,
                                               int y0g, int x0g, int sy0g, int sx0g, int H, int W, int div, int bias, int tid) {
    constexpr int SP = Src::SP;
    const uint32_t lut_a = lds_addr(lut), src_a = lds_addr(tile);
    if (H < 0) {
        const uint32_t org = src_a + (uint32_t)((y0g - sy0g) * SP + (x0g - sx0g) * CH);
        if constexpr (Src::STATIC) {
            constexpr int FULL = NDST / NT, TAIL = NDST - FULL * NT;
#pragma unroll 1
            for (int k = 0; k < FULL; ++k) {
                const int p = tid + k * NT;
                const int ry = p / DPc;
                byte_position(src, kind, lut_a, org + (uint32_t)(ry * (SP - DPc) + p), acc16, dst8, p, div, bias);
            }
            if (TAIL > 0 && tid < TAIL) {
                const int p = tid + FULL * NT;
                const int ry = p / DPc;
                byte_position(src, kind, lut_a, org + (uint32_t)(ry * (SP - DPc) + p), acc16, dst8, p, div, bias);
            }
        } else {
#pragma unroll 1
            for (int p = tid; p < NDST; p += NT) {
                const int ry = p / DPc;
                byte_position(src, kind, lut_a, org + (uint32_t)(ry * (SP - DPc) + p), acc16, dst8, p, div, bias);
            }
        }
        return;
    }
#pragma unroll 1
    for (int p = tid; p < NDST; p += NT) {
        bool in = true;
        int a = center_addr<DPc, SP>(p, y0g, x0g, sy0g, sx0g, H, W, SKIP_OUTSIDE ? &in : nullptr);
        if (SKIP_OUTSIDE && !in) continue;
        byte_position(src, kind, lut_a, src_a + (uint32_t)a, acc16, dst8, p, div, bias);
    }
}
// One phase over an INTERIOR region with a vector-memory source, two positions deep: the pixels of the next position are in
// flight under the lookups of this one.  Threads past the last position of the final round repeat it (loads only).
template <int NDST, int DPc, typename Src, typename Kind>
__device__ __forceinline__ void byte_phase_vmem(const Src& src, Kind kind, const int8_t* lut, int16_t* acc16, uint8_t* dst8, int div, int bias,
                                                int tid) {
    constexpr int ROUNDS = (NDST + NT - 1) / NT, PAIRS = (ROUNDS + 1) / 2;
    const uint32_t lut_a = lds_addr(lut);
    auto issue = [&](PixSet& X, int p) {
        p = p < NDST ? p : NDST - 1;
        const int ry = p / DPc;
        src.issue(X, src.voff(ry, p - ry * DPc));
    };
    auto finish = [&](const PixSet& X, int p) {
        if (NDST % NT != 0 && p >= NDST) return;
        phase_finish(kind, byte_walks<Src::NROT>(lut_a, X.a, X.b, X.c, X.d), acc16, dst8, p, div, bias);
    };
    PixSet A, B;
    issue(A, tid);
#pragma unroll 1
    for (int k = 0; k < PAIRS; ++k) {
        const int p = tid + 2 * k * NT;
        src.ready(A);
        issue(B, p + NT);
        finish(A, p);
        src.ready(B);
        if (k + 1 < PAIRS) issue(A, p + 2 * NT);
        if (2 * k + 1 < ROUNDS) finish(B, p + NT);
    }
}

// ---------------------------------------------------------------------------
// The byte-LUT phase chain (stage 1, stage 2 of LeRF-L): LUT i + 1 rides in registers behind the lookups of LUT i, so that
// only the LDS store of a LUT, not its L2 round trip, stands between two phases.  The chain is
//   first LUT -> LDS, barrier;  per phase: load next, run, barrier, store next, barrier.
// The registers are six named uint4 handed on by reference: an array or a struct that lives across the position loop
// ends up in scratch (a struct with load() / store() methods: 96 bytes of it in every kernel that runs stage 1).
// `pack` = the chain's first LUT, the others follow at LUT_PAD; `body` runs one phase; `mark(k)` is called behind every
// barrier (k = 0: the first LUT has landed, 1 + 2 i: phase i is done, 2 + 2 i: LUT i + 1 has landed) for what a kernel hangs
// there: its stamps, work that hides under the first phase.
// ---------------------------------------------------------------------------
constexpr int LUT_U4 = (LERF_LUT_ENTRIES + 15) / 16, LUT_U4_TAIL = LUT_U4 - 5 * NT;
static_assert(LUT_U4_TAIL > 0 && LUT_U4_TAIL <= NT, "byte LUT = 5 full uint4 rounds + a tail");
__device__ __forceinline__ void lut_regs_load(const uint8_t* __restrict__ src, int tid, uint4& n0, uint4& n1, uint4& n2, uint4& n3,
                                              uint4& n4, uint4& n5) {
    const uint4* s_ = reinterpret_cast<const uint4*>(src);
    n0 = s_[tid]; n1 = s_[tid + NT]; n2 = s_[tid + 2 * NT]; n3 = s_[tid + 3 * NT]; n4 = s_[tid + 4 * NT];
    if (tid < LUT_U4_TAIL) n5 = s_[tid + 5 * NT];
}
__device__ __forceinline__ void lut_regs_store(uint8_t* lut, int tid, const uint4& n0, const uint4& n1, const uint4& n2, const uint4& n3,
                                               const uint4& n4, const uint4& n5) {
    uint4* d_ = reinterpret_cast<uint4*>(lut);
    d_[tid] = n0; d_[tid + NT] = n1; d_[tid + 2 * NT] = n2; d_[tid + 3 * NT] = n3; d_[tid + 4 * NT] = n4;
    if (tid < LUT_U4_TAIL) d_[tid + 5 * NT] = n5;
}
struct NoMark { __device__ __forceinline__ void operator()(int) const {} };
template <int I, int N, typename Body, typename Mark>
__device__ __forceinline__ void lut_chain_step(uint8_t* lut, const uint8_t* __restrict__ pack, int tid, uint4& n0, uint4& n1, uint4& n2,
                                               uint4& n3, uint4& n4, uint4& n5, Body& body, Mark& mark) {
    if constexpr (I + 1 < N) lut_regs_load(pack + (I + 1) * LUT_PAD, tid, n0, n1, n2, n3, n4, n5);
    body(std::integral_constant<int, I>{});
    __syncthreads();
    mark(1 + 2 * I);
    if constexpr (I + 1 < N) {
        lut_regs_store(lut, tid, n0, n1, n2, n3, n4, n5);
        __syncthreads();
        mark(2 + 2 * I);
        lut_chain_step<I + 1, N>(lut, pack, tid, n0, n1, n2, n3, n4, n5, body, mark);
    }
}
// N phases known at compile time: body(std::integral_constant<int, i>) runs phase i
template <int N, typename Body, typename Mark>
__device__ __forceinline__ void lut_chain(uint8_t* lut, const uint8_t* __restrict__ pack, int tid, Body body, Mark mark) {
    uint4 n0, n1, n2, n3, n4, n5 = make_uint4(0, 0, 0, 0);
    copy16<LERF_LUT_ENTRIES>(lut, pack, tid);
    __syncthreads();
    mark(0);
    lut_chain_step<0, N>(lut, pack, tid, n0, n1, n2, n3, n4, n5, body, mark);
}
// n phases at run time (general kernels): body(i, more) runs phase i, more = another one follows
template <typename Body, typename Mark>
__device__ __forceinline__ void lut_chain_rt(uint8_t* lut, const uint8_t* __restrict__ pack, int n, int tid, Body body, Mark mark) {
    uint4 n0, n1, n2, n3, n4, n5 = make_uint4(0, 0, 0, 0);
    copy16<LERF_LUT_ENTRIES>(lut, pack, tid);
    __syncthreads();
    mark(0);
#pragma unroll 1
    for (int i = 0; i < n; ++i) {
        const bool more = i + 1 < n;
        if (more) lut_regs_load(pack + (size_t)(i + 1) * LUT_PAD, tid, n0, n1, n2, n3, n4, n5);
        body(i, more);
        __syncthreads();
        if (more) {
            lut_regs_store(lut, tid, n0, n1, n2, n3, n4, n5);
            __syncthreads();
        }
    }
}
constexpr char kSctModes[3] = {'s', 'c', 't'};         // the published configuration's sampling patterns, in LUT order

// ---------------------------------------------------------------------------
// stage 3 helpers
// ---------------------------------------------------------------------------
// first i in [0,n) with a[i] >= key (a is non-decreasing), all 64 lanes of a wave cooperating:
// 64-way splits, so a table of 8k entries needs three dependent loads instead of thirteen
__device__ __forceinline__ int wave_lower_bound(const int* __restrict__ a, int n, int key, int lane) {
    int lo = 0, hi = n;
    while (hi - lo > 64) {
        const int step = (hi - lo + 63) >> 6;
        const int idx = lo + lane * step;
        const bool less = idx < hi && a[idx] < key;
        const int cnt = __popcll(__ballot(less));          // monotone: the first cnt probes are < key
        const int nlo = cnt > 0 ? lo + (cnt - 1) * step + 1 : lo;
        const int nhi = cnt < 64 ? min(hi, lo + cnt * step) : hi;
        lo = nlo;
        hi = nhi;
    }
    const int idx = lo + lane;
    const bool less = idx < hi && a[idx] < key;
    return lo + __popcll(__ballot(less));
}


// ---- input tile -> LDS.  Interior tiles whose rows all start at the same offset from a 4-byte boundary (frame pitch
//      and frame stride multiples of 4: every RGB frame whose width is a multiple of 4) are fetched as aligned dwords
//      and land in LDS with that offset as a phase (returned); the other tiles go byte by byte with clamped
//      coordinates (np.pad(..., 'edge') in every rotated frame).  Every load of a thread is issued before its first
//      LDS store (one L2/HBM latency); `between()` runs while the loads are in flight.
template <int IY, int IPB, int IP, typename F>
__device__ __forceinline__ int load_input_tile(uint8_t* Ct, const uint8_t* __restrict__ img, int H, int W, int iy0,
                                               int ix0, bool interior, int tid, F between) {
    int cphase = 0;
    const int64_t row0 = ((int64_t)iy0 * W + ix0) * CH;                     // first byte of the region in the frame
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(img) + (uintptr_t)row0;
    const bool dwords = interior && ((W * CH) & 3) == 0 && (reinterpret_cast<uintptr_t>(img) & 3) == 0 &&
                        (iy0 + IY < H || (ix0 * CH - (int)(a0 & 3)) + IP <= W * CH);   // never read past the frame
    if (dwords) {
        cphase = (int)(a0 & 3);
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a0 - (uintptr_t)cphase);
        constexpr int RD = IP / 4, ND = IY * RD, KD = (ND + NT - 1) / NT;
        const int rowdw = (W * CH) >> 2;
        uint32_t v[KD];
#pragma unroll
        for (int k = 0; k < KD; ++k) {
            const int p = min(tid + k * NT, ND - 1);
            const int ry = p / RD;
            v[k] = __builtin_nontemporal_load(&src[(int64_t)ry * rowdw + (p - ry * RD)]);   // read once: leave the L2 to the LUT pack
        }
        between();
#pragma unroll
        for (int k = 0; k < KD; ++k) {
            const int p = tid + k * NT;
            if (p < ND) reinterpret_cast<uint32_t*>(Ct)[p] = v[k];
        }
    } else {
        constexpr int NB = IY * IPB, KI = (NB + NT - 1) / NT;
        uint8_t v[KI];
#pragma unroll
        for (int k = 0; k < KI; ++k) {
            const int p = min(tid + k * NT, NB - 1);
            int ry = p / IPB;
            int r3 = p - ry * IPB;
            int rx = r3 / CH;
            int c = r3 - rx * CH;
            int gy = clampi(iy0 + ry, 0, H - 1), gx = clampi(ix0 + rx, 0, W - 1);
            v[k] = img[((int64_t)gy * W + gx) * CH + c];
        }
        between();
#pragma unroll
        for (int k = 0; k < KI; ++k) {
            const int p = tid + k * NT;
            if (p < NB) {
                const int ry = p / IPB;
                Ct[ry * IP + (p - ry * IPB)] = v[k];
            }
        }
    }
    return cphase;
}

// Workgroups are dealt to the 8 XCDs round-robin (workgroup i runs on XCD i % 8; an affinity, not a guarantee -- nothing
// depends on it but speed).  Handing every XCD a CONTIGUOUS eighth of the (frame, tile) sequence instead of every eighth tile
// keeps the tiles that run side by side on one XCD neighbours in the frame: their input / feat halos and the LUT pieces
// they ask for at the same time meet in that XCD's own L2.  Measured: L2 hit rate 94.8 -> 97.5 %, HBM fetch of the two launches
// 169 -> 73 MB per step, +1.3 % throughput.  A bijection of [0, total) for any total.
// Small launches (under four rounds of workgroups) keep the linear order: their cheap partial tiles at the end of the
// sequence would all land on the last XCD (a 300-tile strip launch took 0.35 instead of 0.27 ms).
__device__ __forceinline__ int xcd_order(int b, int total) {
    if (total < 1024) return b;
    const int x = b & 7, j = b >> 3, q = total >> 3, r = total & 7;
    return x * q + (x < r ? x : r) + j;
}

// ---------------------------------------------------------------------------
// the kernel
// ---------------------------------------------------------------------------
// EMIT = false: the whole SR path.  EMIT = true: stages 1+2 only; the tile's own 64x64 block of
// (hq0,hq1,hq2,feat) dwords goes to P.emit ([H][W][3] uint32) for the warp kernels / the stage API.
// FROM_FEAT = true: stage 1 has been run by s1_kernel over the whole batch; the feat tile (with its halo) is read
// from P.feat instead of being recomputed from the input tile -- stage 1 then costs 64x64 instead of 72x72 positions
// per tile (-21 % of its work) for 6 bytes of extra HBM traffic per LR pixel.
// GEN = true: the general kernels -- any 1..4 sampling patterns per stage (run-time neighbour offsets), scale factors up to
// x8 (large geometry tables, staged late), frames of different sizes in one launch (RaggedTable).  GEN = false: the
// specialised kernels of the published configuration (modes "sct" / "sct", scale < 4.9, one frame size).
// What a workgroup needs to know about ITS frame, as plain values (never a modified copy of the kernel arguments: a
// 600-byte struct that is written through a reference ends up in scratch memory and every later P.x becomes a scratch load --
// the first version of the general kernels ran at half speed for that reason).
struct FrameView {
    const uint8_t* img; uint8_t* out; uint8_t* feat; uint32_t* emit;
    const int* left_r; const float* dis_r; const int* left_c; const float* dis_c;
    const double* dis_r64; const double* dis_c64;
    int H, W, oH, oW, tiles_x, tiles_y;
};
template <bool GEN>
__device__ __forceinline__ FrameView frame_view(const Params& P, const std::conditional_t<GEN, RaggedTable, NoTable>& T, int& bid) {
    FrameView F;
    if constexpr (GEN) {
        if (T.n > 0) {
            int f = 0;
            for (int k = 1; k < T.n; ++k)
                if (bid >= T.d[k].first_block) f = k;
            bid -= T.d[f].first_block;
            F.img = T.d[f].img; F.out = T.d[f].out; F.feat = T.d[f].feat; F.emit = T.d[f].emit;
            F.left_r = T.d[f].left_r; F.dis_r = T.d[f].dis_r; F.left_c = T.d[f].left_c; F.dis_c = T.d[f].dis_c;
            F.dis_r64 = T.d[f].dis_r64; F.dis_c64 = T.d[f].dis_c64;
            F.H = T.d[f].H; F.W = T.d[f].W; F.oH = T.d[f].oH; F.oW = T.d[f].oW;
            F.tiles_x = T.d[f].tiles_x; F.tiles_y = T.d[f].tiles_y;
            return F;
        }
    }
    const int tiles = P.tiles_y * P.tiles_x;
    const int frame = bid / tiles;
    bid -= frame * tiles;
    F.img = P.img + frame * P.in_sn; F.out = P.out + frame * P.out_sn;
    F.feat = P.feat + frame * P.feat_sn; F.emit = P.emit + frame * P.emit_sn;
    F.left_r = P.left_r; F.dis_r = P.dis_r; F.left_c = P.left_c; F.dis_c = P.dis_c;
    F.dis_r64 = P.dis_r64; F.dis_c64 = P.dis_c64;
    F.H = P.H; F.W = P.W; F.oH = P.oH; F.oW = P.oW; F.tiles_x = P.tiles_x; F.tiles_y = P.tiles_y;
    return F;
}

// The warp of one source tile (tile-fused warp, lerf_warp_fused_u8): every output pixel of the tile's box is projected (float64,
// Warp2dNumpy's operation order) and kept when this tile owns it (host::warp_owner_key: last tap row / column inside the tile);
// its 2 x 2 taps are packed dwords (hq0 | hq1 << 8 | hq2 << 16 | feat << 24) of the tile's stage-2 region Dt (origin
// (hy0, hx0), pitch HP dwords) -- the per-pixel arithmetic is warp_px_value_u8, the packed warp kernel's own.
template <int KIND, int HP>
__device__ __forceinline__ void warp_tile(const Params& P, const uint32_t* Dt, int hy0, int hx0, int ty0, int tx0, int H, int W, int tile,
                                          uint8_t* __restrict__ outp, int tid) {
    const WarpGeo& g = P.wgeo;
    const int i0 = P.wboxes[4 * tile], i1 = P.wboxes[4 * tile + 1], j0 = P.wboxes[4 * tile + 2], j1 = P.wboxes[4 * tile + 3];
    const int bw = j1 - j0, n = (i1 - i0) * bw;
    if (n <= 0) return;
    const float gsc = KIND == LERF_KIND_GAUSS ? s3::gauss_scale(P.max_sigma) : 1.0f;
    const unsigned inv_bw = (unsigned)((0xFFFFFFFFull / (unsigned)bw) + 1ull);          // q / bw for q < 2^26 (checked by the launcher)
    for (int q = tid; q < n; q += NT) {
        int di = (int)__umulhi((unsigned)q, inv_bw);
        int dj = q - di * bw;
        if (dj < 0) { --di; dj += bw; } else if (dj >= bw) { ++di; dj -= bw; }
        const int i = i0 + di, j = j0 + dj;
        const WarpPx2 G = warp_px_geometry(g, i, j, H, W);
        const int kr = min(G.rrow[0] + 1, H - 1), kc = min(G.rcol[0] + 1, W - 1);
        if (kr < ty0 || kr >= ty0 + TH || kc < tx0 || kc >= tx0 + TW) continue;
        const float dxs[2] = {G.dx[0] * gsc, G.dx[1] * gsc}, dys[2] = {G.dy[0] * gsc, G.dy[1] * gsc};
        uint8_t* dst = outp + ((int64_t)i * g.oW + j) * CH;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            auto tap = [&](int r, int cc) -> uint32_t { return Dt[(r - hy0) * HP + (cc - hx0) * CH + c]; };
            float res;
            if (warp_px_value_u8<KIND>(G, g, H, W, P.max_sigma, dxs, dys, tap, dst + c, &res)) continue;
            dst[c] = s3::to_u8(res);
        }
    }
}

// ---------------------------------------------------------------------------
// The stages of the kernels up to the hyper region's packed dwords, in the order a workgroup runs them.  Each takes what it
// needs of the tile as plain values (region origins in frame coordinates, LDS pointers) and is inlined into its kernel.
// ---------------------------------------------------------------------------
// ---- input tile (load_input_tile; `between()` rides behind its loads) and stage 1: the byte LUTs of the stage, 4 rotations
//      each (eval_lut_sr.py:541-577), from the region at (fy0, fx0) of D::FY x D::FX pixels into dst8.  mark: see lut_chain.
//      VMEM: interior tiles of device frames read their neighbourhood pixels over the vector-memory path (byte_phase_vmem;
//      the specialised kernel then needs no input tile in LDS at all).  s1_kernel does; in sr_fused_kernel -- 72 x 72
//      positions per tile -- it did not pay: 0.191 vs 0.184 ms per 1080 x 960 block; that kernel's stage 1 shares the CU
//      with nothing else that uses the LDS less.  Pinned host frames (stream.StreamingSR) cross PCIe uncached: never.
//      SKIP_OUTSIDE: see byte_phase_lds.
template <typename D, bool GEN, bool SKIP_OUTSIDE, bool VMEM, typename Between, typename Mark>
__device__ __forceinline__ void stage1(uint8_t* smem, const Params& P, const uint8_t* __restrict__ img, int H, int W, int fy0, int fx0,
                                       bool interior, uint8_t* dst8, int tid, Between between, Mark mark) {
    const int iy0 = fy0 - R1, ix0 = fx0 - R1;
    const int Hc = interior ? -1 : H, Wc = W;
    uint8_t* lut8 = smem + D::OFF_LUT;
    int8_t* lut = reinterpret_cast<int8_t*>(lut8);
    int16_t* acc = reinterpret_cast<int16_t*>(smem + D::OFF_ACC);
    const int div1 = kQ * 3;
    const bool vmem = VMEM && interior && !P.host_input;
    const uint8_t* vorg = img + ((int64_t)fy0 * W + fx0) * CH;
    const int pitch = W * CH;
    if (!GEN && vmem) {
        lut_chain<3>(lut8, P.pack, tid, [&](auto I) {
            constexpr int i = decltype(I)::value;
            byte_phase_vmem<D::NF, D::FP>(VmemStatic<kSctModes[i], 0, 4, 1>(vorg, pitch), PhaseIs<i>{}, lut, acc, dst8, div1, 0, tid);
        }, mark);
        return;
    }
    const int cphase = load_input_tile<D::IY, D::IPB, D::IP>(smem + D::OFF_C, img, H, W, iy0, ix0, interior, tid, between);
    const uint8_t* Ct = smem + D::OFF_C + cphase;
    if constexpr (GEN) {
        // any 1..4 patterns: the same phases with run-time offsets (lerf_luts_t.modes1 order)
        const int dv = kQ * P.n1;
        lut_chain_rt(lut8, P.pack, P.n1, tid, [&](int m, bool more) {
            const int *dyx = P.s1dyx[m], *off = P.s1off[m];
            const PhaseRt kind{m == 0, !more};
            if (vmem) byte_phase_vmem<D::NF, D::FP>(VmemRt<4>(vorg, pitch, dyx), kind, lut, acc, dst8, dv, 0, tid);
            else byte_phase_lds<D::NF, D::FP, SKIP_OUTSIDE>(LdsRt<D::IP, 4>{off}, kind, lut, Ct, acc, dst8, fy0, fx0, iy0, ix0, Hc, Wc, dv, 0, tid);
        }, mark);
    } else {
        lut_chain<3>(lut8, P.pack, tid, [&](auto I) {
            constexpr int i = decltype(I)::value;
            byte_phase_lds<D::NF, D::FP, SKIP_OUTSIDE>(LdsStatic<D::IP, kSctModes[i], 0, 4, 1>{}, PhaseIs<i>{}, lut, Ct, acc, dst8, fy0, fx0, iy0, ix0, Hc, Wc,
                                                       div1, 0, tid);
        }, mark);
    }
}

// ---- feat tile (with its halo) from the stage-1 launch -> Bt; out-of-frame positions take the clamped pixel, which is
//      what stage 1 evaluates for them.  `between()` rides behind the loads
template <typename D, typename Between>
__device__ __forceinline__ void load_feat_tile(uint8_t* Bt, const uint8_t* feat, int H, int W, int fy0, int fx0, bool interior, int tid,
                                               Between between) {
    const uint8_t* __restrict__ fsrc = feat;
    const bool dwords = interior && (D::FP & 3) == 0 && ((W * CH) & 3) == 0 && (reinterpret_cast<uintptr_t>(feat) & 3) == 0 && ((fx0 * CH) & 3) == 0;
    if (dwords) {
        constexpr int RD = D::FP / 4, ND = D::FY * RD, KD = (ND + NT - 1) / NT;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(fsrc + ((int64_t)fy0 * W + fx0) * CH);
        const int rowdw = (W * CH) >> 2;
        uint32_t v[KD];
#pragma unroll
        for (int k = 0; k < KD; ++k) {
            const int p = min(tid + k * NT, ND - 1);
            const int ry = p / RD;
            v[k] = __builtin_nontemporal_load(&src[(int64_t)ry * rowdw + (p - ry * RD)]);
        }
        between();
#pragma unroll
        for (int k = 0; k < KD; ++k) {
            const int p = tid + k * NT;
            if (p < ND) reinterpret_cast<uint32_t*>(Bt)[p] = v[k];
        }
    } else {
        constexpr int KI = (D::NF + NT - 1) / NT;
        uint8_t v[KI];
#pragma unroll
        for (int k = 0; k < KI; ++k) {
            const int p = min(tid + k * NT, D::NF - 1);
            const int ry = p / D::FP;
            const int r3 = p - ry * D::FP;
            const int rx = r3 / CH;
            const int gy = clampi(fy0 + ry, 0, H - 1), gx = clampi(fx0 + rx, 0, W - 1);
            v[k] = fsrc[((int64_t)gy * W + gx) * CH + (r3 - rx * CH)];
        }
        between();
#pragma unroll
        for (int k = 0; k < KI; ++k) {
            const int p = tid + k * NT;
            if (p < D::NF) Bt[p] = v[k];
        }
    }
}

// ---- stage 2, LeRF-L: six byte LUTs (mode x rotation parity), 2 rotations each (eval_lut_sr.py:579-628); the hyper
//      region's (alpha_q, 0, 0, feat-or-0) dwords go to Dt.  feat = the frame's stage-1 output (two-launch path)
template <typename D, bool GEN, bool FROM_FEAT, typename Outside>
__device__ __forceinline__ void stage2_linear(uint8_t* smem, const Params& P, const uint8_t* Bt, uint32_t* Dt, const uint8_t* feat, int W,
                                              int hy0, int hx0, int fy0, int fx0, bool interior, int Hc, int Wc, int tid,
                                              Outside outside_pixel) {
    uint8_t* lut8 = smem + D::OFF_LUT;
    int8_t* lut = reinterpret_cast<int8_t*>(lut8);
    int16_t* acc = reinterpret_cast<int16_t*>(smem + D::OFF_ACC);
    uint8_t* hq8 = smem + D::OFF_C;                   // input tile is dead: reuse for the u8 hyper values
    const uint8_t* s2 = P.pack + (size_t)(GEN ? P.n1 : 3) * LUT_PAD;
    // interior tiles of the two-launch path: the seven neighbourhood pixels of a position come from the stage-1 output
    // in HBM/L2 over the vector-memory path, one position ahead (byte_phase_vmem); these phases are LDS-bound like stage 1
    const bool vm2 = FROM_FEAT && interior;
    const uint8_t* forg = FROM_FEAT ? feat + ((int64_t)hy0 * W + hx0) * CH : nullptr;
    const int fpitch = W * CH;
    if constexpr (GEN) {
        // 2 * n2 LUTs (pattern x rotation parity), offsets of the two rotations of LUT l in P.s2off[l]
        const int dv = kQ * 4 * P.n2;
        lut_chain_rt(lut8, s2, 2 * P.n2, tid, [&](int l, bool more) {
            const int *dyx = P.s2dyx[l], *off = P.s2off[l];
            const PhaseRt kind{l == 0, !more};
            if (vm2) byte_phase_vmem<D::NH, D::HP>(VmemRt<2>(forg, fpitch, dyx), kind, lut, acc, hq8, dv, 127, tid);
            else byte_phase_lds<D::NH, D::HP>(LdsRt<D::FP, 2>{off}, kind, lut, Bt, acc, hq8, hy0, hx0, fy0, fx0, Hc, Wc, dv, 127, tid);
        }, NoMark{});
    } else {
        const int div2 = kQ * 12;
        lut_chain<6>(lut8, s2, tid, [&](auto I) {
            constexpr int i = decltype(I)::value, PAR = i & 1, PH = i == 0 ? 0 : (i == 5 ? 2 : 1);
            constexpr char MODE = kSctModes[i >> 1];
            if (vm2) byte_phase_vmem<D::NH, D::HP>(VmemStatic<MODE, PAR, 2, 2>(forg, fpitch), PhaseIs<PH>{}, lut, acc, hq8, div2, 127, tid);
            else byte_phase_lds<D::NH, D::HP>(LdsStatic<D::FP, MODE, PAR, 2, 2>{}, PhaseIs<PH>{}, lut, Bt, acc, hq8, hy0, hx0, fy0, fx0, Hc, Wc, div2, 127, tid);
        }, NoMark{});
    }
    // pack (alpha_q, 0, 0, feat-or-0) dwords for stage 3
    const bool pad_const = P.pad_mode == LERF_PAD_CONSTANT;
    uint32_t tmp[(D::NH + NT - 1) / NT];
#pragma unroll
    for (int k = 0; k < (D::NH + NT - 1) / NT; ++k) {
        int p = k * NT + tid;
        tmp[k] = 0;
        if (p < D::NH) {
            bool inside;
            int a = center_addr<D::HP, D::FP>(p, hy0, hx0, fy0, fx0, Hc, Wc, &inside);
            uint32_t px = 0u;
            if (inside) px = (uint32_t)Bt[a];
            else if (!pad_const) {
                const int ry = p / D::HP, r3 = p - ry * D::HP, rx = r3 / CH;
                px = outside_pixel(hy0 + ry, hx0 + rx, r3 - rx * CH);
            }
            tmp[k] = (uint32_t)hq8[p] | (px << 24);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < (D::NH + NT - 1) / NT; ++k) {
        int p = k * NT + tid;
        if (p < D::NH) Dt[p] = tmp[k];
    }
}

// row of a feat-tile address: a / FP as one 24-bit multiply and a shift, exact for every address of the tile (checked here)
template <typename D>
constexpr bool feat_row_exact(uint32_t m, int sh) {
    for (uint32_t a = 0; a < (uint32_t)D::NF; ++a)
        if ((uint32_t)(((uint64_t)a * m) >> sh) != a / (uint32_t)D::FP || (uint64_t)a * m >> 32 != 0) return false;
    return true;
}
template <typename D>
__device__ __forceinline__ uint32_t feat_row(uint32_t a) {
    constexpr int SH = 25;
    constexpr uint32_t M = ((1u << SH) + D::FP - 1) / D::FP;
    static_assert(M < (1u << 24) && D::NF <= (1 << 24) && feat_row_exact<D>(M, SH), "a * M >> SH == a / FP for a < NF, in 32 bits");
    return (uint32_t)__umul24(a, M) >> SH;      // (the product passes 2^31: an unsigned shift)
}

// The lean binning of stage2_gauss (exact-x2 LeRF-G kernel, interior tile): the bins of the thread's KH positions, 4 bits each
// (3 = not looked up), and its counts of bins (0, 1) and 2 as stage2_gauss packs them
template <typename D>
__device__ __forceinline__ void lean_bins(const uint8_t* Bt, int tid, uint32_t& qlo, uint32_t& qhi, uint32_t& xa, uint32_t& xb) {
    constexpr int KH = (D::NH + NT - 1) / NT;
    // The thread's positions p0 .. p0 + KH - 1 cross at most one row end: the first kw of them lie in row ry0 from column
    // col0 on, the rest in row ry0 + 1 from column 0.  Looked up: rows below HY - 1, columns below (HX - 1) * CH (the ring
    // exclusion of the generic loop; a position past the region's end has a row >= HY): in row ry0 the positions k < kw - CH,
    // and the positions k >= kw where row ry0 + 1 is in.  All KH bytes are read at once, ahead of the arithmetic.
    static_assert(NBIN == 3 && D::HR > 0 && KH <= (D::HX - 1) * CH, "three bins + the mark 3; a ring; one row end per thread");
    static_assert(((NT * KH - 1) / D::HP + D::HO) * D::FP + D::HO * CH + D::HP <= D::NF, "the reads of the last threads stay in the feat tile");
    const int p0 = tid * KH, ry0 = p0 / D::HP, col0 = p0 - ry0 * D::HP;
    const int kw = D::HP - col0;
    const uint32_t ap0 = (uint32_t)((ry0 + D::HO) * D::FP + D::HO * CH + col0), ap1 = ap0 + (uint32_t)(D::FP - D::HP);
    uint32_t v[KH];
#pragma unroll
    for (int k = 0; k < KH; ++k) v[k] = (uint32_t)Bt[(k >= kw ? ap1 : ap0) + (uint32_t)k];
    // which of the KH positions are looked up, once per thread: bit 4 k of a 64-bit mask (the nibble layout of qlo | qhi << 32)
    constexpr unsigned long long ONES = 0x1111111111111111ull, ALL = ONES & ((1ull << (4 * KH)) - 1ull);
    auto below = [&](int n) { return ONES & ((1ull << (4 * min(max(n, 0), KH))) - 1ull); };      // positions k < n
    const int lim = ry0 < D::HY - 1 ? kw - CH : 0, from = ry0 < D::HY - 2 ? kw : KH;
    const unsigned long long in = below(lim) | (ALL & ~below(from));
    // the bin of a value as two carries of ONE multiply-add: (v + 256 - 16 bin_lo(2)) | (v + 256 - 16 bin_lo(1)) << 16 has
    // v >= 16 bin_lo(2) in bit 8 and v >= 16 bin_lo(1) in bit 24; either flag goes to the position's nibble by a shift and an
    // and-or, the nibble's value is their sum, the bin counts are three population counts -- no compare, no select
    constexpr uint32_t CARRY = ((256u - 16u * (uint32_t)bin_lo(1)) << 16) | (256u - 16u * (uint32_t)bin_lo(2));
    uint32_t f1[2] = {0, 0}, f2[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < KH; ++k) {
        const uint32_t w = (uint32_t)__umul24(v[k], 0x10001u) + CARRY;
        const int t = 4 * (k & 7), h = k >> 3;
        f1[h] |= (t <= 24 ? w >> (24 - t) : w << (t - 24)) & (1u << t);
        f2[h] |= (t >= 8 ? w << (t - 8) : w >> (8 - t)) & (1u << t);
    }
    const uint32_t inlo = (uint32_t)in, inhi = (uint32_t)(in >> 32);
    qlo = (f1[0] + f2[0]) | (((uint32_t)ALL & ~inlo) * 3u);
    qhi = (f1[1] + f2[1]) | (((uint32_t)(ALL >> 32) & ~inhi) * 3u);
    const uint32_t n = (uint32_t)(__popc(inlo) + __popc(inhi));
    const uint32_t n1 = (uint32_t)(__popc(f1[0] & inlo) + __popc(f1[1] & inhi)), n2 = (uint32_t)(__popc(f2[0] & inlo) + __popc(f2[1] & inhi));
    xa = (n - n1) | ((n1 - n2) << 16);
    xb = n2;
}

// ---- stage 2, LeRF-G: packed 3-channel LUT pieces, pixels binned by the top-axis level of their centre; the hyper
//      region's (hq0, hq1, hq2, feat) dwords go to Dt.  LEAN: the exact-x2 kernel, whose interior tiles take the lean set-up
template <typename D, bool GEN, bool LEAN = false>
__device__ __forceinline__ void stage2_gauss(uint8_t* smem, const Params& P, const uint8_t* Bt, uint32_t* Dt, int hy0, int hx0, int fy0,
                                             int fx0, int Hc, int Wc, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    constexpr int MAXR = D::MAXR;
    uint16_t* lst = reinterpret_cast<uint16_t*>(smem + D::OFF_LST);
    int* tab = reinterpret_cast<int*>(smem + D::OFF_TAB);                // [wave][bin] counts
    // Counting sort of the hyper-region positions by bin, every bin padded to whole waves: list entry i belongs to
    // slot round i / NT of thread i % NT, so a 64-entry chunk (one wave in one round) never mixes bins.  One barrier:
    // per-thread histograms -> wave scans -> the 16 x 4 wave totals through LDS -> every wave derives its own bases.
    // Positions of the hyper region that lie outside the frame (tiles on the right / bottom edge, the halo ring of edge
    // tiles) are not looked up at all: stage 3 reads them as replicas of the clamped position (edge-padded hyper maps,
    // zero image), which fill_outside() below copies once the in-frame values exist.  A 28-row strip tile or the
    // last tile row of a 1080-row frame then costs what its in-frame part costs.
    // LEAN (the exact-x2 LeRF-G kernel) && an interior tile: the lean set-up.  Nothing of the region lies outside the frame, so
    // the binning walks its KH consecutive positions by one running address, and the lists get their 0xFFFF only where it is
    // needed (the padding tail of each bin; what the read-back loads from the chunks behind the last bin is discarded).  One wave-uniform branch each.
    const bool lean = LEAN && Hc < 0;
    if (!lean)
        for (int i = tid; i < MAXR * NT / 2; i += NT) reinterpret_cast<uint32_t*>(lst)[i] = 0xFFFFFFFFu;
    constexpr int KH = (D::NH + NT - 1) / NT;
    static_assert(KH <= 15 && NBIN <= 4 && NW == 16, "nibble counts, one byte field per bin, one lane per (wave, bin)");
    uint32_t qlo = 0, qhi = 0;              // 4 bits per owned position p = tid * KH + k: its bin, >= NBIN = not looked up (thread-major lists = position order)
    uint32_t xa, xb;                        // per-thread counts of bins (0, 1) and (2, 3), two 16-bit fields per register
    if (lean) {
        if constexpr (LEAN) lean_bins<D>(Bt, tid, qlo, qhi, xa, xb);
    } else {
        uint32_t hist = 0;                  // one byte per bin
#pragma unroll
        for (int k = 0; k < KH; ++k) {
            const int p = tid * KH + k;
            uint32_t q = 15;
            if (p < D::NH) {
                bool in = true;
                const int a = center_addr<D::HP, D::FP>(p, hy0, hx0, fy0, fx0, Hc, Wc, &in);
                // The last row and the last column of the hyper region are never read by an owned output: a tile owns the
                // outputs whose first tap lies in [t0 - S/2, t0 + T - S/2), so their taps end at t0 + T + S/2 - 2, one short of
                // the region's end (the frame's own trailing outputs reach it -- as out-of-frame positions, which fill_outside()
                // supplies).  Not looked up: 3 % of the positions (66 x 66 -> 65 x 65), 13 slot rounds instead of 14.
                if (D::HR > 0) {
                    const int ry = p / D::HP, r3 = p - ry * D::HP;
                    if (ry == D::HY - 1 || r3 >= (D::HX - 1) * CH) in = false;
                }
                if (in) q = bin_of_level((uint32_t)Bt[a] >> 4);
            }
            if (k < 8) qlo |= q << (4 * k); else qhi |= q << (4 * (k - 8));
            hist += q < NBIN ? 1u << (8 * q) : 0u;
        }
        xa = (hist & 0xFFu) | ((hist << 8) & 0xFF0000u);
        xb = ((hist >> 16) & 0xFFu) | ((hist >> 8) & 0xFF0000u);
    }
    // wave-inclusive scans of the packed count pairs (row shifts + the two row broadcasts of the DPP unit)
    auto wave_scan = [](uint32_t v) {
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);     // row_shr:1
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);     // row_shr:2
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);     // row_shr:4
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);     // row_shr:8
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);     // row_bcast:15
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);     // row_bcast:31
        return v;
    };
    const uint32_t ia = wave_scan(xa), ib = wave_scan(xb);
    if (lane == 63) {
        int* t = tab + wave * 4;
        t[0] = (int)(ia & 0xFFFFu); t[1] = (int)(ia >> 16); t[2] = (int)(ib & 0xFFFFu); t[3] = (int)(ib >> 16);
    }
    __syncthreads();
    // Every wave turns the 16 x 4 wave counts into what it needs itself (lane = w * 4 + b), in registers: the list base
    // of each of its own bins, and -- the same in all waves -- each bin's first chunk and one past its last (a byte
    // each) and the set of non-empty bins.  No second barrier, no table to read back.
    uint32_t ne_bins, cs_pack, ce_pack;          // wave-uniform
    uint32_t cur01, cur23;                       // this thread's list cursors, two 16-bit fields per register
    {
        const int bb = lane & 3;                             // lane = w * 4 + bb
        const int c = tab[lane];
        int incl = c;                                        // scan over the waves of a bin: lanes 4 apart
#pragma unroll
        for (int d = 4; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        const int total = __shfl(incl, 60 + bb);
        const int padded = (total + 63) & ~63;
        int start = padded;                                  // scan over the bins: 4 neighbouring lanes
#pragma unroll
        for (int d = 1; d < 4; d <<= 1) {
            const int up = __shfl_up(start, d, 4);
            if (bb >= d) start += up;
        }
        start -= padded;
        const int base = start + incl - c;                   // list base of (wave w, bin bb)
        const int wl = __builtin_amdgcn_readfirstlane(wave) * 4;
        const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane(base, wl), b1 = (uint32_t)__builtin_amdgcn_readlane(base, wl + 1),
                       b2 = (uint32_t)__builtin_amdgcn_readlane(base, wl + 2), b3 = (uint32_t)__builtin_amdgcn_readlane(base, wl + 3);
        const uint32_t ea = ia - xa, eb = ib - xb;           // counts of the lanes below
        cur01 = ((b0 + (ea & 0xFFFFu)) & 0xFFFFu) | ((b1 + (ea >> 16)) << 16);
        cur23 = ((b2 + (eb & 0xFFFFu)) & 0xFFFFu) | ((b3 + (eb >> 16)) << 16);
        const int sc = start >> 6, ec = (start + padded) >> 6;           // chunks: < 256
        cs_pack = (uint32_t)__builtin_amdgcn_readlane(sc, 0) | ((uint32_t)__builtin_amdgcn_readlane(sc, 1) << 8) |
                  ((uint32_t)__builtin_amdgcn_readlane(sc, 2) << 16) | ((uint32_t)__builtin_amdgcn_readlane(sc, 3) << 24);
        ce_pack = (uint32_t)__builtin_amdgcn_readlane(ec, 0) | ((uint32_t)__builtin_amdgcn_readlane(ec, 1) << 8) |
                  ((uint32_t)__builtin_amdgcn_readlane(ec, 2) << 16) | ((uint32_t)__builtin_amdgcn_readlane(ec, 3) << 24);
        ne_bins = (uint32_t)(__ballot(total > 0) & 0xFull);
        // lean set-up: the lists were not pre-filled.  Wave b marks the padding tail of bin b (at most 63 entries); the chunks
        // behind the last bin stay unwritten, and the slot read-back below does not read them.
        if (lean && wl < NBIN * 4) {
            const int tail = __builtin_amdgcn_readlane(start + total, wl >> 2), npad = __builtin_amdgcn_readlane(padded - total, wl >> 2);
            if (lane < npad) lst[tail + lane] = (uint16_t)0xFFFFu;
        }
    }
    // The next piece rides in registers behind the lookups of the current one: NSLAB x 16 bytes per thread.
    uint4 pr[NSLAB];
#pragma unroll
    for (int i = 0; i < NSLAB; ++i) pr[i] = make_uint4(0, 0, 0, 0);
    const uint8_t* s2p = P.pack + (size_t)(GEN ? P.n1 : 3) * LUT_PAD;          // [LUT l][bin b][PIECE_BYTES], blocks pre-permuted
    const int NL2 = GEN ? 2 * P.n2 : 6;                // stage-2 LUTs: pattern x rotation parity
    auto pre_load = [&](int l, int bq) {
        const uint4* s_ = reinterpret_cast<const uint4*>(s2p + ((size_t)l * NBIN + bq) * PIECE_BYTES) + (wave * 64 + lane);
#pragma unroll
        for (int i = 0; i < NSLAB; ++i) pr[i] = s_[i * NT];
    };
    const int nbins = __builtin_popcount(ne_bins);
    const int nph = nbins * NL2;
    if (nph > 0) pre_load(0, __builtin_ctz(ne_bins));      // in flight during the scatter and the slot set-up
    {
        // scatter: a position's list entry = the thread's cursor of its bin, which then moves on (registers only).
        // The entry is the position's feat-tile ADDRESS (listed positions lie inside the frame, so it is the unclamped
        // one: one increment per position, a row step every HP positions), which the slot set-up then reads back
        // as it is -- no second address computation per slot.
        const int p0 = tid * KH, ry0 = p0 / D::HP;
        uint32_t col = (uint32_t)(p0 - ry0 * D::HP);
        uint32_t ap = (uint32_t)((ry0 + D::HO) * D::FP + D::HO * CH) + col;
#pragma unroll
        for (int k = 0; k < KH; ++k) {
            const uint32_t q = k < 8 ? (qlo >> (4 * k)) & 0xFu : (qhi >> (4 * (k - 8))) & 0xFu;
            if (q < NBIN) {
                const uint32_t pair = q < 2 ? cur01 : cur23;
                const uint32_t v = (q & 1u) ? pair >> 16 : pair & 0xFFFFu;
                lst[v] = (uint16_t)ap;
                const uint32_t inc = (q & 1u) ? 0x10000u : 1u;
                if (q < 2) cur01 += inc; else cur23 += inc;
            }
            ++ap;
            if (++col == (uint32_t)D::HP) { col = 0; ap += (uint32_t)(D::FP - D::HP); }
        }
    }
    __syncthreads();
    // slots -> registers.  Per slot: the feat-tile address of its centre (16 bits, two slots per VGPR) and three
    // accumulators (accA: e0 | e2 << 16 in 16-bit fields; accB: e2 + 256 e1).  Padding lanes of a partly filled wave repeat the wave's
    // first real position (same bin, same LDS words: broadcast reads) into accumulators nobody reads, so the lookup
    // loop needs no per-lane test; `vmask` remembers which slots are real, and the position id comes back out of the
    // address when the sums are finalised (listed positions are inside the frame: the address is not clamped).
    constexpr int MAXP = (MAXR + 1) / 2;
    uint32_t slot2[MAXP];
    uint32_t accA[MAXR], accB[MAXR];
    uint32_t wrounds = 0;                 // bit k: this wave has a real position in round k (wave-uniform)
    uint32_t vmask = 0;                   // bit k: this lane's slot k is real
    const int wvl = LEAN ? __builtin_amdgcn_readfirstlane(wave) : 0;
#pragma unroll
    for (int k = 0; k < MAXR; ++k) {
        uint32_t p = lst[k * NT + tid];
        // lean set-up: a chunk behind the last bin was never written and reads as padding.  Only the rounds whose chunks may lie
        // there carry the test: the bins hold NHL positions, so the first NHL / 64 chunks always belong to one.
        if (16 * k + 15 >= D::NHL / 64 && lean && 16 * k + wvl >= (int)((ce_pack >> (8 * (NBIN - 1))) & 0xFFu)) p = 0xFFFFu;
        uint32_t a = p;
        if (p != 0xFFFFu) vmask |= 1u << k;
        const unsigned long long real = __ballot(p != 0xFFFFu);
        if (real != 0ull) {
            const uint32_t a1 = (uint32_t)__builtin_amdgcn_readlane((int)a, (int)__builtin_ctzll(real));
            if (p == 0xFFFFu) a = a1;
            wrounds |= 1u << k;
        }
        if (k & 1) slot2[k >> 1] |= a << 16; else slot2[k >> 1] = a;
        accA[k] = 0;
        accB[k] = 0;
    }
    __syncthreads();                      // the lists are dead: the first piece may land on them

    LERF_STAMP(7);
    // The piece travels as NSLAB x 16 bytes per thread (wave w, slab i: 1-KiB block B = 16 i + w of the piece, lane L
    // its bytes 16 L..16 L+15) and is stored with ds_write_addtid_b32 (address = M0 + offset + 4*lane, no address
    // VGPR: 128 B/clk/CU against 79 for ds_write_b128).  addtid puts component c of all lanes at block + 256 c + 4 L,
    // so the pack holds every block pre-permuted (global dword 4L+c = logical dword 64c+L) and LDS ends up in
    // natural order.  M0 = the wave's block column; the 16-bit offset reaches 4 slabs.
#define LERF_ADDTID(V, OFF) asm volatile("ds_write_addtid_b32 %0 offset:" #OFF :: "v"(V) : "memory")
#define LERF_ADDTID4(R, OFF0, OFF1, OFF2, OFF3) \
    LERF_ADDTID(R.x, OFF0); LERF_ADDTID(R.y, OFF1); LERF_ADDTID(R.z, OFF2); LERF_ADDTID(R.w, OFF3)
#define LERF_SET_M0(V) asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" :: "s"(V) : "memory")
    auto pre_store = [&]() {
        const uint32_t m0a = __builtin_amdgcn_readfirstlane((uint32_t)D::OFF_X + (uint32_t)wave * 1024u);
        // slab i holds blocks 16 i + wave: the last slab is partial (blocks beyond PIECE_BLOCKS carry no data)
#define LERF_SLAB_OK(I) ((I) < NSLAB && (16 * (I) + 15 < PIECE_BLOCKS || 16 * (I) + wave < PIECE_BLOCKS))
        LERF_SET_M0(m0a);
        if (LERF_SLAB_OK(0)) { LERF_ADDTID4(pr[0], 0, 256, 512, 768); }
        if (LERF_SLAB_OK(1)) { LERF_ADDTID4(pr[1 < NSLAB ? 1 : 0], 16384, 16640, 16896, 17152); }
        if (LERF_SLAB_OK(2)) { LERF_ADDTID4(pr[2 < NSLAB ? 2 : 0], 32768, 33024, 33280, 33536); }
        if (LERF_SLAB_OK(3)) { LERF_ADDTID4(pr[3 < NSLAB ? 3 : 0], 49152, 49408, 49664, 49920); }
        if (NSLAB > 4) {
            LERF_SET_M0(m0a + 65536u);
            if (LERF_SLAB_OK(4)) { LERF_ADDTID4(pr[4 < NSLAB ? 4 : 0], 0, 256, 512, 768); }
            if (LERF_SLAB_OK(5)) { LERF_ADDTID4(pr[5 < NSLAB ? 5 : 0], 16384, 16640, 16896, 17152); }
            if (LERF_SLAB_OK(6)) { LERF_ADDTID4(pr[6 < NSLAB ? 6 : 0], 32768, 33024, 33280, 33536); }
            if (LERF_SLAB_OK(7)) { LERF_ADDTID4(pr[7 < NSLAB ? 7 : 0], 49152, 49408, 49664, 49920); }
        }
        if (NSLAB > 8) {
            LERF_SET_M0(m0a + 81920u);       // slab 5's base: M0 stays below 128 KiB, the offset field supplies the rest
            if (LERF_SLAB_OK(8)) { LERF_ADDTID4(pr[8 < NSLAB ? 8 : 0], 49152, 49408, 49664, 49920); }
        }
        static_assert(NSLAB <= 9, "three M0 windows");
#undef LERF_SLAB_OK
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };
    // phases = (non-empty bin) x (6 LUTs).  The next piece is fetched into registers while the current one is being
    // used, so the L2 latency of the piece copies hides behind the lookups.
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    // per-bin scalars, refreshed when a bin's first LUT comes up (kept loop-carried on purpose: loop-invariant code
    // motion out of an inner per-LUT loop would park every round's slot address in a register of its own)
    int bq = 0, bq_next = 0, l = 0, bi = 0;
    uint32_t ne_left = ne_bins;               // non-empty bins not yet started
    uint32_t act = 0, qbase = 0;
    for (int ph = 0; ph < nph; ++ph) {
        if (l == 0) {
            // its level range, and this wave's rounds: chunk 16 k + wave inside [cs, ce) -- one scalar bit test per
            // unrolled round
            bq = __builtin_ctz(ne_left);
            ne_left &= ne_left - 1u;
            bq_next = ne_left != 0u ? __builtin_ctz(ne_left) : 0;
            const int cs = (int)((cs_pack >> (8 * bq)) & 0xFFu), ce = (int)((ce_pack >> (8 * bq)) & 0xFFu);
            const int klo = cs > wv ? (cs - wv + 15) >> 4 : 0, khi = ce > wv ? (ce - wv + 15) >> 4 : 0;
            act = wrounds & ((1u << khi) - 1u) & ~((1u << klo) - 1u);
            // LDS address of the piece's logical entry 0 (the piece starts at top-axis level bin_lo(bq))
            qbase = lds_addr(smem + D::OFF_X) - (uint32_t)bin_lo(bq) * (kStrideA * 4u);
        }
        const unsigned long long t_copy = LERF_NOW();
        (void)t_copy;
        pre_store();
        Off3 o0, o1;                                     // LUT l = mode (l>>1), rotation parity (l&1)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            o0.o[i] = P.s2off[l][i];
            o1.o[i] = P.s2off[l][3 + i];
        }
        const uint32_t bt_a = lds_addr(Bt);
        const unsigned st_a = kStrideA * 4, st_b = kStrideB * 4, st_c = kStrideC * 4, st_d = kStrideD * 4;   // axis strides, bytes
        __syncthreads();
        if (l < NL2 - 1) pre_load(l + 1, bq);
        else if (bi + 1 < nbins) pre_load(0, bq_next);
        LERF_STAMP_ADD(8, t_copy);
        const unsigned long long t_look = LERF_NOW();
        (void)t_look;
#pragma unroll
        for (int k = 0; k < MAXR; ++k) {
            if ((act >> k) & 1u) {
                const uint32_t sa = (k & 1) ? (slot2[k >> 1] >> 16) : (slot2[k >> 1] & 0xFFFFu);
                // stage A: the 7 pixel reads of the two rotations (high-half loads, see lds_pixel_hi)
                const uint32_t cpa = bt_a + sa;
                uint32_t ra = lds_pixel_hi(cpa);
                uint32_t rb0 = lds_pixel_hi(cpa + (uint32_t)o0.o[0]), rc0 = lds_pixel_hi(cpa + (uint32_t)o0.o[1]),
                         rd0 = lds_pixel_hi(cpa + (uint32_t)o0.o[2]);
                uint32_t rb1 = lds_pixel_hi(cpa + (uint32_t)o1.o[0]), rc1 = lds_pixel_hi(cpa + (uint32_t)o1.o[1]),
                         rd1 = lds_pixel_hi(cpa + (uint32_t)o1.o[2]);
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ra), "+v"(rb0), "+v"(rc0), "+v"(rd0), "+v"(rb1), "+v"(rc1), "+v"(rd1));
                // stage B: both walks (LDS addresses into the piece)
                const int basea = (int)(__umul24(msb_of(ra), kStrideA * 4) + qbase);
                const unsigned ka = key_of(ra, st_a);
                const Walk<4> W0 = simplex_walk<4>(ka, basea, rb0, rc0, rd0, st_b, st_c, st_d);
                const Walk<4> W1 = simplex_walk<4>(ka, basea, rb1, rc1, rd1, st_b, st_c, st_d);
                // stage C: ten dword gathers in flight together
                uint32_t d0[5], d1[5];
#pragma unroll
                for (int n = 0; n < 5; ++n) d0[n] = W0.ld32(n);
#pragma unroll
                for (int n = 0; n < 5; ++n) d1[n] = W1.ld32(n);
                __builtin_amdgcn_sched_barrier(0);
                // stage D: two multiply-adds per corner.  The entry is e0 | 0 << 8 | e2 << 16 | e1 << 24: a 24-bit multiply reads
                // bits 0..23 only, so the (e0, e2) pair needs no mask; the second one multiplies the entry's HIGH HALF
                // (e2 + 256 e1, v_mad_u32_u16 with op_sel) without a shift -- accB = sum w e2 + 256 sum w e1, and the e2
                // sum is already in accA's upper field, so the finalisation takes it out again (round 3: 3 -> 2
                // instructions per corner, 87 -> 77 per slot)
                const unsigned w0[5] = {(unsigned)kQ - W0.f0, W0.f0 - W0.f1, W0.f1 - W0.f2, W0.f2 - W0.f3, W0.f3};
                const unsigned w1[5] = {(unsigned)kQ - W1.f0, W1.f0 - W1.f1, W1.f1 - W1.f2, W1.f2 - W1.f3, W1.f3};
                uint32_t a = accA[k], bb = accB[k];
#pragma unroll
                for (int n = 0; n < 5; ++n) {
                    a = mad_u24(w0[n], d0[n], a);
                    bb = mad_hi16(w0[n], d0[n], bb);
                }
#pragma unroll
                for (int n = 0; n < 5; ++n) {
                    a = mad_u24(w1[n], d1[n], a);
                    bb = mad_hi16(w1[n], d1[n], bb);
                }
                accA[k] = a;
                accB[k] = bb;
            }
        }
        __syncthreads();
        LERF_STAMP_ADD(9, t_look);
        if (++l == NL2) { l = 0; ++bi; }
    }
    LERF_STAMP(10);
    // finalise: hq = rne(clip(N/192 + 127)); entries are biased by +128 -> 12 lookups * 16 * 128 = 24576
    //           N + 127*192 = field - 24576 + 24384 = field - 192
    const int div2 = GEN ? kQ * 4 * P.n2 : kQ * 12;     // general kernels: 4 rotations x n2 patterns (same bias algebra)
#pragma unroll
    for (int k = 0; k < MAXR; ++k) {
        if ((vmask >> k) & 1u) {
            int n0 = (int)(accA[k] & 0xFFFFu) - div2;
            int n2 = (int)(accA[k] >> 16) - div2;
            int n1 = (int)((accB[k] - (accA[k] >> 16)) >> 8) - div2;      // accB = (e2 sum) + 256 (e1 sum), see the slot's MACs
            uint32_t h0 = (uint32_t)rne_div_clip255_fast(n0, div2);
            uint32_t h1 = (uint32_t)rne_div_clip255_fast(n1, div2);
            uint32_t h2 = (uint32_t)rne_div_clip255_fast(n2, div2);
            // feat-tile address -> hyper-region position: row (ry + R2) of pitch FP -> row ry of pitch HP, R2 pixels left
            const uint32_t a = (k & 1) ? (slot2[k >> 1] >> 16) : (slot2[k >> 1] & 0xFFFFu);
            uint32_t row;
            if constexpr (LEAN) row = feat_row<D>(a); else row = a / (uint32_t)D::FP;
            const uint32_t p = a - row * (uint32_t)(D::FP - D::HP) - (uint32_t)(D::HO * D::HP + D::HO * CH);
            Dt[p] = h0 | (h1 << 8) | (h2 << 16) | ((uint32_t)Bt[a] << 24);
        }
    }
}

// ---- fill_outside: out-of-frame positions of the hyper region = the clamped position's hyper bytes, image byte as
//      outside_pixel() gives it (edge tiles of the LeRF-G kernels that run stage 3)
template <typename D, typename Outside>
__device__ __forceinline__ void fill_outside(uint32_t* Dt, int hy0, int hx0, int H, int W, int tid, Outside outside_pixel) {
    __syncthreads();
    for (int p = tid; p < D::NH; p += NT) {
        const int ry = p / D::HP, r3 = p - ry * D::HP, rx = r3 / CH, c = r3 - rx * CH;
        const int gy = hy0 + ry, gx = hx0 + rx;
        const int cy = clampi(gy, 0, H - 1), cx = clampi(gx, 0, W - 1);
        if (cy != gy || cx != gx)
            Dt[p] = (Dt[(cy - hy0) * D::HP + (cx - hx0) * CH + c] & 0x00FFFFFFu) | (outside_pixel(gy, gx, c) << 24);
    }
}

// ---- EMIT: the tile's own block of packed dwords -> emit ([H][W][CH] uint32)
template <typename D>
__device__ __forceinline__ void emit_tile(const uint32_t* Dt, uint32_t* eo, int H, int W, int ty0, int tx0, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    __syncthreads();
    const int rows = min(TH, H - ty0), cols3 = min(TW, W - tx0) * CH;
    for (int il = wave; il < rows; il += NW) {
        const uint32_t* srow = Dt + (il + D::HR) * D::HP + D::HR * CH;
        uint32_t* drow = eo + ((int64_t)(ty0 + il) * W + tx0) * CH;
        for (int x = lane; x < cols3; x += 64) drow[x] = srow[x];
    }
}

// ---------------------------------------------------------------------------
// Stage 3 of the SR kernels, in the order a workgroup runs it: geometry search and staging, row groups and census, ONE task
// form, the tie pass (and the flush of the block forms).  Consecutive output rows that start at the same source row (2 rows
// at x2, 3 at x3 ...) form a row group and share their taps.  What the pieces share is one Stage3, built once.
// ---------------------------------------------------------------------------
// t / n for the task decodings (t * n < 2^32)
struct MagicDiv {
    unsigned n, magic;
    __device__ __forceinline__ explicit MagicDiv(int n_)
        : n((unsigned)n_), magic((unsigned)((0x100000000ull + (unsigned)n_ - 1) / (unsigned)(n_ > 0 ? n_ : 1))) {}
    __device__ __forceinline__ constexpr MagicDiv(unsigned n_, unsigned magic_) : n(n_), magic(magic_) {}
    __device__ __forceinline__ int div(int t) const { return n == 1 ? t : (int)__umulhi((unsigned)t, magic); }   // (ceil(2^32 / 1) does not fit the 32-bit magic)
    // n_ == the power of two N, known at compile time to be the common case (KNOWN: the interior tiles of the X2 kernels):
    // the magic is 2^32 / N, a shift, and the 64-bit division is left to the other tiles
    template <bool KNOWN, int N>
    __device__ __forceinline__ static MagicDiv of(int n_) {
        constexpr bool POW2 = N > 1 && (N & (N - 1)) == 0;               // (TW is one for RGB frames: 64)
        if (KNOWN && POW2 && n_ == N) return MagicDiv((unsigned)N, (unsigned)(0x100000000ull / (unsigned)N));
        return MagicDiv(n_);
    }
};

// The GEOMETRY SOURCE of stage 3: first tap (hyper-region coordinates) and the S distances (LeRF-G: pre-multiplied by
// gauss_scale) of every owned output row / column, the first row of every row group, the first column of every column group
// (LeRF-L block tasks) and an output's float64 distances for the tie pass.  Stage3 and the task functions are written against
// it; there are two:
//   GeoTab  the tile's slice of the caller's tables, staged in LDS (Dims::OFF_GEO) -- any scale factors;
//   GeoX2   the closed form of exact x2 (x2_left / x2_dis, lerf_host_geometry.h) -- the X2 kernels: no table is read.
template <typename D, int S>
struct GeoTab {
    static constexpr bool X2 = false;
    int* lr_; float* dr_; int* lc_; float* dc_; int* grp_; int* cgrp_;
    const double* dis_r64; const double* dis_c64;      // the frame's float64 tables (NULL: tie guard off)
    int i0, j0;                                        // the owned block's first row / column in them
    __device__ __forceinline__ explicit GeoTab(uint8_t* smem)
        : lr_(reinterpret_cast<int*>(smem + D::OFF_GEO)), dr_(reinterpret_cast<float*>(lr_ + D::GEO_ROWS)), lc_(reinterpret_cast<int*>(dr_ + D::GEO_ROWS * S)),
          dc_(reinterpret_cast<float*>(lc_ + D::GEO_COLS)), grp_(reinterpret_cast<int*>(dc_ + D::GEO_COLS * S)),
          cgrp_(reinterpret_cast<int*>(smem + D::OFF_CGRP)), dis_r64(nullptr), dis_c64(nullptr), i0(0), j0(0) {}
    __device__ __forceinline__ int lr(int il) const { return lr_[il]; }
    __device__ __forceinline__ int lc(int jl) const { return lc_[jl]; }
    __device__ __forceinline__ float dr(int il, int b) const { return dr_[il * S + b]; }
    __device__ __forceinline__ float dc(int jl, int a) const { return dc_[jl * S + a]; }
    // ... of row / column 2 * pair + off (the block forms: off is the same for every task of a tile)
    __device__ __forceinline__ float dr_pair(int pair, int off, int b) const { return dr_[(2 * pair + off) * S + b]; }
    __device__ __forceinline__ float dc_pair(int pair, int off, int a) const { return dc_[(2 * pair + off) * S + a]; }
    __device__ __forceinline__ int grp(int g) const { return grp_[g]; }
    __device__ __forceinline__ int cgrp(int h) const { return cgrp_[h]; }
    __device__ __forceinline__ void dis64(int il, int jl, double (&dx)[S], double (&dy)[S]) const {
#pragma unroll
        for (int b = 0; b < S; ++b) dx[b] = dis_r64[(int64_t)(i0 + il) * S + b];
#pragma unroll
        for (int a = 0; a < S; ++a) dy[a] = dis_c64[(int64_t)(j0 + jl) * S + a];
    }
};

template <typename D, int S>
struct GeoX2 {
    static constexpr bool X2 = true;
    static_assert(S == 2, "the exact-x2 flavour serves the 2 x 2 support");
    // lr(il) = (il + rbase) >> 1.  rbase = 1 when the block starts with the frame's single first row (output 0), else 0: the block
    // then starts at an odd output, so row il is an EVEN output of the frame exactly when (il + rbase) is odd.  Columns alike.
    int rbase, cbase;
    int nrow, ncol;
    bool rows_align;                     // (Stage3::rows_align: without it every row is a group of its own)
    float kd[2][S];                      // distance of tap k from an even / odd output, times the kind's scale: formed once per thread
    __device__ __forceinline__ explicit GeoX2(uint8_t*) {}
    __device__ __forceinline__ void set(int i0, int j0, int nrow_, int ncol_, int ty0, int tx0, bool rows_align_, float gscale) {
        rbase = i0 + 1 - 2 * ty0; cbase = j0 + 1 - 2 * tx0;
        nrow = nrow_; ncol = ncol_; rows_align = rows_align_;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int k = 0; k < S; ++k) {
                kd[p][k] = (float)x2_dis(p, k, S) * gscale;         // the product stage3_geo_stage forms
            }
    }
    __device__ __forceinline__ int lr(int il) const { return (il + rbase) >> 1; }
    __device__ __forceinline__ int lc(int jl) const { return (jl + cbase) >> 1; }
    __device__ __forceinline__ float dr(int il, int b) const { return ((il + rbase) & 1) ? kd[0][b] : kd[1][b]; }
    __device__ __forceinline__ float dc(int jl, int a) const { return ((jl + cbase) & 1) ? kd[0][a] : kd[1][a]; }
    // row / column 2 * pair + off: its parity does not depend on the pair -- the block forms' distances are the same for every task
    __device__ __forceinline__ float dr_pair(int, int off, int b) const { return ((off + rbase) & 1) ? kd[0][b] : kd[1][b]; }
    __device__ __forceinline__ float dc_pair(int, int off, int a) const { return ((off + cbase) & 1) ? kd[0][a] : kd[1][a]; }
    // row groups = the runs of equal first taps (pairs; a leading / trailing single), column groups of LeRF-L alike
    __device__ __forceinline__ int grp(int g) const { return rows_align ? min(max(2 * g - rbase, 0), nrow) : g; }
    __device__ __forceinline__ int ngrp() const { return rows_align ? (nrow + rbase + 1) >> 1 : nrow; }
    __device__ __forceinline__ int cgrp(int h) const { return min(max(2 * h - cbase, 0), ncol); }
    __device__ __forceinline__ int ncgrp() const { return (ncol + cbase + 1) >> 1; }
    // rows per group when every group has as many, else 0 (what wave 0 of stage3_census finds in the group table)
    __device__ __forceinline__ int gsame() const {
        const int ng = ngrp();
        if (ng == 0) return 0;
        const int first = grp(1) - grp(0), last = nrow - grp(ng - 1);
        return (first == last && (ng <= 2 || grp(2) - grp(1) == first)) ? first : 0;
    }
    // pair_census of lr / lc: pairs (2h, 2h + 1) -- code 1 -- or, behind the leading single, (2h - 1, 2h) -- code 2; the step
    // of one tap from pair to pair always holds
    __device__ __forceinline__ int rcode() const { return (rbase == 0 || nrow <= 1) ? 1 : 2; }
    __device__ __forceinline__ int ccode() const { return (cbase == 0 || ncol <= 1) ? 1 : 2; }
    __device__ __forceinline__ void dis64(int il, int jl, double (&dx)[S], double (&dy)[S]) const {
#pragma unroll
        for (int b = 0; b < S; ++b) dx[b] = x2_dis(il + rbase + 1, b, S);          // (only the parity of the output index matters)
#pragma unroll
        for (int a = 0; a < S; ++a) dy[a] = x2_dis(jl + cbase + 1, a, S);
    }
};

// ---- owned output rows / columns -> ctl[CTL_I0 .. CTL_J1].  Tables: four wave-parallel searches in the global tables.  X2:
//      arithmetic on the tile's position (x2_owned), no global read; the tie queue is reset here too (the X2 kernels run no census)
template <typename D, bool X2>
__device__ __forceinline__ void stage3_geo_search(const FrameView& F, int tyi, int txi, int ty0, int tx0, int* ctl, int tid) {
    if constexpr (X2) {
        if (tid < 2) {
            int o0, o1;
            if (tid == 0) x2_owned(tyi, F.tiles_y, ty0, TH, F.oH, &o0, &o1);
            else x2_owned(txi, F.tiles_x, tx0, TW, F.oW, &o0, &o1);
            ctl[CTL_I0 + 2 * tid] = o0;
            ctl[CTL_I1 + 2 * tid] = o1;
            if (tid == 0) ctl[CTL_TQ_COUNT] = 0;
        }
        return;
    }
    const int lane = tid & 63, wave = tid >> 6;
    if (wave < 4) {
        const bool rows = wave < 2;
        const int* tab = rows ? F.left_r : F.left_c;
        const int n = rows ? F.oH : F.oW;
        const int ti = rows ? tyi : txi, tn = rows ? F.tiles_y : F.tiles_x, t0 = rows ? ty0 : tx0;
        int r;
        if (!(wave & 1)) r = ti == 0 ? 0 : wave_lower_bound(tab, n, t0 - D::R3, lane);
        else r = ti == tn - 1 ? n : wave_lower_bound(tab, n, t0 + (rows ? TH : TW) - D::R3, lane);
        if (lane == 0) ctl[CTL_I0 + wave] = r;
    }
}
// ---- tables of the owned block into LDS; LeRF-G distances pre-multiplied by (max_sigma/255)*sqrt(0.5 log2 e)
template <typename D, int S, int KIND>
__device__ __forceinline__ void stage3_geo_stage(uint8_t* smem, const FrameView& F, float max_sigma, int hy0, int hx0, const int* ctl,
                                                 int tid) {
    const GeoTab<D, S> g(smem);
    const int gi0 = ctl[CTL_I0], gi1 = ctl[CTL_I1], gj0 = ctl[CTL_J0], gj1 = ctl[CTL_J1];
    const float gscale = KIND == LERF_KIND_GAUSS ? s3::gauss_scale(max_sigma) : 1.0f;
    for (int e = tid; e < gi1 - gi0; e += NT) {
        g.lr_[e] = F.left_r[gi0 + e] - hy0;
#pragma unroll
        for (int b = 0; b < S; ++b) g.dr_[e * S + b] = F.dis_r[(gi0 + e) * S + b] * gscale;
    }
    for (int e = tid; e < gj1 - gj0; e += NT) {
        g.lc_[e] = F.left_c[gj0 + e] - hx0;
#pragma unroll
        for (int a = 0; a < S; ++a) g.dc_[e * S + a] = F.dis_c[(gj0 + e) * S + a] * gscale;
    }
}

// what the stage-3 functions share
template <typename D_, int S_, int KIND_, bool X2_ = false>
struct Stage3 {
    using D = D_;
    static constexpr int S = S_, SS = S_ * S_, KIND = KIND_;
    static constexpr bool GAUSS = KIND_ == LERF_KIND_GAUSS;
    static constexpr int GMAX = S_ == 2 ? 5 : 3;                                       // rows per group (larger runs are split)
    static constexpr bool BLK = GAUSS && (S_ == 2 || S_ == 4) && D::OUT_FITS;          // block tasks (round 4: the 4 x 4 support too)
    static constexpr bool BLKL = KIND_ == LERF_KIND_LINEAR && S_ == 2 && D::OUT_FITS;  // LeRF-L block tasks
    static constexpr int QRP = S_ == 4 ? 2 : 1, QCP = S_ == 4 ? 2 : 1;                 // blocks per quad task (see stage3_quads)
    static constexpr bool QUADS = BLK && QRP * QCP > 1;
    static constexpr bool X2 = X2_;
    std::conditional_t<X2_, GeoX2<D_, S_>, GeoTab<D_, S_>> geo;                        // the geometry source
    const uint32_t* Dt;                  // the hyper region's packed dwords
    uint32_t* tq; int* tq_count;         // tie queue: (il << 16) | xc of the outputs the float32 path could not decide
    uint8_t* outt;                       // block forms: LDS image of the output block, rows at the phase of their address mod 16
    bool guard;                          // tie guard armed: the caller passed the float64 distance tables
    uint8_t* seg0;                       // first byte of the owned block in the frame
    int64_t rowpitch;                    // bytes per output row
    bool rows_align;                     // dword columns line up across the rows of a group
    int i0, j0, nrow, ncol;              // the owned block
    int ncolc, ndw, ophase;              // bytes and dword columns per row, seg0 mod 16
    MagicDiv by_ndw;                     // dword-column tasks: task -> row group (computed once: every variant of them divides by it)
    // the census (read_census, behind the barrier that follows stage3_census)
    int ngrp, gsame, rcode, ccode, ncgrp;
    bool lin_ok;

    __device__ __forceinline__ Stage3(uint8_t* smem, const Params& P, const FrameView& F, uint8_t* outp, int* ctl, int ty0, int tx0)
        : geo(smem), by_ndw(1) {
        Dt = reinterpret_cast<const uint32_t*>(smem + D::OFF_D);
        tq = reinterpret_cast<uint32_t*>(smem + D::OFF_TQ);
        tq_count = ctl + CTL_TQ_COUNT;                       // zeroed by stage3_census, with the group table (X2: by stage3_geo_search)
        outt = smem + D::OFF_OUT;
        guard = F.dis_r64 != nullptr;
        i0 = ctl[CTL_I0]; j0 = ctl[CTL_J0];
        nrow = ctl[CTL_I1] - i0; ncol = ctl[CTL_J1] - j0;
        if constexpr (X2) {                                  // (closed forms of the tile's position: keep them scalar)
            i0 = __builtin_amdgcn_readfirstlane(i0); j0 = __builtin_amdgcn_readfirstlane(j0);
            nrow = __builtin_amdgcn_readfirstlane(nrow); ncol = __builtin_amdgcn_readfirstlane(ncol);
        }
        ncolc = ncol * CH;
        // bytes per output row: dense, or the caller's pitch (a rank's block of 1919 / 1921 output columns lives in rows padded to a
        // 16-byte multiple so that its tiles keep the dword-column / block tasks -- dense, every row was a group of its own)
        rowpitch = P.out_pitch > 0 ? (int64_t)P.out_pitch : (int64_t)F.oW * CH;      // (ragged launches: always dense)
        seg0 = outp + (int64_t)i0 * rowpitch + (int64_t)j0 * CH;
        rows_align = (rowpitch & 3) == 0;
        // dword columns per row: when every row of the block starts on a 4-byte boundary the block needs no slack column, and
        // a 384-byte tile row is exactly 96 dwords = whole 128-byte lines per wave store
        const bool seg_aligned = rows_align && (reinterpret_cast<uintptr_t>(seg0) & 3u) == 0;
        ndw = seg_aligned ? (ncolc + 3) >> 2 : (ncolc + 6) >> 2;
        ophase = (int)(reinterpret_cast<uintptr_t>(seg0) & 15u);
        if constexpr (X2) {
            geo.set(i0, j0, nrow, ncol, ty0, tx0, rows_align, GAUSS ? s3::gauss_scale(P.max_sigma) : 1.0f);
        } else {
            geo.dis_r64 = F.dis_r64; geo.dis_c64 = F.dis_c64; geo.i0 = i0; geo.j0 = j0;
        }
    }
    // what the census found (tables: behind the barrier that follows stage3_census; X2: the same facts from the closed form)
    __device__ __forceinline__ void read_census(const int* ctl) {
        if constexpr (X2) {
            ngrp = geo.ngrp();
            gsame = __builtin_amdgcn_readfirstlane(geo.gsame());
            rcode = __builtin_amdgcn_readfirstlane(geo.rcode()); ccode = __builtin_amdgcn_readfirstlane(geo.ccode());
            ncgrp = __builtin_amdgcn_readfirstlane(geo.ncgrp());
            lin_ok = BLKL;
            by_ndw = MagicDiv(ndw);
            return;
        }
        ngrp = ctl[CTL_NGRP];
        gsame = __builtin_amdgcn_readfirstlane(ctl[CTL_GSAME]);
        rcode = __builtin_amdgcn_readfirstlane(ctl[CTL_RCODE]); ccode = __builtin_amdgcn_readfirstlane(ctl[CTL_CCODE]);
        if constexpr (BLKL) lin_ok = ctl[CTL_LIN_ROWS_OK] != 0 && ctl[CTL_LIN_COLS_OK] != 0;   // (LeRF-G: slot 26 is rcode, 27 unwritten)
        else lin_ok = false;
        ncgrp = 0;                                           // (stage3_blocks_lin reads CTL_NCGRP itself)
        by_ndw = MagicDiv(ndw);
    }
};

// Do the entries of a first-tap table pair up as (2h, 2h + 1) -- code 1 -- or, behind a leading single (the frame's top /
// left edge), as (2h - 1, 2h) -- code 2?  A trailing single is fine either way.  step: pair h + 1 starts exactly one tap
// behind pair h (x2).  One wave; lane 0 writes the answers.
__device__ __forceinline__ void pair_census(const int* t, int n, int lane, int* code, int* step) {
    bool ok0 = true, ok1 = true, step1 = true;
    for (int base = 0; base < n; base += 64) {
        const int k = base + lane;
        if (k + 1 < n && t[k + 1] != t[k]) { if (k & 1) ok1 = false; else ok0 = false; }
        if (!(k & 1) && k + 2 < n && t[k + 2] != t[k] + 1) step1 = false;
    }
    const bool p0 = __ballot(!ok0) == 0ull, p1 = __ballot(!ok1) == 0ull, q1 = __ballot(!step1) == 0ull;
    if (lane == 0) { *code = p0 ? 1 : (p1 ? 2 : 0); *step = q1 ? 1 : 0; }
}

// ---- the row-group table (wave 0) and what the block forms ask about the tile's rows and columns (waves 1, 2).  Table
//      geometry only: at exact x2 every answer is a closed form of the tile's position (GeoX2, Stage3::read_census), and
//      the tie queue was reset by stage3_geo_search -- the X2 kernels run no census and skip its barrier
template <typename X_>
__device__ __forceinline__ void stage3_census(const X_& X, int* ctl, int tid) {
  if constexpr (!X_::X2) {
    constexpr int KIND = X_::KIND, GMAX = X_::GMAX;
    const int lane = tid & 63, wave = tid >> 6;
    const int nrow = X.nrow, ncol = X.ncol;
    const int* g_lr = X.geo.lr_;
    const int* g_lc = X.geo.lc_;
    int* g_grp = X.geo.grp_;
    if (wave == 0) {
        int ng = 0;
        for (int base = 0; base < nrow; base += 64) {
            const int il = base + lane;
            bool start = false;
            if (il < nrow)
                start = il == 0 || !X.rows_align || g_lr[il] != g_lr[il - 1] || (il >= GMAX && g_lr[il - GMAX] == g_lr[il]);
            const unsigned long long m = __ballot(start);
            if (start) g_grp[ng + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] = il;
            ng += __popcll(m);
        }
        if (lane == 0) g_grp[ng] = nrow;
        // every group of the tile the same size (integer scale factors, away from the frame's top and bottom): the
        // task loop then runs with that size as a compile-time constant, without a row test per tap set
        const int g0 = ng > 0 ? g_grp[1] - g_grp[0] : 0;
        bool same = true, small = true;                      // small: no group of more than two rows (block tasks of LeRF-L)
        for (int base = 0; base < ng; base += 64) {
            const int idx = base + lane;
            if (idx < ng && g_grp[idx + 1] - g_grp[idx] != g0) same = false;
            if (X_::BLKL && idx < ng && g_grp[idx + 1] - g_grp[idx] > 2) small = false;
        }
        const bool uniform = __ballot(!same) == 0ull;
        if (lane == 0) {
            ctl[CTL_NGRP] = ng;
            ctl[CTL_GSAME] = uniform ? g0 : 0;
            ctl[CTL_TQ_COUNT] = 0;
        }
        if constexpr (X_::BLKL) {
            const bool ok = __ballot(!small) == 0ull;
            if (lane == 0) ctl[CTL_LIN_ROWS_OK] = ok ? 1 : 0;
        }
    } else if (wave == 1 && X_::BLKL) {
        // LeRF-L block tasks: the columns in groups of at most two that share their taps (runs of equal left taps, every
        // second column of a run starts a group); the table lies behind the output image, over the dead stage-2 areas
        int* g_cgrp = X.geo.cgrp_;
        constexpr int NCMAX = 2 * TW + 14;
        int nc = 0;
        for (int base = 0; base < ncol; base += 64) {
            const int jl = base + lane;
            bool start = false;
            if (jl < ncol) {
                int back = 0;                                // columns of the same run to the left
                while (back < 16 && jl - back - 1 >= 0 && g_lc[jl - back - 1] == g_lc[jl]) ++back;
                start = (back & 1) == 0;
            }
            const unsigned long long m = __ballot(start);
            if (start) {
                const int idx = nc + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                if (idx < NCMAX) g_cgrp[idx] = jl;
            }
            nc += __popcll(m);
        }
        if (lane == 0) {
            if (nc <= NCMAX) g_cgrp[nc] = ncol;
            ctl[CTL_NCGRP] = nc;
            ctl[CTL_LIN_COLS_OK] = (nc <= NCMAX) ? 1 : 0;
        }
    } else if (wave == 1) {
        pair_census(g_lc, ncol, lane, &ctl[CTL_CCODE], &ctl[CTL_CSTEP]);
    } else if (wave == 2 && KIND == LERF_KIND_GAUSS) {
        pair_census(g_lr, nrow, lane, &ctl[CTL_RCODE], &ctl[CTL_RSTEP]);
    }
  }
}

// ---- output (il, xc) of the owned block (row, byte column) re-evaluated in float64 exactly as the reference does
//      (lerf_stage3.h, tie guard): its taps from the packed dwords, its float64 distances from the geometry source (the
//      frame's float64 tables, or the closed form -- the same bits)
template <typename X_>
__device__ __forceinline__ uint8_t resolve_output(const X_& X, float max_sigma, int il, int xc) {
    using D = typename X_::D;
    constexpr int S = X_::S;
    const int jl = xc / CH;
    const int c = xc - jl * CH;
    const uint32_t* dp = X.Dt + X.geo.lr(il) * D::HP + X.geo.lc(jl) * CH + c;
    double dx[S], dy[S];
    X.geo.dis64(il, jl, dx, dy);
    return s3::resolve_taps_u8<X_::GAUSS, S>([&](int a, int b) __attribute__((always_inline)) { return dp[b * D::HP + a * CH]; }, dx, dy, max_sigma);
}
// bit q of the result: output q of a task lies within kTieEps of a rounding tie
template <int N>
__device__ __forceinline__ unsigned tie_mask(const float (&dist)[N]) {
    unsigned m = 0;
#pragma unroll
    for (int q = 0; q < N; ++q)
        if (__builtin_fabsf(dist[q]) > 0.5f - s3::kTieEps) m |= 1u << q;
    return m;
}
// The undecided outputs of one task (bits of `mask`; decode(q, il, xc) names output q) are queued for the pass behind the
// task loop; only a full queue is worked off on the spot, the byte handed to patch(q, byte).  Rare: one round per queued
// output of the lane, not per output.
template <typename X_, typename Decode, typename Patch>
__device__ __forceinline__ void queue_ties(const X_& X, const Params& P, unsigned mask, Decode decode, Patch patch) {
    while (mask != 0) {
        const int q = __builtin_ctz(mask);
        mask &= mask - 1;
        int il, xc;
        decode(q, il, xc);
        const int slot = atomicAdd(X.tq_count, 1);
        if (slot < P.tq_cap) {
            X.tq[slot] = ((uint32_t)il << 16) | (uint32_t)xc;
            continue;
        }
        patch(q, resolve_output(X, P.max_sigma, il, xc));
    }
}
// the tail of an output of the block forms: xf -> its byte in the LDS image (when the block has this output), its distance
// from the rounded value (0 when it has not) and the running maximum of |distance|
__device__ __forceinline__ void put_block_byte(float xf, bool have, uint8_t* dst, float& dist, float& dmax) {
    const float rr = __builtin_rintf(xf);
    dist = have ? xf - rr : 0.0f;
    dmax = __builtin_fmaxf(dmax, __builtin_fabsf(dist));
    if (have) *dst = (uint8_t)__builtin_amdgcn_cvt_pk_u8_f32(rr, 0u, 0u);
}

// ---- dword-column tasks: one task = (row group, one 4-byte-aligned output dword column); the tap loads, the u8 -> f32
//      conversions and the column-only terms are done once per group, the rows pay one multiply and two FMAs per tap.
//      Same code for the 2x2 and the 4x4 support.  GS = rows per group, 0 = read it per group.
template <int GS, typename X_>
__device__ __forceinline__ void stage3_tasks(const X_& X, const Params& P, int tid) {
    using D = typename X_::D;
    constexpr int S = X_::S, SS = X_::SS, KIND = X_::KIND;
    constexpr int GN = GS > 0 ? GS : X_::GMAX;
    const auto& G = X.geo;
    const uint32_t* Dt = X.Dt;
    const int ndw = X.ndw, ncolc = X.ncolc;
    const int64_t rowpitch = X.rowpitch;
    const float ms255 = P.max_sigma * (1.0f / 255.0f);
    const int ntask = X.ngrp * ndw;
    for (int t = tid; t < ntask; t += NT) {
        const int g = X.by_ndw.div(t);
        const int dw = t - g * ndw;
        const int il0 = G.grp(g);
        const int gs = GS > 0 ? GS : G.grp(g + 1) - il0;
        uint8_t* seg = X.seg0 + il0 * rowpitch;
        const int a0 = (int)(reinterpret_cast<uintptr_t>(seg) & 3u);
        const int b0 = dw * 4 - a0;
        const int lr = G.lr(il0);
        uint32_t packed[GN];
        // tie detection: the 2x2 kernels keep every output's distance from its rounded value and a running maximum
        // (one v_max per output, the ties are looked for only when the maximum says there is one); the 4x4 kernel has
        // no registers for that and sets a bit per output
        constexpr bool DIST = S == 2;
        float dist[DIST ? GN * 4 : 1];                        // [r*4+u]
        float dmax = 0.0f;
        unsigned tiebits = 0;                                 // bit r*4+u
#pragma unroll
        for (int r = 0; r < GN; ++r) packed[r] = 0;
        s3::f2 DXP[S];                                        // packed 4x4 path: (row 0, row 1) distances of row tap b
        if constexpr (KIND == LERF_KIND_GAUSS && S == 4 && GS == 2) {
#pragma unroll
            for (int b = 0; b < S; ++b) { DXP[b].x = G.dr(il0, b); DXP[b].y = G.dr(il0 + 1, b); }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int xc = min(max(b0 + u, 0), ncolc - 1);    // clamped; invalid bytes are not stored
            const int jl = xc / CH;
            const int c = xc - jl * CH;
            const int lc = G.lc(jl);
            if constexpr (KIND == LERF_KIND_GAUSS && S == 4 && GS == 2) {
                // The 4x4 support, two rows per group, in PACKED float32 over the two rows (lane x = row 0, lane y = row 1):
                // per tap and row PAIR one v_pk_mul (tx), two v_pk_fma (the form), one v_pk_add and one v_pk_fma (the sums)
                // instead of ten scalar operations; a tap's four scalars sit two to a register pair -- (p0, ty^2) and
                // (k1, value) -- and are read through op_sel.  Same operations in the same order: the same bytes.
                s3::f2 PT[SS], KV[SS];
#pragma unroll
                for (int a = 0; a < S; ++a) {
                    const float dy = G.dc(jl, a);
#pragma unroll
                    for (int b = 0; b < S; ++b) {
                        const uint32_t d = Dt[(lr + b) * D::HP + (lc + a) * CH + c];
                        const float tyv = s3::gauss_t_u8((float)((d >> 16) & 0xFFu), dy);
                        PT[a * S + b].x = s3::gauss_m2rho_u8((float)(d & 0xFFu)) * tyv;
                        PT[a * S + b].y = tyv * tyv;
                        KV[a * S + b].x = (float)((d >> 8) & 0xFFu);
                        KV[a * S + b].y = (float)(d >> 24);
                    }
                }
                s3::f2 NUM, DEN;
#pragma unroll
                for (int a = 0; a < S; ++a)
#pragma unroll
                    for (int b = 0; b < S; ++b) {
                        const int k = a * S + b;
                        const s3::f2 TX = s3::pk_mul_blo(DXP[b], KV[k]);                       // k1 * dx[r][b]
                        const s3::f2 E = s3::pk_fma_pb<false>(TX, PT[k], s3::pk_fma_ppb<true>(TX, PT[k]));   // fma(tx, p0, fma(tx, tx, ty2))
                        s3::f2 W;
                        W.x = __builtin_amdgcn_exp2f(-E.x);
                        W.y = __builtin_amdgcn_exp2f(-E.y);
                        if (k == 0) {
                            DEN = W;
                            NUM = s3::pk_mul_bhi_after_trans(W, KV[k]);
                        } else {
                            DEN = DEN + W;                                                  // (compiler-generated: see s3::BlockTap)
                            NUM = s3::pk_fma_bhi_after_trans(W, KV[k], NUM);
                        }
                    }
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const float xf = s3::finish_div(r ? NUM.y : NUM.x, r ? DEN.y : DEN.x);
                    bool tie;
                    packed[r] = s3::pack_u8_tie(xf, u, packed[r], &tie);
                    if (tie) tiebits |= 1u << (r * 4 + u);
                }
                continue;
            }
            // shared by the rows of the group: per tap (a = column offset major, numpy meshgrid 'xy' :95-98; b = row offset)
            float p0[SS], k1[SS], ty[SS], v[SS];
#pragma unroll
            for (int a = 0; a < S; ++a) {
                const float dy = G.dc(jl, a);
#pragma unroll
                for (int b = 0; b < S; ++b) {
                    const uint32_t d = Dt[(lr + b) * D::HP + (lc + a) * CH + c];
                    v[a * S + b] = (float)(d >> 24);
                    const float k0 = (float)(d & 0xFFu);
                    if (KIND == LERF_KIND_GAUSS) {
                        // column-only terms of the quadratic form: p0 <- (-2 rho) ty, ty <- ty^2 (gauss_form_cols)
                        const float tyv = s3::gauss_t_u8((float)((d >> 16) & 0xFFu), dy);
                        p0[a * S + b] = s3::gauss_m2rho_u8(k0) * tyv;
                        k1[a * S + b] = (float)((d >> 8) & 0xFFu);
                        ty[a * S + b] = tyv * tyv;
                    } else {
                        const float alpha = s3::lin_alpha_u8(k0, ms255);
                        p0[a * S + b] = alpha;
                        ty[a * S + b] = s3::lin_factor(alpha, dy, s3::dist_class_f(dy));
                        k1[a * S + b] = 0.0f;
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < GN; ++r) {
                if (r < gs) {
                    float e[SS];
#pragma unroll
                    for (int a = 0; a < S; ++a)
#pragma unroll
                        for (int b = 0; b < S; ++b) {
                            const float dx = G.dr(il0 + r, b);
                            if (KIND == LERF_KIND_GAUSS)
                                e[a * S + b] = s3::gauss_form_cols(s3::gauss_t_u8(k1[a * S + b], dx), ty[a * S + b], p0[a * S + b]);
                            else
                                e[a * S + b] = s3::lin_factor(p0[a * S + b], dx, s3::dist_class_f(dx)) * ty[a * S + b];
                        }
                    const float xf = s3::finish<KIND == LERF_KIND_GAUSS, SS, true, true, true>(e, v);
                    if (DIST) {
                        packed[r] = s3::pack_u8_dist(xf, u, packed[r], &dist[DIST ? r * 4 + u : 0]);
                        dmax = __builtin_fmaxf(dmax, __builtin_fabsf(dist[DIST ? r * 4 + u : 0]));
                    } else {
                        bool tie;
                        packed[r] = s3::pack_u8_tie(xf, u, packed[r], &tie);
                        if (tie) tiebits |= 1u << (r * 4 + u);
                    }
                }
            }
        }
        if ((DIST ? dmax > 0.5f - s3::kTieEps : tiebits != 0) && X.guard) {
            unsigned tiemask = tiebits;
            if (DIST) {
#pragma unroll
                for (int q = 0; q < GN * 4; ++q)
                    if ((GS > 0 || (q >> 2) < gs) && __builtin_fabsf(dist[DIST ? q : 0]) > 0.5f - s3::kTieEps) tiemask |= 1u << q;
            }
            queue_ties(X, P, tiemask,
                       [&](int q, int& il, int& xc) __attribute__((always_inline)) { il = il0 + (q >> 2); xc = min(max(b0 + (q & 3), 0), ncolc - 1); },
                       [&](int q, uint32_t r8) __attribute__((always_inline)) {
                           const int r = q >> 2, u = q & 3;
#pragma unroll
                           for (int rr = 0; rr < GN; ++rr)       // (a select per row: `packed` is indexed by constants only and stays in registers)
                               packed[rr] = rr == r ? (packed[rr] & ~(0xFFu << (8 * u))) | (r8 << (8 * u)) : packed[rr];
                       });
        }
#pragma unroll
        for (int r = 0; r < GN; ++r) {
            if (r < gs) {
                uint8_t* sr = seg + r * rowpitch;
                if (b0 >= 0 && b0 + 3 < ncolc) {
                    // streaming store: the output is never re-read here, keep the LUT pack resident in L2 instead
                    __builtin_nontemporal_store(packed[r], reinterpret_cast<uint32_t*>(sr + b0));
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (b0 + u >= 0 && b0 + u < ncolc) sr[b0 + u] = (uint8_t)(packed[r] >> (8 * u));
                }
            }
        }
    }
}

// ---- block tasks: tiles whose output rows AND columns come in pairs that share their taps (integer x2, away from
//      the frame's top and left).  One task = the 2 x 2 outputs of a (row pair, column pair), all CH channels: the
//      four tap dwords of a channel are loaded and converted once for four outputs instead of once for two, the
//      column-only terms serve both rows and the row-only products both columns (43 instead of 63 VALU instructions
//      per output), and a tile is exactly 4 tasks per thread.  The bytes are assembled in an LDS image of the tile's
//      output block (ties are patched there) and leave as whole 16-byte chunks.  Same arithmetic, operation for
//      operation, as stage3_tasks: the outputs are bit-identical.  UNI: pairs from row 0 / column 0 on, even counts.
template <bool UNI, typename X_>
__device__ __forceinline__ void stage3_blocks(const X_& X, const Params& P, int tid) {
    if constexpr (X_::BLK) {
        using D = typename X_::D;
        constexpr int S = X_::S;
        const auto& G = X.geo;
        const int nrow = X.nrow, ncol = X.ncol, ophase = X.ophase;
        const int rofs = UNI ? 0 : X.rcode - 1, cofs = UNI ? 0 : X.ccode - 1;
        const int ncg = (ncol + cofs + 1) >> 1;
        const int nblk = ((nrow + rofs + 1) >> 1) * ncg;
        const MagicDiv by_ncg = MagicDiv::of<X_::X2, TW>(ncg);
        for (int t = tid; t < nblk; t += NT) {
            const int g = by_ncg.div(t);
            const int h = t - g * ncg;
            const int il0 = 2 * g - rofs, jl0 = 2 * h - cofs;
            const int lr = G.lr(UNI ? il0 : max(il0, 0)), lc = G.lc(UNI ? jl0 : max(jl0, 0));
            // distances as PAIRS: DX[b] = (row 0, row 1) of row tap b, DY[a] = (column 0, column 1) of column tap a
            s3::f2 DX[S], DY[S];
#pragma unroll
            for (int b = 0; b < S; ++b) { DX[b].x = G.dr_pair(g, -rofs, b); DX[b].y = G.dr_pair(g, 1 - rofs, b); }
#pragma unroll
            for (int a = 0; a < S; ++a) { DY[a].x = G.dc_pair(h, -cofs, a); DY[a].y = G.dc_pair(h, 1 - cofs, a); }
            const uint32_t* dp = X.Dt + lr * D::HP + lc * CH;
            uint8_t* ob = X.outt + il0 * D::OUT_PITCH + ophase + jl0 * CH;
            float dist[4 * CH];                                  // [c][r][q]
            float dmax = 0.0f;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                s3::f2 NUM[2], DEN[2];                           // [row r], lanes = the two columns
#pragma unroll
                for (int a = 0; a < S; ++a)
#pragma unroll
                    for (int b = 0; b < S; ++b) {
                        const s3::BlockTap T(dp[b * D::HP + a * CH + c]);
                        s3::f2 P0, TY2;
                        T.cols(DY[a], P0, TY2);
                        T.sum(T.rows(DX[b]), P0, TY2, a == 0 && b == 0, NUM, DEN);
                    }
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const float den = q ? DEN[r].y : DEN[r].x, num = q ? NUM[r].y : NUM[r].x;
                        const bool have = UNI || ((unsigned)(il0 + r) < (unsigned)nrow && (unsigned)(jl0 + q) < (unsigned)ncol);
                        put_block_byte(s3::finish_div(num, den), have, ob + r * D::OUT_PITCH + q * CH + c, dist[(c * 2 + r) * 2 + q], dmax);
                    }
            }
            if (dmax > 0.5f - s3::kTieEps && X.guard)
                queue_ties(X, P, tie_mask(dist),
                           [&](int q, int& il, int& xc) __attribute__((always_inline)) { il = il0 + ((q >> 1) & 1); xc = (jl0 + (q & 1)) * CH + (q >> 2); },
                           [&](int q, uint32_t r8) __attribute__((always_inline)) { ob[((q >> 1) & 1) * D::OUT_PITCH + (q & 1) * CH + (q >> 2)] = (uint8_t)r8; });
        }
    }
}

// ---- quad tasks (round 5): RP x CP neighbouring blocks of an INTERIOR x2 tile in one task.  Pair h + 1 starts exactly one
//      tap right of / below pair h (CTL_CSTEP, CTL_RSTEP), so the (S + RP - 1) x (S + CP - 1) taps of the task serve up to
//      RP x CP blocks each: a tap's load and u8 -> f32 conversions once per task instead of once per block (S = 4,
//      2 x 2 blocks: 25 instead of 64), its column-only terms once per column pair (40 instead of 64), its row
//      products once per row pair.  Every output still sums ITS S x S taps in the order (a outer, b inner) with the
//      operations of stage3_blocks: identical bytes.  One task per thread on a 64 x 64 tile with 2 x 2 blocks.
//      Measured (A/B on one box, profiles/r05_experiments.txt): S = 4: 2 x 2 blocks +1.7 % (23.58 -> 23.99 Gpix/s; 2 x 1: +1.6 %,
//      1 x 2: +1.2 %) -- the four v_exp_f32 per (tap, block) and their packed consumers are not shared, they are 3/4 of a
//      tap's issue time; S = 2: 2 x 2 blocks -1.4 % (one 48-output task per thread hides less latency than four of 12), 2 x 1
//      and 1 x 2 +-0: the 2 x 2 support keeps its single blocks (Stage3::QRP, QCP).
template <typename X_>
__device__ __forceinline__ void stage3_quads(const X_& X, const Params& P, int tid) {
    if constexpr (X_::QUADS) {
        using D = typename X_::D;
        constexpr int S = X_::S, RP = X_::QRP, CP = X_::QCP, TR = S + RP - 1, TC = S + CP - 1;
        const auto& G = X.geo;
        const int ophase = X.ophase;
        const int ncq = (X.ncol >> 1) / CP;
        const int ntq = ((X.nrow >> 1) / RP) * ncq;
        const MagicDiv by_ncq(ncq);
        for (int t = tid; t < ntq; t += NT) {
            const int g = by_ncq.div(t);
            const int h = t - g * ncq;
            const int il0 = 2 * RP * g, jl0 = 2 * CP * h;
            const int lr = G.lr(il0), lc = G.lc(jl0);
            s3::f2 DX[RP][S], DY[CP][S];               // [pair][tap]: lanes = the two rows / the two columns of the pair
#pragma unroll
            for (int rp = 0; rp < RP; ++rp)
#pragma unroll
                for (int b = 0; b < S; ++b) { DX[rp][b].x = G.dr_pair(RP * g + rp, 0, b); DX[rp][b].y = G.dr_pair(RP * g + rp, 1, b); }
#pragma unroll
            for (int cp = 0; cp < CP; ++cp)
#pragma unroll
                for (int a = 0; a < S; ++a) { DY[cp][a].x = G.dc_pair(CP * h + cp, 0, a); DY[cp][a].y = G.dc_pair(CP * h + cp, 1, a); }
            const uint32_t* dp = X.Dt + lr * D::HP + lc * CH;
            uint8_t* ob = X.outt + il0 * D::OUT_PITCH + ophase + jl0 * CH;
#pragma unroll 1
            for (int c = 0; c < CH; ++c) {
                s3::f2 NUM[RP][CP][2], DEN[RP][CP][2];   // [row pair][column pair][row of the pair], lanes = columns of the pair
#pragma unroll
                for (int A = 0; A < TC; ++A) {
#pragma unroll
                    for (int B = 0; B < TR; ++B) {
                        const s3::BlockTap T(dp[B * D::HP + A * CH + c]);
                        s3::f2 P0[CP], TY2[CP], TX[RP];
#pragma unroll
                        for (int cp = 0; cp < CP; ++cp) {
                            const int a = A - cp;
                            if (a >= 0 && a < S) T.cols(DY[cp][a < 0 ? 0 : (a >= S ? 0 : a)], P0[cp], TY2[cp]);
                        }
#pragma unroll
                        for (int rp = 0; rp < RP; ++rp) {
                            const int b = B - rp;
                            if (b >= 0 && b < S) TX[rp] = T.rows(DX[rp][b < 0 ? 0 : (b >= S ? 0 : b)]);
                        }
#pragma unroll
                        for (int cp = 0; cp < CP; ++cp) {
                            const int a = A - cp;
                            if (a < 0 || a >= S) continue;
#pragma unroll
                            for (int rp = 0; rp < RP; ++rp) {
                                const int b = B - rp;
                                if (b < 0 || b >= S) continue;
                                T.sum(TX[rp], P0[cp], TY2[cp], a == 0 && b == 0, NUM[rp][cp], DEN[rp][cp]);
                            }
                        }
                    }
                }
                float dist[RP * CP * 4];                 // [rp][cp][r][q]
                float dmax = 0.0f;
#pragma unroll
                for (int rp = 0; rp < RP; ++rp)
#pragma unroll
                    for (int cp = 0; cp < CP; ++cp)
#pragma unroll
                        for (int r = 0; r < 2; ++r)
#pragma unroll
                            for (int q = 0; q < 2; ++q) {
                                const float den = q ? DEN[rp][cp][r].y : DEN[rp][cp][r].x, num = q ? NUM[rp][cp][r].y : NUM[rp][cp][r].x;
                                put_block_byte(s3::finish_div(num, den), true, ob + (2 * rp + r) * D::OUT_PITCH + (2 * cp + q) * CH + c,
                                               dist[((rp * CP + cp) * 2 + r) * 2 + q], dmax);
                            }
                if (dmax > 0.5f - s3::kTieEps && X.guard)
                    queue_ties(X, P, tie_mask(dist),
                               [&](int k, int& il, int& xc) __attribute__((always_inline)) {
                                   const int rp = (k >> 2) / CP, cp = (k >> 2) - rp * CP;
                                   il = il0 + 2 * rp + ((k >> 1) & 1);
                                   xc = (jl0 + 2 * cp + (k & 1)) * CH + c;
                               },
                               [&](int k, uint32_t r8) __attribute__((always_inline)) {
                                   const int rp = (k >> 2) / CP, cp = (k >> 2) - rp * CP;
                                   ob[(2 * rp + ((k >> 1) & 1)) * D::OUT_PITCH + (2 * cp + (k & 1)) * CH + c] = (uint8_t)r8;
                               });
            }
        }
    }
}

// ---- LeRF-L block tasks (amplified-linear weights, 2 x 2 support): row groups and column groups of ONE or two
//      members (x1.5 gives groups of 1, 2, 1, 2 ..., x2 pairs; the frame edges singles), one task = the up to 2 x 2
//      outputs of a (row group, column group), all channels.  The dword-column tasks ran the general five-row form
//      here (a group's size is not uniform at x1.5) and evaluated every tap's row factor per output; the block forms
//      a tap's column factor once per column, its row factor once per row.  Weights as in lerf_stage3.h: the factor of
//      a distance x is max(1 - alpha |x|, 0) for |x| <= 1 and 0 outside -- alpha * x + 1 (x < 0) and 1 - alpha * x
//      (x >= 0) are the same float32 operations on |x| -- so the bytes are those of stage3_tasks.
template <typename X_>
__device__ __forceinline__ void stage3_blocks_lin(const X_& X, const Params& P, const int* ctl, int tid) {
    if constexpr (X_::BLKL) {
        using D = typename X_::D;
        const auto& G = X.geo;
        const int ophase = X.ophase;
        const float ms255 = P.max_sigma * (1.0f / 255.0f);
        const int ncg = X_::X2 ? X.ncgrp : __builtin_amdgcn_readfirstlane(ctl[CTL_NCGRP]);
        const int nblk = X.ngrp * ncg;
        const MagicDiv by_ncg = MagicDiv::of<X_::X2, TW>(ncg);
        for (int t = tid; t < nblk; t += NT) {
            const int g = by_ncg.div(t);
            const int h = t - g * ncg;
            const int il0 = G.grp(g), jl0 = G.cgrp(h);
            const bool two_r = G.grp(g + 1) - il0 > 1, two_c = G.cgrp(h + 1) - jl0 > 1;
            const int lr = G.lr(il0), lc = G.lc(jl0);
            // |distance| and inside-the-support mask (1 / 0) of the two rows [r][row tap b] and the two columns [q][column
            // tap a]; a single's second member reads its neighbour's entries (computed, never stored)
            float ax[2][2], mx[2][2], ay[2][2], my[2][2];
            auto abs_and_mask = [](auto d, float (&a)[2][2], float (&m)[2][2]) __attribute__((always_inline)) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float dk = d(k >> 1, k & 1);                   // (member, tap)
                    a[k >> 1][k & 1] = __builtin_fabsf(dk);
                    m[k >> 1][k & 1] = s3::dist_class_f(dk) != 0 ? 1.0f : 0.0f;
                }
            };
            abs_and_mask([&](int r, int b) __attribute__((always_inline)) { return G.dr(il0 + r, b); }, ax, mx);
            abs_and_mask([&](int q, int a) __attribute__((always_inline)) { return G.dc(jl0 + q, a); }, ay, my);
            const uint32_t* dp = X.Dt + lr * D::HP + lc * CH;
            uint8_t* ob = X.outt + il0 * D::OUT_PITCH + ophase + jl0 * CH;
            float dist[4 * CH];                                  // [c][r][q]
            float dmax = 0.0f;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                float v[4], fy[2][4], fx[2][4];
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const uint32_t d = dp[b * D::HP + a * CH + c];
                        v[a * 2 + b] = (float)(d >> 24);
                        const float alpha = s3::lin_alpha_u8((float)(d & 0xFFu), ms255);
#pragma unroll
                        for (int q = 0; q < 2; ++q) fy[q][a * 2 + b] = s3::lin_factor_abs(alpha, ay[q][a], my[q][a]);
#pragma unroll
                        for (int r = 0; r < 2; ++r) fx[r][a * 2 + b] = s3::lin_factor_abs(alpha, ax[r][b], mx[r][b]);
                    }
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        float e[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) e[k] = fx[r][k] * fy[q][k];
                        const bool have = (r == 0 || two_r) && (q == 0 || two_c);
                        put_block_byte(s3::finish<false, 4, true, true, true>(e, v), have, ob + r * D::OUT_PITCH + q * CH + c,
                                       dist[(c * 2 + r) * 2 + q], dmax);
                    }
            }
            if (dmax > 0.5f - s3::kTieEps && X.guard)
                queue_ties(X, P, tie_mask(dist),
                           [&](int q, int& il, int& xc) __attribute__((always_inline)) { il = il0 + ((q >> 1) & 1); xc = (jl0 + (q & 1)) * CH + (q >> 2); },
                           [&](int q, uint32_t r8) __attribute__((always_inline)) { ob[((q >> 1) & 1) * D::OUT_PITCH + (q & 1) * CH + (q >> 2)] = (uint8_t)r8; });
        }
    }
}

// ---- the LDS image of the output block -> the frame: whole 16-byte chunks with streaming stores, the ragged ends of a
//      row (the neighbouring tiles' bytes share those chunks) dword by dword and byte by byte
template <typename X_>
__device__ __forceinline__ void flush_blocks(const X_& X, int tid) {
    using D = typename X_::D;
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    const int ophase = X.ophase, ncolc = X.ncolc, nrow = X.nrow;
    const int64_t rowpitch = X.rowpitch;
    const uint8_t* outt = X.outt;
    const int nchunk = (ophase + ncolc + 15) >> 4;
    const MagicDiv by_nchunk(nchunk);
    uint8_t* gbase = X.seg0 - ophase;
    const int total = nrow * nchunk;
    const int full_lo = ophase == 0 ? 0 : 1, full_hi = ((ophase + ncolc) & 15) == 0 ? nchunk : nchunk - 1;   // whole chunks of a row
    for (int i = tid; i < total; i += NT) {
        const int row = by_nchunk.div(i);
        const int ch = i - row * nchunk;
        if (ch >= full_lo && ch < full_hi) {
            const v4u x = *reinterpret_cast<const v4u*>(outt + row * D::OUT_PITCH + ch * 16);
            uint8_t* dst = gbase + row * rowpitch + ch * 16;
            // streaming stores for the 64-byte lines this tile writes completely; the first and the last line of a row
            // are shared with the neighbouring tiles and go through the L2 (regular stores), which merges the two
            // tiles' halves into one line -- as streaming stores they were two partial-line writes each (+67 MB per step)
            const uintptr_t line = reinterpret_cast<uintptr_t>(dst) & ~(uintptr_t)63;
            const uintptr_t r0 = reinterpret_cast<uintptr_t>(gbase + row * rowpitch) + (uintptr_t)ophase;
            if (line >= r0 && line + 64 <= r0 + (uintptr_t)ncolc) __builtin_nontemporal_store(x, reinterpret_cast<v4u*>(dst));
            else *reinterpret_cast<v4u*>(dst) = x;
        }
    }
    // the ragged chunks, two per row at most, in a loop of their own (a few waves take it once, instead of every
    // wave dragging the byte path through every round of the loop above)
    for (int i = tid; i < 2 * nrow; i += NT) {
        const int row = i >> 1;
        const int ch = (i & 1) ? nchunk - 1 : 0;
        if (ch >= full_lo && ch < full_hi) continue;             // that end of the row is a whole chunk
        if ((i & 1) && nchunk == 1) continue;                    // a one-chunk row: its first-chunk lane has it
        const uint8_t* src = outt + row * D::OUT_PITCH + ch * 16;
        uint8_t* dst = gbase + row * rowpitch + ch * 16;
        const int lo = max(ophase - ch * 16, 0), hi = min(ophase + ncolc - ch * 16, 16);
        const v4u x = *reinterpret_cast<const v4u*>(src);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t w = x[k];
            if (lo <= 4 * k && hi >= 4 * k + 4) {
                *reinterpret_cast<uint32_t*>(dst + 4 * k) = w;
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (4 * k + u >= lo && 4 * k + u < hi) dst[4 * k + u] = (uint8_t)(w >> (8 * u));
            }
        }
    }
}

// ---- tie pass: the queued outputs in float64, one per lane.  IMAGE (block forms): each patches its byte in the LDS image,
//      between two barriers, before the image leaves in one piece.  Otherwise each patches its byte in the frame, behind the
//      task loop's dword stores (drained and fenced by the barrier).
template <bool IMAGE, typename X_>
__device__ __forceinline__ void stage3_ties(const X_& X, const Params& P, int tid) {
    using D = typename X_::D;
    if (IMAGE) {
        __syncthreads();
        LERF_STAMP(15);
    }
    if (!X.guard) return;
    if (!IMAGE) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    const int nq = min(*X.tq_count, P.tq_cap);
    for (int i = tid; i < nq; i += NT) {
        const uint32_t e = X.tq[i];
        const int il = (int)(e >> 16), xc = (int)(e & 0xFFFFu);
        const uint8_t r8 = resolve_output(X, P.max_sigma, il, xc);
        if (IMAGE) X.outt[il * D::OUT_PITCH + X.ophase + xc] = r8;
        else X.seg0[il * X.rowpitch + xc] = r8;
    }
    if (IMAGE && nq > 0) __syncthreads();
}

// KINDW = LERF_KIND_* (| LERF_FUSED_WARP: stage 3 is the homographic warp of the tile's own output pixels, warp_tile())
constexpr int LERF_FUSED_WARP = 16;
// X2: the exact-x2 flavour -- whole frames at scale 2.0 on both axes (LERF_GEO_EXACT_X2): stage 3 takes its geometry from the
// closed form (GeoX2) instead of the caller's tables: no search in left_r / left_c, no staging of the tile's slices, no census
template <int S, int KINDW, bool EMIT, bool FROM_FEAT = false, bool GEN = false, bool X2 = false>
__global__ void __launch_bounds__(NT)
sr_fused_kernel(Params P, std::conditional_t<GEN, RaggedTable, NoTable> T) {
    constexpr int KIND = KINDW & 15;
    constexpr bool WARP = (KINDW & LERF_FUSED_WARP) != 0;
    static_assert(!X2 || (!EMIT && !WARP && CH == 3 && S == 2), "exact-x2 flavour: the RGB SR kernels that run stage 3, 2 x 2 support");
    static_assert(!X2 || Dims<S, GEN, EMIT>::GEO_EARLY, "exact-x2 flavour: the specialised RGB layout (geometry slot early: nothing to stage late)");
    static_assert(!WARP || (!EMIT && S == 2 && CH == 3 && !GEN), "tile-fused warp: RGB, 2 x 2 support, specialised kernel");
    using D = Dims<S, GEN, EMIT>;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x;

    int bid = xcd_order((int)blockIdx.x, (int)gridDim.x);
    const FrameView F = frame_view<GEN>(P, T, bid);
    const int tyi = bid / F.tiles_x, txi = bid - tyi * F.tiles_x;
    const int ty0 = P.ty_org + tyi * TH, tx0 = P.tx_org + txi * TW;
    const int H = F.H, W = F.W;
    const uint8_t* __restrict__ img = F.img;
    uint8_t* __restrict__ outp = F.out;

    // region origins in frame coordinates
    const int hy0 = ty0 - D::HR, hx0 = tx0 - D::HR;
    const int fy0 = ty0 - D::R3 - R2, fx0 = tx0 - D::R3 - R2;
    const int iy0 = fy0 - R1, ix0 = fx0 - R1;

    uint8_t* Bt = smem + D::OFF_B;
    int* ctl = reinterpret_cast<int*>(smem + D::OFF_CTL);
    // interior tile: the whole input region lies inside the frame, so no coordinate is ever clamped and the
    // centre addresses reduce to a multiply-add (center_addr's H < 0 path); ~80 % of the tiles of a 1080p frame
    const bool interior = FROM_FEAT ? (fy0 >= 0 && fx0 >= 0 && fy0 + D::FY <= F.H && fx0 + D::FX <= F.W)
                                    : (iy0 >= 0 && ix0 >= 0 && iy0 + D::IY <= F.H && ix0 + D::IX <= F.W);
    const int Hc = interior ? -1 : F.H, Wc = F.W;

    LERF_STAMP_RT(13);
    LERF_STAMP(0);
#ifdef LERF_STAMPS
    if (tid == 0) { P.stamps[(size_t)blockIdx.x * 16 + 8] = 0; P.stamps[(size_t)blockIdx.x * 16 + 9] = 0; P.stamps[(size_t)blockIdx.x * 16 + 15] = 0; }
#endif
    // ---- the feat tile: stage 1 on the input tile (the geometry search rides behind the tile's loads, the staging of its
    //      results, which are in ctl by then, behind phase s), or the output of the stage-1 launch
    // (shorthands: the search and the staging are called early for S = 2 RGB -- under stage 1 or the feat load -- and late otherwise)
    auto geo_search = [&]() { stage3_geo_search<D, X2>(F, tyi, txi, ty0, tx0, ctl, tid); };
    auto geo_stage = [&]() { if constexpr (!X2) stage3_geo_stage<D, S, KIND>(smem, F, P.max_sigma, hy0, hx0, ctl, tid); };
    auto early_search = [&]() { if (D::GEO_EARLY && !EMIT && !WARP) geo_search(); };
    if constexpr (!FROM_FEAT) {
        stage1<D, GEN, false, false>(smem, P, img, H, W, fy0, fx0, interior, Bt, tid, early_search, [&](int k) {
            if (k == 0) {
                if (D::GEO_EARLY && !EMIT && !WARP) geo_stage();
                LERF_STAMP(1);
            } else {
                LERF_STAMP(1 + k);                                   // 2 .. 6: the phases and LUT stores of the specialised kernels
            }
        });
    } else {
        load_feat_tile<D>(Bt, F.feat, H, W, fy0, fx0, interior, tid, early_search);
        __syncthreads();
        if (D::GEO_EARLY && !EMIT && !WARP) geo_stage();
        LERF_STAMP(6);
    }

    uint32_t* Dt = reinterpret_cast<uint32_t*>(smem + D::OFF_D);

    // image byte stage 3 sees at a hyper-region position OUTSIDE the frame: np.pad(input, pad_vec, mode=self.pad_mode)
    // (resize_right2d_numpy.py:143, 208) -- zero for the default "constant", otherwise the feat byte at the remapped
    // coordinate (inside the feat tile for edge / reflect / symmetric; wrap may reach the far side of the frame, which
    // the two-launch path reads from the stage-1 output in HBM)
    const int pad_mode = P.pad_mode;
    auto outside_pixel = [&](int gy, int gx, int c) -> uint32_t {
        if (pad_mode == LERF_PAD_CONSTANT) return 0u;
        bool zy, zx;
        const int sy = pad_index(gy, H, pad_mode, &zy), sx = pad_index(gx, W, pad_mode, &zx);
        const int ry = sy - fy0, rx = sx - fx0;
        if (ry >= 0 && ry < D::FY && rx >= 0 && rx < D::FX) return (uint32_t)Bt[ry * D::FP + rx * CH + c];
        if (FROM_FEAT) return (uint32_t)F.feat[((int64_t)sy * W + sx) * CH + c];
        return 0u;                      // not reached: the host sends wrap padding through the two-launch path
    };

    // ---- stage 2: the hyper region's packed dwords
    if constexpr (KIND == LERF_KIND_LINEAR)
        stage2_linear<D, GEN, FROM_FEAT>(smem, P, Bt, Dt, F.feat, W, hy0, hx0, fy0, fx0, interior, Hc, Wc, tid, outside_pixel);
    else
        stage2_gauss<D, GEN, X2>(smem, P, Bt, Dt, hy0, hx0, fy0, fx0, Hc, Wc, tid);
    if (!EMIT && !WARP && KIND == LERF_KIND_GAUSS && Hc >= 0) fill_outside<D>(Dt, hy0, hx0, H, W, tid, outside_pixel);

    if constexpr (WARP) {
        // ---- stage 3 of the warp: the output pixels this tile owns, taps from the tile's packed dwords in LDS
        __syncthreads();
        warp_tile<KIND, D::HP>(P, Dt, hy0, hx0, ty0, tx0, H, W, tyi * F.tiles_x + txi, outp, tid);
        return;
    }
    if (EMIT) {
        emit_tile<D>(Dt, F.emit, H, W, ty0, tx0, tid);
        return;
    }

    // ---- stage 3 geometry of the owned output block (staged here for S = 4; S = 2 did it at kernel start)
    if (!D::GEO_EARLY) {
        geo_search();
        __syncthreads();
        geo_stage();
    }
    __syncthreads();
    using X3 = Stage3<D, S, KIND, X2>;
    X3 X(smem, P, F, outp, ctl, ty0, tx0);
    LERF_STAMP(11);
    // ---- stage 3: the row-group table and the census of the tile's rows and columns, then the cheapest task form they allow
    //      (all forms give the same bytes), then the outputs the float32 path could not decide
    if constexpr (!X2) {
        stage3_census(X, ctl, tid);
        __syncthreads();
    }
    X.read_census(ctl);
    const bool image_ok = X.rows_align && (X.rowpitch & 15) == 0 && X.nrow <= D::OUT_ROWS && X.ophase + X.ncolc <= D::OUT_PITCH;
    const bool blk = X3::BLK && image_ok && X.rcode != 0 && X.ccode != 0;
    // interior tiles: pairs from row 0 / column 0 on, even counts -- no validity tests; tiles at the frame's edges: a leading
    // and / or trailing single row or column, handled as a pair whose other member is not stored
    const bool blk_uni = blk && X.rcode == 1 && X.ccode == 1 && ((X.nrow | X.ncol) & 1) == 0;
    const bool quad = X3::QUADS && blk_uni && __builtin_amdgcn_readfirstlane(ctl[CTL_CSTEP]) != 0 && __builtin_amdgcn_readfirstlane(ctl[CTL_RSTEP]) != 0 &&
                      ((X.nrow >> 1) % X3::QRP) == 0 && ((X.ncol >> 1) % X3::QCP) == 0;
    const bool blkl = X3::BLKL && __builtin_amdgcn_readfirstlane((image_ok && X.lin_ok) ? 1 : 0) != 0;
    // the constant-size variants of the dword-column tasks cover the integer scale factors (x2 -> 2 rows per group, ...);
    // anything else reads the group size per task
    constexpr bool WIDE = KIND == LERF_KIND_GAUSS && S == 2;      // x3 / x4 variants where the registers allow
    // (max_sigma <= s3::kNoShiftMaxSigma here: the host sends larger values to the float64 direct kernel, lerf_fused.hip)
    if (quad) stage3_quads(X, P, tid);
    else if (blk_uni) stage3_blocks<true>(X, P, tid);
    else if (blk) stage3_blocks<false>(X, P, tid);
    else if (blkl) stage3_blocks_lin(X, P, ctl, tid);      // (ctl: it reads CTL_NCGRP itself -- read for every tile it cost SGPR spills, profiles/stage3_calls_resources.txt)
    else if (X.gsame == 2) stage3_tasks<2>(X, P, tid);
    else if (WIDE && X.gsame == 3) stage3_tasks<WIDE ? 3 : 0>(X, P, tid);
    else if (WIDE && X.gsame == 4) stage3_tasks<WIDE ? 4 : 0>(X, P, tid);
    else stage3_tasks<0>(X, P, tid);
    if (blk || blkl) {
        // block tasks: the queued outputs are patched in the LDS image, which then leaves in one piece
        stage3_ties<true>(X, P, tid);
        flush_blocks(X, tid);
    } else {
        stage3_ties<false>(X, P, tid);
    }
#ifdef LERF_STAMPS
    __syncthreads();
    LERF_STAMP(12);
    LERF_STAMP_RT(14);
#endif
}

// ---------------------------------------------------------------------------
// stage 1 alone, one 64x64 block per workgroup with no halo (two-launch path): input tile (block + 3 px) -> the
// three byte LUTs, 4 rotations each -> feat bytes to P.feat.  Same phases as in sr_fused_kernel.
// ---------------------------------------------------------------------------
constexpr int up16c(int x) { return (x + 15) / 16 * 16; }
struct DimsA {
    static constexpr int FY = TH, FX = TW, FP = FX * CH, NF = FY * FP;
    static constexpr int IY = FY + 2 * R1, IX = FX + 2 * R1, IPB = IX * CH, IP = (IPB + 3 + 3) / 4 * 4, NI = IY * IP;
    static constexpr int OFF_LUT = 0;
    static constexpr int OFF_C = LUT_PAD;
    static constexpr int OFF_ACC = OFF_C + up16c(NI);
    static constexpr int OFF_F = OFF_ACC + up16c(NF * 2);
    static constexpr int LDS_BYTES = OFF_F + up16c(NF);
};

template <bool GEN = false>
__global__ void __launch_bounds__(NT)
s1_kernel(Params P, std::conditional_t<GEN, RaggedTable, NoTable> T) {
    using D = DimsA;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x;
    int bid = xcd_order((int)blockIdx.x, (int)gridDim.x);
    const FrameView F = frame_view<GEN>(P, T, bid);
    const int tyi = bid / F.tiles_x, txi = bid - tyi * F.tiles_x;
    // (P.ty_org, P.tx_org) = origin of the stage-1 region: (0, 0) for whole frames, the region of interest widened by the
    // reach of stages 2 + 3 for a rank's block (launch_fused_t)
    const int fy0 = P.ty_org + tyi * TH, fx0 = P.tx_org + txi * TW;
    const int iy0 = fy0 - R1, ix0 = fx0 - R1;
    const int H = F.H, W = F.W;
    const uint8_t* __restrict__ img = F.img;
    const bool interior = iy0 >= 0 && ix0 >= 0 && iy0 + D::IY <= H && ix0 + D::IX <= W;
    uint8_t* Ft = smem + D::OFF_F;
    LERF_STAMP(0);
    // positions outside the frame are not evaluated; interior tiles read their pixels over the vector-memory path
    stage1<D, GEN, true, true>(smem, P, img, H, W, fy0, fx0, interior, Ft, tid, []() {}, NoMark{});
    LERF_STAMP(1);
    // the block's rows to P.feat
    uint8_t* __restrict__ fdst = F.feat;
    const int rows = min(TH, H - fy0), cols3 = min(TW, W - fx0) * CH;
    const bool dwords = cols3 == D::FP && ((W * CH) & 3) == 0 && (reinterpret_cast<uintptr_t>(F.feat) & 3) == 0;
    if (dwords) {
        constexpr int RD = D::FP / 4;
        uint32_t* dst = reinterpret_cast<uint32_t*>(fdst + ((int64_t)fy0 * W + fx0) * CH);
        const int rowdw = (W * CH) >> 2;
        for (int i = tid; i < rows * RD; i += NT) {
            const int r = i / RD;
            __builtin_nontemporal_store(reinterpret_cast<const uint32_t*>(Ft)[i], &dst[(int64_t)r * rowdw + (i - r * RD)]);
        }
    } else {
        for (int i = tid; i < rows * cols3; i += NT) {
            const int r = i / cols3, c3 = i - r * cols3;
            fdst[((int64_t)(fy0 + r) * W + fx0) * CH + c3] = Ft[r * D::FP + c3];
        }
    }
#ifdef LERF_STAMPS
    __syncthreads();
    LERF_STAMP(2);
#endif
}

#undef LERF_ADDTID
#undef LERF_ADDTID4
#undef LERF_SET_M0


// ---------------------------------------------------------------------------
// host side of this instance
// ---------------------------------------------------------------------------
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per kernel and device instead of once per launch
template <auto KERN>
static int ensure_lds(int bytes) {
    static std::atomic<uint64_t> done{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return LERF_ELAUNCH;
    const uint64_t bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_relaxed) & bit) return LERF_OK;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess)
        return LERF_ELAUNCH;
    done.fetch_or(bit, std::memory_order_relaxed);
    return LERF_OK;
}

inline size_t feat_slice_bytes(int H, int W) { return ((size_t)H * W * CH + 15) / 16 * 16; }

template <int S, int KIND, bool EMIT, bool GEN, bool X2 = false>
static int launch_fused_t(const FusedArgs& a, hipStream_t st) {
    using D = Dims<S, GEN, EMIT>;
    using TableT = std::conditional_t<GEN, RaggedTable, NoTable>;
    const lerf_luts_t* L = a.luts;
    Params P{};
    P.tq_cap = a.tq_cap == 0 ? D::TQ_CAP : (a.tq_cap < 0 ? 0 : (a.tq_cap > D::TQ_CAP ? D::TQ_CAP : a.tq_cap));
    P.pad_mode = a.pad_mode;
    P.host_input = a.host_input ? 1 : 0;
    P.out_pitch = a.out_pitch;
    P.img = a.img; P.in_sn = a.in_sn; P.out = a.out; P.out_sn = a.out_sn;
    P.H = a.H; P.W = a.W; P.oH = a.oH; P.oW = a.oW;
    const bool roi = a.roi_h > 0 && a.roi_w > 0;
    P.ty_org = roi ? a.roi_y : 0; P.tx_org = roi ? a.roi_x : 0;
    P.tiles_y = ((roi ? a.roi_h : a.H) + TH - 1) / TH;
    P.tiles_x = ((roi ? a.roi_w : a.W) + TW - 1) / TW;
    P.pack = (const uint8_t*)L->fused_pack;
    P.left_r = a.left_r; P.dis_r = a.dis_r; P.left_c = a.left_c; P.dis_c = a.dis_c;
    P.dis_r64 = a.dis_r64; P.dis_c64 = a.dis_c64;
    P.max_sigma = a.max_sigma;
    P.n1 = L->n_modes1; P.n2 = L->n_modes2;
    P.stamps = EMIT ? nullptr : (unsigned long long*)a.workspace;
    for (int l = 0; l < 2 * P.n2; ++l) pattern_tables(L->modes2[l >> 1], l & 1, 2, 2, D::FP, P.s2off[l], P.s2dyx[l]);
    P.emit = (uint32_t*)a.emit; P.emit_sn = a.emit_sn;
    P.feat = nullptr; P.feat_sn = 0;
    if constexpr ((KIND & LERF_FUSED_WARP) != 0) {
        if (!a.wgeo || !a.wboxes || a.workspace == nullptr || a.roi_h > 0 || a.items != nullptr) return LERF_EINVAL;
        P.wgeo = *a.wgeo;
        P.wboxes = a.wboxes;
    }
    auto set_s1off = [&](Params& Q, int ip) {          // stage-1 pattern offsets; ip = pitch of the input tile of the kernel that runs it
        for (int m = 0; m < Q.n1; ++m) pattern_tables(L->modes1[m], 0, 1, 4, ip, Q.s1off[m], Q.s1dyx[m]);
    };
    set_s1off(P, D::IP);
    bool two = a.workspace != nullptr && !(a.flags & LERF_GEO_SINGLE_LAUNCH);
#ifdef LERF_STAMPS
    // diagnostic build: the stamps live at the START of the workspace -- [n x tiles x 16] of the stages-2+3 (or single) launch,
    // then [n x stage-1 blocks x 16] of s1_kernel, then (two launches) the stage-1 output.  A workspace too small for
    // all three keeps the single launch (tools/stamps.py sizes it).
    size_t stamp_bytes = 0;
    {
        const size_t per = 16 * sizeof(unsigned long long);
        const size_t nb = (size_t)a.n * P.tiles_y * P.tiles_x;
        stamp_bytes = ((2 * nb + nb / 4 + 64) * per + 255) & ~(size_t)255;   // both areas (the stage-1 grid of a region is a little larger)
        two = two && a.items == nullptr && !EMIT && a.workspace_bytes >= stamp_bytes + (size_t)a.n * feat_slice_bytes(a.H, a.W);
    }
#endif
    auto ka = s1_kernel<GEN>;
    auto kb = sr_fused_kernel<S, KIND, EMIT, true, GEN, X2>;
    auto kc = sr_fused_kernel<S, KIND, EMIT, false, GEN, X2>;
    int rc;
    if (two) {
        if ((rc = ensure_lds<s1_kernel<GEN>>(DimsA::LDS_BYTES)) != LERF_OK) return rc;
        if ((rc = ensure_lds<sr_fused_kernel<S, KIND, EMIT, true, GEN, X2>>(D::LDS_BYTES)) != LERF_OK) return rc;
    } else if ((rc = ensure_lds<sr_fused_kernel<S, KIND, EMIT, false, GEN, X2>>(D::LDS_BYTES)) != LERF_OK) return rc;

    if constexpr (GEN && !X2) {
        if (a.items != nullptr) {
            // frames of different sizes: chunks of RAGGED_MAX descriptors per launch (pair)
            size_t ws_off = 0;
            for (int i0 = 0; i0 < a.n_items; i0 += RAGGED_MAX) {
                RaggedTable T{};
                T.n = a.n_items - i0 < RAGGED_MAX ? a.n_items - i0 : RAGGED_MAX;
                int64_t blocks = 0;
                for (int k = 0; k < T.n; ++k) {
                    const FusedItem& it = a.items[i0 + k];
                    FrameDesc& d = T.d[k];
                    d.img = it.img; d.out = it.out; d.emit = (uint32_t*)it.emit;
                    d.left_r = it.left_r; d.dis_r = it.dis_r; d.left_c = it.left_c; d.dis_c = it.dis_c;
                    d.dis_r64 = (it.dis_r64 && it.dis_c64) ? it.dis_r64 : nullptr;
                    d.dis_c64 = (it.dis_r64 && it.dis_c64) ? it.dis_c64 : nullptr;
                    d.H = it.H; d.W = it.W; d.oH = it.oH; d.oW = it.oW;
                    d.tiles_x = (it.W + TW - 1) / TW; d.tiles_y = (it.H + TH - 1) / TH;
                    d.first_block = (int)blocks;
                    blocks += (int64_t)d.tiles_x * d.tiles_y;
                    d.feat = two ? (uint8_t*)a.workspace + ws_off : nullptr;
                    if (two) ws_off += feat_slice_bytes(it.H, it.W);
                }
                if (blocks > 0x7FFFFFFF) return LERF_EUNSUPPORTED;
                // every tile of the tie guard needs both float64 tables: the kernel tests P.dis_r64 (set per frame)
                if (two) {
                    Params Pa = P;
                    set_s1off(Pa, DimsA::IP);
                    hipLaunchKernelGGL(ka, dim3((unsigned)blocks), dim3(NT), DimsA::LDS_BYTES, st, Pa, T);
                    hipLaunchKernelGGL(kb, dim3((unsigned)blocks), dim3(NT), D::LDS_BYTES, st, P, T);
                } else {
                    hipLaunchKernelGGL(kc, dim3((unsigned)blocks), dim3(NT), D::LDS_BYTES, st, P, T);
                }
            }
            return LERF_OK;
        }
    }
    const int64_t blocks = (int64_t)a.n * P.tiles_y * P.tiles_x;
    if (blocks > 0x7FFFFFFF) return LERF_EUNSUPPORTED;
    TableT T{};
    // two launches when the caller's workspace can hold the stage-1 output of the batch: stage 1 without halo
    // recomputation, then stages 2+3 from it
    if (two) {
        P.feat = (uint8_t*)a.workspace;
#ifdef LERF_STAMPS
        P.feat += stamp_bytes;
#endif
        P.feat_sn = (int64_t)feat_slice_bytes(a.H, a.W);
        Params Pa = P;
#ifdef LERF_STAMPS
        Pa.stamps = P.stamps + (size_t)blocks * 16;
#endif
        set_s1off(Pa, DimsA::IP);
        int64_t blocks1 = blocks;
        if (roi) {
            // region of interest: stage 1 over the region widened by the reach of stages 2 + 3 (whole 64 x 64 blocks from an
            // origin on a 4-pixel boundary, so that the feat rows keep their aligned dword stores; a block that reaches past
            // the widened region computes valid stage-1 values nobody reads)
            const int reach = R2 + D::R3;
            const int y0 = a.roi_y - reach > 0 ? a.roi_y - reach : 0, x0 = a.roi_x - reach > 0 ? (a.roi_x - reach) & ~3 : 0;
            const int y1 = a.roi_y + a.roi_h + reach < a.H ? a.roi_y + a.roi_h + reach : a.H;
            const int x1 = a.roi_x + a.roi_w + reach < a.W ? a.roi_x + a.roi_w + reach : a.W;
            Pa.ty_org = y0; Pa.tx_org = x0;
            Pa.tiles_y = (y1 - y0 + TH - 1) / TH; Pa.tiles_x = (x1 - x0 + TW - 1) / TW;
            blocks1 = (int64_t)a.n * Pa.tiles_y * Pa.tiles_x;
            if (blocks1 > 0x7FFFFFFF) return LERF_EUNSUPPORTED;
        }
        hipLaunchKernelGGL(ka, dim3((unsigned)blocks1), dim3(NT), DimsA::LDS_BYTES, st, Pa, T);
        hipLaunchKernelGGL(kb, dim3((unsigned)blocks), dim3(NT), D::LDS_BYTES, st, P, T);
        return LERF_OK;
    }
    hipLaunchKernelGGL(kc, dim3((unsigned)blocks), dim3(NT), D::LDS_BYTES, st, P, T);
    return LERF_OK;
}

// The exact-x2 flavour serves a launch whose caller vouches for x2 tables of the whole frame (LERF_GEO_EXACT_X2) and whose
// sizes say the same: out = 2 x in on both axes, no region of interest (a region's owned ranges start at arbitrary origins: it
// keeps the table path), one frame size.  A set bit with other sizes runs the table path.  LERF_GEO_FORCE_TABLES: diagnostic.
// The 2 x 2 support only (LeRF-G and LeRF-L): the 4 x 4 kernels have no register for the closed form's constants.
static bool takes_x2(const FusedArgs& a) {
    if (!(a.flags & LERF_GEO_EXACT_X2) || (a.flags & LERF_GEO_FORCE_TABLES) || CH != 3 || a.items != nullptr) return false;
    if (a.S != 2) return false;
    if (a.roi_h > 0 && a.roi_w > 0) return false;
    return (int64_t)a.oH == 2 * (int64_t)a.H && (int64_t)a.oW == 2 * (int64_t)a.W;
}

// dispatch over (support, kind) for one (EMIT, GEN) family of this instance
template <bool GEN>
static int launch_sr(const FusedArgs& a, hipStream_t st) {
#ifdef LERF_FUSED_X2          // (lerf_fused.hip: the specialised RGB kernels, 64-row tiles)
    if (takes_x2(a)) {
        if (a.kind == LERF_KIND_GAUSS) return launch_fused_t<2, LERF_KIND_GAUSS, false, GEN, true>(a, st);
        if (a.kind == LERF_KIND_LINEAR) return launch_fused_t<2, LERF_KIND_LINEAR, false, GEN, true>(a, st);
        return LERF_EUNSUPPORTED;
    }
#endif
    if (a.kind == LERF_KIND_GAUSS) {
        if (a.S == 2) return launch_fused_t<2, LERF_KIND_GAUSS, false, GEN>(a, st);
        if (a.S == 4) return launch_fused_t<4, LERF_KIND_GAUSS, false, GEN>(a, st);
    } else if (a.kind == LERF_KIND_LINEAR) {
        if (a.S == 2) return launch_fused_t<2, LERF_KIND_LINEAR, false, GEN>(a, st);
    }
    return LERF_EUNSUPPORTED;
}
#ifdef LERF_FUSED_WITH_WARP
static int launch_warp(const FusedArgs& a, hipStream_t st) {
    if (a.kind == LERF_KIND_GAUSS) return launch_fused_t<2, LERF_KIND_GAUSS | LERF_FUSED_WARP, false, false>(a, st);
    if (a.kind == LERF_KIND_LINEAR) return launch_fused_t<2, LERF_KIND_LINEAR | LERF_FUSED_WARP, false, false>(a, st);
    return LERF_EUNSUPPORTED;
}
#endif
template <bool GEN>
static int launch_stages(const FusedArgs& a, hipStream_t st) {
    if (a.luts->oC == 3) return launch_fused_t<2, LERF_KIND_GAUSS, true, GEN>(a, st);
    if (a.luts->oC == 1) return launch_fused_t<2, LERF_KIND_LINEAR, true, GEN>(a, st);
    return LERF_EUNSUPPORTED;
}

}  // namespace LERF_FUSED_NS
}  // namespace lerf
