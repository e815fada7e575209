// Coordinate maps built, upsampled, composed and inverted on the device: the maps lerf_remap reads (lerf_remap_geo_t.coords), written by
// kernels instead of host numpy + an upload.  The arithmetic of every entry is lerf_coords_models.h (float64, + - * / only, no
// FMA contraction; the fisheye and equirect models, codes 16 and 17, take their square root and arc tangents from the same header,
// not from a math library).
//
// ONE TEXT FOR DEVICE AND HOST.  Every one-thread-per-entry operation is a small functor op(i, j, s) -- entry (i, j) of set s -- that
// holds its operands by value (BuildOp, BuildDevOp, ReprojectOp, MeshOp, ComposeOp, InvertOp, ComposeBwdOp, InvertBwdOp, SplatOp, SplatBwdOp; the
// notes on loads, stores and atomics are with each).  Two runners with one call shape execute it:
//   OnDevice{stream}   launches entry_kernel<OP>: block 64 x 4 (4 waves, one row of 64 entries each, so a wave's stores are 64
//                      consecutive entries of a row), grid (ceil(oW / 64), ceil(oH / 4), sets), the (i, j) guard, blockIdx.z = the set
//   OnHost{}           the plain s, i, j loop over host pointers
// A BATCH is the same launch with sets > 1: every chained operation (mesh, compose, invert, the two adjoints, the three passes of the
// rasteriser, the two passes of the mesh adjoint) takes one set stride per operand, set s works on base + s * set_stride, and the
// single-map entry points are n_sets = 1 of the same code.  The set is blockIdx.z, so the offsets are scalar.
// and every operation is ONE function template over the runner (coords::build, mesh, compose, ...): the argument checks, the dtype and
// model dispatch, run(Op{...}, oH, oW[, sets]).  The C entry points lerf_coords_X_batched / lerf_coords_X_batched_host are that template
// with one runner or the other, and lerf_coords_X / lerf_coords_X_host call those with n_sets = 1 and set strides 0, so the device and
// the host twin, the single map and the batch cannot drift apart: they agree bit for bit by construction (the two float scatters
// excepted, below).  THE ARGUMENT CHECKS are one operand table per call (Operand, check_call, after the kernels):
// an entry point lists its operands with their roles and its scalar rules ONCE, and one function judges them; which operands may
// intersect is derived from the roles (a WRITTEN operand intersects no other), not listed.  Add2 is the float scatter of the map adjoints: two float64 atomicAdd where compiled for the device, a plain add on the host; AddPlane is the same pattern for one plane of an image (the forward warp, lerf_splat; its arithmetic is lerf_splat_point.h).
// The three float scatters (SplatOp, ComposeBwdOp, InvertBwdOp) also run under a THIRD pair of runners, OrderedOnDevice / OrderedOnHost
// (after the scatter runners): the same op four times over a caller-owned workspace -- count, scan, fill, sort and sum (ordered_passes_
// device / _host) -- which adds in the host twin's order and so IS bit-equal to it (the _ordered entry points).
// MapReader is the one strided-map reader handed to the *_point functions; a dense float64 gradient [h][w][2] is a map of row stride 2w.
//
// The rasterising inverse (lerf_coords_invert_raster) is three passes: KeyFillOp and ResolveOp are per-entry functors under the two
// runners above; RasterOp is a SCATTER operation, one call per cell of F, under ScatterOnDevice{stream} (cell_kernel<OP>, the same
// block and grid, a 64-bit integer atomic min) / ScatterOnHost{} (the row-major loop, a plain min).  An integer minimum does not
// depend on the order of its operands, so this scatter IS bit-equal between the two and from run to run.
// The triangle-mesh rasteriser (lerf_coords_trimesh) draws an INDEXED mesh with the same per-pixel functions in five
// passes: KeyFillOp, TriCountOp and TriResolveOp are per-entry functors under the two runners; the raster pass is trimesh_raster_kernel,
// one wave per (face, 4 x 16 pixel tile) item of a scanned item list (TriRasterOnDevice), or the plain loop over faces and their boxes
// (TriRasterOnHost).  Its notes are with it, after the ordered scatter's scan.  Its adjoint (lerf_coords_trimesh_bwd) is a
// face pass of its own shape (trimesh_bwd_face_kernel: one workgroup per face, a fixed reduction tree) and the ordered scatter's four
// passes (the same two functions) over TriVertexOp, whose entries are the faces (TriBwdOnDevice / TriBwdOnHost, after the ordered runners).
//
// Kernels of their own shape (unchanged by the above):
//   coords_mesh_bwd_{rows,cols}_kernel      the adjoint of the mesh upsample, map = Wr . ctrl . Wc^T  =>  grad_ctrl = Wr^T . grad_map . Wc,
//                                           in two gather-shaped passes, each sum in a fixed order and without atomics:
//       rows   tmp[a][j] = sum_i Wr[i][a] grad_map[i][j]: a block owns vertex row a and 64 columns; its 4 waves take the rows of a's
//              reach i = lo + w, lo + w + 4, ... (any reach beyond 4 rows takes more than one pass of the block), every lane keeps
//              its own running sum, the 4 partial sums meet in LDS and wave 0 adds them in the order 0, 1, 2, 3
//       cols   grad_ctrl[a][b] += sum_j Wc[j][b] tmp[a][j]: ONE wave per vertex; lane l takes the columns lo + l, lo + l + 64, ...
//              (a reach beyond 64 columns takes more than one pass), then a shuffle tree (offsets 32, 16, .. 1), lane 0 is the
//              vertex's one writer (load-add-store: the accumulate contract of lerf_remap_bwd)
//       The weight Wr[i][a] is recomputed from mesh_axis -- the forward's own function -- for every row of a conservative reach
//       (mesh_reach); rows without a tap on a weigh exactly 0 and are skipped, so the transpose is exact, clamped border taps
//       of the bicubic included.  A 33 x 61 mesh under 2160 x 3840: 270 rows per vertex row in pass 1 (68 per wave), 252 columns per
//       vertex in pass 2 (4 per lane); grad_map is read 4 times (bicubic) or twice (bilinear), coalesced, tmp is 2 MB.
//   coords_build_bwd_{partial,sum}_kernel   the adjoint of the builders, grad_params[s][k] += sum over the entries of dp[k] (model_point_bwd):
//                                           a reduction of 9 / 8 / 21 / 17 / 13 sums over every entry, in two passes, fixed order, no atomics
//       partial  a block owns 64 columns x a band of 64 rows of one set; wave w takes the rows w, w + 4, ... of the band (16 per lane),
//                every lane keeps its n_params running sums in registers; a shuffle tree (offsets 32 .. 1) per sum, the 4 wave sums meet in
//                LDS and are added in the order 0, 1, 2, 3; ONE partial vector per block goes to the workspace ([set][k][block])
//       sum      ONE wave per (set, k): lane l adds the partials l, l + 64, ..., the same tree, lane 0 is the one writer (load-add-store)
//       2160 x 3840: 2 040 blocks a set in pass 1 (8 per CU), 343 KB of partials for the 21 sums of brown; grad_map is read once, coalesced
//       The host twin emulates the two passes lane by lane (two_pass_sums_host); the runner pair is TwoPassOnDevice / TwoPassOnHost.
//   coords_reproject_bwd_kernel             the adjoint of reproject: pass 1's grid, band and lanes over reproject_point_bwd; every lane adds d depth
//                                           into grad_depth at its own entries (one writer) and, when grad_params is wanted, keeps 12 running
//                                           sums that leave as the block's partial vector for coords_build_bwd_sum_kernel -- the same fixed order
//       2160 x 3840: 2 040 blocks a set, 196 KB of partials; depth, grad_map and grad_depth are each touched once, coalesced
//   coords_math_kernel                      sqrt_pm / atan_pm / atan2_pm of lerf_coords_models.h, one thread per element: what the fisheye and
//                                           equirect models are built on, exported so that their bit-equality with the host is tested directly
//
// Addresses: entry_kernel guards (i, j) against the tile; a functor writes entry (i, j) of `out` only, and reads ctrl / A at indices that
// mesh_axis / compose_axis clamp into the operand after clipping the position in floating point (no value of B reaches an int
// conversion unclipped).  The inverse reads init at entry (i, j) only and F at the three corners of its start and at cells
// compose_axis picks for the iterate (fH, fW >= 2, so i0 + 1 <= fH - 1), whatever F, init or the iterate hold.  The passes of the
// mesh adjoint index grad_map inside [oH][oW], tmp inside [gh][oW], grad_ctrl inside [gh][gw].  The adjoints of compose and invert read
// B / G, grad_out and grad_b at entry (i, j) only, and read A / F and add into grad_a / grad_f at the cell compose_axis picks (aH, aW,
// fH, fW >= 2 are checked on the host, so i0 + 1 <= n - 1), whatever the maps hold.  The kernels that read device parameters index
// params and grad_params inside [n_sets][n_params], out and grad_map at (set, i, j) with set < n_sets, i < oH, j < oW, the workspace
// inside [n_sets][n_params][blocks]; no parameter value forms an address.  The rasterising inverse: cell_kernel guards (i, j) against
// the cells [fH - 1][fW - 1] and reads F and depth at the cell's four corners; a triangle's pixel box is clipped onto the tile in
// floating point before its conversion to int (raster_axis), so keys is indexed inside [oH][oW] whatever F holds; the resolve reads
// keys at entry (i, j) and F at the three vertices of the triangle the key names -- a key this call's raster pass wrote, t < 2 (fH - 1)
// (fW - 1) -- and writes entry (i, j) of out.  coords_math_kernel reads x (and y, for atan2 only) and writes
// out at element e < n alone; no argument value forms an address.  In a batch every statement above holds inside set s of the operand, base + s * set_stride
// with s = blockIdx.z < n_sets: the host has checked that a set's extent lies inside its stride (or that the stride is 0 for an operand
// that may be shared), so set s ends before set s + 1 begins.
#include "lerf_common.h"
#include "lerf_coords_models.h"
#include "lerf_splat_point.h"

#include <cmath>
#include <initializer_list>
#include <vector>

namespace lerf {
namespace coords {

constexpr int CB_COLS = 64, CB_ROWS = 4;     // block = 4 waves, one row of 64 entries each

template <typename TO>
LERF_HD inline void store_entry(TO* out, int64_t stride, int i, int j, const Point& q) {
    Entry<TO> v;
    v.r = (TO)q.r;                               // float32: the float64 value rounded once, here
    v.c = (TO)q.c;
    *reinterpret_cast<Entry<TO>*>(out + (int64_t)i * stride + 2 * (int64_t)j) = v;
}

template <typename T>
LERF_HD inline Point load_entry(const T* m, int64_t stride, int i, int j) {
    const Entry<T> v = *reinterpret_cast<const Entry<T>*>(m + (int64_t)i * stride + 2 * (int64_t)j);
    return {(double)v.r, (double)v.c};
}

// a map operand under the strided contract, read at (row, col): what the *_point functions take as READ / LOAD
template <typename T>
struct MapReader {
    const T* m;
    int64_t stride;
    LERF_HD Point operator()(int r, int c) const { return load_entry(m, stride, r, c); }
    LERF_HD MapReader set(int s, int64_t set_stride) const;      // the reader of set s
};

// Operands of a batch: set s of an operand lies at base + s * set_stride elements; s is blockIdx.z on the device, so the offset is
// wave-uniform (scalar registers), and a single-map call is n_sets = 1 with every set stride 0.  A set stride of 0 shares the operand.
// s is never negative: multiplied as unsigned 32 x 64 bits, which spares the scalar unit the sign extension's multiply and add.
LERF_HD inline int64_t set_offset(int s, int64_t set_stride) { return (int64_t)((uint64_t)(uint32_t)s * (uint64_t)set_stride); }
template <typename T>
LERF_HD inline MapReader<T> MapReader<T>::set(int s, int64_t set_stride) const { return {m + set_offset(s, set_stride), stride}; }

// the scatter of the two adjoints: grad [h][w][2] dense float64.  Device: two float64 atomicAdd per tap into global memory -- equal
// from run to run up to the rounding of a reordered sum, like the image and hyper gradients of lerf_remap_bwd.  Host: a plain add.
struct Add2 {
    double* grad;
    int w;
    LERF_HD void operator()(int r, int c, double dr, double dc) const {
        double* p = grad + 2 * ((int64_t)r * w + c);
#ifdef __HIP_DEVICE_COMPILE__
        atomicAdd(p, dr);
        atomicAdd(p + 1, dc);
#else
        p[0] += dr;
        p[1] += dc;
#endif
    }
};

// The combiners of the ORDERED scatter (OrderedOnDevice / OrderedOnHost, after the runners): the three scatter operations hand their
// combiner calls to whatever apply() is given -- Add2 / AddPlane by default, or one of these.  Each answers both call shapes, the map
// adjoints' (row, col, dr, dc) over a frame `w` wide and the splat's (plane, q, v); q is the TARGET, the element index in its frame.
//   CountAt   pass 1: one uint32 atomic increment of count[q] per call (the splat runs with one plane: per tap, not per plane)
//   FillAt    pass 3: slot = cursor[q]++ (atomic, returning), list[slot] = e -- the entry that called
//   Keep2At / KeepPlaneAt   pass 4: the host branch of Add2 / AddPlane, a plain p = p + r into global memory, for calls whose target is
//             q and no other; the thread that owns q is the element's only writer
struct CountAt {
    uint32_t* count;
    int w;
    LERF_HD void bump(int64_t q) const {
#ifdef __HIP_DEVICE_COMPILE__
        atomicAdd(count + q, 1u);
#else
        count[q] += 1u;
#endif
    }
    LERF_HD void operator()(int r, int c, double, double) const { bump((int64_t)r * w + c); }
    LERF_HD void operator()(int k, int64_t q, double) const { if (k == 0) bump(q); }
};

struct FillAt {
    uint32_t* cursor;
    uint32_t* list;
    uint32_t e;
    int w;
    LERF_HD void put(int64_t q) const {
#ifdef __HIP_DEVICE_COMPILE__
        const uint32_t slot = atomicAdd(cursor + q, 1u);
#else
        const uint32_t slot = cursor[q]++;
#endif
        list[slot] = e;
    }
    LERF_HD void operator()(int r, int c, double, double) const { put((int64_t)r * w + c); }
    LERF_HD void operator()(int k, int64_t q, double) const { if (k == 0) put(q); }
};

struct Keep2At {
    double* grad;
    int w;
    int64_t q;
    LERF_HD void operator()(int r, int c, double dr, double dc) const {
#pragma clang fp contract(off)
        if ((int64_t)r * w + c != q) return;
        double* p = grad + 2 * q;
        p[0] = p[0] + dr;
        p[1] = p[1] + dc;
    }
    LERF_HD void poison() const { grad[2 * q] = grad[2 * q + 1] = __builtin_nan(""); }
};

template <typename T>
struct KeepPlaneAt {
    T* acc;
    int64_t plane, q;
    int planes;
    LERF_HD void operator()(int k, int64_t at, double v) const {
#pragma clang fp contract(off)
        if (at != q) return;
        T* p = acc + (int64_t)k * plane + q;
        const T r = (T)v;                            // rounded once, here: AddPlane's statement
        *p = *p + r;
    }
    LERF_HD void poison() const {
        for (int k = 0; k < planes; ++k) acc[(int64_t)k * plane + q] = (T)__builtin_nan("");
    }
};

// ------------------------------------------------------------------------------------------------ the per-entry operations
// the model's point of pixel (i0 + i, j0 + j), ONE 16-byte (float64) or 8-byte (float32) store; the parameters travel by value
template <int MODEL, typename TO>
struct BuildOp {
    Params prm;
    TO* out;
    int64_t stride;
    int i0, j0;
    LERF_HD void operator()(int i, int j, int) const { store_entry(out, stride, i, j, model_point<MODEL>(prm.p, i0 + i, j0 + j)); }
};

// BuildOp with the parameters in DEVICE memory, [n_sets][n_params] float64: set s reads its own at a wave-uniform address (scalar
// loads) and writes map s; model_point is called unchanged, so map s is bit-equal to lerf_coords_build of the same doubles
template <int MODEL, typename TO>
struct BuildDevOp {
    const double* params;
    TO* out;
    int64_t set_stride, stride;
    int i0, j0;
    LERF_HD void operator()(int i, int j, int s) const {
        const double* p = params + (size_t)s * model_params(MODEL);
        store_entry(out + (int64_t)s * set_stride, stride, i, j, model_point<MODEL>(p, i0 + i, j0 + j));
    }
};

// one entry of reproject (reproject_point): the set's 12 parameters at a wave-uniform address (scalar loads), ONE 4- or 8-byte load of
// the entry's depth (a wave reads 64 consecutive ones), one map store and, with depth_out, one 4-byte store of zo
template <int KIND, typename TD, typename TO>
struct ReprojectOp {
    const double* params;
    const TD* depth;
    TO* out;
    float* zo;
    int64_t depth_set, out_set, stride, zo_set;
    int oW, i0, j0;
    LERF_HD void operator()(int i, int j, int s) const {
        const int64_t e = (int64_t)i * oW + j;
        const Reprojected r = reproject_point<KIND>(params + (size_t)s * kReprojectParams, (double)depth[set_offset(s, depth_set) + e], i0 + i, j0 + j);
        store_entry(out + set_offset(s, out_set), stride, i, j, r.q);
        if (zo) zo[set_offset(s, zo_set) + e] = (float)r.zo;            // rounded once, here
    }
};

// 2 x 2 or 4 x 4 control entries per entry, read through the caches (the control mesh is small -- 33 x 61 x 2 doubles are 32 KB -- and
// neighbouring lanes read the same entries, so the loads are broadcasts out of L1 / L2; staging it in LDS would cost every block of
// 256 entries a 32-KB fill for the 4 to 16 entries a lane needs); one store
template <int INTERP, typename TC, typename TO>
struct MeshOp {
    const TC* ctrl;
    int gh, gw, full_h, full_w;
    TO* out;
    int64_t stride;
    int i0, j0;
    int64_t ctrl_set, out_set;
    LERF_HD void operator()(int i, int j, int s) const {
        store_entry(out + set_offset(s, out_set), stride, i, j,
                    mesh_point<INTERP>(ctrl + set_offset(s, ctrl_set), gh, gw, full_h, full_w, i0 + i, j0 + j));
    }
};

// one load of B, up to four of A, one store
template <typename TA, typename TB, typename TO>
struct ComposeOp {
    MapReader<TA> A;
    int aH, aW;
    MapReader<TB> B;
    TO* out;
    int64_t stride;
    int64_t a_set, b_set, out_set;
    LERF_HD void operator()(int i, int j, int s) const {
        const Point q = B.set(s, b_set)(i, j);
        store_entry(out + set_offset(s, out_set), stride, i, j, compose_point(q.r, q.c, aH, aW, A.set(s, a_set)));
    }
};

// one entry of the inverse: Newton's method on the piecewise-bilinear F (invert_point), four dependent 16-byte gathers of one cell of
// F per pass, read through the caches like compose's taps (neighbouring targets walk neighbouring cells); on the device a lane leaves
// the loop when its residual meets tol and the wave runs as long as its slowest lane; ONE store per entry, after the loop; no LDS, no
// atomics, float64 throughout.  init.m == nullptr: the affine start (three more loads of F, the same entries for every lane: broadcasts)
template <typename TF, typename TI, typename TO>
struct InvertOp {
    MapReader<TF> F;
    int fH, fW;
    MapReader<TI> init;
    TO* out;
    int64_t stride;
    int i0, j0, max_iter;
    double tol;
    int64_t f_set, init_set, out_set;
    LERF_HD void operator()(int i, int j, int s) const {
        const double q_r = (double)(i0 + i), q_c = (double)(j0 + j);
        const MapReader<TF> Fs = F.set(s, f_set);
        const Point u0 = init.m ? init.set(s, init_set)(i, j) : invert_start(q_r, q_c, fH, fW, Fs);
        store_entry(out + set_offset(s, out_set), stride, i, j, invert_point(q_r, q_c, fH, fW, u0, max_iter, tol, Fs));
    }
};

// the adjoint of compose (compose_bwd_point): one load of B and of grad_out; the inner gradient reads the four corners of the cell of A
// and has ONE writer per entry -- a plain 16-byte load-add-store into grad_b, bit-equal from run to run and between device and host; the
// outer gradient is a data-dependent bilinear scatter, up to four taps through Add2 into grad_a.  A null grad_a issues no scatter, a
// null grad_b no loads of A.  No LDS, no workspace.
template <typename TA, typename TB>
struct ComposeBwdOp {
    MapReader<TA> A;
    int aH, aW;
    MapReader<TB> B;
    MapReader<double> gout;
    double *gA, *gB;
    int64_t a_set, b_set, gout_set, ga_set, gb_set;
    LERF_HD void operator()(int i, int j, int s) const { apply(i, j, s, Add2{gA + set_offset(s, ga_set), aW}); }
    // the operation with the outer gradient's taps handed to `add`
    template <typename ADD>
    LERF_HD void apply(int i, int j, int s, ADD add) const {
#pragma clang fp contract(off)
        const Point q = B.set(s, b_set)(i, j);
        const Point d = compose_bwd_point(q.r, q.c, gout.set(s, gout_set)(i, j), aH, aW, gA != nullptr, gB != nullptr, A.set(s, a_set), add);
        if (gB) {
            double* gb = gB + set_offset(s, gb_set);
            const Point v = load_entry(gb, gout.stride, i, j);
            store_entry(gb, gout.stride, i, j, Point{v.r + d.r, v.c + d.c});
        }
    }
    // what the ordered runners ask of a scatter operation: its target frame, the scatter alone (what passes 1, 3 and 4 run), the rest
    // alone (one writer already: run as today), the combiner that keeps target q of set s
    LERF_HD int target_h() const { return aH; }
    LERF_HD int target_w() const { return aW; }
    bool has_scatter() const { return gA != nullptr; }
    bool has_rest() const { return gB != nullptr; }
    LERF_HD ComposeBwdOp scatter_only() const { ComposeBwdOp o = *this; o.gB = nullptr; return o; }
    LERF_HD ComposeBwdOp taps_only() const { return scatter_only(); }
    ComposeBwdOp rest_only() const { ComposeBwdOp o = *this; o.gA = nullptr; o.ga_set = 0; return o; }      // a null base takes no offset
    LERF_HD Keep2At keep_at(int s, int64_t q) const { return {gA + set_offset(s, ga_set), aW, q}; }
};

// the adjoint of invert by the implicit function theorem (invert_bwd_point): one load of G and of grad_out, the four corners of one cell
// of F, the 2 x 2 solve v = -J^-T g, the scatter of v through Add2 into grad_f
template <typename TF, typename TG>
struct InvertBwdOp {
    MapReader<TF> F;
    int fH, fW;
    MapReader<TG> G;
    MapReader<double> gout;
    double* gF;
    int64_t f_set, g_set, gout_set, gf_set;
    LERF_HD void operator()(int i, int j, int s) const { apply(i, j, s, Add2{gF + set_offset(s, gf_set), fW}); }
    template <typename ADD>
    LERF_HD void apply(int i, int j, int s, ADD add) const {
        const Point u = G.set(s, g_set)(i, j);
        invert_bwd_point(u.r, u.c, gout.set(s, gout_set)(i, j), fH, fW, F.set(s, f_set), add);
    }
    LERF_HD int target_h() const { return fH; }
    LERF_HD int target_w() const { return fW; }
    bool has_scatter() const { return true; }
    bool has_rest() const { return false; }
    LERF_HD InvertBwdOp scatter_only() const { return *this; }
    LERF_HD InvertBwdOp taps_only() const { return *this; }
    InvertBwdOp rest_only() const { return *this; }
    LERF_HD Keep2At keep_at(int s, int64_t q) const { return {gF + set_offset(s, gf_set), fW, q}; }
};

// The rasterising inverse (raster_cell / raster_resolve of lerf_coords_models.h) in three passes over caller-owned keys [oH][oW]:
//   KeyFillOp     per entry: the key of an untouched pixel (all ones), one 8-byte store
//   RasterOp      per CELL of F, under the scatter runners below: four 16-byte (float64) loads of the cell's corners -- a wave reads one
//                 row of 65 neighbouring vertices twice, coalesced -- four 4-byte loads of depth when given, then for each of the two
//                 triangles a loop over its clipped box (at most max_span x max_span <= 64 x 64 pixels) and ONE 64-bit min per covered
//                 pixel, handed to the runner's MINKEY.  The loop is data-dependent: a wave runs as long as its largest box.
//   ResolveOp     per entry: one 8-byte load of the key, three gathers of F at the winning triangle, one store; a single writer
template <typename TF>
struct RasterOp {
    MapReader<TF> F;
    int fW;
    const float* depth;
    int orient, max_span, i0, j0, oH, oW;
    int64_t f_set, depth_set;
    template <typename MINKEY>
    LERF_HD void operator()(int i, int j, int s, MINKEY minkey) const {
        raster_cell(i, j, fW, F.set(s, f_set), depth ? depth + set_offset(s, depth_set) : nullptr, orient, max_span, i0, j0, oH, oW, minkey);
    }
};

struct KeyFillOp {
    uint64_t* keys;
    int oW;
    int64_t keys_set;
    LERF_HD void operator()(int i, int j, int s) const { keys[set_offset(s, keys_set) + (int64_t)i * oW + j] = kNoKey; }
};

template <typename TF, typename TO>
struct ResolveOp {
    MapReader<TF> F;
    int fW;
    const uint64_t* keys;
    TO* out;
    int64_t stride;
    int i0, j0, oW;
    int64_t f_set, keys_set, out_set;
    LERF_HD void operator()(int i, int j, int s) const {
        store_entry(out + set_offset(s, out_set), stride, i, j,
                    raster_resolve(keys[set_offset(s, keys_set) + (int64_t)i * oW + j], fW, (double)(i0 + i), (double)(j0 + j), F.set(s, f_set)));
    }
};

// The forward warp by summation splatting (splat_point of lerf_splat_point.h): one call per SOURCE pixel (i, j) of set s -- ONE 8- or
// 16-byte load of its map entry, one load of its weight when a weight plane is given, then the loop over the C (+ 1) planes INSIDE the
// thread: one load of x_k (a wave reads 64 consecutive values of a row) and up to four adds through AddPlane, the Add2 pattern for one
// plane of T: one no-return atomicAdd of T where compiled for the device, a plain add on the host.  The planes are outermost in
// memory ([C + 1][oH][oW]), so for a smooth map the 64 lanes of a wave add, per tap and plane, into 64 neighbouring values of one row.
// No LDS, no workspace.  Equal from run to run up to the rounding of a reordered sum in T.
template <typename T>
struct AddPlane {
    T* acc;
    int64_t plane;
    LERF_HD void operator()(int k, int64_t q, double v) const {
        T* p = acc + (int64_t)k * plane + q;
        const T r = (T)v;                            // rounded once, here
#ifdef __HIP_DEVICE_COMPILE__
        atomicAdd(p, r);
#else
        *p = *p + r;
#endif
    }
};

template <typename T, typename TF>
struct SplatOp {
    const T* x;
    MapReader<TF> F;
    const T* m;
    T* acc;
    int C, W, oH, oW;
    bool norm;
    int64_t x_set, f_set, m_set, acc_set, in_plane, out_plane;
    LERF_HD void operator()(int i, int j, int s) const {
        const int64_t e = (int64_t)i * W + j;
        const T* xs = x + set_offset(s, x_set) + e;
        const int64_t plane = in_plane;
        splat_point(F.set(s, f_set)(i, j), m ? (double)m[set_offset(s, m_set) + e] : 1.0, C, norm, oH, oW,
                    [xs, plane](int k) { return (double)xs[(int64_t)k * plane]; }, AddPlane<T>{acc + set_offset(s, acc_set), out_plane});
    }
    // operator() with the adds handed to `add`.  The statement is written twice ON PURPOSE: routed through apply(), the atomic kernel
    // schedules its conversions to T differently (the same instructions, one VGPR fewer), and this file promises that it compiles to
    // the device code it had.  Both hand the same operands to the one splat_point.
    template <typename ADD>
    LERF_HD void apply(int i, int j, int s, ADD add) const {
        const int64_t e = (int64_t)i * W + j;
        const T* xs = x + set_offset(s, x_set) + e;
        const int64_t plane = in_plane;
        splat_point(F.set(s, f_set)(i, j), m ? (double)m[set_offset(s, m_set) + e] : 1.0, C, norm, oH, oW,
                    [xs, plane](int k) { return (double)xs[(int64_t)k * plane]; }, add);
    }
    // the ordered runners' view (ComposeBwdOp): the passes that only look for the taps run ONE plane, so a tap is counted and listed once
    LERF_HD int target_h() const { return oH; }
    LERF_HD int target_w() const { return oW; }
    bool has_scatter() const { return true; }
    bool has_rest() const { return false; }
    LERF_HD SplatOp scatter_only() const { return *this; }
    LERF_HD SplatOp taps_only() const { SplatOp o = *this; o.C = 1; o.norm = false; return o; }
    SplatOp rest_only() const { return *this; }
    LERF_HD KeepPlaneAt<T> keep_at(int s, int64_t q) const { return {acc + set_offset(s, acc_set), out_plane, q, C + (norm ? 1 : 0)}; }
};

// the adjoint of the splat (splat_bwd_point): a GATHER -- per source pixel the same map entry and weight, per plane one load of x_k (when
// grad_M or grad_F is wanted) and up to four loads of G at the taps, read through the caches like compose's taps; ONE writer per
// source pixel and plain stores (a T per plane of grad_X, a T of grad_M, one 16-byte entry of grad_F), no atomics: bit-equal between device
// and host and from run to run.  A null gradient pointer skips that half (wave-uniform).
template <typename T, typename TF>
struct SplatBwdOp {
    const T* x;
    MapReader<TF> F;
    const T* m;
    const T* g;
    T* gx;
    T* gm;
    double* gf;
    int C, W, oH, oW;
    bool norm;
    int64_t x_set, f_set, m_set, g_set, gx_set, gm_set, gf_set, in_plane, out_plane;
    LERF_HD void operator()(int i, int j, int s) const {
        const int64_t e = (int64_t)i * W + j, iplane = in_plane, oplane = out_plane;
        const T* xs = x + set_offset(s, x_set) + e;
        const T* gs = g + set_offset(s, g_set);
        T* gxs = gx ? gx + set_offset(s, gx_set) + e : nullptr;
        const SplatGrad d = splat_bwd_point(F.set(s, f_set)(i, j), m ? (double)m[set_offset(s, m_set) + e] : 1.0, C, norm, oH, oW, gx != nullptr,
                                            gm != nullptr, gf != nullptr, [xs, iplane](int k) { return (double)xs[(int64_t)k * iplane]; },
                                            [gs, oplane](int k, int64_t q) { return (double)gs[(int64_t)k * oplane + q]; },
                                            [gxs, iplane](int k, double v) { gxs[(int64_t)k * iplane] = (T)v; });
        if (gm) gm[set_offset(s, gm_set) + e] = (T)d.m;
        if (gf) store_entry(gf + set_offset(s, gf_set), 2 * (int64_t)W, i, j, d.f);
    }
};

// ------------------------------------------------------------------------------------------------ the two runners
// 8 waves per SIMD (64 VGPRs) hold for every operation; stated, so that the bicubic mesh over a float64 control mesh stays at 64, not 66
template <typename OP>
__global__ void __launch_bounds__(CB_COLS * CB_ROWS) __attribute__((amdgpu_waves_per_eu(8))) entry_kernel(const OP op, int oH, int oW) {
    const int j = blockIdx.x * CB_COLS + threadIdx.x, i = blockIdx.y * CB_ROWS + threadIdx.y;
    if (i >= oH || j >= oW) return;
    op(i, j, (int)blockIdx.z);
}

struct OnDevice {
    hipStream_t stream;
    template <typename OP>
    int operator()(const OP& op, int oH, int oW, int sets = 1) const {
        clear_stale_error();
        const dim3 grid((oW + CB_COLS - 1) / CB_COLS, (oH + CB_ROWS - 1) / CB_ROWS, sets);
        hipLaunchKernelGGL(entry_kernel<OP>, grid, dim3(CB_COLS, CB_ROWS), 0, stream, op, oH, oW);
        return launch_status();
    }
};

struct OnHost {
    template <typename OP>
    int operator()(const OP& op, int oH, int oW, int sets = 1) const {
        for (int s = 0; s < sets; ++s)
            for (int i = 0; i < oH; ++i)
                for (int j = 0; j < oW; ++j) op(i, j, s);
        return LERF_OK;
    }
};

// The two runners of a SCATTER operation op(i, j, s, minkey) -- one call per cell (i, j) of [cH][cW] of set s, which hands (index, key)
// pairs to minkey: keys[index] = min(keys[index], key), keys = the plane of set s (keys + s * keys_set).  The runner owns the combiner,
// the operation owns the arithmetic:
//   ScatterOnDevice{stream}   cell_kernel<OP>: the block and grid of entry_kernel, one thread per cell; KeyMinDevice = one 64-bit
//                             unsigned atomic min into global memory (a single hardware instruction on gfx950, no return value).  A
//                             plain load first: keys only decrease, so a key that is already smaller stays smaller and the atomic
//                             is skipped; a stale load costs an atomic that changes nothing.
//   ScatterOnHost{}           the row-major loop over cells, KeyMinHost = a plain min
// A minimum over integers does not depend on the order of its operands: the two agree bit for bit, as do two runs.
struct KeyMinDevice {
    uint64_t* keys;
    __device__ void operator()(int64_t e, uint64_t key) const {
        unsigned long long* p = reinterpret_cast<unsigned long long*>(keys + e);
        if (__atomic_load_n(p, __ATOMIC_RELAXED) < key) return;
        atomicMin(p, (unsigned long long)key);
    }
};

struct KeyMinHost {
    uint64_t* keys;
    void operator()(int64_t e, uint64_t key) const { keys[e] = key < keys[e] ? key : keys[e]; }
};

template <typename OP>
__global__ void __launch_bounds__(CB_COLS * CB_ROWS) cell_kernel(const OP op, int cH, int cW, uint64_t* keys, int64_t keys_set) {
    const int j = blockIdx.x * CB_COLS + threadIdx.x, i = blockIdx.y * CB_ROWS + threadIdx.y;
    if (i >= cH || j >= cW) return;
    op(i, j, (int)blockIdx.z, KeyMinDevice{keys + (int64_t)blockIdx.z * keys_set});
}

struct ScatterOnDevice {
    hipStream_t stream;
    template <typename OP>
    int operator()(const OP& op, int cH, int cW, uint64_t* keys, int sets = 1, int64_t keys_set = 0) const {
        clear_stale_error();
        const dim3 grid((cW + CB_COLS - 1) / CB_COLS, (cH + CB_ROWS - 1) / CB_ROWS, sets);
        hipLaunchKernelGGL(cell_kernel<OP>, grid, dim3(CB_COLS, CB_ROWS), 0, stream, op, cH, cW, keys, keys_set);
        return launch_status();
    }
};

struct ScatterOnHost {
    template <typename OP>
    int operator()(const OP& op, int cH, int cW, uint64_t* keys, int sets = 1, int64_t keys_set = 0) const {
        for (int s = 0; s < sets; ++s)
            for (int i = 0; i < cH; ++i)
                for (int j = 0; j < cW; ++j) op(i, j, s, KeyMinHost{keys + set_offset(s, keys_set)});
        return LERF_OK;
    }
};

// ------------------------------------------------------------------------------------------------ the ordered scatter
// The two runners of a float scatter operation whose sums must not depend on the order the hardware takes: the call shape of OnDevice /
// OnHost, over a caller-owned workspace, in four passes that run THE SAME op under four combiners --
//   1 count   entry_kernel over the entries, CountAt: count[s][q] += 1 per combiner call; integer adds, so the counts are exact
//   2 scan    the exclusive prefix sum of count per set (scan_exclusive_u32, below) = the start of every target's segment of `list`;
//             its first level also folds the largest count into the header (an integer atomic max)
//   3 fill    entry_kernel again, FillAt: list[s][cursor[s][q]++] = e; afterwards cursor[q] is the END of q's segment and cursor[q - 1]
//             (0 for q = 0) its start -- one array serves count, start and end; the order inside a segment is whatever the atomics gave
//   4 sum     ordered_sum_kernel, one thread per target: sort the segment ascending (sort_segment), walk it, skip an id equal to the
//             one before (an entry listed twice runs once), and re-run the op for each entry e = i W + j under keep_at(s, q): the plain
//             p = p + r of the host branch, for calls whose target is q only.  Entry order, then tap order inside the entry, then the
//             planes each on their own element: the order of OnHost, from the same statements, so the sums are the host twin's bits.
//             A target with more adders than max_adders is not sorted or summed: every plane of it becomes NaN (the thread's run
//             time is bounded; the caller reads the header and refuses the result).
// then the part of the op that had one writer all along (has_rest: compose's inner gradient), as today.
// WORKSPACE, in uint32 words: header [4] (word 0 reserved and zeroed, word 1 = kOrderedMaxWord the largest count, 2 and 3 zero), cursor
// [n_sets][n_targets], list [n_sets][4 n_entries], scan partials [n_sets][scan_partials(n_targets)].
// Addresses: CountAt / FillAt index count / cursor at a target the op hands out -- the element it would have added into, inside
// [tH][tW] by the op's own clamps and frame tests; a slot is below the segment's end because pass 3 repeats pass 1's calls exactly (the
// operands are not written between them: the workspace intersects none); list holds e < n_entries; the sum reads list inside
// [start, end) with end <= 4 n_entries and writes element q of every plane only.
constexpr int kScanThreads = 256, kScanPerThread = 4, kScanBlock = kScanThreads * kScanPerThread;
constexpr int kOrderedHeaderWords = 4, kOrderedMaxWord = 1;
constexpr uint32_t kInsertionMax = 16;      // segments up to here: insertion sort; longer: heap sort

// the scan partials one set of n elements needs: one word per block of every level that has more than one block
inline int64_t scan_partials(int64_t n) {
    int64_t total = 0;
    while (n > kScanBlock) {
        n = (n + kScanBlock - 1) / kScanBlock;
        total += n;
    }
    return total;
}

// a block scans its kScanBlock elements of set blockIdx.y in place (exclusive) and writes their sum to sums[block] (when given); a
// thread owns 4 consecutive elements, the 256 thread sums are scanned in LDS (Hillis-Steele, 8 steps); max_out: the largest element
// seen, one atomic max per wave that saw one above 0
__global__ void __launch_bounds__(kScanThreads)
scan_block_kernel(uint32_t* __restrict__ data, int64_t n, int64_t set_stride, uint32_t* __restrict__ sums, int64_t sums_stride,
                  uint32_t* __restrict__ max_out) {
    __shared__ uint32_t part[kScanThreads];
    data += (int64_t)blockIdx.y * set_stride;
    const int64_t base = ((int64_t)blockIdx.x * kScanThreads + threadIdx.x) * kScanPerThread;
    uint32_t v[kScanPerThread], sum = 0, big = 0;
#pragma unroll
    for (int k = 0; k < kScanPerThread; ++k) {
        v[k] = base + k < n ? data[base + k] : 0u;
        sum += v[k];
        big = v[k] > big ? v[k] : big;
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const uint32_t add = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - sum;      // exclusive over the threads
#pragma unroll
    for (int k = 0; k < kScanPerThread; ++k) {
        if (base + k < n) data[base + k] = run;
        run += v[k];
    }
    if (sums && threadIdx.x == kScanThreads - 1) sums[(int64_t)blockIdx.y * sums_stride + blockIdx.x] = part[threadIdx.x];
    if (max_out) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const uint32_t other = (uint32_t)__shfl_xor((int)big, o, 64);
            big = other > big ? other : big;
        }
        if ((threadIdx.x & 63) == 0 && big) atomicMax(max_out, big);
    }
}

// the add-back: every element of block b gains the scanned sum of the blocks before it
__global__ void __launch_bounds__(kScanThreads)
scan_add_kernel(uint32_t* __restrict__ data, int64_t n, int64_t set_stride, const uint32_t* __restrict__ sums, int64_t sums_stride) {
    data += (int64_t)blockIdx.y * set_stride;
    const uint32_t add = sums[(int64_t)blockIdx.y * sums_stride + blockIdx.x];
    const int64_t base = ((int64_t)blockIdx.x * kScanThreads + threadIdx.x) * kScanPerThread;
#pragma unroll
    for (int k = 0; k < kScanPerThread; ++k)
        if (base + k < n) data[base + k] += add;
}

// data [sets][n] (sets `set_stride` words apart) -> its exclusive prefix sums per set, in place, modulo 2^32; partials: [sets][P],
// P = scan_partials(n).  Plain passes in stream order -- block scans, the scan of the block sums (this function again, one level
// up), the add-back -- and no workgroup waits for another.  n <= 2^32 - 1: at most four levels.
inline void scan_exclusive_u32(hipStream_t stream, uint32_t* data, int64_t n, int sets, int64_t set_stride, uint32_t* partials, uint32_t* max_out) {
    const int64_t P = scan_partials(n);
    int64_t len = n, off = 0, stride = set_stride;
    uint32_t* level = data;
    struct { uint32_t* data; int64_t n, stride, off; } up[4];
    int levels = 0;
    while (true) {
        const int64_t blocks = (len + kScanBlock - 1) / kScanBlock;
        uint32_t* sums = blocks > 1 ? partials + off : nullptr;
        hipLaunchKernelGGL(scan_block_kernel, dim3((unsigned)blocks, sets), dim3(kScanThreads), 0, stream, level, len, stride, sums, P,
                           levels == 0 ? max_out : (uint32_t*)nullptr);
        if (blocks <= 1) break;
        up[levels++] = {level, len, stride, off};
        level = sums;
        len = blocks;
        stride = P;
        off += blocks;
    }
    while (levels-- > 0) {
        const int64_t blocks = (up[levels].n + kScanBlock - 1) / kScanBlock;
        hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)blocks, sets), dim3(kScanThreads), 0, stream, up[levels].data, up[levels].n,
                           up[levels].stride, partials + up[levels].off, P);
    }
}

inline void scan_exclusive_u32_host(uint32_t* data, int64_t n) {
    uint32_t run = 0;
    for (int64_t k = 0; k < n; ++k) {
        const uint32_t v = data[k];
        data[k] = run;
        run += v;
    }
}

// ascending, in place, by the segment's one owner: insertion sort up to kInsertionMax ids, heap sort (no recursion, n log n at worst) beyond
LERF_HD inline void sort_segment(uint32_t* a, uint32_t n) {
    if (n <= kInsertionMax) {
        for (uint32_t k = 1; k < n; ++k) {
            const uint32_t v = a[k];
            uint32_t h = k;
            for (; h > 0 && a[h - 1] > v; --h) a[h] = a[h - 1];
            a[h] = v;
        }
        return;
    }
    const auto sift = [a](uint32_t root, uint32_t end) {      // the max-heap property below `root`, inside [0, end)
        const uint32_t v = a[root];
        while (true) {
            uint32_t child = 2 * root + 1;
            if (child >= end) break;
            if (child + 1 < end && a[child + 1] > a[child]) ++child;
            if (a[child] <= v) break;
            a[root] = a[child];
            root = child;
        }
        a[root] = v;
    };
    for (uint32_t k = n / 2; k-- > 0;) sift(k, n);
    for (uint32_t end = n - 1; end > 0; --end) {
        const uint32_t top = a[0];
        a[0] = a[end];
        a[end] = top;
        sift(0, end);
    }
}

// ------------------------------------------------------------------------------------------------ the triangle-mesh rasteriser
// An INDEXED mesh drawn into a map: invert_raster's per-pixel arithmetic (closed watertight inside test, 64-bit (depth, face) key, integer
// atomic min) over faces of any size.  One thread per cell cannot serve a face hundreds of pixels wide, so the faces are BINNED into item
// tiles -- kTileRows x kTileCols = 4 x 16 pixels of the key plane, aligned to the plane -- and one WAVE draws one (face, tile) item, a
// pixel a lane: its 64 atomics are four runs of 16 consecutive keys (128 bytes).  Five passes in stream order, no sync, no read-back:
//   1 fill     KeyFillOp under entry_kernel
//   2 count    TriCountOp under entry_kernel, one thread per face: the set-up (tri_setup) and the number of item tiles of its clipped
//              box (tri_tiles), a uint32 in count[set][f]; slot F of every set holds 0
//   3 scan     scan_exclusive_u32 over the CONCATENATED [n_sets (F + 1)] counts: start[g] = the first item of face slot g, and the last
//              slot (a pad, count 0) holds the total.  One item list spans the batch, so the sets balance each other.
//   4 raster   trimesh_raster_kernel: a grid fixed by sizes the host knows; wave k takes the items [k n, (k + 1) n), n = ceil(total / waves),
//              total read from start.  One upper_bound for the face of its first item, then a forward walk (++g while item >= start[g + 1],
//              guarded by the last slot); per item the wave re-runs the face's set-up and its lanes take the tile's 64 pixels through
//              tri_pixel and KeyMinDevice.  The search, the walk and the set-up are wave-uniform.
//   5 resolve  TriResolveOp under entry_kernel: one key load, the face's indices, three positions and three attributes, one store
// The host twin runs passes 1 and 5 under OnHost and, for pass 2 - 4, the plain loop over sets, faces and box pixels with KeyMinHost: an
// integer minimum does not depend on the order, so the tile shape and the chunking cannot show in the result.
// Addresses: an index is compared UNSIGNED against V (Va) before it forms an address (tri_index_ok); a pixel is drawn only inside the
// face's clipped box, which raster_axis's rule puts inside the tile in floating point before the conversion to int, so keys is indexed
// inside [oH][oW] WHATEVER start holds; the walk over start stops at its last slot, and an item number beyond the face's recomputed tile
// count is dropped; count is written at slots < n_sets (F + 1) only.  The resolve reads the face a key names only when it is < F.
template <typename TP>
struct TriMesh {
    const TP* pos;
    int V, Va;
    const int32_t* faces;
    const int32_t* attr_faces;
    int F;
    const float* depth;
    const void* w;      // float32 or float64 (w_f64)
    bool w_f64;
    int orient, max_span, i0, j0, oH, oW;
    int64_t pos_set, faces_set, afaces_set, depth_set, w_set;

    // face f of set s with its vertices read: t, the indices into attr (ai) and the three w (1 without); false: an index outside the mesh
    LERF_HD bool read(int s, int f, TriFace* t, int32_t* ai, double* wv) const {
        const int32_t* fp = faces + set_offset(s, faces_set) + 3 * (int64_t)f;
        const int32_t* ap = attr_faces ? attr_faces + set_offset(s, afaces_set) + 3 * (int64_t)f : fp;
        t->ia = fp[0]; t->ib = fp[1]; t->ic = fp[2];
        ai[0] = ap[0]; ai[1] = ap[1]; ai[2] = ap[2];
        if (!tri_index_ok(t->ia, t->ib, t->ic, V) || !tri_index_ok(ai[0], ai[1], ai[2], Va)) return false;
        const TP* p = pos + set_offset(s, pos_set);
        t->A = load_entry(p, 0, 0, t->ia);
        t->B = load_entry(p, 0, 0, t->ib);
        t->C = load_entry(p, 0, 0, t->ic);
        t->zA = t->zB = t->zC = 0.0f;
        if (depth) {
            const float* d = depth + set_offset(s, depth_set);
            t->zA = d[t->ia]; t->zB = d[t->ib]; t->zC = d[t->ic];
        }
        wv[0] = wv[1] = wv[2] = 1.0;
        if (w && w_f64) {
            const double* q = (const double*)w + set_offset(s, w_set);
            wv[0] = q[t->ia]; wv[1] = q[t->ib]; wv[2] = q[t->ic];
        } else if (w) {
            const float* q = (const float*)w + set_offset(s, w_set);
            wv[0] = (double)q[t->ia]; wv[1] = (double)q[t->ib]; wv[2] = (double)q[t->ic];
        }
        return true;
    }

    LERF_HD bool setup(int s, int f, TriFace* t, RasterBox* box) const {
        int32_t ai[3];
        double wv[3];
        return read(s, f, t, ai, wv) && tri_setup(*t, depth != nullptr, w != nullptr, wv[0], wv[1], wv[2], orient, max_span, i0, j0, oH, oW, box);
    }
};

// the face slots [n_sets][F + 1] as an entry grid of 4 rows: slot = i * cw + j, cw = ceil((F + 1) / 4)
constexpr int kTriCountRows = 4;

template <typename TP>
struct TriCountOp {
    TriMesh<TP> mesh;
    uint32_t* count;
    int cw;
    LERF_HD void operator()(int i, int j, int s) const {
        const int64_t slot = (int64_t)i * cw + j;
        if (slot > mesh.F) return;
        uint32_t n = 0;
        TriFace t;
        RasterBox box;
        if (slot < mesh.F && mesh.setup(s, (int)slot, &t, &box)) {
            const TriTiles tt = tri_tiles(box, mesh.i0, mesh.j0);
            n = (uint32_t)tt.ntr * (uint32_t)tt.ntc;
        }
        count[(int64_t)s * ((int64_t)mesh.F + 1) + slot] = n;
    }
};

template <typename TP, typename TA, typename TO>
struct TriResolveOp {
    TriMesh<TP> mesh;
    const TA* attr;
    const uint64_t* keys;
    TO* out;
    int64_t stride;
    float* depth_out;
    int64_t attr_set, keys_set, out_set, dout_set;
    LERF_HD void operator()(int i, int j, int s) const {
        const uint64_t key = keys[set_offset(s, keys_set) + (int64_t)i * mesh.oW + j];
        Point u{__builtin_nan(""), __builtin_nan("")};
        float z = __builtin_nanf("");
        TriFace t;
        int32_t ai[3];
        double wv[3];
        if (key != kNoKey && (uint32_t)key < (uint32_t)mesh.F && mesh.read(s, (int)(uint32_t)key, &t, ai, wv)) {
            const TA* a = attr + set_offset(s, attr_set);
            u = tri_attr(t, load_entry(a, 0, 0, ai[0]), load_entry(a, 0, 0, ai[1]), load_entry(a, 0, 0, ai[2]), mesh.w != nullptr, wv[0], wv[1], wv[2],
                         (double)(mesh.i0 + i), (double)(mesh.j0 + j));
            z = key_depth(key);
        }
        store_entry(out + set_offset(s, out_set), stride, i, j, u);
        if (depth_out) depth_out[set_offset(s, dout_set) + (int64_t)i * mesh.oW + j] = z;
    }
};

constexpr int kTriWaves = 4;           // waves per block of the raster pass
constexpr int kTriBlocks = 2048;       // its largest grid: 8 blocks per CU of 256

// the blocks of the raster pass, from sizes alone: no more waves than there can be items
inline unsigned tri_blocks(uint64_t max_items) {
    const uint64_t want = (max_items + kTriWaves - 1) / kTriWaves;
    return (unsigned)(want < 1 ? 1 : want > (uint64_t)kTriBlocks ? (uint64_t)kTriBlocks : want);
}

template <typename TP>
__global__ void __launch_bounds__(64 * kTriWaves)
trimesh_raster_kernel(const TriMesh<TP> mesh, const uint32_t* __restrict__ start, uint32_t n_slots, uint64_t* keys, int64_t keys_set) {
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kTriWaves + threadIdx.x / 64));
    const uint32_t waves = gridDim.x * kTriWaves;
    const uint32_t total = start[n_slots - 1];
    const uint32_t per = (uint32_t)(((uint64_t)total + waves - 1) / waves);
    const uint64_t first64 = (uint64_t)wave * per;
    if (first64 >= total) return;                                  // an empty chunk
    const uint32_t first = (uint32_t)first64;
    const uint32_t end = total - first < per ? total : first + per;
    uint32_t lo = 0, hi = n_slots;                                 // upper_bound: the first slot whose start is beyond `first`
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (start[mid] <= first) lo = mid + 1;
        else hi = mid;
    }
    if (lo == 0) return;                                           // start[0] is 0 after an exclusive scan
    uint32_t g = (uint32_t)__builtin_amdgcn_readfirstlane((int)(lo - 1));
    const uint32_t slots = (uint32_t)mesh.F + 1u;
    int s = (int)(g / slots), f = (int)(g % slots);
    const int lane = threadIdx.x & 63, lr = lane / kTileCols, lc = lane % kTileCols;
    for (uint32_t item = first; item < end; ++item) {
        while (g + 1 < n_slots && item >= start[g + 1]) {          // zero-count slots are stepped over; the last slot ends the walk
            ++g;
            if (++f == (int)slots) { f = 0; ++s; }
        }
        if (g + 1 >= n_slots || f >= mesh.F) return;               // the pad slots hold no items
        TriFace t;
        RasterBox box;
        if (!mesh.setup(s, f, &t, &box)) continue;
        const TriTiles tt = tri_tiles(box, mesh.i0, mesh.j0);
        const uint32_t k = item - start[g];
        if (k >= (uint32_t)tt.ntr * (uint32_t)tt.ntc) continue;
        const int rr = (tt.tr0 + (int)(k / (uint32_t)tt.ntc)) * kTileRows + lr, qq = (tt.tc0 + (int)(k % (uint32_t)tt.ntc)) * kTileCols + lc;
        if (rr < box.r0 - mesh.i0 || rr > box.r1 - mesh.i0 || qq < box.c0 - mesh.j0 || qq > box.c1 - mesh.j0) continue;
        tri_pixel(t, box, mesh.depth != nullptr, (uint32_t)f, mesh.i0 + rr, mesh.j0 + qq, mesh.i0, mesh.j0, mesh.oW,
                  KeyMinDevice{keys + set_offset(s, keys_set)});
    }
}

// passes 2 - 4 on the device; count: [n_slots] uint32, partials: the scan's
struct TriRasterOnDevice {
    hipStream_t stream;
    template <typename TP>
    int operator()(const TriMesh<TP>& mesh, uint64_t* keys, int64_t keys_set, int n_sets, uint32_t* count, uint64_t max_items) const {
        const int64_t n_slots = (int64_t)n_sets * ((int64_t)mesh.F + 1);
        const int cw = (int)(((int64_t)mesh.F + kTriCountRows) / kTriCountRows);
        int rc = OnDevice{stream}(TriCountOp<TP>{mesh, count, cw}, kTriCountRows, cw, n_sets);
        if (rc != LERF_OK) return rc;
        clear_stale_error();
        scan_exclusive_u32(stream, count, n_slots, 1, n_slots, count + n_slots, nullptr);
        hipLaunchKernelGGL(trimesh_raster_kernel<TP>, dim3(tri_blocks(max_items)), dim3(64 * kTriWaves), 0, stream, mesh, count, (uint32_t)n_slots,
                           keys, keys_set);
        return launch_status();
    }
};

// the plain loop over sets, faces and the pixels of their boxes
struct TriRasterOnHost {
    template <typename TP>
    int operator()(const TriMesh<TP>& mesh, uint64_t* keys, int64_t keys_set, int n_sets, uint32_t*, uint64_t) const {
        for (int s = 0; s < n_sets; ++s)
            for (int f = 0; f < mesh.F; ++f) {
                TriFace t;
                RasterBox box;
                if (!mesh.setup(s, f, &t, &box)) continue;
                for (int r = box.r0; r <= box.r1; ++r)
                    for (int q = box.c0; q <= box.c1; ++q)
                        tri_pixel(t, box, mesh.depth != nullptr, (uint32_t)f, r, q, mesh.i0, mesh.j0, mesh.oW, KeyMinHost{keys + set_offset(s, keys_set)});
            }
        return LERF_OK;
    }
};

// pass 4 for target q of set s; op: the scatter_only() form; cursor and list: the set's own; W: the width of the ENTRY grid
template <typename OP>
LERF_HD inline void ordered_sum_target(const OP& op, int s, int64_t q, const uint32_t* cursor, uint32_t* list, int W, uint32_t max_adders) {
    const uint32_t start = q ? cursor[q - 1] : 0u, n = cursor[q] - start;
    if (n == 0) return;
    const auto keep = op.keep_at(s, q);
    if (n > max_adders) {
        keep.poison();
        return;
    }
    uint32_t* seg = list + start;
    sort_segment(seg, n);
    uint32_t last = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t e = seg[k];
        if (k && e == last) continue;
        last = e;
        op.apply((int)(e / (uint32_t)W), (int)(e % (uint32_t)W), s, keep);
    }
}

template <typename OP>
struct CountPass {
    OP op;      // the taps_only() form
    uint32_t* count;
    int64_t n_targets;
    LERF_HD void operator()(int i, int j, int s) const { op.apply(i, j, s, CountAt{count + (int64_t)s * n_targets, op.target_w()}); }
};

template <typename OP>
struct FillPass {
    OP op;
    uint32_t *cursor, *list;
    int64_t n_targets, n_slots;
    int W;
    LERF_HD void operator()(int i, int j, int s) const {
        op.apply(i, j, s, FillAt{cursor + (int64_t)s * n_targets, list + (int64_t)s * n_slots, (uint32_t)i * (uint32_t)W + (uint32_t)j, op.target_w()});
    }
};

// one thread per target, 256 a block, the set is blockIdx.y; a wave's threads own 64 neighbouring targets
template <typename OP>
__global__ void __launch_bounds__(256)
ordered_sum_kernel(const OP op, int64_t n_targets, const uint32_t* __restrict__ cursor, uint32_t* __restrict__ list, int64_t n_slots, int W,
                   uint32_t max_adders) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n_targets) return;
    const int s = (int)blockIdx.y;
    ordered_sum_target(op, s, q, cursor + (int64_t)s * n_targets, list + (int64_t)s * n_slots, W, max_adders);
}

// one target space of a call as passes 1 - 4 see it: where the largest count goes, the cursor [sets][n_targets], the list [sets][n_slots]
// and the scan's partials; OrderedLayout and TriBwdLayout each hand one out
struct OrderedView {
    uint32_t *max_word, *cursor, *list, *scan;
    int64_t n_targets, n_slots;
};

struct OrderedLayout {
    int64_t n_entries, n_targets, n_slots, partials;
    uint32_t *header, *cursor, *list, *scan;
    OrderedLayout(void* ws, int64_t entries, int64_t targets, int sets)
        : n_entries(entries), n_targets(targets), n_slots(4 * entries), partials(scan_partials(targets)) {
        header = (uint32_t*)ws;
        cursor = header + kOrderedHeaderWords;
        list = cursor + (int64_t)sets * n_targets;
        scan = list + (int64_t)sets * n_slots;
    }
    OrderedView view() const { return {header + kOrderedMaxWord, cursor, list, scan, n_targets, n_slots}; }
    static size_t bytes(int64_t entries, int64_t targets, int sets) {
        return sizeof(uint32_t) * ((size_t)kOrderedHeaderWords + (size_t)sets * ((size_t)targets + 4 * (size_t)entries + (size_t)scan_partials(targets)));
    }
};

// THE FOUR PASSES, once per side: op over the entry grid [eH][eW] of every set into the view's zeroed cursor (zeroing stays with the
// callers: the ordered scatter clears header and cursor in one memset, the mesh adjoint the cursor once per target space).  Device:
// plain launches in stream order, the launch status looked at after every pass.
template <typename OP>
int ordered_passes_device(hipStream_t stream, const OP& op, int eH, int eW, int sets, const OrderedView& v, int max_adders) {
    const OnDevice run{stream};
    int rc = run(CountPass<OP>{op.taps_only(), v.cursor, v.n_targets}, eH, eW, sets);
    if (rc != LERF_OK) return rc;
    clear_stale_error();
    scan_exclusive_u32(stream, v.cursor, v.n_targets, sets, v.n_targets, v.scan, v.max_word);
    rc = launch_status();
    if (rc != LERF_OK) return rc;
    rc = run(FillPass<OP>{op.taps_only(), v.cursor, v.list, v.n_targets, v.n_slots, eW}, eH, eW, sets);
    if (rc != LERF_OK) return rc;
    clear_stale_error();
    hipLaunchKernelGGL(ordered_sum_kernel<OP>, dim3((unsigned)((v.n_targets + 255) / 256), sets), dim3(256), 0, stream, op.scatter_only(), v.n_targets,
                       v.cursor, v.list, v.n_slots, eW, (uint32_t)max_adders);
    return launch_status();
}

// the same four passes, serially; pass 3 walks the entries in DESCENDING order, so every segment of two or more ids reaches the sort
// reversed and the sort, the duplicate skip and the cap run here as they do on the device
template <typename OP>
void ordered_passes_host(const OP& op, int eH, int eW, int sets, const OrderedView& v, int max_adders) {
    OnHost{}(CountPass<OP>{op.taps_only(), v.cursor, v.n_targets}, eH, eW, sets);
    for (int s = 0; s < sets; ++s) {
        uint32_t* c = v.cursor + (int64_t)s * v.n_targets;
        for (int64_t q = 0; q < v.n_targets; ++q) *v.max_word = c[q] > *v.max_word ? c[q] : *v.max_word;
        scan_exclusive_u32_host(c, v.n_targets);
    }
    const FillPass<OP> fill{op.taps_only(), v.cursor, v.list, v.n_targets, v.n_slots, eW};
    for (int s = 0; s < sets; ++s)
        for (int i = eH - 1; i >= 0; --i)
            for (int j = eW - 1; j >= 0; --j) fill(i, j, s);
    const OP scatter = op.scatter_only();
    for (int s = 0; s < sets; ++s)
        for (int64_t q = 0; q < v.n_targets; ++q)
            ordered_sum_target(scatter, s, q, v.cursor + (int64_t)s * v.n_targets, v.list + (int64_t)s * v.n_slots, eW, (uint32_t)max_adders);
}

struct OrderedOnDevice {
    hipStream_t stream;
    void* ws;
    int max_adders;
    template <typename OP>
    int operator()(const OP& op, int oH, int oW, int sets = 1) const {
        clear_stale_error();
        const OrderedLayout L(ws, (int64_t)oH * oW, (int64_t)op.target_h() * op.target_w(), sets);
        if (hipMemsetAsync(ws, 0, sizeof(uint32_t) * (kOrderedHeaderWords + (size_t)sets * L.n_targets), stream) != hipSuccess) return LERF_ELAUNCH;
        if (op.has_scatter()) {
            const int rc = ordered_passes_device(stream, op, oH, oW, sets, L.view(), max_adders);
            if (rc != LERF_OK) return rc;
        }
        return op.has_rest() ? OnDevice{stream}(op.rest_only(), oH, oW, sets) : LERF_OK;
    }
};

struct OrderedOnHost {
    void* ws;
    int max_adders;
    template <typename OP>
    int operator()(const OP& op, int oH, int oW, int sets = 1) const {
        const OrderedLayout L(ws, (int64_t)oH * oW, (int64_t)op.target_h() * op.target_w(), sets);
        for (int k = 0; k < kOrderedHeaderWords; ++k) L.header[k] = 0;
        for (int64_t k = 0; k < (int64_t)sets * L.n_targets; ++k) L.cursor[k] = 0;
        if (op.has_scatter()) ordered_passes_host(op, oH, oW, sets, L.view(), max_adders);
        return op.has_rest() ? OnHost{}(op.rest_only(), oH, oW, sets) : LERF_OK;
    }
};

// ------------------------------------------------------------------------------------------------ the adjoint of the triangle mesh
// Gradients of the resolve's attribute with respect to attr, pos and w at FIXED VISIBILITY (the keys of the forward), in two passes whose
// sums have ONE order, the statement's (tri_bwd_thread, tri_face_terms: the top of lerf_coords_models.h), on the device and in the host twin:
//   face pass    trimesh_bwd_face_kernel: one workgroup of kTriBwdWaves = 4 waves per (set, face), grid (F, n_sets).  The set-up and the
//                clipped box are the forward's (TriMesh::read, tri_setup, tri_tiles); a skipped face exits at once.  Thread 64 r + l owns
//                lane pixel l of the item tiles r, r + 4, ...; 6 (15 with w) running sums in registers, one 8-byte load of the key per
//                pixel and one 16-byte load of grad_out for a pixel the face won only; a butterfly over the lanes per sum, the four waves
//                through LDS as ((p0 + p1) + p2) + p3, and thread 0 stores the face's 15 terms at terms[set][f][15].
//   vertex pass  the ordered scatter's four passes (count, scan, fill, sort and sum) over TriVertexOp, whose ENTRIES are the faces (entry grid
//                1 x F) and whose TARGETS are the vertices: a drawn face hands its three corners' terms to the combiner, so vertex v's one
//                writer adds them in ascending (face, corner) order into what the gradient holds.  Two target spaces, one after the other over
//                the same cursor and list: the vertices of `faces` (grad_pos and grad_w from one segment) and those of attr_faces (grad_attr);
//                a face that names one attribute twice is listed twice and, by the duplicate skip, runs once and delivers both corners.
// WORKSPACE, 8-byte aligned: header [4] uint32 (word 1 the largest valence of either space), terms [n_sets][F][15] float64, cursor
// [n_sets][max(V, Va)] uint32, list [n_sets][3 F] uint32, scan partials [n_sets][scan_partials(max(V, Va))].
// Addresses: the face pass indexes keys and grad_out inside the face's clipped box, which tri_axis puts inside [oH][oW] in floating point
// before the conversion to int, and terms at (set, f) with f < F; TriVertexOp hands out a corner's index only after tri_index_ok compared it
// against V and Va, so cursor and the gradients are indexed inside [V] / [Va]; a face lists at most 3 ids, the list holds 3 F per set.
struct KeepVertexAt {
    double *g2, *g1;      // [n][2] and [n], either may be null
    int64_t q;
    LERF_HD void operator()(int, int c, double dr, double dc) const {
#pragma clang fp contract(off)
        if ((int64_t)c != q || !g2) return;
        double* p = g2 + 2 * q;
        p[0] = p[0] + dr;
        p[1] = p[1] + dc;
    }
    LERF_HD void operator()(int, int64_t at, double v) const {
#pragma clang fp contract(off)
        if (at != q || !g1) return;
        g1[q] = g1[q] + v;
    }
    LERF_HD void poison() const {
        if (g2) g2[2 * q] = g2[2 * q + 1] = __builtin_nan("");
        if (g1) g1[q] = __builtin_nan("");
    }
};

// SPACE 0: targets = the vertices of `faces`, g2 = grad_pos, g1 = grad_w;  SPACE 1: targets = the vertices of attr_faces, g2 = grad_attr
template <typename TP, int SPACE>
struct TriVertexOp {
    TriMesh<TP> mesh;
    const double* terms;      // [n_sets][F][15]; null: the taps alone (count and fill)
    double *g2, *g1;
    int64_t g2_set, g1_set;
    int n;                    // V or Va
    template <typename ADD>
    LERF_HD void apply(int, int f, int s, ADD add) const {
        TriFace t;
        int32_t ai[3];
        double wv[3];
        RasterBox box;
        if (!mesh.read(s, f, &t, ai, wv) ||
            !tri_setup(t, mesh.depth != nullptr, mesh.w != nullptr, wv[0], wv[1], wv[2], mesh.orient, mesh.max_span, mesh.i0, mesh.j0, mesh.oH, mesh.oW, &box))
            return;
        const int32_t idx[3] = {SPACE ? ai[0] : t.ia, SPACE ? ai[1] : t.ib, SPACE ? ai[2] : t.ic};
        const double* T = terms ? terms + ((int64_t)s * mesh.F + f) * kTriBwdTerms : nullptr;
        for (int k = 0; k < 3; ++k) {
            const int o = 5 * k + (SPACE ? 0 : 2);
            add(0, (int)idx[k], T ? T[o] : 0.0, T ? T[o + 1] : 0.0);
            if (SPACE == 0 && T && g1) add(1, (int64_t)idx[k], T[5 * k + 4]);      // plane 1: neither counted nor listed (CountAt, FillAt)
        }
    }
    LERF_HD int target_h() const { return 1; }
    LERF_HD int target_w() const { return n; }
    LERF_HD TriVertexOp scatter_only() const { return *this; }
    LERF_HD TriVertexOp taps_only() const { TriVertexOp o = *this; o.terms = nullptr; return o; }
    LERF_HD KeepVertexAt keep_at(int s, int64_t q) const {
        return {g2 ? g2 + set_offset(s, g2_set) : nullptr, g1 ? g1 + set_offset(s, g1_set) : nullptr, q};
    }
};

struct TriBwdLayout {
    int64_t n_max, n_slots, partials;
    uint32_t *header, *cursor, *list, *scan;
    double* terms;
    TriBwdLayout(void* ws, int64_t F, int64_t V, int64_t Va, int sets) : n_max(V > Va ? V : Va), n_slots(3 * F), partials(scan_partials(V > Va ? V : Va)) {
        header = (uint32_t*)ws;
        terms = (double*)(header + kOrderedHeaderWords);
        cursor = (uint32_t*)(terms + (int64_t)sets * F * kTriBwdTerms);
        list = cursor + (int64_t)sets * n_max;
        scan = list + (int64_t)sets * n_slots;
    }
    OrderedView view(int64_t n_targets) const { return {header + kOrderedMaxWord, cursor, list, scan, n_targets, n_slots}; }      // V or Va
    static size_t bytes(int64_t F, int64_t V, int64_t Va, int sets) {
        const int64_t n = V > Va ? V : Va;
        return sizeof(uint32_t) * kOrderedHeaderWords + sizeof(double) * (size_t)sets * (size_t)F * kTriBwdTerms +
               sizeof(uint32_t) * (size_t)sets * ((size_t)n + 3 * (size_t)F + (size_t)scan_partials(n));
    }
};

template <typename TP, typename TA, bool HAS_W>
__global__ void __launch_bounds__(64 * kTriBwdWaves)
trimesh_bwd_face_kernel(const TriMesh<TP> mesh, const TA* __restrict__ attr, int64_t attr_set, const uint64_t* __restrict__ keys, int64_t keys_set,
                        const double* __restrict__ gout, int64_t gout_set, double* __restrict__ terms) {
#pragma clang fp contract(off)
    constexpr int NS = HAS_W ? kTriBwdTerms : 6;
    __shared__ double wsum[kTriBwdWaves][NS];
    const int f = (int)blockIdx.x, s = (int)blockIdx.y;
    const int r = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64)), l = threadIdx.x & 63;
    TriFace t;
    int32_t ai[3];
    double wv[3];
    RasterBox box;
    if (!mesh.read(s, f, &t, ai, wv) ||
        !tri_setup(t, mesh.depth != nullptr, HAS_W, wv[0], wv[1], wv[2], mesh.orient, mesh.max_span, mesh.i0, mesh.j0, mesh.oH, mesh.oW, &box))
        return;                                                          // the whole workgroup: f and s are the block's
    const TA* a = attr + set_offset(s, attr_set);
    const Point aA = load_entry(a, 0, 0, ai[0]), aB = load_entry(a, 0, 0, ai[1]), aC = load_entry(a, 0, 0, ai[2]);
    const TriGrads G = tri_grads(t, box.area2);
    double acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = 0.0;
    tri_bwd_thread<HAS_W>(t, box, G, aA, aB, aC, wv[0], wv[1], wv[2], (uint32_t)f, mesh.i0, mesh.j0, mesh.oW, keys + set_offset(s, keys_set),
                          gout + set_offset(s, gout_set), r, l, acc);
#pragma unroll
    for (int k = 0; k < NS; ++k) {
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) acc[k] = acc[k] + __shfl_xor(acc[k], m, 64);
        if (l == 0) wsum[r][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double S[kTriBwdTerms], T[kTriBwdTerms];
#pragma unroll
    for (int k = 0; k < kTriBwdTerms; ++k) S[k] = 0.0;
#pragma unroll
    for (int k = 0; k < NS; ++k) S[HAS_W ? k : 5 * (k / 2) + (k & 1)] = ((wsum[0][k] + wsum[1][k]) + wsum[2][k]) + wsum[3][k];
    tri_face_terms(G, aA, aB, aC, HAS_W, S, T);
    double* dst = terms + ((int64_t)s * mesh.F + f) * kTriBwdTerms;
#pragma unroll
    for (int k = 0; k < kTriBwdTerms; ++k) dst[k] = T[k];
}

// the face pass of the host twin: the 256 slots of every face one after the other, the same tree
template <typename TP, typename TA, bool HAS_W>
void trimesh_bwd_faces_host(const TriMesh<TP>& mesh, const TA* attr, int64_t attr_set, const uint64_t* keys, int64_t keys_set, const double* gout,
                            int64_t gout_set, int n_sets, double* terms) {
#pragma clang fp contract(off)
    constexpr int NS = HAS_W ? kTriBwdTerms : 6, NT = 64 * kTriBwdWaves;
    std::vector<double> part((size_t)NT * NS);
    for (int s = 0; s < n_sets; ++s)
        for (int f = 0; f < mesh.F; ++f) {
            TriFace t;
            int32_t ai[3];
            double wv[3];
            RasterBox box;
            if (!mesh.read(s, f, &t, ai, wv) ||
                !tri_setup(t, mesh.depth != nullptr, HAS_W, wv[0], wv[1], wv[2], mesh.orient, mesh.max_span, mesh.i0, mesh.j0, mesh.oH, mesh.oW, &box))
                continue;
            const TA* a = attr + set_offset(s, attr_set);
            const Point aA = load_entry(a, 0, 0, ai[0]), aB = load_entry(a, 0, 0, ai[1]), aC = load_entry(a, 0, 0, ai[2]);
            const TriGrads G = tri_grads(t, box.area2);
            for (int th = 0; th < NT; ++th) {
                double* acc = &part[(size_t)th * NS];
                for (int k = 0; k < NS; ++k) acc[k] = 0.0;
                tri_bwd_thread<HAS_W>(t, box, G, aA, aB, aC, wv[0], wv[1], wv[2], (uint32_t)f, mesh.i0, mesh.j0, mesh.oW, keys + set_offset(s, keys_set),
                                      gout + set_offset(s, gout_set), th / 64, th % 64, acc);
            }
            double S[kTriBwdTerms], T[kTriBwdTerms];
            for (int k = 0; k < kTriBwdTerms; ++k) S[k] = 0.0;
            for (int k = 0; k < NS; ++k) {
                double p[kTriBwdWaves];
                for (int r = 0; r < kTriBwdWaves; ++r) {
                    double x[64], y[64];
                    for (int l = 0; l < 64; ++l) x[l] = part[(size_t)(64 * r + l) * NS + k];
                    for (int m = 32; m > 0; m >>= 1) {
                        for (int l = 0; l < 64; ++l) y[l] = x[l] + x[l ^ m];
                        for (int l = 0; l < 64; ++l) x[l] = y[l];
                    }
                    p[r] = x[0];
                }
                S[HAS_W ? k : 5 * (k / 2) + (k & 1)] = ((p[0] + p[1]) + p[2]) + p[3];
            }
            tri_face_terms(G, aA, aB, aC, HAS_W, S, T);
            double* dst = terms + ((int64_t)s * mesh.F + f) * kTriBwdTerms;
            for (int k = 0; k < kTriBwdTerms; ++k) dst[k] = T[k];
        }
}

// the two runners of the adjoint: the face pass, then the vertex pass per target space that is wanted
struct TriBwdOnDevice {
    hipStream_t stream;
    template <typename OP>
    int vertices(const OP& op, const TriBwdLayout& L, int F, int sets, int max_adders) const {
        if (hipMemsetAsync(L.cursor, 0, sizeof(uint32_t) * (size_t)sets * (size_t)op.n, stream) != hipSuccess) return LERF_ELAUNCH;
        return ordered_passes_device(stream, op, 1, F, sets, L.view(op.n), max_adders);
    }
    template <typename TP, typename TA>
    int operator()(const TriMesh<TP>& mesh, const TA* attr, int64_t attr_set, const uint64_t* keys, int64_t keys_set, const double* gout,
                   int64_t gout_set, int n_sets, double* gattr, int64_t gattr_set, double* gpos, int64_t gpos_set, double* gw, int64_t gw_set, void* ws,
                   int max_adders) const {
        const TriBwdLayout L(ws, mesh.F, mesh.V, mesh.Va, n_sets);
        clear_stale_error();
        if (hipMemsetAsync(L.header, 0, sizeof(uint32_t) * kOrderedHeaderWords, stream) != hipSuccess) return LERF_ELAUNCH;
        const dim3 grid((unsigned)mesh.F, (unsigned)n_sets), block(64 * kTriBwdWaves);
        if (mesh.w)
            hipLaunchKernelGGL((trimesh_bwd_face_kernel<TP, TA, true>), grid, block, 0, stream, mesh, attr, attr_set, keys, keys_set, gout, gout_set, L.terms);
        else
            hipLaunchKernelGGL((trimesh_bwd_face_kernel<TP, TA, false>), grid, block, 0, stream, mesh, attr, attr_set, keys, keys_set, gout, gout_set, L.terms);
        int rc = launch_status();
        if (rc != LERF_OK) return rc;
        if (gpos || gw) rc = vertices(TriVertexOp<TP, 0>{mesh, L.terms, gpos, gw, gpos_set, gw_set, mesh.V}, L, mesh.F, n_sets, max_adders);
        if (rc != LERF_OK) return rc;
        if (gattr) rc = vertices(TriVertexOp<TP, 1>{mesh, L.terms, gattr, nullptr, gattr_set, 0, mesh.Va}, L, mesh.F, n_sets, max_adders);
        return rc;
    }
};

struct TriBwdOnHost {
    template <typename OP>
    int vertices(const OP& op, const TriBwdLayout& L, int F, int sets, int max_adders) const {
        for (int64_t k = 0; k < (int64_t)sets * op.n; ++k) L.cursor[k] = 0;
        ordered_passes_host(op, 1, F, sets, L.view(op.n), max_adders);
        return LERF_OK;
    }
    template <typename TP, typename TA>
    int operator()(const TriMesh<TP>& mesh, const TA* attr, int64_t attr_set, const uint64_t* keys, int64_t keys_set, const double* gout,
                   int64_t gout_set, int n_sets, double* gattr, int64_t gattr_set, double* gpos, int64_t gpos_set, double* gw, int64_t gw_set, void* ws,
                   int max_adders) const {
        const TriBwdLayout L(ws, mesh.F, mesh.V, mesh.Va, n_sets);
        for (int k = 0; k < kOrderedHeaderWords; ++k) L.header[k] = 0;
        if (mesh.w) trimesh_bwd_faces_host<TP, TA, true>(mesh, attr, attr_set, keys, keys_set, gout, gout_set, n_sets, L.terms);
        else trimesh_bwd_faces_host<TP, TA, false>(mesh, attr, attr_set, keys, keys_set, gout, gout_set, n_sets, L.terms);
        if (gpos || gw) vertices(TriVertexOp<TP, 0>{mesh, L.terms, gpos, gw, gpos_set, gw_set, mesh.V}, L, mesh.F, n_sets, max_adders);
        if (gattr) vertices(TriVertexOp<TP, 1>{mesh, L.terms, gattr, nullptr, gattr_set, 0, mesh.Va}, L, mesh.F, n_sets, max_adders);
        return LERF_OK;
    }
};

// pass 1 of the adjoint: grid (ceil(oW / 64), gh, sets), block (64, 4); set s reads gmap + s * gmap_set (in entries) and owns tmp [s][gh][oW]
template <int INTERP>
__global__ void __launch_bounds__(CB_COLS * CB_ROWS)
coords_mesh_bwd_rows_kernel(const double2* __restrict__ gmap, int oH, int oW, int gh, double2* __restrict__ tmp, int64_t gmap_set) {
#pragma clang fp contract(off)
    __shared__ double2 part[CB_ROWS][CB_COLS];
    gmap += (int64_t)blockIdx.z * gmap_set;
    tmp += (int64_t)blockIdx.z * gh * oW;
    const int a = blockIdx.y, j = blockIdx.x * CB_COLS + threadIdx.x, w = threadIdx.y;
    int lo, hi;
    mesh_reach<INTERP>(a, oH, gh, &lo, &hi);
    double2 acc = make_double2(0.0, 0.0);
    if (j < oW)
        for (int i = lo + w; i <= hi; i += CB_ROWS) {
            const double wt = mesh_weight_on<INTERP>(i, oH, gh, a);
            if (wt == 0.0) continue;
            const double2 g = gmap[(int64_t)i * oW + j];
            acc.x = acc.x + wt * g.x;
            acc.y = acc.y + wt * g.y;
        }
    part[w][threadIdx.x] = acc;
    __syncthreads();
    if (w == 0 && j < oW) {
        double2 s = part[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < CB_ROWS; ++k) {
            s.x = s.x + part[k][threadIdx.x].x;
            s.y = s.y + part[k][threadIdx.x].y;
        }
        tmp[(int64_t)a * oW + j] = s;
    }
}

// pass 2: grid (gw, gh, sets), block 64 = one wave per vertex; set s reads tmp [s][gh][oW] and adds into gctrl + s * gctrl_set (in entries)
template <int INTERP>
__global__ void __launch_bounds__(64)
coords_mesh_bwd_cols_kernel(const double2* __restrict__ tmp, int oW, int gw, double2* __restrict__ gctrl, int64_t gctrl_set) {
#pragma clang fp contract(off)
    tmp += (int64_t)blockIdx.z * gridDim.y * oW;
    gctrl += (int64_t)blockIdx.z * gctrl_set;
    const int b = blockIdx.x, a = blockIdx.y, lane = threadIdx.x;
    int lo, hi;
    mesh_reach<INTERP>(b, oW, gw, &lo, &hi);
    double sx = 0.0, sy = 0.0;
    for (int j = lo + lane; j <= hi; j += 64) {
        const double wt = mesh_weight_on<INTERP>(j, oW, gw, b);
        if (wt == 0.0) continue;
        const double2 t = tmp[(int64_t)a * oW + j];
        sx = sx + wt * t.x;
        sy = sy + wt * t.y;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sx = sx + __shfl_down(sx, off, 64);
        sy = sy + __shfl_down(sy, off, 64);
    }
    if (lane == 0) {
        double2* dst = gctrl + (int64_t)a * gw + b;
        double2 v = *dst;
        v.x += sx;
        v.y += sy;
        *dst = v;
    }
}

static_assert(kBwdCols == CB_COLS && kBwdWaves == CB_ROWS && kBwdBand % kBwdWaves == 0, "the band of the build backward is the block's");

// pass 1 of the build backward: grid (ceil(oW / 64), ceil(oH / 64), n_sets), block (64, 4); part [n_sets][NP][nblk]
template <int MODEL>
__global__ void __launch_bounds__(CB_COLS * CB_ROWS)
coords_build_bwd_partial_kernel(const double* __restrict__ params, const double2* __restrict__ gmap, int oH, int oW, int i0, int j0,
                                double* __restrict__ part) {
#pragma clang fp contract(off)
    constexpr int NP = model_params(MODEL);
    __shared__ double wsum[kBwdWaves][NP];
    const int s = blockIdx.z, w = threadIdx.y, j = blockIdx.x * CB_COLS + threadIdx.x;
    const double* p = params + (size_t)s * NP;
    const double2* g = gmap + (size_t)s * oH * oW;
    double acc[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) acc[k] = 0.0;
    if (j < oW)
        for (int i = blockIdx.y * kBwdBand + w; i < oH && i < (int)(blockIdx.y + 1) * kBwdBand; i += kBwdWaves) {
            const double2 gv = g[(int64_t)i * oW + j];
            double dp[NP];
            model_point_bwd<MODEL>(p, i0 + i, j0 + j, Point{gv.x, gv.y}, dp);
#pragma unroll
            for (int k = 0; k < NP; ++k) acc[k] = acc[k] + dp[k];
        }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[k] = acc[k] + __shfl_down(acc[k], off, 64);
        if (threadIdx.x == 0) wsum[w][k] = acc[k];
    }
    __syncthreads();
    const int k = threadIdx.y * CB_COLS + threadIdx.x;
    if (k < NP) {
        const int nblk = gridDim.x * gridDim.y, blk = blockIdx.y * gridDim.x + blockIdx.x;
        part[((size_t)s * NP + k) * nblk + blk] = ((wsum[0][k] + wsum[1][k]) + wsum[2][k]) + wsum[3][k];
    }
}

// pass 2: grid (n_params, n_sets), block 64 = one wave per sum
__global__ void __launch_bounds__(64)
coords_build_bwd_sum_kernel(const double* __restrict__ part, int nblk, double* __restrict__ gparams) {
#pragma clang fp contract(off)
    const size_t e = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    const double* src = part + e * nblk;
    double v = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 64) v = v + src[b];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
    if (threadIdx.x == 0) gparams[e] = gparams[e] + v;
}

// the adjoint of reproject (reproject_point_bwd) in the shape of the build backward's pass 1 -- the same grid, block, band and lanes; part
// [n_sets][12][nblk].  Every lane is the ONE writer of grad_depth at its entries (a plain load-add-store); SUMS: the 12 running sums, the
// trees and the block's partial vector, then coords_build_bwd_sum_kernel as pass 2.  gzo, gdepth: null = not given (wave-uniform).
template <int KIND, typename TD, bool SUMS>
__global__ void __launch_bounds__(CB_COLS * CB_ROWS)
coords_reproject_bwd_kernel(const double* __restrict__ params, const TD* __restrict__ depth, int64_t depth_set, const double2* __restrict__ gmap,
                            const double* __restrict__ gzo, int oH, int oW, int i0, int j0, double* __restrict__ gdepth,
                            double* __restrict__ part) {
#pragma clang fp contract(off)
    constexpr int NP = kReprojectParams;
    __shared__ double wsum[kBwdWaves][NP];
    const int s = blockIdx.z, w = threadIdx.y, j = blockIdx.x * CB_COLS + threadIdx.x;
    const double* p = params + (size_t)s * NP;
    const TD* dep = depth + set_offset(s, depth_set);
    const size_t plane = (size_t)s * oH * oW;
    double acc[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) acc[k] = 0.0;
    if (j < oW)
        for (int i = blockIdx.y * kBwdBand + w; i < oH && i < (int)(blockIdx.y + 1) * kBwdBand; i += kBwdWaves) {
            const int64_t e = (int64_t)i * oW + j;
            const double2 gv = gmap[plane + e];
            double dp[NP];
            const double dd = reproject_point_bwd<KIND>(p, (double)dep[e], i0 + i, j0 + j, Point{gv.x, gv.y}, gzo ? gzo[plane + e] : 0.0, dp);
            if (gdepth) gdepth[plane + e] = gdepth[plane + e] + dd;
            if (SUMS) {
#pragma unroll
                for (int k = 0; k < NP; ++k) acc[k] = acc[k] + dp[k];
            }
        }
    if (!SUMS) return;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[k] = acc[k] + __shfl_down(acc[k], off, 64);
        if (threadIdx.x == 0) wsum[w][k] = acc[k];
    }
    __syncthreads();
    const int k = threadIdx.y * CB_COLS + threadIdx.x;
    if (k < NP) {
        const int nblk = gridDim.x * gridDim.y, blk = blockIdx.y * gridDim.x + blockIdx.x;
        part[((size_t)s * NP + k) * nblk + blk] = ((wsum[0][k] + wsum[1][k]) + wsum[2][k]) + wsum[3][k];
    }
}

// the three-way choice of lerf_coords_math for element e; y is read for atan2 alone
LERF_HD inline double math_element(int op, const double* x, const double* y, int64_t e) {
    return op == LERF_MATH_SQRT ? sqrt_pm(x[e]) : op == LERF_MATH_ATAN ? atan_pm(x[e]) : atan2_pm(x[e], y[e]);
}

// the helpers of the lens models on their own (lerf_coords_math): one thread per element, grid ceil(n / 256)
__global__ void __launch_bounds__(256)
coords_math_kernel(int op, const double* __restrict__ x, const double* __restrict__ y, int64_t n, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    out[e] = math_element(op, x, y, e);
}

// ------------------------------------------------------------------------------------------------ argument checks (host)
inline bool float_dtype(int dt) { return dt == LERF_F32 || dt == LERF_F64; }
inline size_t entry_bytes(int dt) { return dt == LERF_F32 ? 8 : 16; }

// ONE OPERAND TABLE PER CALL.  Every entry point states its operands (Operand), each with its ROLE, and its scalar rules (one bool),
// and check_call judges them: the one place that looks at a pointer, an alignment, a dtype, a row stride, a set stride or an overlap,
// for a single map (n_sets = 1, set strides 0) and for a batch alike.  WHICH OPERANDS MAY INTERSECT is not listed but derived from the
// roles: an operand the call writes intersects no other operand of the call (check_call; its two stated exceptions are there).
//
// One operand over the n_sets sets of a call: set s at p + s * set_stride elements of `el` bytes, each set `span` elements from its
// first to one past its last (the ONE place an extent is computed: the constructors below); pairs: the elements are (row, col) pairs
// (maps, gradients), so the set stride is even; SHARE: a set stride of 0 (one operand for all sets) is allowed; OPTIONAL: may be null
// (init, depth, a skipped gradient, the workspace the host twin does not have) and then passes every check; WRITTEN: the call writes
// it (an output, keys, a gradient, a workspace).  shape_ok is false for a descriptor made of a dtype code or dimensions that are not
// valid: its extent means nothing, and check_call refuses it first.
enum : unsigned { SHARE = 1, OPTIONAL = 2, WRITTEN = 4 };
struct Operand {
    const void* p;
    size_t el, align;
    int64_t span, set_stride;
    bool pairs, share, optional, written, shape_ok, rows_ok;
};

// a map under the strided contract: [h][w] entries of dtype dt, rows `stride` elements apart (even, >= 2 w), h, w >= min_hw
inline Operand map_operand(const void* p, int dt, int64_t stride, int h, int w, int64_t set_stride, unsigned flags = 0, int min_hw = 1) {
    const bool null_ok = !p && (flags & OPTIONAL);
    return {p, entry_bytes(dt) / 2, entry_bytes(dt), (int64_t)(h - 1) * stride + 2 * (int64_t)w, set_stride, true, (flags & SHARE) != 0,
            (flags & OPTIONAL) != 0, (flags & WRITTEN) != 0, null_ok || (float_dtype(dt) && h >= min_hw && w >= min_hw),
            !(stride & 1) && stride >= 2 * (int64_t)w};
}
// a dense gradient (float64) or control mesh [h][w][2]: the map of row stride 2 w
inline Operand dense_operand(const void* p, int dt, int h, int w, int64_t set_stride, unsigned flags = 0, int min_hw = 1) {
    return map_operand(p, dt, 2 * (int64_t)w, h, w, set_stride, flags, min_hw);
}
// a dense plane [h][w] of scalars of `el` bytes (keys, depth); its dimensions are those of a map of the same call, checked there
inline Operand plane_operand(const void* p, size_t el, int h, int w, int64_t set_stride, unsigned flags = 0) {
    return {p, el, el, (int64_t)h * w, set_stride, false, (flags & SHARE) != 0, (flags & OPTIONAL) != 0, (flags & WRITTEN) != 0, true, true};
}
// `bytes` bytes per set, the sets one behind the other (params, grad_params, the partials of the two-pass adjoints)
inline Operand bytes_operand(const void* p, int64_t bytes, size_t align, unsigned flags = 0) {
    return {p, 1, align, bytes, bytes, false, false, (flags & OPTIONAL) != 0, (flags & WRITTEN) != 0, true, true};
}
// a workspace of `bytes` bytes for the WHOLE call (the rasteriser's, the mesh adjoint's, the ordered scatter's): one extent, shared, written
inline Operand workspace_operand(const void* p, int64_t bytes, size_t align) { return {p, 1, align, bytes, 0, false, true, false, true, true, true}; }
// a parameter block [n_sets][n_params] float64 (params, grad_params)
inline Operand params_operand(const void* p, int n_params, unsigned flags = 0) { return bytes_operand(p, 8 * (int64_t)n_params, sizeof(double), flags); }

// the bytes of two operands over the whole batch (first element of set 0 to one past the last of the last set) intersect
inline bool operands_overlap(int n_sets, const Operand& x, const Operand& y) {
    if (!x.p || !y.p) return false;
    const uintptr_t a = (uintptr_t)x.p, b = (uintptr_t)y.p;
    const size_t an = (size_t)((int64_t)(n_sets - 1) * x.set_stride + x.span) * x.el, bn = (size_t)((int64_t)(n_sets - 1) * y.set_stride + y.span) * y.el;
    return a < b + bn && b < a + an;
}

// THE TWO EXCEPTIONS to "a written operand intersects no other": batch_only -- mesh, compose and the mesh adjoint judge overlaps for
// n_sets > 1 only, their single-map forms have always allowed them; Allow -- compose's out may lie on b when it IS b (in place).
struct Allow { int written = -1, other = -1; };      // indices into the call's table

// The judgement of a call, in the order the return codes have had since the batched forms exist: a descriptor without a shape and
// n_sets < 1 are LERF_EINVAL, n_sets beyond the grid's z is `too_many` (LERF_EUNSUPPORTED for the chained operations), then the scalar
// rules, every operand's pointer, alignment, row stride and set stride, and the overlaps -- every present WRITTEN operand against
// every other present operand, over the whole batch: LERF_EINVAL.  A refused call launches nothing.
inline int check_call(int n_sets, std::initializer_list<Operand> ops, bool rules, int too_many = LERF_EUNSUPPORTED, bool batch_only = false,
                      Allow allow = {}) {
    for (const Operand& o : ops)
        if (!o.shape_ok) return LERF_EINVAL;
    if (n_sets < 1) return LERF_EINVAL;
    if (n_sets > 65535) return too_many;
    if (!rules) return LERF_EINVAL;
    for (const Operand& o : ops) {
        if (!o.p && o.optional) continue;
        if (!o.p || (size_t)(uintptr_t)o.p % o.align != 0 || !o.rows_ok) return LERF_EINVAL;
        if (o.set_stride < 0 || (o.pairs && (o.set_stride & 1))) return LERF_EINVAL;
        if (n_sets > 1 && o.set_stride < o.span && !(o.share && o.set_stride == 0)) return LERF_EINVAL;
    }
    if (batch_only && n_sets == 1) return LERF_OK;
    const int n = (int)ops.size();
    for (int x = 0; x < n; ++x)
        for (int y = 0; y < n; ++y)
            if (x != y && ops.begin()[x].written && !(x == allow.written && y == allow.other) && operands_overlap(n_sets, ops.begin()[x], ops.begin()[y]))
                return LERF_EINVAL;
    return LERF_OK;
}

inline bool tile_ok(int oH, int oW, int i0, int j0) {
    return i0 >= 0 && j0 >= 0 && (int64_t)i0 + oH <= 0x7fffffff && (int64_t)j0 + oW <= 0x7fffffff && (oH + CB_ROWS - 1) / CB_ROWS <= 65535;
}

inline int build_args(int model, const double* params, int n_params, const void* out, int out_dtype, int64_t stride, int oH, int oW,
                      int i0, int j0, Params& prm) {
    const int rc = check_call(1, {map_operand(out, out_dtype, stride, oH, oW, 0, WRITTEN)},
                              params && tile_ok(oH, oW, i0, j0) && model_params(model) >= 0 && n_params == model_params(model));
    if (rc != LERF_OK) return rc;
    for (int k = 0; k < kMaxParams; ++k) prm.p[k] = 0.0;
    for (int k = 0; k < n_params; ++k) {
        if (!std::isfinite(params[k])) return LERF_EINVAL;
        prm.p[k] = params[k];
    }
    return LERF_OK;
}

// device parameters cannot be inspected here: their count, the pointers and the layout of the n_sets maps are what is checked.  For
// this one and the two-pass adjoints, n_sets beyond the grid's z is LERF_EINVAL
inline int build_dev_args(int model, const double* params, int n_sets, int n_params, const void* out, int out_dtype, int64_t set_stride,
                          int64_t stride, int oH, int oW, int i0, int j0) {
    return check_call(n_sets, {params_operand(params, n_params), map_operand(out, out_dtype, stride, oH, oW, set_stride, WRITTEN)}, tile_ok(oH, oW, i0, j0) && model_params(model) >= 0 && n_params == model_params(model), LERF_EINVAL);
}

// run F with MODEL = the compile-time constant of a model code the argument checks have accepted
#define LERF_COORDS_MODEL(code, MODEL, ...)                                                                  \
    do {                                                                                                     \
        switch (code) {                                                                                      \
            case LERF_COORDS_HOMOGRAPHY: { constexpr int MODEL = LERF_COORDS_HOMOGRAPHY; __VA_ARGS__; } break; \
            case LERF_COORDS_RADIAL: { constexpr int MODEL = LERF_COORDS_RADIAL; __VA_ARGS__; } break;       \
            case LERF_COORDS_BROWN: { constexpr int MODEL = LERF_COORDS_BROWN; __VA_ARGS__; } break;         \
            case LERF_COORDS_FISHEYE: { constexpr int MODEL = LERF_COORDS_FISHEYE; __VA_ARGS__; } break;     \
            default: { constexpr int MODEL = LERF_COORDS_EQUIRECT; __VA_ARGS__; } break;                     \
        }                                                                                                    \
    } while (0)

inline int math_args(int op, const double* x, const double* y, int64_t n, const double* out) {
    if (op != LERF_MATH_SQRT && op != LERF_MATH_ATAN && op != LERF_MATH_ATAN2) return LERF_EINVAL;
    if (!x || !out || (op == LERF_MATH_ATAN2 && !y) || n < 0 || n > 0x7fffffff) return LERF_EINVAL;
    return LERF_OK;
}

// run F with the C++ type of a float dtype code
#define LERF_COORDS_DT(code, T, ...)          \
    do {                                      \
        if ((code) == LERF_F32) { using T = float; __VA_ARGS__; } \
        else { using T = double; __VA_ARGS__; } \
    } while (0)

// What an _ordered entry point adds to its sibling's table: the workspace as one more operand (4-byte aligned, one extent for the
// whole call, intersecting no other operand) and three rules -- it is there, it holds ordered_bytes, max_adders >= 1.  The plain
// entry points pass none (ord == nullptr) and their tables judge as before.  Sizes the uint32 ids cannot hold are judged FIRST, before
// any pointer: LERF_EUNSUPPORTED.
struct OrderedArgs {
    void* ws;
    size_t ws_bytes;
    int max_adders;
};

inline bool ordered_sizes_ok(int64_t n_entries, int64_t n_targets) { return 4 * n_entries <= 0xffffffffLL && n_targets <= 0xffffffffLL; }

inline Operand ordered_ws_operand(const OrderedArgs* ord, int64_t n_entries, int64_t n_targets, int n_sets) {
    if (!ord) return bytes_operand(nullptr, 0, 4, OPTIONAL);
    const bool sane = n_sets >= 1 && n_sets <= 65535 && n_entries >= 1 && n_targets >= 1 && ordered_sizes_ok(n_entries, n_targets);
    return workspace_operand(ord->ws, sane ? (int64_t)OrderedLayout::bytes(n_entries, n_targets, n_sets) : 0, 4);
}

inline bool ordered_rules(const OrderedArgs* ord, const Operand& ws) {
    return !ord || (ord->ws && ord->max_adders >= 1 && ord->ws_bytes >= (size_t)ws.span);
}

// ------------------------------------------------------------------------------------------------ the operations, over a runner
template <typename RUN>
int build(RUN run, int model, const double* params, int n_params, void* out, int out_dtype, int64_t stride, int oH, int oW, int i0, int j0) {
    Params prm;
    const int rc = build_args(model, params, n_params, out, out_dtype, stride, oH, oW, i0, j0, prm);
    if (rc != LERF_OK) return rc;
    LERF_COORDS_MODEL(model, MODEL, LERF_COORDS_DT(out_dtype, TO, return run(BuildOp<MODEL, TO>{prm, (TO*)out, stride, i0, j0}, oH, oW)));
}

template <typename RUN>
int build_dev(RUN run, int model, const double* params, int n_sets, int n_params, void* out, int out_dtype, int64_t set_stride,
              int64_t stride, int oH, int oW, int i0, int j0) {
    const int rc = build_dev_args(model, params, n_sets, n_params, out, out_dtype, set_stride, stride, oH, oW, i0, j0);
    if (rc != LERF_OK) return rc;
    LERF_COORDS_MODEL(model, MODEL, LERF_COORDS_DT(out_dtype, TO,
        return run(BuildDevOp<MODEL, TO>{params, (TO*)out, set_stride, stride, i0, j0}, oH, oW, n_sets)));
}

// Each of the chained operations below takes n_sets and one set stride per operand; a single-map entry point is the batched one with
// n_sets = 1 and every set stride 0.  Each states its table once: the operands with their roles (a WRITTEN one intersects no other,
// over the whole batch; batch_only: judged in a batch only, where the single-map form has always allowed it), the scalar rules.
template <typename RUN>
int mesh(RUN run, const void* ctrl, int ctrl_dtype, int gh, int gw, int interp, int full_h, int full_w, void* out, int out_dtype,
         int64_t stride, int oH, int oW, int i0, int j0, int n_sets, int64_t ctrl_set, int64_t out_set) {
    const int rc = check_call(n_sets, {dense_operand(ctrl, ctrl_dtype, gh, gw, ctrl_set, 0, 2), map_operand(out, out_dtype, stride, oH, oW, out_set, WRITTEN)},
                              (interp == LERF_MESH_BILINEAR || interp == LERF_MESH_BICUBIC) && tile_ok(oH, oW, i0, j0) && full_h >= 1 && full_w >= 1 &&
                                  (int64_t)i0 + oH <= full_h && (int64_t)j0 + oW <= full_w,
                              LERF_EUNSUPPORTED, /*batch_only=*/true);
    if (rc != LERF_OK) return rc;
    LERF_COORDS_DT(ctrl_dtype, TC, LERF_COORDS_DT(out_dtype, TO, {
        if (interp == LERF_MESH_BILINEAR)
            return run(MeshOp<LERF_MESH_BILINEAR, TC, TO>{(const TC*)ctrl, gh, gw, full_h, full_w, (TO*)out, stride, i0, j0, ctrl_set, out_set},
                       oH, oW, n_sets);
        return run(MeshOp<LERF_MESH_BICUBIC, TC, TO>{(const TC*)ctrl, gh, gw, full_h, full_w, (TO*)out, stride, i0, j0, ctrl_set, out_set},
                   oH, oW, n_sets);
    }));
}

template <typename RUN>
int compose(RUN run, const void* a, int a_dtype, int64_t a_stride, int aH, int aW, const void* b, int b_dtype, int64_t b_stride, void* out,
            int out_dtype, int64_t o_stride, int oH, int oW, int n_sets, int64_t a_set, int64_t b_set, int64_t out_set) {
    enum { A, B, OUT };
    const bool in_place = out == b && out_dtype == b_dtype && o_stride == b_stride && out_set == b_set;
    const int rc = check_call(n_sets,
                              {map_operand(a, a_dtype, a_stride, aH, aW, a_set, SHARE), map_operand(b, b_dtype, b_stride, oH, oW, b_set),
                               map_operand(out, out_dtype, o_stride, oH, oW, out_set, WRITTEN)},
                              tile_ok(oH, oW, 0, 0), LERF_EUNSUPPORTED, /*batch_only=*/true, in_place ? Allow{OUT, B} : Allow{});
    if (rc != LERF_OK) return rc;
    LERF_COORDS_DT(a_dtype, TA, LERF_COORDS_DT(b_dtype, TB, LERF_COORDS_DT(out_dtype, TO,
        return run(ComposeOp<TA, TB, TO>{{(const TA*)a, a_stride}, aH, aW, {(const TB*)b, b_stride}, (TO*)out, o_stride, a_set, b_set, out_set},
                   oH, oW, n_sets))));
}

template <typename RUN>
int invert(RUN run, const void* f, int f_dtype, int64_t f_stride, int fH, int fW, const void* init, int init_dtype, int64_t i_stride,
           void* out, int out_dtype, int64_t o_stride, int oH, int oW, int i0, int j0, int max_iter, double tol, int n_sets, int64_t f_set,
           int64_t init_set, int64_t out_set) {
    const int rc = check_call(n_sets,
                              {map_operand(f, f_dtype, f_stride, fH, fW, f_set, SHARE), map_operand(init, init_dtype, i_stride, oH, oW, init_set, SHARE | OPTIONAL),
                               map_operand(out, out_dtype, o_stride, oH, oW, out_set, WRITTEN)},
                              fH >= 2 && fW >= 2 && tile_ok(oH, oW, i0, j0) && max_iter >= 1 && max_iter <= 64 && tol >= 0.0 && std::isfinite(tol));
    if (rc != LERF_OK) return rc;
    if (!init) init_dtype = LERF_F64;                     // a null init is never read: one instantiation serves
    LERF_COORDS_DT(f_dtype, TF, LERF_COORDS_DT(init_dtype, TI, LERF_COORDS_DT(out_dtype, TO,
        return run(InvertOp<TF, TI, TO>{{(const TF*)f, f_stride}, fH, fW, {(const TI*)init, i_stride}, (TO*)out, o_stride, i0, j0, max_iter, tol,
                                        f_set, init_set, out_set},
                   oH, oW, n_sets))));
}

// fill, raster, resolve: three launches in stream order (the host: three loops), no sync, no allocation
template <typename RUN, typename SCATTER>
int invert_raster(RUN run, SCATTER scatter, const void* f, int f_dtype, int64_t f_stride, int fH, int fW, const float* depth, void* out,
                  int out_dtype, int64_t o_stride, int oH, int oW, int i0, int j0, int max_span, int orient, uint64_t* keys, int n_sets,
                  int64_t f_set, int64_t depth_set, int64_t out_set, int64_t keys_set) {
    // the cells: a triangle's number fits the key's 32 bits, their rows the grid's y
    const bool cells_ok = 2 * (int64_t)(fH - 1) * (int64_t)(fW - 1) < ((int64_t)1 << 32) && (fH - 1 + CB_ROWS - 1) / CB_ROWS <= 65535;
    int rc = check_call(n_sets,
                        {map_operand(f, f_dtype, f_stride, fH, fW, f_set, SHARE), plane_operand(depth, sizeof(float), fH, fW, depth_set, SHARE | OPTIONAL),
                         map_operand(out, out_dtype, o_stride, oH, oW, out_set, WRITTEN), plane_operand(keys, sizeof(uint64_t), oH, oW, keys_set, WRITTEN)},
                        fH >= 2 && fW >= 2 && tile_ok(oH, oW, i0, j0) && cells_ok && max_span >= 1 && max_span <= kMaxSpan && orient >= -1 && orient <= 1);
    if (rc != LERF_OK) return rc;
    rc = run(KeyFillOp{keys, oW, keys_set}, oH, oW, n_sets);
    if (rc != LERF_OK) return rc;
    LERF_COORDS_DT(f_dtype, TF,
        rc = scatter(RasterOp<TF>{{(const TF*)f, f_stride}, fW, depth, orient, max_span, i0, j0, oH, oW, f_set, depth_set}, fH - 1, fW - 1, keys,
                     n_sets, keys_set));
    if (rc != LERF_OK) return rc;
    LERF_COORDS_DT(f_dtype, TF, LERF_COORDS_DT(out_dtype, TO,
        return run(ResolveOp<TF, TO>{{(const TF*)f, f_stride}, fW, keys, (TO*)out, o_stride, i0, j0, oW, f_set, keys_set, out_set}, oH, oW, n_sets)));
}

// The triangle-mesh rasteriser.  THE SIZE RULE is judged from sizes alone, before any pointer: the item list is indexed
// by uint32, so n_sets * F * b <= 2^32 - 1 with b the most item tiles one face can have (tri_axis_tiles per axis), and the scan's
// n_sets * (F + 1) slots fit too.  0: the sizes are not valid or beyond the rule.
inline uint64_t tri_max_items(int64_t F, int n_sets, int oH, int oW, int max_span) {
    if (F < 1 || F > 0x7fffffffLL || n_sets < 1 || n_sets > 65535 || oH < 1 || oW < 1 || max_span < 0) return 0;
    const uint64_t b = (uint64_t)tri_axis_tiles(oH, max_span, kTileRows) * (uint64_t)tri_axis_tiles(oW, max_span, kTileCols);
    const uint64_t faces = (uint64_t)n_sets * (uint64_t)F, cap = 0xffffffffULL;
    if (faces + (uint64_t)n_sets > cap || b > cap || faces > cap / b) return 0;
    return faces * b;
}

inline int64_t tri_workspace_words(int64_t F, int n_sets) {
    if (F < 1 || F > 0x7fffffffLL || n_sets < 1 || n_sets > 65535 || (int64_t)n_sets * (F + 1) > 0xffffffffLL) return 0;
    const int64_t n_slots = (int64_t)n_sets * (F + 1);
    return n_slots + scan_partials(n_slots);
}

// fill, count, scan, raster, resolve in stream order (the host: fill, the loop over faces, resolve); no sync, no allocation, no read-back
template <typename RUN, typename RASTER>
int trimesh(RUN run, RASTER raster, const void* pos, int pos_dtype, int V, const void* attr, int attr_dtype, int Va, const int32_t* faces,
            const int32_t* attr_faces, int F, const float* depth, const void* w, int w_dtype, void* out, int out_dtype, int64_t o_stride, int oH, int oW, int i0,
            int j0, int max_span, int orient, uint64_t* keys, float* depth_out, void* workspace, size_t workspace_bytes, int n_sets, int64_t pos_set,
            int64_t attr_set, int64_t faces_set, int64_t afaces_set, int64_t depth_set, int64_t w_set, int64_t out_set, int64_t keys_set,
            int64_t dout_set) {
    const bool sizes = V >= 1 && Va >= 1 && F >= 1 && oH >= 1 && oW >= 1 && n_sets >= 1 && n_sets <= 65535 && max_span >= 0 && max_span <= kMaxTriSpan;
    const uint64_t max_items = sizes ? tri_max_items(F, n_sets, oH, oW, max_span) : 0;
    if (sizes && !max_items) return LERF_EUNSUPPORTED;
    const int64_t words = sizes ? tri_workspace_words(F, n_sets) : 0;
    int rc = check_call(n_sets,
                        {dense_operand(pos, pos_dtype, V, 1, pos_set, SHARE), dense_operand(attr, attr_dtype, Va, 1, attr_set, SHARE),
                         plane_operand(faces, sizeof(int32_t), F, 3, faces_set, SHARE),
                         plane_operand(attr_faces, sizeof(int32_t), F, 3, afaces_set, SHARE | OPTIONAL),
                         plane_operand(depth, sizeof(float), V, 1, depth_set, SHARE | OPTIONAL), plane_operand(w, w_dtype == LERF_F64 ? sizeof(double) : sizeof(float), V, 1, w_set, SHARE | OPTIONAL),
                         map_operand(out, out_dtype, o_stride, oH, oW, out_set, WRITTEN), plane_operand(keys, sizeof(uint64_t), oH, oW, keys_set, WRITTEN),
                         plane_operand(depth_out, sizeof(float), oH, oW, dout_set, OPTIONAL | WRITTEN), workspace_operand(workspace, 4 * words, 4)},
                        sizes && tile_ok(oH, oW, i0, j0) && (!w || float_dtype(w_dtype)) && orient >= -1 && orient <= 1 && !(depth_out && !depth) && workspace_bytes >= (size_t)(4 * words));
    if (rc != LERF_OK) return rc;
    rc = run(KeyFillOp{keys, oW, keys_set}, oH, oW, n_sets);
    if (rc != LERF_OK) return rc;
    LERF_COORDS_DT(pos_dtype, TP, {
        const TriMesh<TP> mesh{(const TP*)pos, V, Va, faces, attr_faces, F, depth, w, w_dtype == LERF_F64, orient, max_span, i0, j0, oH, oW,
                               pos_set, faces_set, afaces_set, depth_set, w_set};
        rc = raster(mesh, keys, keys_set, n_sets, (uint32_t*)workspace, max_items);
        if (rc != LERF_OK) return rc;
        LERF_COORDS_DT(attr_dtype, TA, LERF_COORDS_DT(out_dtype, TO,
            return run(TriResolveOp<TP, TA, TO>{mesh, (const TA*)attr, keys, (TO*)out, o_stride, depth_out, attr_set, keys_set, out_set, dout_set},
                       oH, oW, n_sets)));
    });
}

// The adjoint of the triangle mesh.  THE SIZE RULE, from sizes alone and before any pointer: the forward's (the item tiles
// of a face are counted in uint32), and F <= 2^24 - 1: the face pass is one workgroup of 256 threads a face, and a face lists three ids.
constexpr int64_t kTriBwdMaxFaces = 0xffffff;

inline size_t tri_bwd_workspace_bytes(int64_t F, int64_t V, int64_t Va, int n_sets) {
    if (F < 1 || F > kTriBwdMaxFaces || V < 1 || V > 0x7fffffffLL || Va < 1 || Va > 0x7fffffffLL || n_sets < 1 || n_sets > 65535) return 0;
    return TriBwdLayout::bytes(F, V, Va, n_sets);
}

// the face pass, then the vertex pass per wanted target space, in stream order (the host: the same loops); no sync, no allocation, no read-back
template <typename RUN>
int trimesh_bwd(RUN run, const void* pos, int pos_dtype, int V, const void* attr, int attr_dtype, int Va, const int32_t* faces, const int32_t* attr_faces,
                int F, const float* depth, const void* w, int w_dtype, int oH, int oW, int i0, int j0, int max_span, int orient, const uint64_t* keys,
                const double* grad_out, double* grad_attr, double* grad_pos, double* grad_w, void* workspace, size_t workspace_bytes, int max_adders,
                int n_sets, int64_t pos_set, int64_t attr_set, int64_t faces_set, int64_t afaces_set, int64_t depth_set, int64_t w_set, int64_t keys_set,
                int64_t gout_set, int64_t gattr_set, int64_t gpos_set, int64_t gw_set) {
    const bool sizes = V >= 1 && Va >= 1 && F >= 1 && oH >= 1 && oW >= 1 && n_sets >= 1 && n_sets <= 65535 && max_span >= 0 && max_span <= kMaxTriSpan;
    if (sizes && (!tri_max_items(F, n_sets, oH, oW, max_span) || F > kTriBwdMaxFaces)) return LERF_EUNSUPPORTED;
    const size_t need = sizes ? tri_bwd_workspace_bytes(F, V, Va, n_sets) : 0;
    const int rc = check_call(n_sets,
                              {dense_operand(pos, pos_dtype, V, 1, pos_set, SHARE), dense_operand(attr, attr_dtype, Va, 1, attr_set, SHARE),
                               plane_operand(faces, sizeof(int32_t), F, 3, faces_set, SHARE),
                               plane_operand(attr_faces, sizeof(int32_t), F, 3, afaces_set, SHARE | OPTIONAL),
                               plane_operand(depth, sizeof(float), V, 1, depth_set, SHARE | OPTIONAL),
                               plane_operand(w, w_dtype == LERF_F64 ? sizeof(double) : sizeof(float), V, 1, w_set, SHARE | OPTIONAL),
                               plane_operand(keys, sizeof(uint64_t), oH, oW, keys_set), dense_operand(grad_out, LERF_F64, oH, oW, gout_set),
                               dense_operand(grad_attr, LERF_F64, Va, 1, gattr_set, OPTIONAL | WRITTEN),
                               dense_operand(grad_pos, LERF_F64, V, 1, gpos_set, OPTIONAL | WRITTEN),
                               plane_operand(grad_w, sizeof(double), V, 1, gw_set, OPTIONAL | WRITTEN), workspace_operand(workspace, (int64_t)need, 8)},
                              sizes && tile_ok(oH, oW, i0, j0) && (!w || float_dtype(w_dtype)) && orient >= -1 && orient <= 1 &&
                                  (grad_attr || grad_pos || grad_w) && !(grad_w && !w) && max_adders >= 1 && workspace_bytes >= need);
    if (rc != LERF_OK) return rc;
    LERF_COORDS_DT(pos_dtype, TP, {
        const TriMesh<TP> mesh{(const TP*)pos, V, Va, faces, attr_faces, F, depth, w, w_dtype == LERF_F64, orient, max_span, i0, j0, oH, oW,
                               pos_set, faces_set, afaces_set, depth_set, w_set};
        LERF_COORDS_DT(attr_dtype, TA,
            return run(mesh, (const TA*)attr, attr_set, keys, keys_set, grad_out, gout_set, n_sets, grad_attr, gattr_set, grad_pos, gpos_set, grad_w, gw_set,
                       workspace, max_adders));
    });
}

template <typename RUN>
int compose_bwd(RUN run, const void* a, int a_dtype, int64_t a_stride, int aH, int aW, const void* b, int b_dtype, int64_t b_stride,
                const double* grad_out, int oH, int oW, double* grad_a, double* grad_b, int n_sets, int64_t a_set, int64_t b_set, int64_t gout_set,
                int64_t ga_set, int64_t gb_set, const OrderedArgs* ord = nullptr) {
    const bool one_ga_many_a = n_sets > 1 && grad_a && ga_set == 0 && a_set != 0;      // one gradient buffer belongs to ONE shared outer map
    const bool two_writers = ord && n_sets > 1 && grad_a && ga_set == 0;               // ordered: a target has ONE owner, so one set
    const int64_t n_entries = (int64_t)oH * oW, n_targets = (int64_t)aH * aW;
    if (ord && aH >= 2 && aW >= 2 && oH >= 1 && oW >= 1 && !ordered_sizes_ok(n_entries, n_targets)) return LERF_EUNSUPPORTED;
    const Operand ws = ordered_ws_operand(ord, n_entries, n_targets, n_sets);
    const int rc = check_call(n_sets,
                              {map_operand(a, a_dtype, a_stride, aH, aW, a_set, SHARE), map_operand(b, b_dtype, b_stride, oH, oW, b_set),
                               dense_operand(grad_out, LERF_F64, oH, oW, gout_set), dense_operand(grad_a, LERF_F64, aH, aW, ga_set, SHARE | OPTIONAL | WRITTEN),
                               dense_operand(grad_b, LERF_F64, oH, oW, gb_set, OPTIONAL | WRITTEN), ws},
                              aH >= 2 && aW >= 2 && tile_ok(oH, oW, 0, 0) && (grad_a || grad_b) && !one_ga_many_a && !two_writers &&
                                  ordered_rules(ord, ws));
    if (rc != LERF_OK) return rc;
    LERF_COORDS_DT(a_dtype, TA, LERF_COORDS_DT(b_dtype, TB,
        return run(ComposeBwdOp<TA, TB>{{(const TA*)a, a_stride}, aH, aW, {(const TB*)b, b_stride}, {grad_out, 2 * (int64_t)oW}, grad_a, grad_b,
                                        a_set, b_set, gout_set, ga_set, gb_set},
                   oH, oW, n_sets)));
}

template <typename RUN>
int invert_bwd(RUN run, const void* f, int f_dtype, int64_t f_stride, int fH, int fW, const void* g, int g_dtype, int64_t g_stride,
               const double* grad_out, int oH, int oW, double* grad_f, int n_sets, int64_t f_set, int64_t g_set, int64_t gout_set, int64_t gf_set,
               const OrderedArgs* ord = nullptr) {
    const int64_t n_entries = (int64_t)oH * oW, n_targets = (int64_t)fH * fW;
    if (ord && fH >= 2 && fW >= 2 && oH >= 1 && oW >= 1 && !ordered_sizes_ok(n_entries, n_targets)) return LERF_EUNSUPPORTED;
    const Operand ws = ordered_ws_operand(ord, n_entries, n_targets, n_sets);
    // grad_f is never shared between sets (no SHARE: a set stride of 0 in a batch is refused), so a target has one owner
    const int rc = check_call(n_sets,
                              {map_operand(f, f_dtype, f_stride, fH, fW, f_set, SHARE), map_operand(g, g_dtype, g_stride, oH, oW, g_set),
                               dense_operand(grad_out, LERF_F64, oH, oW, gout_set), dense_operand(grad_f, LERF_F64, fH, fW, gf_set, WRITTEN), ws},
                              fH >= 2 && fW >= 2 && tile_ok(oH, oW, 0, 0) && ordered_rules(ord, ws));
    if (rc != LERF_OK) return rc;
    LERF_COORDS_DT(f_dtype, TF, LERF_COORDS_DT(g_dtype, TG,
        return run(InvertBwdOp<TF, TG>{{(const TF*)f, f_stride}, fH, fW, {(const TG*)g, g_stride}, {grad_out, 2 * (int64_t)oW}, grad_f, f_set, g_set,
                                       gout_set, gf_set},
                   oH, oW, n_sets)));
}

// run F with KIND = the compile-time constant of a depth kind the argument checks have accepted
#define LERF_COORDS_KIND(code, KIND, ...)                                          \
    do {                                                                           \
        if ((code) == LERF_DEPTH_Z) { constexpr int KIND = LERF_DEPTH_Z; __VA_ARGS__; } \
        else { constexpr int KIND = LERF_DEPTH_INVERSE; __VA_ARGS__; }             \
    } while (0)

inline bool depth_kind(int kind) { return kind == LERF_DEPTH_Z || kind == LERF_DEPTH_INVERSE; }
inline size_t depth_bytes(int dt) { return dt == LERF_F32 ? sizeof(float) : sizeof(double); }

template <typename RUN>
int reproject(RUN run, int kind, const double* params, int n_sets, const void* depth, int depth_dtype, int64_t depth_set, void* out, int out_dtype,
              int64_t out_set, int64_t stride, float* depth_out, int64_t zo_set, int oH, int oW, int i0, int j0) {
    const int rc = check_call(n_sets,
                              {params_operand(params, kReprojectParams), plane_operand(depth, depth_bytes(depth_dtype), oH, oW, depth_set, SHARE),
                               map_operand(out, out_dtype, stride, oH, oW, out_set, WRITTEN),
                               plane_operand(depth_out, sizeof(float), oH, oW, zo_set, OPTIONAL | WRITTEN)},
                              depth_kind(kind) && float_dtype(depth_dtype) && tile_ok(oH, oW, i0, j0), LERF_EINVAL);
    if (rc != LERF_OK) return rc;
    LERF_COORDS_KIND(kind, KIND, LERF_COORDS_DT(depth_dtype, TD, LERF_COORDS_DT(out_dtype, TO,
        return run(ReprojectOp<KIND, TD, TO>{params, (const TD*)depth, (TO*)out, depth_out, depth_set, out_set, stride, zo_set, oW, i0, j0},
                   oH, oW, n_sets))));
}

// `planes` dense planes [h][w] of scalars of `el` bytes, one behind the other (an NCHW image, the accumulator, their gradients)
inline Operand planes_operand(const void* p, size_t el, int planes, int h, int w, int64_t set_stride, unsigned flags = 0) {
    return {p, el, el, (int64_t)planes * h * w, set_stride, false, (flags & SHARE) != 0, (flags & OPTIONAL) != 0, (flags & WRITTEN) != 0, true, true};
}

inline bool splat_dims(int dtype, int C, int H, int W, int oH, int oW) {
    return float_dtype(dtype) && C >= 1 && C < 0x7fffffff && H >= 1 && W >= 1 && tile_ok(H, W, 0, 0) && oH >= 1 && oW >= 1;      // the grid is the SOURCE's
}

// the forward warp: x [n_sets][C][H][W], f the map of the SOURCE frame [H][W], m [n_sets][H][W] or null, acc [n_sets][C + norm][oH][oW]
template <typename RUN>
int splat(RUN run, const void* x, int dtype, int C, int H, int W, int64_t x_set, const void* f, int f_dtype, int64_t f_stride, int64_t f_set,
          const void* m, int64_t m_set, void* acc, int with_norm, int oH, int oW, int64_t acc_set, int n_sets, const OrderedArgs* ord = nullptr) {
    const size_t el = depth_bytes(dtype);
    const int64_t n_entries = (int64_t)H * W, n_targets = (int64_t)oH * oW;
    if (ord && H >= 1 && W >= 1 && oH >= 1 && oW >= 1 && !ordered_sizes_ok(n_entries, n_targets)) return LERF_EUNSUPPORTED;
    const Operand ws = ordered_ws_operand(ord, n_entries, n_targets, n_sets);
    // acc is never shared between sets (no SHARE: a set stride of 0 in a batch is refused), so a target has one owner
    const int rc = check_call(n_sets,
                              {planes_operand(x, el, C, H, W, x_set), map_operand(f, f_dtype, f_stride, H, W, f_set, SHARE),
                               planes_operand(m, el, 1, H, W, m_set, OPTIONAL), planes_operand(acc, el, C + (with_norm ? 1 : 0), oH, oW, acc_set, WRITTEN), ws},
                              splat_dims(dtype, C, H, W, oH, oW) && (with_norm == 0 || with_norm == 1) && ordered_rules(ord, ws), LERF_EINVAL);
    if (rc != LERF_OK) return rc;
    LERF_COORDS_DT(dtype, T, LERF_COORDS_DT(f_dtype, TF,
        return run(SplatOp<T, TF>{(const T*)x, {(const TF*)f, f_stride}, (const T*)m, (T*)acc, C, W, oH, oW, with_norm != 0, x_set, f_set, m_set,
                                  acc_set, (int64_t)H * W, (int64_t)oH * oW},
                   H, W, n_sets)));
}

// its adjoint: g [n_sets][C + norm][oH][oW]; grad_x like x, grad_m like m (dtype T), grad_f float64 [n_sets][H][W][2]; each may be null
template <typename RUN>
int splat_bwd(RUN run, const void* x, int dtype, int C, int H, int W, int64_t x_set, const void* f, int f_dtype, int64_t f_stride,
              int64_t f_set, const void* m, int64_t m_set, const void* g, int with_norm, int oH, int oW, int64_t g_set, void* grad_x,
              int64_t gx_set, void* grad_m, int64_t gm_set, double* grad_f, int64_t gf_set, int n_sets) {
    const size_t el = depth_bytes(dtype);
    const int rc = check_call(n_sets,
                              {planes_operand(x, el, C, H, W, x_set), map_operand(f, f_dtype, f_stride, H, W, f_set, SHARE),
                               planes_operand(m, el, 1, H, W, m_set, OPTIONAL), planes_operand(g, el, C + (with_norm ? 1 : 0), oH, oW, g_set),
                               planes_operand(grad_x, el, C, H, W, gx_set, OPTIONAL | WRITTEN), planes_operand(grad_m, el, 1, H, W, gm_set, OPTIONAL | WRITTEN),
                               dense_operand(grad_f, LERF_F64, H, W, gf_set, OPTIONAL | WRITTEN)},
                              splat_dims(dtype, C, H, W, oH, oW) && (with_norm == 0 || with_norm == 1) && (grad_x || grad_m || grad_f), LERF_EINVAL);
    if (rc != LERF_OK) return rc;
    LERF_COORDS_DT(dtype, T, LERF_COORDS_DT(f_dtype, TF,
        return run(SplatBwdOp<T, TF>{(const T*)x, {(const TF*)f, f_stride}, (const T*)m, (const T*)g, (T*)grad_x, (T*)grad_m, grad_f, C, W, oH, oW,
                                     with_norm != 0, x_set, f_set, m_set, g_set, gx_set, gm_set, gf_set, (int64_t)H * W, (int64_t)oH * oW},
                   H, W, n_sets)));
}

// The fixed-order sum of the build backward and of the reproject backward on the host, lane by lane: the device's bands, trees and two
// passes (the top of lerf_coords_models.h).  entry(s, i, j, dp) fills dp[n_params] of one entry; grad_params == nullptr: every entry is
// visited once and nothing is summed.
template <typename ENTRY>
void two_pass_sums_host(int n_sets, int n_params, int oH, int oW, double* grad_params, ENTRY entry) {
#pragma clang fp contract(off)
    const int nbx = (oW + kBwdCols - 1) / kBwdCols, nby = (oH + kBwdBand - 1) / kBwdBand, nblk = nbx * nby;
    std::vector<double> part((size_t)n_params * nblk);
    std::vector<double> lanes((size_t)kMaxParams * 64);
    for (int s = 0; s < n_sets; ++s) {
        for (int by = 0; by < nby; ++by)
            for (int bx = 0; bx < nbx; ++bx) {
                double wsum[kBwdWaves][kMaxParams];
                for (int w = 0; w < kBwdWaves; ++w) {
                    for (int l = 0; l < 64; ++l) {
                        const int j = bx * kBwdCols + l;
                        double acc[kMaxParams];
                        for (int k = 0; k < n_params; ++k) acc[k] = 0.0;
                        if (j < oW)
                            for (int i = by * kBwdBand + w; i < oH && i < (by + 1) * kBwdBand; i += kBwdWaves) {
                                double dp[kMaxParams];
                                entry(s, i, j, dp);
                                for (int k = 0; k < n_params; ++k) acc[k] = acc[k] + dp[k];
                            }
                        for (int k = 0; k < n_params; ++k) lanes[(size_t)k * 64 + l] = acc[k];
                    }
                    for (int k = 0; k < n_params; ++k) wsum[w][k] = tree64(&lanes[(size_t)k * 64]);
                }
                for (int k = 0; k < n_params; ++k)
                    part[(size_t)k * nblk + by * nbx + bx] = ((wsum[0][k] + wsum[1][k]) + wsum[2][k]) + wsum[3][k];
            }
        if (!grad_params) continue;
        for (int k = 0; k < n_params; ++k) {
            double v[64];
            for (int l = 0; l < 64; ++l) {
                double acc = 0.0;
                for (int b = l; b < nblk; b += 64) acc = acc + part[(size_t)k * nblk + b];
                v[l] = acc;
            }
            double* dst = grad_params + (size_t)s * n_params + k;
            *dst = *dst + tree64(v);
        }
    }
}

// The runners of the two-pass adjoints: TwoPassOnDevice{stream, partials} launches pass 1 and, with grad_params, pass 2 (kPartials: the
// operation's table judges the caller's partials); TwoPassOnHost{} is two_pass_sums_host over the same per-entry statement.
struct TwoPassOnDevice {
    static constexpr bool kPartials = true;
    hipStream_t stream;
    double* partials;
    static dim3 grid(int n_sets, int oH, int oW) { return dim3((oW + kBwdCols - 1) / kBwdCols, (oH + kBwdBand - 1) / kBwdBand, n_sets); }
    int pass2(int n_params, int n_sets, const dim3& g1, double* grad_params) const {
        if (grad_params) hipLaunchKernelGGL(coords_build_bwd_sum_kernel, dim3(n_params, n_sets), dim3(64), 0, stream, partials, (int)(g1.x * g1.y), grad_params);
        return launch_status();
    }
    template <int MODEL>
    int build(const double* params, int n_sets, const double* grad_map, int oH, int oW, int i0, int j0, double* grad_params) const {
        clear_stale_error();
        const dim3 g1 = grid(n_sets, oH, oW);
        hipLaunchKernelGGL((coords_build_bwd_partial_kernel<MODEL>), g1, dim3(CB_COLS, CB_ROWS), 0, stream, params, reinterpret_cast<const double2*>(grad_map),
                           oH, oW, i0, j0, partials);
        return pass2(model_params(MODEL), n_sets, g1, grad_params);
    }
    template <int KIND, typename TD>
    int reproject(const double* params, int n_sets, const TD* depth, int64_t depth_set, const double* grad_map, const double* grad_zo, int oH, int oW,
                  int i0, int j0, double* grad_depth, double* grad_params) const {
        clear_stale_error();
        const dim3 g1 = grid(n_sets, oH, oW), b1(CB_COLS, CB_ROWS);
        const double2* gm = reinterpret_cast<const double2*>(grad_map);
        if (grad_params)
            hipLaunchKernelGGL((coords_reproject_bwd_kernel<KIND, TD, true>), g1, b1, 0, stream, params, depth, depth_set, gm, grad_zo, oH, oW, i0, j0,
                               grad_depth, partials);
        else
            hipLaunchKernelGGL((coords_reproject_bwd_kernel<KIND, TD, false>), g1, b1, 0, stream, params, depth, depth_set, gm, grad_zo, oH, oW, i0, j0,
                               grad_depth, (double*)nullptr);
        return pass2(kReprojectParams, n_sets, g1, grad_params);
    }
};

struct TwoPassOnHost {
    static constexpr bool kPartials = false;
    template <int MODEL>
    int build(const double* params, int n_sets, const double* grad_map, int oH, int oW, int i0, int j0, double* grad_params) const {
#pragma clang fp contract(off)
        constexpr int NP = model_params(MODEL);
        two_pass_sums_host(n_sets, NP, oH, oW, grad_params, [&](int s, int i, int j, double* dp) {
            model_point_bwd<MODEL>(params + (size_t)s * NP, i0 + i, j0 + j, load_entry(grad_map + 2 * (size_t)s * oH * oW, 2 * (int64_t)oW, i, j), dp);
        });
        return LERF_OK;
    }
    template <int KIND, typename TD>
    int reproject(const double* params, int n_sets, const TD* depth, int64_t depth_set, const double* grad_map, const double* grad_zo, int oH, int oW,
                  int i0, int j0, double* grad_depth, double* grad_params) const {
#pragma clang fp contract(off)
        two_pass_sums_host(n_sets, kReprojectParams, oH, oW, grad_params, [&](int s, int i, int j, double* dp) {
            const int64_t e = (int64_t)i * oW + j, pe = (int64_t)s * oH * oW + e;
            const double dd = reproject_point_bwd<KIND>(params + (size_t)s * kReprojectParams, (double)depth[set_offset(s, depth_set) + e], i0 + i, j0 + j,
                                                        load_entry(grad_map + 2 * (size_t)s * oH * oW, 2 * (int64_t)oW, i, j), grad_zo ? grad_zo[pe] : 0.0, dp);
            if (grad_depth) grad_depth[pe] = grad_depth[pe] + dd;
        });
        return LERF_OK;
    }
};

// the partials as an operand: one vector per block and set where the runner keeps them (the device) and they are `wanted`
inline Operand partials_operand(const void* ws, int n_params, int oH, int oW, bool wanted) {
    return bytes_operand(wanted ? ws : nullptr, (int64_t)lerf_coords_build_bwd_workspace_bytes(n_params, 1, oH, oW), 16, wanted ? WRITTEN : OPTIONAL);
}

// the adjoint of the builders and of reproject: the table, the dispatch, the runner
template <typename RUN>
int build_bwd(RUN run, int model, const double* params, int n_sets, int n_params, const double* grad_map, int oH, int oW, int i0, int j0,
              double* grad_params, void* workspace, size_t workspace_bytes) {
    const int rc = check_call(n_sets,
                              {params_operand(params, n_params), dense_operand(grad_map, LERF_F64, oH, oW, 2 * (int64_t)oH * oW),
                               params_operand(grad_params, n_params, WRITTEN), partials_operand(workspace, n_params, oH, oW, RUN::kPartials)},
                              (!RUN::kPartials || workspace_bytes >= lerf_coords_build_bwd_workspace_bytes(n_params, n_sets, oH, oW)) && tile_ok(oH, oW, i0, j0) &&
                                  model_params(model) >= 0 && n_params == model_params(model),
                              LERF_EINVAL);
    if (rc != LERF_OK) return rc;
    LERF_COORDS_MODEL(model, MODEL, return run.template build<MODEL>(params, n_sets, grad_map, oH, oW, i0, j0, grad_params));
}

template <typename RUN>
int reproject_bwd(RUN run, int kind, const double* params, int n_sets, const void* depth, int depth_dtype, int64_t depth_set, const double* grad_map,
                  const double* grad_zo, int oH, int oW, int i0, int j0, double* grad_depth, double* grad_params, void* workspace, size_t workspace_bytes) {
    const int64_t plane = (int64_t)oH * oW;
    const bool partials = RUN::kPartials && grad_params;
    const int rc = check_call(n_sets,
                              {params_operand(params, kReprojectParams), plane_operand(depth, depth_bytes(depth_dtype), oH, oW, depth_set, SHARE),
                               dense_operand(grad_map, LERF_F64, oH, oW, 2 * plane), plane_operand(grad_zo, sizeof(double), oH, oW, plane, OPTIONAL),
                               plane_operand(grad_depth, sizeof(double), oH, oW, plane, OPTIONAL | WRITTEN),
                               params_operand(grad_params, kReprojectParams, OPTIONAL | WRITTEN),
                               partials_operand(workspace, kReprojectParams, oH, oW, partials)},
                              depth_kind(kind) && float_dtype(depth_dtype) && tile_ok(oH, oW, i0, j0) && (grad_depth || grad_params) &&
                                  (!partials || workspace_bytes >= lerf_coords_reproject_bwd_workspace_bytes(n_sets, oH, oW)),
                              LERF_EINVAL);
    if (rc != LERF_OK) return rc;
    LERF_COORDS_KIND(kind, KIND, LERF_COORDS_DT(depth_dtype, TD,
        return run.template reproject<KIND, TD>(params, n_sets, (const TD*)depth, depth_set, grad_map, grad_zo, oH, oW, i0, j0, grad_depth, grad_params)));
}

}  // namespace coords
}  // namespace lerf

using namespace lerf;
using namespace lerf::coords;

extern "C" {

int lerf_coords_build(int model, const double* params, int n_params, void* out, int out_dtype, int64_t row_stride, int oH, int oW,
                      int i0, int j0, void* stream) {
    return build(OnDevice{(hipStream_t)stream}, model, params, n_params, out, out_dtype, row_stride, oH, oW, i0, j0);
}

int lerf_coords_build_host(int model, const double* params, int n_params, void* out, int out_dtype, int64_t row_stride, int oH, int oW,
                           int i0, int j0) {
    return build(OnHost{}, model, params, n_params, out, out_dtype, row_stride, oH, oW, i0, j0);
}

int lerf_coords_build_dev(int model, const double* params_dev, int n_sets, int n_params, void* out, int out_dtype, int64_t set_stride,
                          int64_t row_stride, int oH, int oW, int i0, int j0, void* stream) {
    return build_dev(OnDevice{(hipStream_t)stream}, model, params_dev, n_sets, n_params, out, out_dtype, set_stride, row_stride, oH, oW, i0, j0);
}

// the batched forms: the one way into each template (the single-map entry points below call these with n_sets = 1, set strides 0)
int lerf_coords_mesh_batched(const void* ctrl, int ctrl_dtype, int gh, int gw, int interp, int full_h, int full_w, void* out, int out_dtype,
                             int64_t row_stride, int oH, int oW, int i0, int j0, int n_sets, int64_t ctrl_set_stride, int64_t out_set_stride,
                             void* stream) {
    return mesh(OnDevice{(hipStream_t)stream}, ctrl, ctrl_dtype, gh, gw, interp, full_h, full_w, out, out_dtype, row_stride, oH, oW, i0, j0, n_sets,
                ctrl_set_stride, out_set_stride);
}

int lerf_coords_mesh_batched_host(const void* ctrl, int ctrl_dtype, int gh, int gw, int interp, int full_h, int full_w, void* out, int out_dtype,
                                  int64_t row_stride, int oH, int oW, int i0, int j0, int n_sets, int64_t ctrl_set_stride,
                                  int64_t out_set_stride) {
    return mesh(OnHost{}, ctrl, ctrl_dtype, gh, gw, interp, full_h, full_w, out, out_dtype, row_stride, oH, oW, i0, j0, n_sets, ctrl_set_stride,
                out_set_stride);
}

int lerf_coords_compose_batched(const void* a, int a_dtype, int64_t a_row_stride, int aH, int aW, const void* b, int b_dtype,
                                int64_t b_row_stride, void* out, int out_dtype, int64_t out_row_stride, int oH, int oW, int n_sets,
                                int64_t a_set_stride, int64_t b_set_stride, int64_t out_set_stride, void* stream) {
    return compose(OnDevice{(hipStream_t)stream}, a, a_dtype, a_row_stride, aH, aW, b, b_dtype, b_row_stride, out, out_dtype, out_row_stride, oH, oW,
                   n_sets, a_set_stride, b_set_stride, out_set_stride);
}

int lerf_coords_compose_batched_host(const void* a, int a_dtype, int64_t a_row_stride, int aH, int aW, const void* b, int b_dtype,
                                     int64_t b_row_stride, void* out, int out_dtype, int64_t out_row_stride, int oH, int oW, int n_sets,
                                     int64_t a_set_stride, int64_t b_set_stride, int64_t out_set_stride) {
    return compose(OnHost{}, a, a_dtype, a_row_stride, aH, aW, b, b_dtype, b_row_stride, out, out_dtype, out_row_stride, oH, oW, n_sets,
                   a_set_stride, b_set_stride, out_set_stride);
}

int lerf_coords_invert_batched(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW, const void* init, int init_dtype,
                               int64_t init_row_stride, void* out, int out_dtype, int64_t out_row_stride, int oH, int oW, int i0, int j0,
                               int max_iter, double tol, int n_sets, int64_t f_set_stride, int64_t init_set_stride, int64_t out_set_stride,
                               void* stream) {
    return invert(OnDevice{(hipStream_t)stream}, f, f_dtype, f_row_stride, fH, fW, init, init_dtype, init_row_stride, out, out_dtype,
                  out_row_stride, oH, oW, i0, j0, max_iter, tol, n_sets, f_set_stride, init_set_stride, out_set_stride);
}

int lerf_coords_invert_batched_host(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW, const void* init, int init_dtype,
                                    int64_t init_row_stride, void* out, int out_dtype, int64_t out_row_stride, int oH, int oW, int i0, int j0,
                                    int max_iter, double tol, int n_sets, int64_t f_set_stride, int64_t init_set_stride,
                                    int64_t out_set_stride) {
    return invert(OnHost{}, f, f_dtype, f_row_stride, fH, fW, init, init_dtype, init_row_stride, out, out_dtype, out_row_stride, oH, oW, i0, j0,
                  max_iter, tol, n_sets, f_set_stride, init_set_stride, out_set_stride);
}

int lerf_coords_invert_raster_batched(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW, const float* depth, void* out,
                                      int out_dtype, int64_t out_row_stride, int oH, int oW, int i0, int j0, int max_span, int orient,
                                      uint64_t* keys, int n_sets, int64_t f_set_stride, int64_t depth_set_stride, int64_t out_set_stride,
                                      int64_t keys_set_stride, void* stream) {
    return invert_raster(OnDevice{(hipStream_t)stream}, ScatterOnDevice{(hipStream_t)stream}, f, f_dtype, f_row_stride, fH, fW, depth, out,
                         out_dtype, out_row_stride, oH, oW, i0, j0, max_span, orient, keys, n_sets, f_set_stride, depth_set_stride,
                         out_set_stride, keys_set_stride);
}

int lerf_coords_invert_raster_batched_host(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW, const float* depth, void* out,
                                           int out_dtype, int64_t out_row_stride, int oH, int oW, int i0, int j0, int max_span, int orient,
                                           uint64_t* keys, int n_sets, int64_t f_set_stride, int64_t depth_set_stride, int64_t out_set_stride,
                                           int64_t keys_set_stride) {
    return invert_raster(OnHost{}, ScatterOnHost{}, f, f_dtype, f_row_stride, fH, fW, depth, out, out_dtype, out_row_stride, oH, oW, i0, j0,
                         max_span, orient, keys, n_sets, f_set_stride, depth_set_stride, out_set_stride, keys_set_stride);
}

size_t lerf_coords_trimesh_workspace_bytes(int64_t F, int n_sets) { return sizeof(uint32_t) * (size_t)tri_workspace_words(F, n_sets); }

int lerf_coords_trimesh_batched(const void* pos, int pos_dtype, int V, const void* attr, int attr_dtype, int Va, const int32_t* faces,
                                const int32_t* attr_faces, int F, const float* depth, const void* w, int w_dtype, void* out, int out_dtype,
                                int64_t out_row_stride, int oH, int oW, int i0, int j0, int max_span, int orient, uint64_t* keys, float* depth_out,
                                void* workspace, size_t workspace_bytes, int n_sets, int64_t pos_set_stride, int64_t attr_set_stride,
                                int64_t faces_set_stride, int64_t attr_faces_set_stride, int64_t depth_set_stride, int64_t w_set_stride,
                                int64_t out_set_stride, int64_t keys_set_stride, int64_t depth_out_set_stride, void* stream) {
    return trimesh(OnDevice{(hipStream_t)stream}, TriRasterOnDevice{(hipStream_t)stream}, pos, pos_dtype, V, attr, attr_dtype, Va, faces, attr_faces, F,
                   depth, w, w_dtype, out, out_dtype, out_row_stride, oH, oW, i0, j0, max_span, orient, keys, depth_out, workspace, workspace_bytes, n_sets,
                   pos_set_stride, attr_set_stride, faces_set_stride, attr_faces_set_stride, depth_set_stride, w_set_stride, out_set_stride,
                   keys_set_stride, depth_out_set_stride);
}

int lerf_coords_trimesh_batched_host(const void* pos, int pos_dtype, int V, const void* attr, int attr_dtype, int Va, const int32_t* faces,
                                     const int32_t* attr_faces, int F, const float* depth, const void* w, int w_dtype, void* out, int out_dtype,
                                     int64_t out_row_stride, int oH, int oW, int i0, int j0, int max_span, int orient, uint64_t* keys,
                                     float* depth_out, void* workspace, size_t workspace_bytes, int n_sets, int64_t pos_set_stride,
                                     int64_t attr_set_stride, int64_t faces_set_stride, int64_t attr_faces_set_stride, int64_t depth_set_stride,
                                     int64_t w_set_stride, int64_t out_set_stride, int64_t keys_set_stride, int64_t depth_out_set_stride) {
    return trimesh(OnHost{}, TriRasterOnHost{}, pos, pos_dtype, V, attr, attr_dtype, Va, faces, attr_faces, F, depth, w, w_dtype, out, out_dtype,
                   out_row_stride, oH, oW, i0, j0, max_span, orient, keys, depth_out, workspace, workspace_bytes, n_sets, pos_set_stride,
                   attr_set_stride, faces_set_stride, attr_faces_set_stride, depth_set_stride, w_set_stride, out_set_stride, keys_set_stride,
                   depth_out_set_stride);
}

int lerf_coords_trimesh(const void* pos, int pos_dtype, int V, const void* attr, int attr_dtype, int Va, const int32_t* faces,
                        const int32_t* attr_faces, int F, const float* depth, const void* w, int w_dtype, void* out, int out_dtype, int64_t out_row_stride,
                        int oH, int oW, int i0, int j0, int max_span, int orient, uint64_t* keys, float* depth_out, void* workspace,
                        size_t workspace_bytes, void* stream) {
    return lerf_coords_trimesh_batched(pos, pos_dtype, V, attr, attr_dtype, Va, faces, attr_faces, F, depth, w, w_dtype, out, out_dtype, out_row_stride, oH,
                                       oW, i0, j0, max_span, orient, keys, depth_out, workspace, workspace_bytes, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, stream);
}

int lerf_coords_trimesh_host(const void* pos, int pos_dtype, int V, const void* attr, int attr_dtype, int Va, const int32_t* faces,
                             const int32_t* attr_faces, int F, const float* depth, const void* w, int w_dtype, void* out, int out_dtype, int64_t out_row_stride,
                             int oH, int oW, int i0, int j0, int max_span, int orient, uint64_t* keys, float* depth_out, void* workspace,
                             size_t workspace_bytes) {
    return lerf_coords_trimesh_batched_host(pos, pos_dtype, V, attr, attr_dtype, Va, faces, attr_faces, F, depth, w, w_dtype, out, out_dtype, out_row_stride,
                                            oH, oW, i0, j0, max_span, orient, keys, depth_out, workspace, workspace_bytes, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0);
}

size_t lerf_coords_trimesh_bwd_workspace_bytes(int64_t F, int64_t V, int64_t Va, int n_sets) { return tri_bwd_workspace_bytes(F, V, Va, n_sets); }

int lerf_coords_trimesh_bwd_batched(const void* pos, int pos_dtype, int V, const void* attr, int attr_dtype, int Va, const int32_t* faces,
                                    const int32_t* attr_faces, int F, const float* depth, const void* w, int w_dtype, int oH, int oW, int i0, int j0,
                                    int max_span, int orient, const uint64_t* keys, const double* grad_out, double* grad_attr, double* grad_pos,
                                    double* grad_w, void* workspace, size_t workspace_bytes, int max_adders, int n_sets, int64_t pos_set_stride,
                                    int64_t attr_set_stride, int64_t faces_set_stride, int64_t attr_faces_set_stride, int64_t depth_set_stride,
                                    int64_t w_set_stride, int64_t keys_set_stride, int64_t grad_out_set_stride, int64_t grad_attr_set_stride,
                                    int64_t grad_pos_set_stride, int64_t grad_w_set_stride, void* stream) {
    return trimesh_bwd(TriBwdOnDevice{(hipStream_t)stream}, pos, pos_dtype, V, attr, attr_dtype, Va, faces, attr_faces, F, depth, w, w_dtype, oH, oW, i0, j0,
                       max_span, orient, keys, grad_out, grad_attr, grad_pos, grad_w, workspace, workspace_bytes, max_adders, n_sets, pos_set_stride,
                       attr_set_stride, faces_set_stride, attr_faces_set_stride, depth_set_stride, w_set_stride, keys_set_stride, grad_out_set_stride,
                       grad_attr_set_stride, grad_pos_set_stride, grad_w_set_stride);
}

int lerf_coords_trimesh_bwd_batched_host(const void* pos, int pos_dtype, int V, const void* attr, int attr_dtype, int Va, const int32_t* faces,
                                         const int32_t* attr_faces, int F, const float* depth, const void* w, int w_dtype, int oH, int oW, int i0, int j0,
                                         int max_span, int orient, const uint64_t* keys, const double* grad_out, double* grad_attr, double* grad_pos,
                                         double* grad_w, void* workspace, size_t workspace_bytes, int max_adders, int n_sets, int64_t pos_set_stride,
                                         int64_t attr_set_stride, int64_t faces_set_stride, int64_t attr_faces_set_stride, int64_t depth_set_stride,
                                         int64_t w_set_stride, int64_t keys_set_stride, int64_t grad_out_set_stride, int64_t grad_attr_set_stride,
                                         int64_t grad_pos_set_stride, int64_t grad_w_set_stride) {
    return trimesh_bwd(TriBwdOnHost{}, pos, pos_dtype, V, attr, attr_dtype, Va, faces, attr_faces, F, depth, w, w_dtype, oH, oW, i0, j0, max_span, orient,
                       keys, grad_out, grad_attr, grad_pos, grad_w, workspace, workspace_bytes, max_adders, n_sets, pos_set_stride, attr_set_stride,
                       faces_set_stride, attr_faces_set_stride, depth_set_stride, w_set_stride, keys_set_stride, grad_out_set_stride, grad_attr_set_stride,
                       grad_pos_set_stride, grad_w_set_stride);
}

int lerf_coords_trimesh_bwd(const void* pos, int pos_dtype, int V, const void* attr, int attr_dtype, int Va, const int32_t* faces,
                            const int32_t* attr_faces, int F, const float* depth, const void* w, int w_dtype, int oH, int oW, int i0, int j0, int max_span,
                            int orient, const uint64_t* keys, const double* grad_out, double* grad_attr, double* grad_pos, double* grad_w, void* workspace,
                            size_t workspace_bytes, int max_adders, void* stream) {
    return lerf_coords_trimesh_bwd_batched(pos, pos_dtype, V, attr, attr_dtype, Va, faces, attr_faces, F, depth, w, w_dtype, oH, oW, i0, j0, max_span, orient,
                                           keys, grad_out, grad_attr, grad_pos, grad_w, workspace, workspace_bytes, max_adders, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                           0, stream);
}

int lerf_coords_trimesh_bwd_host(const void* pos, int pos_dtype, int V, const void* attr, int attr_dtype, int Va, const int32_t* faces,
                                 const int32_t* attr_faces, int F, const float* depth, const void* w, int w_dtype, int oH, int oW, int i0, int j0,
                                 int max_span, int orient, const uint64_t* keys, const double* grad_out, double* grad_attr, double* grad_pos, double* grad_w,
                                 void* workspace, size_t workspace_bytes, int max_adders) {
    return lerf_coords_trimesh_bwd_batched_host(pos, pos_dtype, V, attr, attr_dtype, Va, faces, attr_faces, F, depth, w, w_dtype, oH, oW, i0, j0, max_span,
                                                orient, keys, grad_out, grad_attr, grad_pos, grad_w, workspace, workspace_bytes, max_adders, 1, 0, 0, 0, 0, 0,
                                                0, 0, 0, 0, 0, 0);
}

int lerf_coords_compose_bwd_batched(const void* a, int a_dtype, int64_t a_row_stride, int aH, int aW, const void* b, int b_dtype,
                                    int64_t b_row_stride, const double* grad_out, int oH, int oW, double* grad_a, double* grad_b, int n_sets,
                                    int64_t a_set_stride, int64_t b_set_stride, int64_t grad_out_set_stride, int64_t grad_a_set_stride,
                                    int64_t grad_b_set_stride, void* stream) {
    return compose_bwd(OnDevice{(hipStream_t)stream}, a, a_dtype, a_row_stride, aH, aW, b, b_dtype, b_row_stride, grad_out, oH, oW, grad_a, grad_b,
                       n_sets, a_set_stride, b_set_stride, grad_out_set_stride, grad_a_set_stride, grad_b_set_stride);
}

int lerf_coords_compose_bwd_batched_host(const void* a, int a_dtype, int64_t a_row_stride, int aH, int aW, const void* b, int b_dtype,
                                         int64_t b_row_stride, const double* grad_out, int oH, int oW, double* grad_a, double* grad_b,
                                         int n_sets, int64_t a_set_stride, int64_t b_set_stride, int64_t grad_out_set_stride,
                                         int64_t grad_a_set_stride, int64_t grad_b_set_stride) {
    return compose_bwd(OnHost{}, a, a_dtype, a_row_stride, aH, aW, b, b_dtype, b_row_stride, grad_out, oH, oW, grad_a, grad_b, n_sets,
                       a_set_stride, b_set_stride, grad_out_set_stride, grad_a_set_stride, grad_b_set_stride);
}

int lerf_coords_invert_bwd_batched(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW, const void* g, int g_dtype,
                                   int64_t g_row_stride, const double* grad_out, int oH, int oW, double* grad_f, int n_sets,
                                   int64_t f_set_stride, int64_t g_set_stride, int64_t grad_out_set_stride, int64_t grad_f_set_stride,
                                   void* stream) {
    return invert_bwd(OnDevice{(hipStream_t)stream}, f, f_dtype, f_row_stride, fH, fW, g, g_dtype, g_row_stride, grad_out, oH, oW, grad_f, n_sets,
                      f_set_stride, g_set_stride, grad_out_set_stride, grad_f_set_stride);
}

int lerf_coords_invert_bwd_batched_host(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW, const void* g, int g_dtype,
                                        int64_t g_row_stride, const double* grad_out, int oH, int oW, double* grad_f, int n_sets,
                                        int64_t f_set_stride, int64_t g_set_stride, int64_t grad_out_set_stride, int64_t grad_f_set_stride) {
    return invert_bwd(OnHost{}, f, f_dtype, f_row_stride, fH, fW, g, g_dtype, g_row_stride, grad_out, oH, oW, grad_f, n_sets, f_set_stride,
                      g_set_stride, grad_out_set_stride, grad_f_set_stride);
}

// the single-map entry points: the batched one with one set
int lerf_coords_mesh(const void* ctrl, int ctrl_dtype, int gh, int gw, int interp, int full_h, int full_w, void* out, int out_dtype,
                     int64_t row_stride, int oH, int oW, int i0, int j0, void* stream) {
    return lerf_coords_mesh_batched(ctrl, ctrl_dtype, gh, gw, interp, full_h, full_w, out, out_dtype, row_stride, oH, oW, i0, j0, 1, 0, 0, stream);
}

int lerf_coords_mesh_host(const void* ctrl, int ctrl_dtype, int gh, int gw, int interp, int full_h, int full_w, void* out, int out_dtype,
                          int64_t row_stride, int oH, int oW, int i0, int j0) {
    return lerf_coords_mesh_batched_host(ctrl, ctrl_dtype, gh, gw, interp, full_h, full_w, out, out_dtype, row_stride, oH, oW, i0, j0, 1, 0, 0);
}

int lerf_coords_compose(const void* a, int a_dtype, int64_t a_row_stride, int aH, int aW, const void* b, int b_dtype, int64_t b_row_stride,
                        void* out, int out_dtype, int64_t out_row_stride, int oH, int oW, void* stream) {
    return lerf_coords_compose_batched(a, a_dtype, a_row_stride, aH, aW, b, b_dtype, b_row_stride, out, out_dtype, out_row_stride, oH, oW, 1, 0, 0, 0, stream);
}

int lerf_coords_compose_host(const void* a, int a_dtype, int64_t a_row_stride, int aH, int aW, const void* b, int b_dtype,
                             int64_t b_row_stride, void* out, int out_dtype, int64_t out_row_stride, int oH, int oW) {
    return lerf_coords_compose_batched_host(a, a_dtype, a_row_stride, aH, aW, b, b_dtype, b_row_stride, out, out_dtype, out_row_stride, oH, oW, 1, 0, 0, 0);
}

int lerf_coords_invert(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW, const void* init, int init_dtype,
                       int64_t init_row_stride, void* out, int out_dtype, int64_t out_row_stride, int oH, int oW, int i0, int j0, int max_iter,
                       double tol, void* stream) {
    return lerf_coords_invert_batched(f, f_dtype, f_row_stride, fH, fW, init, init_dtype, init_row_stride, out, out_dtype, out_row_stride, oH, oW,
                                      i0, j0, max_iter, tol, 1, 0, 0, 0, stream);
}

int lerf_coords_invert_host(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW, const void* init, int init_dtype,
                            int64_t init_row_stride, void* out, int out_dtype, int64_t out_row_stride, int oH, int oW, int i0, int j0,
                            int max_iter, double tol) {
    return lerf_coords_invert_batched_host(f, f_dtype, f_row_stride, fH, fW, init, init_dtype, init_row_stride, out, out_dtype, out_row_stride, oH,
                                           oW, i0, j0, max_iter, tol, 1, 0, 0, 0);
}

int lerf_coords_invert_raster(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW, const float* depth, void* out, int out_dtype,
                              int64_t out_row_stride, int oH, int oW, int i0, int j0, int max_span, int orient, uint64_t* keys, void* stream) {
    return lerf_coords_invert_raster_batched(f, f_dtype, f_row_stride, fH, fW, depth, out, out_dtype, out_row_stride, oH, oW, i0, j0, max_span,
                                             orient, keys, 1, 0, 0, 0, 0, stream);
}

int lerf_coords_invert_raster_host(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW, const float* depth, void* out,
                                   int out_dtype, int64_t out_row_stride, int oH, int oW, int i0, int j0, int max_span, int orient,
                                   uint64_t* keys) {
    return lerf_coords_invert_raster_batched_host(f, f_dtype, f_row_stride, fH, fW, depth, out, out_dtype, out_row_stride, oH, oW, i0, j0, max_span,
                                                  orient, keys, 1, 0, 0, 0, 0);
}

int lerf_coords_compose_bwd(const void* a, int a_dtype, int64_t a_row_stride, int aH, int aW, const void* b, int b_dtype, int64_t b_row_stride,
                            const double* grad_out, int oH, int oW, double* grad_a, double* grad_b, void* stream) {
    return lerf_coords_compose_bwd_batched(a, a_dtype, a_row_stride, aH, aW, b, b_dtype, b_row_stride, grad_out, oH, oW, grad_a, grad_b, 1, 0, 0, 0, 0,
                                           0, stream);
}

int lerf_coords_compose_bwd_host(const void* a, int a_dtype, int64_t a_row_stride, int aH, int aW, const void* b, int b_dtype,
                                 int64_t b_row_stride, const double* grad_out, int oH, int oW, double* grad_a, double* grad_b) {
    return lerf_coords_compose_bwd_batched_host(a, a_dtype, a_row_stride, aH, aW, b, b_dtype, b_row_stride, grad_out, oH, oW, grad_a, grad_b, 1, 0, 0,
                                                0, 0, 0);
}

int lerf_coords_invert_bwd(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW, const void* g, int g_dtype, int64_t g_row_stride,
                           const double* grad_out, int oH, int oW, double* grad_f, void* stream) {
    return lerf_coords_invert_bwd_batched(f, f_dtype, f_row_stride, fH, fW, g, g_dtype, g_row_stride, grad_out, oH, oW, grad_f, 1, 0, 0, 0, 0, stream);
}

int lerf_coords_invert_bwd_host(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW, const void* g, int g_dtype,
                                int64_t g_row_stride, const double* grad_out, int oH, int oW, double* grad_f) {
    return lerf_coords_invert_bwd_batched_host(f, f_dtype, f_row_stride, fH, fW, g, g_dtype, g_row_stride, grad_out, oH, oW, grad_f, 1, 0, 0, 0, 0);
}

size_t lerf_coords_mesh_bwd_workspace_bytes(int gh, int gw, int oH, int oW) {
    if (gh < 2 || gw < 2 || oH < 1 || oW < 1) return 0;
    return (size_t)gh * (size_t)oW * 2 * sizeof(double);
}

int lerf_coords_mesh_bwd_batched(const double* grad_map, int oH, int oW, int interp, int gh, int gw, double* grad_ctrl, void* workspace,
                                 size_t workspace_bytes, int n_sets, int64_t gmap_set, int64_t gctrl_set, void* stream) {
    if (!grad_map || !grad_ctrl || !workspace) return LERF_EINVAL;          // this entry point names a null pointer before it looks at n_sets
    const size_t per_set = lerf_coords_mesh_bwd_workspace_bytes(gh, gw, oH, oW);
    const int rc = check_call(n_sets,
                              {dense_operand(grad_map, LERF_F64, oH, oW, gmap_set), dense_operand(grad_ctrl, LERF_F64, gh, gw, gctrl_set, WRITTEN, 2),
                               bytes_operand(workspace, (int64_t)per_set, 16, WRITTEN)},
                              (interp == LERF_MESH_BILINEAR || interp == LERF_MESH_BICUBIC) && workspace_bytes >= (size_t)n_sets * per_set && gh <= 65535,
                              LERF_EUNSUPPORTED, /*batch_only=*/true);
    if (rc != LERF_OK) return rc;
    clear_stale_error();
    hipStream_t st = (hipStream_t)stream;
    const dim3 b1(CB_COLS, CB_ROWS), g1((oW + CB_COLS - 1) / CB_COLS, gh, n_sets), b2(64), g2(gw, gh, n_sets);
    const double2* gm = reinterpret_cast<const double2*>(grad_map);
    double2* tmp = reinterpret_cast<double2*>(workspace);
    double2* gc = reinterpret_cast<double2*>(grad_ctrl);
    const int64_t gm_set = gmap_set / 2, gc_set = gctrl_set / 2;              // in entries
    if (interp == LERF_MESH_BILINEAR) {
        hipLaunchKernelGGL((coords_mesh_bwd_rows_kernel<LERF_MESH_BILINEAR>), g1, b1, 0, st, gm, oH, oW, gh, tmp, gm_set);
        hipLaunchKernelGGL((coords_mesh_bwd_cols_kernel<LERF_MESH_BILINEAR>), g2, b2, 0, st, tmp, oW, gw, gc, gc_set);
    } else {
        hipLaunchKernelGGL((coords_mesh_bwd_rows_kernel<LERF_MESH_BICUBIC>), g1, b1, 0, st, gm, oH, oW, gh, tmp, gm_set);
        hipLaunchKernelGGL((coords_mesh_bwd_cols_kernel<LERF_MESH_BICUBIC>), g2, b2, 0, st, tmp, oW, gw, gc, gc_set);
    }
    return launch_status();
}

int lerf_coords_mesh_bwd(const double* grad_map, int oH, int oW, int interp, int gh, int gw, double* grad_ctrl, void* workspace,
                         size_t workspace_bytes, void* stream) {
    return lerf_coords_mesh_bwd_batched(grad_map, oH, oW, interp, gh, gw, grad_ctrl, workspace, workspace_bytes, 1, 0, 0, stream);
}

size_t lerf_coords_build_bwd_workspace_bytes(int n_params, int n_sets, int oH, int oW) {
    if (n_params < 1 || n_params > kMaxParams || n_sets < 1 || n_sets > 65535 || oH < 1 || oW < 1) return 0;
    return (size_t)n_sets * (size_t)n_params * (size_t)build_bwd_blocks(oH, oW) * sizeof(double);
}

int lerf_coords_build_bwd(int model, const double* params_dev, int n_sets, int n_params, const double* grad_map, int oH, int oW, int i0, int j0,
                          double* grad_params, void* workspace, size_t workspace_bytes, void* stream) {
    return build_bwd(TwoPassOnDevice{(hipStream_t)stream, (double*)workspace}, model, params_dev, n_sets, n_params, grad_map, oH, oW, i0, j0, grad_params,
                     workspace, workspace_bytes);
}

int lerf_coords_math(int op, const double* x, const double* y, int64_t n, double* out, void* stream) {
    const int rc = math_args(op, x, y, n, out);
    if (rc != LERF_OK) return rc;
    if (n == 0) return LERF_OK;
    clear_stale_error();
    hipLaunchKernelGGL(coords_math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, op, x, y, n, out);
    return launch_status();
}

// the host twin that is not a runner away: a plain loop
int lerf_coords_math_host(int op, const double* x, const double* y, int64_t n, double* out) {
    const int rc = math_args(op, x, y, n, out);
    if (rc != LERF_OK) return rc;
    for (int64_t e = 0; e < n; ++e) out[e] = math_element(op, x, y, e);
    return LERF_OK;
}

int lerf_coords_build_bwd_host(int model, const double* params, int n_sets, int n_params, const double* grad_map, int oH, int oW, int i0, int j0,
                               double* grad_params) {
    return build_bwd(TwoPassOnHost{}, model, params, n_sets, n_params, grad_map, oH, oW, i0, j0, grad_params, nullptr, 0);
}

int lerf_coords_reproject(int kind, const double* params_dev, int n_sets, const void* depth, int depth_dtype, int64_t depth_set_stride, void* out,
                          int out_dtype, int64_t out_set_stride, int64_t out_row_stride, float* depth_out, int64_t depth_out_set_stride, int oH,
                          int oW, int i0, int j0, void* stream) {
    return reproject(OnDevice{(hipStream_t)stream}, kind, params_dev, n_sets, depth, depth_dtype, depth_set_stride, out, out_dtype, out_set_stride,
                     out_row_stride, depth_out, depth_out_set_stride, oH, oW, i0, j0);
}

int lerf_coords_reproject_host(int kind, const double* params, int n_sets, const void* depth, int depth_dtype, int64_t depth_set_stride, void* out,
                               int out_dtype, int64_t out_set_stride, int64_t out_row_stride, float* depth_out, int64_t depth_out_set_stride,
                               int oH, int oW, int i0, int j0) {
    return reproject(OnHost{}, kind, params, n_sets, depth, depth_dtype, depth_set_stride, out, out_dtype, out_set_stride, out_row_stride, depth_out,
                     depth_out_set_stride, oH, oW, i0, j0);
}

size_t lerf_coords_reproject_bwd_workspace_bytes(int n_sets, int oH, int oW) {
    return lerf_coords_build_bwd_workspace_bytes(kReprojectParams, n_sets, oH, oW);
}

int lerf_coords_reproject_bwd(int kind, const double* params_dev, int n_sets, const void* depth, int depth_dtype, int64_t depth_set_stride,
                              const double* grad_map, const double* grad_depth_out, int oH, int oW, int i0, int j0, double* grad_depth,
                              double* grad_params, void* workspace, size_t workspace_bytes, void* stream) {
    return reproject_bwd(TwoPassOnDevice{(hipStream_t)stream, (double*)workspace}, kind, params_dev, n_sets, depth, depth_dtype, depth_set_stride, grad_map,
                         grad_depth_out, oH, oW, i0, j0, grad_depth, grad_params, workspace, workspace_bytes);
}

int lerf_coords_reproject_bwd_host(int kind, const double* params, int n_sets, const void* depth, int depth_dtype, int64_t depth_set_stride,
                                   const double* grad_map, const double* grad_depth_out, int oH, int oW, int i0, int j0, double* grad_depth,
                                   double* grad_params) {
    return reproject_bwd(TwoPassOnHost{}, kind, params, n_sets, depth, depth_dtype, depth_set_stride, grad_map, grad_depth_out, oH, oW, i0, j0, grad_depth,
                         grad_params, nullptr, 0);
}

int lerf_splat(const void* x, int dtype, int C, int H, int W, int64_t x_set_stride, const void* f, int f_dtype, int64_t f_row_stride,
               int64_t f_set_stride, const void* m, int64_t m_set_stride, void* acc, int with_norm, int oH, int oW, int64_t acc_set_stride,
               int n_sets, void* stream) {
    return splat(OnDevice{(hipStream_t)stream}, x, dtype, C, H, W, x_set_stride, f, f_dtype, f_row_stride, f_set_stride, m, m_set_stride, acc,
                 with_norm, oH, oW, acc_set_stride, n_sets);
}

int lerf_splat_host(const void* x, int dtype, int C, int H, int W, int64_t x_set_stride, const void* f, int f_dtype, int64_t f_row_stride,
                    int64_t f_set_stride, const void* m, int64_t m_set_stride, void* acc, int with_norm, int oH, int oW,
                    int64_t acc_set_stride, int n_sets) {
    return splat(OnHost{}, x, dtype, C, H, W, x_set_stride, f, f_dtype, f_row_stride, f_set_stride, m, m_set_stride, acc, with_norm, oH, oW,
                 acc_set_stride, n_sets);
}

int lerf_splat_bwd(const void* x, int dtype, int C, int H, int W, int64_t x_set_stride, const void* f, int f_dtype, int64_t f_row_stride,
                   int64_t f_set_stride, const void* m, int64_t m_set_stride, const void* g, int with_norm, int oH, int oW,
                   int64_t g_set_stride, void* grad_x, int64_t grad_x_set_stride, void* grad_m, int64_t grad_m_set_stride, double* grad_f,
                   int64_t grad_f_set_stride, int n_sets, void* stream) {
    return splat_bwd(OnDevice{(hipStream_t)stream}, x, dtype, C, H, W, x_set_stride, f, f_dtype, f_row_stride, f_set_stride, m, m_set_stride, g,
                     with_norm, oH, oW, g_set_stride, grad_x, grad_x_set_stride, grad_m, grad_m_set_stride, grad_f, grad_f_set_stride, n_sets);
}

int lerf_splat_bwd_host(const void* x, int dtype, int C, int H, int W, int64_t x_set_stride, const void* f, int f_dtype, int64_t f_row_stride,
                        int64_t f_set_stride, const void* m, int64_t m_set_stride, const void* g, int with_norm, int oH, int oW,
                        int64_t g_set_stride, void* grad_x, int64_t grad_x_set_stride, void* grad_m, int64_t grad_m_set_stride,
                        double* grad_f, int64_t grad_f_set_stride, int n_sets) {
    return splat_bwd(OnHost{}, x, dtype, C, H, W, x_set_stride, f, f_dtype, f_row_stride, f_set_stride, m, m_set_stride, g, with_norm, oH, oW,
                     g_set_stride, grad_x, grad_x_set_stride, grad_m, grad_m_set_stride, grad_f, grad_f_set_stride, n_sets);
}

// ---- the ordered scatter: the same operation templates under OrderedOnDevice / OrderedOnHost
size_t lerf_scatter_ordered_workspace_bytes(int64_t n_entries, int64_t n_targets, int n_sets) {
    if (n_entries < 1 || n_targets < 1 || n_sets < 1 || n_sets > 65535 || !ordered_sizes_ok(n_entries, n_targets)) return 0;
    return OrderedLayout::bytes(n_entries, n_targets, n_sets);
}

int lerf_scan_exclusive_u32_block(void) { return kScanBlock; }

size_t lerf_scan_exclusive_u32_workspace_bytes(int64_t n) { return n < 1 || n > 0xffffffffLL ? 0 : sizeof(uint32_t) * (size_t)scan_partials(n); }

int lerf_scan_exclusive_u32(uint32_t* data, int64_t n, void* workspace, size_t workspace_bytes, void* stream) {
    if (!data || (uintptr_t)data % 4 != 0 || n < 1 || n > 0xffffffffLL) return LERF_EINVAL;
    const size_t need = lerf_scan_exclusive_u32_workspace_bytes(n);
    if (need) {
        if (!workspace || (uintptr_t)workspace % 4 != 0 || workspace_bytes < need) return LERF_EINVAL;
        const uintptr_t a = (uintptr_t)data, b = (uintptr_t)workspace;
        if (a < b + need && b < a + 4 * (size_t)n) return LERF_EINVAL;
    }
    clear_stale_error();
    scan_exclusive_u32((hipStream_t)stream, data, n, 1, n, (uint32_t*)workspace, nullptr);
    return launch_status();
}

int lerf_scan_exclusive_u32_host(uint32_t* data, int64_t n) {
    if (!data || (uintptr_t)data % 4 != 0 || n < 1 || n > 0xffffffffLL) return LERF_EINVAL;
    scan_exclusive_u32_host(data, n);
    return LERF_OK;
}

int lerf_splat_ordered(const void* x, int dtype, int C, int H, int W, int64_t x_set_stride, const void* f, int f_dtype, int64_t f_row_stride,
                       int64_t f_set_stride, const void* m, int64_t m_set_stride, void* acc, int with_norm, int oH, int oW,
                       int64_t acc_set_stride, int n_sets, void* workspace, size_t workspace_bytes, int max_adders, void* stream) {
    const OrderedArgs ord{workspace, workspace_bytes, max_adders};
    return splat(OrderedOnDevice{(hipStream_t)stream, workspace, max_adders}, x, dtype, C, H, W, x_set_stride, f, f_dtype, f_row_stride,
                 f_set_stride, m, m_set_stride, acc, with_norm, oH, oW, acc_set_stride, n_sets, &ord);
}

int lerf_splat_ordered_host(const void* x, int dtype, int C, int H, int W, int64_t x_set_stride, const void* f, int f_dtype,
                            int64_t f_row_stride, int64_t f_set_stride, const void* m, int64_t m_set_stride, void* acc, int with_norm, int oH,
                            int oW, int64_t acc_set_stride, int n_sets, void* workspace, size_t workspace_bytes, int max_adders) {
    const OrderedArgs ord{workspace, workspace_bytes, max_adders};
    return splat(OrderedOnHost{workspace, max_adders}, x, dtype, C, H, W, x_set_stride, f, f_dtype, f_row_stride, f_set_stride, m, m_set_stride,
                 acc, with_norm, oH, oW, acc_set_stride, n_sets, &ord);
}

int lerf_coords_compose_bwd_batched_ordered(const void* a, int a_dtype, int64_t a_row_stride, int aH, int aW, const void* b, int b_dtype,
                                            int64_t b_row_stride, const double* grad_out, int oH, int oW, double* grad_a, double* grad_b,
                                            int n_sets, int64_t a_set_stride, int64_t b_set_stride, int64_t grad_out_set_stride,
                                            int64_t grad_a_set_stride, int64_t grad_b_set_stride, void* workspace, size_t workspace_bytes,
                                            int max_adders, void* stream) {
    const OrderedArgs ord{workspace, workspace_bytes, max_adders};
    return compose_bwd(OrderedOnDevice{(hipStream_t)stream, workspace, max_adders}, a, a_dtype, a_row_stride, aH, aW, b, b_dtype, b_row_stride,
                       grad_out, oH, oW, grad_a, grad_b, n_sets, a_set_stride, b_set_stride, grad_out_set_stride, grad_a_set_stride,
                       grad_b_set_stride, &ord);
}

int lerf_coords_compose_bwd_batched_ordered_host(const void* a, int a_dtype, int64_t a_row_stride, int aH, int aW, const void* b, int b_dtype,
                                                 int64_t b_row_stride, const double* grad_out, int oH, int oW, double* grad_a, double* grad_b,
                                                 int n_sets, int64_t a_set_stride, int64_t b_set_stride, int64_t grad_out_set_stride,
                                                 int64_t grad_a_set_stride, int64_t grad_b_set_stride, void* workspace, size_t workspace_bytes,
                                                 int max_adders) {
    const OrderedArgs ord{workspace, workspace_bytes, max_adders};
    return compose_bwd(OrderedOnHost{workspace, max_adders}, a, a_dtype, a_row_stride, aH, aW, b, b_dtype, b_row_stride, grad_out, oH, oW, grad_a,
                       grad_b, n_sets, a_set_stride, b_set_stride, grad_out_set_stride, grad_a_set_stride, grad_b_set_stride, &ord);
}

int lerf_coords_invert_bwd_batched_ordered(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW, const void* g, int g_dtype,
                                           int64_t g_row_stride, const double* grad_out, int oH, int oW, double* grad_f, int n_sets,
                                           int64_t f_set_stride, int64_t g_set_stride, int64_t grad_out_set_stride, int64_t grad_f_set_stride,
                                           void* workspace, size_t workspace_bytes, int max_adders, void* stream) {
    const OrderedArgs ord{workspace, workspace_bytes, max_adders};
    return invert_bwd(OrderedOnDevice{(hipStream_t)stream, workspace, max_adders}, f, f_dtype, f_row_stride, fH, fW, g, g_dtype, g_row_stride,
                      grad_out, oH, oW, grad_f, n_sets, f_set_stride, g_set_stride, grad_out_set_stride, grad_f_set_stride, &ord);
}

int lerf_coords_invert_bwd_batched_ordered_host(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW, const void* g, int g_dtype,
                                                int64_t g_row_stride, const double* grad_out, int oH, int oW, double* grad_f, int n_sets,
                                                int64_t f_set_stride, int64_t g_set_stride, int64_t grad_out_set_stride,
                                                int64_t grad_f_set_stride, void* workspace, size_t workspace_bytes, int max_adders) {
    const OrderedArgs ord{workspace, workspace_bytes, max_adders};
    return invert_bwd(OrderedOnHost{workspace, max_adders}, f, f_dtype, f_row_stride, fH, fW, g, g_dtype, g_row_stride, grad_out, oH, oW, grad_f,
                      n_sets, f_set_stride, g_set_stride, grad_out_set_stride, grad_f_set_stride, &ord);
}

int lerf_coords_compose_bwd_ordered(const void* a, int a_dtype, int64_t a_row_stride, int aH, int aW, const void* b, int b_dtype,
                                    int64_t b_row_stride, const double* grad_out, int oH, int oW, double* grad_a, double* grad_b,
                                    void* workspace, size_t workspace_bytes, int max_adders, void* stream) {
    return lerf_coords_compose_bwd_batched_ordered(a, a_dtype, a_row_stride, aH, aW, b, b_dtype, b_row_stride, grad_out, oH, oW, grad_a, grad_b, 1,
                                                   0, 0, 0, 0, 0, workspace, workspace_bytes, max_adders, stream);
}

int lerf_coords_compose_bwd_ordered_host(const void* a, int a_dtype, int64_t a_row_stride, int aH, int aW, const void* b, int b_dtype,
                                         int64_t b_row_stride, const double* grad_out, int oH, int oW, double* grad_a, double* grad_b,
                                         void* workspace, size_t workspace_bytes, int max_adders) {
    return lerf_coords_compose_bwd_batched_ordered_host(a, a_dtype, a_row_stride, aH, aW, b, b_dtype, b_row_stride, grad_out, oH, oW, grad_a,
                                                        grad_b, 1, 0, 0, 0, 0, 0, workspace, workspace_bytes, max_adders);
}

int lerf_coords_invert_bwd_ordered(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW, const void* g, int g_dtype,
                                   int64_t g_row_stride, const double* grad_out, int oH, int oW, double* grad_f, void* workspace,
                                   size_t workspace_bytes, int max_adders, void* stream) {
    return lerf_coords_invert_bwd_batched_ordered(f, f_dtype, f_row_stride, fH, fW, g, g_dtype, g_row_stride, grad_out, oH, oW, grad_f, 1, 0, 0, 0,
                                                  0, workspace, workspace_bytes, max_adders, stream);
}

int lerf_coords_invert_bwd_ordered_host(const void* f, int f_dtype, int64_t f_row_stride, int fH, int fW, const void* g, int g_dtype,
                                        int64_t g_row_stride, const double* grad_out, int oH, int oW, double* grad_f, void* workspace,
                                        size_t workspace_bytes, int max_adders) {
    return lerf_coords_invert_bwd_batched_ordered_host(f, f_dtype, f_row_stride, fH, fW, g, g_dtype, g_row_stride, grad_out, oH, oW, grad_f, 1, 0,
                                                       0, 0, 0, workspace, workspace_bytes, max_adders);
}

}  // extern "C"
