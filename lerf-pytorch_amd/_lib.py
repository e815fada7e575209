"""ctypes binding of liblerf_hip.so (C ABI: include/lerf_hip.h).

There is no CPU fallback: if the shared library is missing or a device entry
point is called without a GPU, this module raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# The in-tree product library.  The package reads NO environment variable for this: diagnostic builds (cycle stamps, A/B
# variants under csrc/build_*/) are selected explicitly by the tools that own them, through use_library() before the first
# call (tools/stamps.py, `bench.py --lib`, which prints the path in its JSON line).
LIB_PATH = os.path.join(_HERE, "liblerf_hip.so")

LERF_MAX_MODES = 5
LERF_LUT_ENTRIES = 83521
LERF_MAX_SUPPORT = 8
LERF_U8, LERF_F32, LERF_F64, LERF_I16 = 0, 1, 2, 3
KIND_GAUSS, KIND_LINEAR, KIND_NEAREST, KIND_CUBIC, KIND_BILINEAR, KIND_LANCZOS2, KIND_LANCZOS3 = range(7)
KINDS = {"gauss": KIND_GAUSS, "linear": KIND_LINEAR, "nearest": KIND_NEAREST, "cubic": KIND_CUBIC,
         "bilinear": KIND_BILINEAR, "lanczos2": KIND_LANCZOS2, "lanczos3": KIND_LANCZOS3}

# image padding rules (include/lerf_hip.h LERF_PAD_*), by their np.pad and F.pad names
PAD_MODES = {"constant": 0, "edge": 1, "replicate": 1, "reflect": 2, "symmetric": 3, "wrap": 4, "circular": 4}
NUMPY_PAD_MODES = ("constant", "edge", "reflect", "symmetric", "wrap")
TORCH_PAD_MODES = ("constant", "replicate", "reflect", "circular")


def pad_mode_code(name, allowed):
    """LERF_PAD_* of a pad_mode the reference's class would hand to np.pad / F.pad.  The index-remapping modes are
    implemented; numpy's statistical ones (linear_ramp, maximum, mean, median, minimum, empty) are not."""
    if name not in allowed:
        raise NotImplementedError("pad_mode {!r} is not implemented (supported: {})".format(name, ", ".join(allowed)))
    return PAD_MODES[name]


EXPORTS = [
    "lerf_abi_version", "lerf_strerror", "lerf_device_count", "lerf_mode_offsets", "lerf_sr_axis_tables", "lerf_sr_axis_tables_f32",
    "lerf_sr_x2_tables", "lerf_sr_x2_owned", "lerf_sr_geometry_flags",
    "lerf_out_size", "lerf_invert3x3", "lerf_warp_pads", "lerf_lut_interp_i16", "lerf_lut_interp", "lerf_lut_interp_ex", "lerf_numer_epilogue_f32", "lerf_fused_lutpack_bytes", "lerf_fused_lutpack_build",
    "lerf_lut_stages_u8",
    "lerf_resize", "lerf_warp", "lerf_sr_fused_workspace_bytes", "lerf_sr_fused_supported", "lerf_sr_fused_u8",
    "lerf_sr_ragged_workspace_bytes", "lerf_sr_fused_ragged_u8", "lerf_stages_ragged_workspace_bytes", "lerf_stages_packed_ragged_u8",
    "lerf_stages_packed_u8", "lerf_unpack_stages", "lerf_warp_packed", "lerf_rect_copy_u8",
    "lerf_warp_tile_boxes", "lerf_warp_fused_supported", "lerf_warp_fused_u8",
    "lerf_remap", "lerf_remap_packed", "lerf_remap_host_geometry", "lerf_remap_batched", "lerf_remap_packed_batched",
    "lerf_metric_y_sse_u8", "lerf_metric_ssim_y_u8", "lerf_metric_masked_sse_u8",
    "lerf_swf2lut_interp_f32", "lerf_swf2lut_interp_bwd_f32", "lerf_resize_bwd_f32", "lerf_warp_bwd", "lerf_remap_bwd",
    "lerf_remap_bwd_batched",
    "lerf_srnet_weight_floats", "lerf_srnet_to_lut", "lerf_srnet_fwd_f32", "lerf_srnet_bwd_workspace_bytes", "lerf_srnet_bwd_f32",
    "lerf_imdn_weight_floats", "lerf_imdn_workspace_bytes", "lerf_imdn_fwd_f32",
    "lerf_imdn_saved_bytes", "lerf_imdn_fwd_train_f32", "lerf_imdn_bwd_workspace_bytes", "lerf_imdn_bwd_f32",
    "lerf_rr_axis", "lerf_rr_adjoint_csr", "lerf_patch_batch_u8",
    "lerf_coords_build", "lerf_coords_build_host", "lerf_coords_mesh", "lerf_coords_mesh_host", "lerf_coords_mesh_bwd_workspace_bytes",
    "lerf_coords_mesh_bwd", "lerf_coords_compose", "lerf_coords_compose_host", "lerf_coords_invert", "lerf_coords_invert_host",
    "lerf_coords_invert_raster", "lerf_coords_invert_raster_host", "lerf_coords_compose_bwd", "lerf_coords_compose_bwd_host", "lerf_coords_invert_bwd", "lerf_coords_invert_bwd_host",
    "lerf_coords_build_dev", "lerf_coords_build_bwd_workspace_bytes", "lerf_coords_build_bwd", "lerf_coords_build_bwd_host", "lerf_coords_math", "lerf_coords_math_host",
    "lerf_coords_mesh_batched", "lerf_coords_mesh_batched_host", "lerf_coords_mesh_bwd_batched", "lerf_coords_compose_batched", "lerf_coords_compose_batched_host",
    "lerf_coords_invert_batched", "lerf_coords_invert_batched_host", "lerf_coords_invert_raster_batched", "lerf_coords_invert_raster_batched_host",
    "lerf_coords_compose_bwd_batched", "lerf_coords_compose_bwd_batched_host", "lerf_coords_invert_bwd_batched", "lerf_coords_invert_bwd_batched_host",
    "lerf_coords_reproject", "lerf_coords_reproject_host", "lerf_coords_reproject_bwd_workspace_bytes", "lerf_coords_reproject_bwd",
    "lerf_coords_reproject_bwd_host",
    "lerf_splat", "lerf_splat_host", "lerf_splat_bwd", "lerf_splat_bwd_host",
    "lerf_scatter_ordered_workspace_bytes", "lerf_splat_ordered", "lerf_splat_ordered_host",
    "lerf_coords_compose_bwd_ordered", "lerf_coords_compose_bwd_ordered_host", "lerf_coords_compose_bwd_batched_ordered",
    "lerf_coords_compose_bwd_batched_ordered_host", "lerf_coords_invert_bwd_ordered", "lerf_coords_invert_bwd_ordered_host",
    "lerf_coords_invert_bwd_batched_ordered", "lerf_coords_invert_bwd_batched_ordered_host",
    "lerf_scan_exclusive_u32_block", "lerf_scan_exclusive_u32_workspace_bytes", "lerf_scan_exclusive_u32", "lerf_scan_exclusive_u32_host",
    "lerf_coords_trimesh_workspace_bytes", "lerf_coords_trimesh", "lerf_coords_trimesh_host", "lerf_coords_trimesh_batched",
    "lerf_coords_trimesh_batched_host",
    "lerf_coords_trimesh_bwd_workspace_bytes", "lerf_coords_trimesh_bwd", "lerf_coords_trimesh_bwd_host", "lerf_coords_trimesh_bwd_batched",
    "lerf_coords_trimesh_bwd_batched_host",
    "lerf_ubench_lds_gather",
]


class LerfError(RuntimeError):
    pass


class Plane(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("dtype", C.c_int), ("sy", C.c_int64), ("sx", C.c_int64), ("sc", C.c_int64)]


class EpiOp(C.Structure):
    _fields_ = [("op", C.c_int), ("a", C.c_double), ("b", C.c_double)]


class Luts(C.Structure):
    _fields_ = [
        ("n_modes1", C.c_int), ("n_modes2", C.c_int),
        ("modes1", C.c_char * LERF_MAX_MODES), ("modes2", C.c_char * LERF_MAX_MODES),
        ("oC", C.c_int),
        ("s1", C.c_void_p * LERF_MAX_MODES),
        ("s2", (C.c_void_p * 2) * LERF_MAX_MODES),
        ("fused_pack", C.c_void_p),
    ]


class SrGeo(C.Structure):
    _fields_ = [
        ("S", C.c_int), ("out_h", C.c_int), ("out_w", C.c_int),
        ("left_r", C.c_void_p), ("dis_r", C.c_void_p), ("left_c", C.c_void_p), ("dis_c", C.c_void_p),
        ("dis_r64", C.c_void_p), ("dis_c64", C.c_void_p),
        ("pad_mode", C.c_int),
        ("tie_queue_cap", C.c_int),                                   # 0 = default, n > 0 = n entries, < 0 = no queue
        ("roi_y", C.c_int), ("roi_x", C.c_int), ("roi_h", C.c_int), ("roi_w", C.c_int),   # 0-sized = whole frame
        ("flags", C.c_int),                                           # GEO_* bits (ABI 5)
        ("out_row_pitch", C.c_int),                                   # bytes between output rows of lerf_sr_fused_u8, 0 = dense
    ]


GEO_FORCE_GENERAL, GEO_SINGLE_LAUNCH, GEO_INPUT_DEVICE, GEO_INPUT_HOST, GEO_X2_TABLES, GEO_NO_PERSIST = 1, 2, 4, 8, 16, 32
GEO_TILE_ROWS_64, GEO_TILE_ROWS_32, GEO_TILE_ROWS_16 = 64, 128, 256
GEO_EXACT_X2, GEO_FORCE_TABLES = 512, 1024      # the caller's promise of whole-frame x2 tables / diagnostic: the table path anyway


class SrItem(C.Structure):          # lerf_sr_item_t: one frame of a ragged launch
    _fields_ = [("img", C.c_void_p), ("out", C.c_void_p), ("H", C.c_int), ("W", C.c_int), ("geo", SrGeo)]


class StageItem(C.Structure):       # lerf_stage_item_t
    _fields_ = [("img", C.c_void_p), ("packed", C.c_void_p), ("H", C.c_int), ("W", C.c_int)]


class Rect(C.Structure):            # lerf_rect_t
    _fields_ = [("y", C.c_int), ("x", C.c_int), ("h", C.c_int), ("w", C.c_int), ("off", C.c_int64)]


LERF_MAX_RECTS = 8


class WarpGeo(C.Structure):
    _fields_ = [
        ("S", C.c_int), ("out_h", C.c_int), ("out_w", C.c_int),
        ("minv", C.c_double * 9),
        ("pad_r_lo", C.c_int), ("pad_r_hi", C.c_int), ("pad_c_lo", C.c_int), ("pad_c_hi", C.c_int),
        ("pad_mode", C.c_int),
        ("out_y0", C.c_int), ("out_x0", C.c_int), ("src_y0", C.c_int),       # ABI 7: a rectangle of the output from a band of the source
    ]


REMAP_PADS_FROM_MAP = -1

# coordinate-map builders (include/lerf_hip.h LERF_COORDS_*, LERF_MESH_*)
COORDS_MODELS = {"homography": 0, "radial": 1, "brown": 2, "fisheye": 16, "equirect": 17}
COORDS_MODEL_PARAMS = {"homography": 9, "radial": 8, "brown": 21, "fisheye": 17, "equirect": 13}
COORDS_MATH_OPS = {"sqrt": 0, "atan": 1, "atan2": 2}
MESH_INTERPS = {"bilinear": 0, "bicubic": 1}


class RemapGeo(C.Structure):       # lerf_remap_geo_t
    _fields_ = [
        ("S", C.c_int), ("out_h", C.c_int), ("out_w", C.c_int),
        ("coords", C.c_void_p), ("coords_dtype", C.c_int), ("row_stride", C.c_int64),
        ("pad_mode", C.c_int),
        ("pad_r_lo", C.c_int), ("pad_c_lo", C.c_int),                        # REMAP_PADS_FROM_MAP: derived from coords[0][0]
    ]


class RrAxis(C.Structure):         # lerf_rr_axis_t
    _fields_ = [("n_in", C.c_int), ("n_out", C.c_int), ("taps", C.c_int), ("left", C.c_void_p), ("row_ptr", C.c_void_p),
                ("idx", C.c_void_p), ("w", C.c_void_p), ("pad_mode", C.c_int)]


class PatchDesc(C.Structure):      # lerf_patch_desc_t
    _fields_ = [("lr_off", C.c_int64), ("hr_off", C.c_int64), ("lr_h", C.c_int32), ("lr_w", C.c_int32), ("lr_pitch", C.c_int32),
                ("hr_h", C.c_int32), ("hr_w", C.c_int32), ("hr_pitch", C.c_int32), ("li", C.c_int32), ("lj", C.c_int32),
                ("hi", C.c_int32), ("hj", C.c_int32), ("chan", C.c_int32), ("fliplr", C.c_int32), ("flipud", C.c_int32),
                ("k", C.c_int32)]


# the same layout as a numpy record: a batch of descriptors is one array, uploaded in one copy
PATCH_DESC_DTYPE = np.dtype([(n, np.int64 if t is C.c_int64 else np.int32) for n, t in PatchDesc._fields_])
assert PATCH_DESC_DTYPE.itemsize == C.sizeof(PatchDesc) == 72


_lib = None


def use_library(path):
    """tools only: load another build of liblerf_hip.so (same ABI) instead of the product library.  Must come before the first
    library call of the process; the choice is visible as `_lib.LIB_PATH`."""
    global LIB_PATH
    if _lib is not None:
        raise LerfError("use_library(%s): liblerf_hip.so is already loaded from %s" % (path, LIB_PATH))
    LIB_PATH = os.path.abspath(path)


def lib():
    """Load liblerf_hip.so once; raise loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LerfError(
            "liblerf_hip.so not found at %s -- build it with `python __graft_entry__.py` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback." % LIB_PATH)
    # ONE HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so and liblerf_hip.so depends on the same
    # SONAME, so whichever is loaded first serves both.  With liblerf_hip.so first, torch ends up on the system runtime it
    # was not built for and the first kernel launch fails with "no ROCm-capable device" (seen when a numpy-class test ran
    # before anything had imported torch); torch first, and both use torch's.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    L.lerf_abi_version.restype = C.c_int
    L.lerf_strerror.restype = C.c_char_p
    L.lerf_strerror.argtypes = [C.c_int]
    L.lerf_device_count.restype = C.c_int
    L.lerf_mode_offsets.argtypes = [C.c_char, C.c_int, C.c_void_p, C.c_void_p]
    L.lerf_sr_axis_tables.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.lerf_sr_axis_tables_f32.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.lerf_sr_x2_tables.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.lerf_sr_x2_owned.argtypes = [C.c_int, C.c_int, C.c_void_p]
    L.lerf_sr_geometry_flags.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int] + [C.c_void_p] * 6
    L.lerf_out_size.argtypes = [C.c_int, C.c_double]
    L.lerf_invert3x3.argtypes = [C.c_void_p, C.c_void_p]
    L.lerf_warp_pads.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.lerf_lut_interp_i16.argtypes = [C.POINTER(Plane), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.lerf_lut_interp.argtypes = [C.POINTER(Plane), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(Plane), C.c_void_p]
    L.lerf_lut_interp_ex.argtypes = [C.POINTER(Plane), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(Plane), C.c_int, C.c_void_p]
    L.lerf_numer_epilogue_f32.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.lerf_warp_tile_boxes.argtypes = [C.POINTER(WarpGeo), C.c_int, C.c_int, C.c_void_p]
    L.lerf_warp_fused_supported.argtypes = [C.c_int, C.POINTER(Luts), C.POINTER(WarpGeo), C.c_int, C.c_int, C.c_int, C.c_double]
    L.lerf_warp_fused_u8.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Luts), C.POINTER(WarpGeo), C.c_void_p,
                                     C.c_int, C.c_double, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]
    L.lerf_fused_lutpack_bytes.restype = C.c_size_t
    L.lerf_fused_lutpack_bytes.argtypes = [C.POINTER(Luts)]
    L.lerf_fused_lutpack_build.argtypes = [C.POINTER(Luts), C.c_void_p, C.c_void_p]
    L.lerf_lut_stages_u8.argtypes = [C.POINTER(Plane), C.c_int, C.c_int, C.c_int, C.POINTER(Luts),
                                     C.POINTER(Plane), C.POINTER(Plane), C.c_void_p]
    L.lerf_resize.argtypes = [C.POINTER(Plane), C.POINTER(Plane), C.c_int, C.c_int, C.c_int, C.POINTER(SrGeo),
                              C.c_int, C.c_double, C.POINTER(Plane), C.c_void_p]
    L.lerf_warp.argtypes = [C.POINTER(Plane), C.POINTER(Plane), C.c_int, C.c_int, C.c_int, C.POINTER(WarpGeo),
                            C.c_int, C.c_double, C.POINTER(Plane), C.c_void_p]
    L.lerf_stages_packed_u8.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Luts),
                                        C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]
    L.lerf_unpack_stages.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.lerf_warp_packed.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(WarpGeo), C.c_int, C.c_double,
                                   C.POINTER(Plane), C.c_int64, C.c_void_p]
    L.lerf_remap.argtypes = [C.POINTER(Plane), C.POINTER(Plane), C.c_int, C.c_int, C.c_int, C.POINTER(RemapGeo),
                             C.c_int, C.c_double, C.POINTER(Plane), C.c_void_p]
    L.lerf_remap_packed.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(RemapGeo), C.c_int, C.c_double,
                                    C.POINTER(Plane), C.c_int64, C.c_void_p]
    # one map per sample: geo describes map 0, then n_maps, map_stride (elements) and, for the planar forms, planes per map
    L.lerf_remap_batched.argtypes = [C.POINTER(Plane), C.POINTER(Plane), C.c_int, C.c_int, C.c_int, C.POINTER(RemapGeo), C.c_int,
                                     C.c_int64, C.c_int, C.c_int, C.c_double, C.POINTER(Plane), C.c_void_p]
    L.lerf_remap_packed_batched.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(RemapGeo), C.c_int,
                                            C.c_int64, C.c_int, C.c_double, C.POINTER(Plane), C.c_int64, C.c_void_p]
    L.lerf_remap_host_geometry.argtypes = [C.POINTER(RemapGeo), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]
    L.lerf_rect_copy_u8.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(Rect), C.c_int, C.c_int,
                                    C.c_void_p]
    L.lerf_sr_fused_supported.argtypes = [C.c_int, C.POINTER(Luts), C.POINTER(SrGeo), C.c_int, C.c_int, C.c_int, C.c_double]
    L.lerf_sr_ragged_workspace_bytes.restype = C.c_size_t
    L.lerf_sr_ragged_workspace_bytes.argtypes = [C.POINTER(SrItem), C.c_int, C.c_int]
    L.lerf_sr_fused_ragged_u8.argtypes = [C.POINTER(SrItem), C.c_int, C.c_int, C.POINTER(Luts), C.c_int, C.c_double, C.c_void_p,
                                          C.c_size_t, C.c_void_p]
    L.lerf_stages_ragged_workspace_bytes.restype = C.c_size_t
    L.lerf_stages_ragged_workspace_bytes.argtypes = [C.POINTER(StageItem), C.c_int, C.c_int]
    L.lerf_stages_packed_ragged_u8.argtypes = [C.POINTER(StageItem), C.c_int, C.c_int, C.POINTER(Luts), C.c_void_p, C.c_size_t,
                                               C.c_void_p]
    L.lerf_sr_fused_workspace_bytes.restype = C.c_size_t
    L.lerf_sr_fused_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    L.lerf_sr_fused_u8.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Luts),
                                   C.POINTER(SrGeo), C.c_int, C.c_double, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]
    L.lerf_metric_y_sse_u8.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_void_p]
    L.lerf_metric_ssim_y_u8.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.lerf_metric_masked_sse_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.lerf_swf2lut_interp_f32.argtypes = [C.c_void_p, C.c_int, C.c_char, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p]
    L.lerf_swf2lut_interp_bwd_f32.argtypes = [C.c_void_p, C.c_int, C.c_char, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.lerf_resize_bwd_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(SrGeo),
                                      C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.lerf_warp_bwd.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(WarpGeo),
                                C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.lerf_remap_bwd.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(RemapGeo),
                                 C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.lerf_remap_bwd_batched.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(RemapGeo),
                                         C.c_int, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
    L.lerf_srnet_weight_floats.restype = C.c_size_t
    L.lerf_srnet_weight_floats.argtypes = [C.c_int]
    L.lerf_srnet_to_lut.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.lerf_srnet_fwd_f32.argtypes = [C.c_void_p, C.c_int, C.c_char, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p]
    L.lerf_srnet_bwd_workspace_bytes.restype = C.c_size_t
    L.lerf_srnet_bwd_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    L.lerf_srnet_bwd_f32.argtypes = [C.c_void_p, C.c_int, C.c_char, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.lerf_imdn_weight_floats.restype = C.c_size_t
    L.lerf_imdn_weight_floats.argtypes = [C.c_int, C.c_int, C.c_int]
    L.lerf_imdn_workspace_bytes.restype = C.c_size_t
    L.lerf_imdn_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    L.lerf_imdn_fwd_f32.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.lerf_imdn_saved_bytes.restype = C.c_size_t
    L.lerf_imdn_saved_bytes.argtypes = [C.c_int] * 6
    L.lerf_imdn_fwd_train_f32.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.lerf_imdn_bwd_workspace_bytes.restype = C.c_size_t
    L.lerf_imdn_bwd_workspace_bytes.argtypes = [C.c_int] * 6
    L.lerf_imdn_bwd_f32.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.lerf_rr_axis.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.POINTER(RrAxis), C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.lerf_rr_adjoint_csr.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p]
    L.lerf_patch_batch_u8.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]
    _build = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int]
    _mesh = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int]
    _compose = [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int]
    L.lerf_coords_build.argtypes, L.lerf_coords_build_host.argtypes = _build + [C.c_void_p], _build
    L.lerf_coords_mesh.argtypes, L.lerf_coords_mesh_host.argtypes = _mesh + [C.c_void_p], _mesh
    L.lerf_coords_compose.argtypes, L.lerf_coords_compose_host.argtypes = _compose + [C.c_void_p], _compose
    _invert = [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int,
               C.c_int, C.c_int, C.c_int, C.c_double]
    L.lerf_coords_invert.argtypes, L.lerf_coords_invert_host.argtypes = _invert + [C.c_void_p], _invert
    _raster = [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
               C.c_int, C.c_int, C.c_void_p]
    L.lerf_coords_invert_raster.argtypes, L.lerf_coords_invert_raster_host.argtypes = _raster + [C.c_void_p], _raster
    _compose_bwd = [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    _invert_bwd = [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.lerf_coords_compose_bwd.argtypes, L.lerf_coords_compose_bwd_host.argtypes = _compose_bwd + [C.c_void_p], _compose_bwd
    L.lerf_coords_invert_bwd.argtypes, L.lerf_coords_invert_bwd_host.argtypes = _invert_bwd + [C.c_void_p], _invert_bwd
    L.lerf_coords_mesh_bwd_workspace_bytes.restype = C.c_size_t
    L.lerf_coords_mesh_bwd_workspace_bytes.argtypes = [C.c_int] * 4
    L.lerf_coords_mesh_bwd.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.lerf_coords_build_dev.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int,
                                        C.c_int, C.c_int, C.c_void_p]
    _build_bwd = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.lerf_coords_build_bwd.argtypes, L.lerf_coords_build_bwd_host.argtypes = _build_bwd + [C.c_void_p, C.c_size_t, C.c_void_p], _build_bwd
    _math = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.lerf_coords_math.argtypes, L.lerf_coords_math_host.argtypes = _math + [C.c_void_p], _math
    L.lerf_coords_build_bwd_workspace_bytes.restype = C.c_size_t
    L.lerf_coords_build_bwd_workspace_bytes.argtypes = [C.c_int] * 4
    # the batched forms: the single-map arguments, n_sets, one set stride per operand (then the stream)
    for name, single, n_strides in (("mesh", _mesh, 2), ("compose", _compose, 3), ("invert", _invert, 3), ("invert_raster", _raster, 4),
                                    ("compose_bwd", _compose_bwd, 5), ("invert_bwd", _invert_bwd, 4)):
        batched = single + [C.c_int] + [C.c_int64] * n_strides
        getattr(L, "lerf_coords_%s_batched" % name).argtypes = batched + [C.c_void_p]
        getattr(L, "lerf_coords_%s_batched_host" % name).argtypes = batched
    L.lerf_coords_mesh_bwd_batched.argtypes = L.lerf_coords_mesh_bwd.argtypes[:-1] + [C.c_int, C.c_int64, C.c_int64, C.c_void_p]
    _reproject = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                  C.c_int, C.c_int, C.c_int, C.c_int]
    L.lerf_coords_reproject.argtypes, L.lerf_coords_reproject_host.argtypes = _reproject + [C.c_void_p], _reproject
    _reproject_bwd = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                      C.c_void_p, C.c_void_p]
    L.lerf_coords_reproject_bwd.argtypes = _reproject_bwd + [C.c_void_p, C.c_size_t, C.c_void_p]
    L.lerf_coords_reproject_bwd_host.argtypes = _reproject_bwd
    L.lerf_coords_reproject_bwd_workspace_bytes.restype = C.c_size_t
    L.lerf_coords_reproject_bwd_workspace_bytes.argtypes = [C.c_int] * 3
    _splat_in = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int64]
    _splat = _splat_in + [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int]
    _splat_bwd = _splat_in + [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64] + [C.c_void_p, C.c_int64] * 3 + [C.c_int]
    L.lerf_splat.argtypes, L.lerf_splat_host.argtypes = _splat + [C.c_void_p], _splat
    L.lerf_splat_bwd.argtypes, L.lerf_splat_bwd_host.argtypes = _splat_bwd + [C.c_void_p], _splat_bwd
    # the ordered scatter: the sibling's arguments, then workspace, workspace_bytes, max_adders (then the stream)
    _ordered = [C.c_void_p, C.c_size_t, C.c_int]
    L.lerf_scatter_ordered_workspace_bytes.restype = C.c_size_t
    L.lerf_scatter_ordered_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int]
    L.lerf_splat_ordered.argtypes, L.lerf_splat_ordered_host.argtypes = _splat + _ordered + [C.c_void_p], _splat + _ordered
    for name, single, n_strides in (("compose_bwd", _compose_bwd, 5), ("invert_bwd", _invert_bwd, 4)):
        batched = single + [C.c_int] + [C.c_int64] * n_strides
        getattr(L, "lerf_coords_%s_ordered" % name).argtypes = single + _ordered + [C.c_void_p]
        getattr(L, "lerf_coords_%s_ordered_host" % name).argtypes = single + _ordered
        getattr(L, "lerf_coords_%s_batched_ordered" % name).argtypes = batched + _ordered + [C.c_void_p]
        getattr(L, "lerf_coords_%s_batched_ordered_host" % name).argtypes = batched + _ordered
    L.lerf_scan_exclusive_u32_workspace_bytes.restype = C.c_size_t
    L.lerf_scan_exclusive_u32_workspace_bytes.argtypes = [C.c_int64]
    L.lerf_scan_exclusive_u32.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]
    L.lerf_scan_exclusive_u32_host.argtypes = [C.c_void_p, C.c_int64]
    # pos, attr, faces, attr_faces, F, depth, w and its dtype; out and its tile; max_span, orient, keys, depth_out; workspace; (n_sets, nine set strides)
    _trimesh = ([C.c_void_p, C.c_int, C.c_int] * 2 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] +
                [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_int, C.c_int, C.c_void_p, C.c_void_p] +
                [C.c_void_p, C.c_size_t])
    _trimesh_batched = _trimesh + [C.c_int] + [C.c_int64] * 9
    L.lerf_coords_trimesh_workspace_bytes.restype = C.c_size_t
    L.lerf_coords_trimesh_workspace_bytes.argtypes = [C.c_int64, C.c_int]
    L.lerf_coords_trimesh.argtypes, L.lerf_coords_trimesh_host.argtypes = _trimesh + [C.c_void_p], _trimesh
    L.lerf_coords_trimesh_batched.argtypes, L.lerf_coords_trimesh_batched_host.argtypes = _trimesh_batched + [C.c_void_p], _trimesh_batched
    _trimesh_bwd = ([C.c_void_p, C.c_int, C.c_int] * 2 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_int] * 6 +
                    [C.c_void_p] * 5 + [C.c_void_p, C.c_size_t, C.c_int])
    _trimesh_bwd_batched = _trimesh_bwd + [C.c_int] + [C.c_int64] * 11
    L.lerf_coords_trimesh_bwd_workspace_bytes.restype = C.c_size_t
    L.lerf_coords_trimesh_bwd_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int]
    L.lerf_coords_trimesh_bwd.argtypes, L.lerf_coords_trimesh_bwd_host.argtypes = _trimesh_bwd + [C.c_void_p], _trimesh_bwd
    L.lerf_coords_trimesh_bwd_batched.argtypes = _trimesh_bwd_batched + [C.c_void_p]
    L.lerf_coords_trimesh_bwd_batched_host.argtypes = _trimesh_bwd_batched
    L.lerf_ubench_lds_gather.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    for name in EXPORTS:          # AttributeError here = the .so does not match include/lerf_hip.h
        getattr(L, name)
    if L.lerf_abi_version() != 7:
        raise LerfError("liblerf_hip.so ABI version mismatch")
    _lib = L
    return L


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().lerf_strerror(rc).decode()
        if rc == -1:
            raise ValueError("%s: %s" % (what, msg))
        raise LerfError("%s: %s (code %d)" % (what, msg, rc))


# ------------------------------------------------------------------ host-side helpers (no GPU needed)
_MODE_OFFSETS = {}


def mode_offsets(mode: str, rot: int):
    """(dy[4], dx[4]) int8 of a sampling pattern rotated `rot` quarter turns (lerf_mode_offsets); cached: a pure function"""
    hit = _MODE_OFFSETS.get((mode, int(rot)))
    if hit is not None:
        return hit[0].copy(), hit[1].copy()
    dy, dx = _mode_offsets(mode, rot)
    _MODE_OFFSETS[(mode, int(rot))] = (dy.copy(), dx.copy())
    return dy, dx


def _mode_offsets(mode: str, rot: int):
    dy = np.zeros(4, np.int8)
    dx = np.zeros(4, np.int8)
    rc = lib().lerf_mode_offsets(mode.encode()[:1] if mode else b"\0", int(rot), dy.ctypes.data, dx.ctypes.data)
    if rc != 0:
        raise ValueError("Mode {} not implemented.".format(mode))     # resample/eval_lut_sr.py:84
    return dy, dx


def out_size(n_in: int, scale: float) -> int:
    return int(lib().lerf_out_size(int(n_in), float(scale)))


def sr_axis_tables(n_in: int, n_out: int, scale: float, S: int):
    left = np.zeros(n_out, np.int32)
    dis64 = np.zeros((n_out, S), np.float64)
    dis32 = np.zeros((n_out, S), np.float32)
    pads = np.zeros(2, np.int32)
    check(lib().lerf_sr_axis_tables(int(n_in), int(n_out), float(scale), int(S), left.ctypes.data,
                                    dis64.ctypes.data, dis32.ctypes.data, pads.ctypes.data), "lerf_sr_axis_tables")
    return left, dis64, dis32, (int(pads[0]), int(pads[1]))


def sr_x2_tables(n_out: int, S: int):
    """(left, dis64, dis32) of exact x2 in closed form (lerf_sr_x2_tables): what sr_axis_tables(n, 2 n, 2.0, S) gives, bit for bit"""
    left = np.empty(n_out, np.int32)
    dis64 = np.empty((n_out, S), np.float64)
    dis32 = np.empty((n_out, S), np.float32)
    check(lib().lerf_sr_x2_tables(int(n_out), int(S), left.ctypes.data, dis64.ctypes.data, dis32.ctypes.data), "lerf_sr_x2_tables")
    return left, dis64, dis32


def sr_x2_owned(n_in: int, tile: int):
    """[tiles][2] int32: the outputs [o0, o1) every tile of `tile` LR pixels owns along an axis of n_in pixels at exact x2"""
    r = np.empty(((int(n_in) + int(tile) - 1) // int(tile), 2), np.int32)
    check(lib().lerf_sr_x2_owned(int(n_in), int(tile), r.ctypes.data), "lerf_sr_x2_owned")
    return r


def sr_geometry_flags(in_hw, out_hw, scales, S, left_r, dis_r64, dis_r32, left_c, dis_c64, dis_c32) -> int:
    """GEO_EXACT_X2 when the host tables of both axes are the exact x2 tables of the whole frame (lerf_sr_geometry_flags), else 0"""
    arrs = [np.ascontiguousarray(a, t) for a, t in ((left_r, np.int32), (dis_r64, np.float64), (dis_r32, np.float32),
                                                    (left_c, np.int32), (dis_c64, np.float64), (dis_c32, np.float32))]
    if arrs[0].size != out_hw[0] or arrs[3].size != out_hw[1] or any(a.size != n * S for a, n in
                                                                     zip(arrs[1:3] + arrs[4:6], (out_hw[0],) * 2 + (out_hw[1],) * 2)):
        return 0
    return int(lib().lerf_sr_geometry_flags(int(in_hw[0]), int(in_hw[1]), int(out_hw[0]), int(out_hw[1]), float(scales[0]), float(scales[1]),
                                            int(S), *[a.ctypes.data for a in arrs]))


def sr_axis_tables_f32(n_in: int, n_out: int, scale: float, S: int):
    """float32 tables of the reference's torch classes (resize_right2d_torch.py:48-103)."""
    left = np.zeros(n_out, np.int32)
    dis32 = np.zeros((n_out, S), np.float32)
    pads = np.zeros(2, np.int32)
    check(lib().lerf_sr_axis_tables_f32(int(n_in), int(n_out), float(scale), int(S), left.ctypes.data,
                                        dis32.ctypes.data, pads.ctypes.data), "lerf_sr_axis_tables_f32")
    return left, dis32.astype(np.float64), dis32, (int(pads[0]), int(pads[1]))


def warp_pads(minv: np.ndarray, in_hw, out_hw, S: int):
    """pads (r_lo, r_hi, c_lo, c_hi) for the INVERSE homography (np.linalg.inv of the matrix)."""
    m = np.ascontiguousarray(minv, dtype=np.float64).reshape(9)
    pads = np.zeros(4, np.int32)
    check(lib().lerf_warp_pads(m.ctypes.data, int(in_hw[0]), int(in_hw[1]), int(out_hw[0]), int(out_hw[1]), int(S),
                               pads.ctypes.data), "lerf_warp_pads")
    return tuple(int(p) for p in pads)


def remap_host_geometry(coords: np.ndarray, in_hw, S: int, pads=None):
    """What the remap kernels derive from a coordinate map, on the host (lerf_remap_host_geometry): coords float64 / float32
    [oH, oW, 2] -> (gr, gc float64 [oH, oW], lr, lc int32 [oH, oW], (pad_r_lo, pad_c_lo)); pads=None: derived from coords[0, 0]."""
    c = np.asarray(coords)
    if c.ndim != 3 or c.shape[2] != 2 or c.dtype not in (np.float32, np.float64):
        raise ValueError("coords must be a float32 / float64 [oH, oW, 2] array")
    c = np.ascontiguousarray(c)
    oH, oW = c.shape[:2]
    g = RemapGeo()
    g.S, g.out_h, g.out_w = int(S), oH, oW
    g.coords, g.coords_dtype, g.row_stride = c.ctypes.data, (LERF_F32 if c.dtype == np.float32 else LERF_F64), 2 * oW
    g.pad_r_lo, g.pad_c_lo = (REMAP_PADS_FROM_MAP, REMAP_PADS_FROM_MAP) if pads is None else (int(pads[0]), int(pads[1]))
    gr, gc = np.zeros((oH, oW), np.float64), np.zeros((oH, oW), np.float64)
    lr, lc = np.zeros((oH, oW), np.int32), np.zeros((oH, oW), np.int32)
    out = np.zeros(2, np.int32)
    check(lib().lerf_remap_host_geometry(C.byref(g), int(in_hw[0]), int(in_hw[1]), gr.ctypes.data, gc.ctypes.data, lr.ctypes.data,
                                         lc.ctypes.data, out.ctypes.data), "lerf_remap_host_geometry")
    return gr, gc, lr, lc, (int(out[0]), int(out[1]))


# ------------------------------------------------------------------ coordinate maps: one marshaller for host arrays and device tensors
class _Operands:
    """What the coords_* wrappers ask of their operands, written once.  HostOperands (numpy arrays, the lerf_coords_*_host entry
    points) and DeviceOperands (torch device tensors, the current stream) supply the primitives."""

    def is_float(self, a):
        return a.dtype == self.f32 or a.dtype == self.f64

    def code(self, a):
        return LERF_F32 if a.dtype == self.f32 else LERF_F64

    def map(self, a, what):
        """(a, row stride in elements) of a map under the strided contract: [h, w, 2] float32 / float64, pairs contiguous, rows free"""
        if not self.is_array(a) or a.ndim != 3 or a.shape[2] != 2 or a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError("%s must be %s [h, w, 2]" % (what, self.noun))
        if not self.is_float(a):
            raise ValueError("%s must be float32 or float64, not %s" % (what, a.dtype))
        s = self.strides(a)
        if s[2] != 1 or s[1] != 2 or s[0] is None:
            raise ValueError("%s: contiguous (row, col) pairs, column stride 2" % what)
        return a, s[0]

    def out(self, out, out_hw, dtype, default, device, what):
        """a new map of `dtype` (None: `default`) or the checked `out`, with its row stride"""
        oH, oW = int(out_hw[0]), int(out_hw[1])
        if out is None:
            if oH < 1 or oW < 1:
                raise ValueError("%s: out_hw must be positive" % what)
            out = self.new((oH, oW, 2), self.dtype(dtype, default, what), device)
        elif tuple(out.shape[:2]) != (oH, oW):
            raise ValueError("%s: out must be [%d, %d, 2]" % (what, oH, oW))
        return self.map(out, "out")

    def batch(self, a, what, out=False):
        """(a, row stride, set stride, B) of a batch of maps [B, h, w, 2], set stride in elements like the row stride; a single map
        [h, w, 2] gives B = 0 and set stride 0 (in a batched call: one map shared by every set).  A batch is passed through when its
        strides meet the C contract (pairs contiguous, even row and set strides, sets that do not overlap); any other view of an
        input is made contiguous, any other view of an output is refused."""
        if not (self.is_array(a) and a.ndim == 4):
            a, s = self.map(a, what)
            return a, s, 0, 0
        if a.shape[3] != 2 or min(a.shape[:3]) < 1:
            raise ValueError("%s must be %s [B, h, w, 2]" % (what, self.noun))
        if not self.is_float(a):
            raise ValueError("%s must be float32 or float64, not %s" % (what, a.dtype))
        for copy in (False, True):
            if copy:
                if out:
                    raise ValueError("%s: contiguous (row, col) pairs, even row and set strides, sets that do not overlap" % what)
                a = self.contiguous(a)
            s = self.strides(a)
            B, h, w = a.shape[:3]
            if s[3] == 1 and s[2] == 2 and s[1] is not None and s[1] % 2 == 0 and s[1] >= 2 * w and (
                    B == 1 or (s[0] is not None and s[0] % 2 == 0 and s[0] >= (h - 1) * s[1] + 2 * w)):
                return a, s[1], (0 if B == 1 else s[0]), B
        raise ValueError("%s: contiguous (row, col) pairs, column stride 2" % what)

    def outs(self, out, B, out_hw, dtype, default, device, what):
        """out() for a batch: a new [B, oH, oW, 2] or the checked `out`, with its row and set strides (B == 0: one map, set stride 0)"""
        if not B:
            return self.out(out, out_hw, dtype, default, device, what) + (0,)
        oH, oW = int(out_hw[0]), int(out_hw[1])
        if out is None:
            if oH < 1 or oW < 1:
                raise ValueError("%s: out_hw must be positive" % what)
            out = self.new((B, oH, oW, 2), self.dtype(dtype, default, what), device)
        elif not self.is_array(out) or tuple(out.shape[:3]) != (B, oH, oW):
            raise ValueError("%s: out must be [%d, %d, %d, 2]" % (what, B, oH, oW))
        return self.batch(out, "out", out=True)[:3]

    def run(self, name, B, anchor, args, set_strides):
        """ONE library call: the single-map entry point `name`, or (B > 0) its batched form with n_sets = B and the set strides"""
        if B:
            self.call(name + "_batched" + self.suffix, anchor, *args, B, *[int(x) for x in set_strides])
        else:
            self.call(name + self.suffix, anchor, *args)

    def grad(self, g, shape, device, what):
        """a dense float64 gradient buffer [h, w, 2] (None: a zeroed one)"""
        if g is None:
            return self.new(shape, self.f64, device, zero=True)
        if not self.is_array(g) or g.dtype != self.f64 or tuple(g.shape) != tuple(shape) or not self.is_contiguous(g) or self.device(g) != device:
            raise ValueError("%s must be a contiguous float64 %s beside the maps" % (what, list(shape)))
        return g

    def dense(self, a, shape, dtype, device, what):
        """a contiguous buffer of `dtype` and `shape` beside the maps (None: a new one)"""
        if a is None:
            return self.new(shape, dtype, device)
        if not self.is_array(a) or a.dtype != dtype or tuple(a.shape) != tuple(shape) or not self.is_contiguous(a) or self.device(a) != device:
            raise ValueError("%s must be a contiguous %s %s beside the maps" % (what, getattr(dtype, "__name__", dtype), list(shape)))
        return a

    def one_device(self, what, names, first, *others):
        for a in others:
            if a is not None and self.device(a) != self.device(first):
                raise ValueError("%s: %s live on different devices" % (what, " and ".join(names)))

    def operand(self, a, stride):
        return self.ptr(a), self.code(a), stride

    def run_ordered(self, name, B, anchor, args, set_strides, n_entries, n_targets, max_adders):
        """run() for the _ordered form of `name`: the same arguments, then a workspace of
        lerf_scatter_ordered_workspace_bytes and the cap.  set_strides None: the entry point takes n_sets among its own arguments
        (lerf_splat).  Afterwards the header's largest count is READ BACK -- one 4-byte copy, and on the device a synchronisation of the
        stream -- and a count above max_adders raises LerfError: the elements over the cap hold NaN."""
        max_adders = int(max_adders)
        if max_adders < 1:
            raise ValueError("%s_ordered: max_adders must be at least 1" % name)
        n_sets = max(int(B), 1)
        nbytes = int(lib().lerf_scatter_ordered_workspace_bytes(int(n_entries), int(n_targets), n_sets))
        if not nbytes:
            raise LerfError("%s_ordered: %d entries into %d targets are beyond the 32-bit ids of the ordered scatter" % (name, n_entries, n_targets))
        ws = self.scratch(nbytes, self.device(anchor))
        tail = (self.ptr(ws), nbytes, max_adders)
        if set_strides is None:
            self.call(name + "_ordered" + self.suffix, anchor, *args, *tail)
        elif B:
            self.call(name + "_batched_ordered" + self.suffix, anchor, *args, B, *[int(x) for x in set_strides], *tail)
        else:
            self.call(name + "_ordered" + self.suffix, anchor, *args, *tail)
        most = self.max_count(ws)
        if most > max_adders:
            raise LerfError("%s_ordered: %d entries add into one element, more than max_adders = %d (that element holds NaN); raise "
                            "max_adders or use the atomic path" % (name, most, max_adders))
        return most


ORDERED_MAX_COUNT_OFFSET = 4          # LERF_ORDERED_MAX_COUNT_OFFSET: the byte offset of the largest count in the workspace header


def scan_block():
    """the block length B of lerf_scan_exclusive_u32 (the seams of its levels lie at multiples of B and of B * B)"""
    return int(lib().lerf_scan_exclusive_u32_block())


def ordered_workspace_bytes(n_entries, n_targets, n_sets=1):
    """lerf_scatter_ordered_workspace_bytes; its formula in Python is ordered_workspace_formula"""
    return int(lib().lerf_scatter_ordered_workspace_bytes(int(n_entries), int(n_targets), int(n_sets)))


def ordered_workspace_formula(n_entries, n_targets, n_sets=1):
    """the documented layout in bytes: header [4], cursor [n_sets][n_targets], list [n_sets][4 n_entries], scan partials [n_sets][P]"""
    B, n, P = scan_block(), int(n_targets), 0
    while n > B:
        n = -(-n // B)
        P += n
    return 4 * (4 + int(n_sets) * (int(n_targets) + 4 * int(n_entries) + P))


def scan_exclusive_u32_host(data):
    """lerf_scan_exclusive_u32_host: the exclusive prefix sums (modulo 2^32) of a contiguous uint32 numpy vector, in place"""
    if not isinstance(data, np.ndarray) or data.dtype != np.uint32 or data.ndim != 1 or not data.flags.c_contiguous:
        raise ValueError("lerf_scan_exclusive_u32_host: data must be a contiguous uint32 vector")
    check(lib().lerf_scan_exclusive_u32_host(data.ctypes.data, int(data.size)), "lerf_scan_exclusive_u32_host")
    return data


class HostOperands(_Operands):
    suffix, noun, f32, f64, key, i32 = "_host", "a numpy array", np.float32, np.float64, np.uint64, np.int32
    is_array = staticmethod(lambda a: isinstance(a, np.ndarray))
    strides = staticmethod(lambda a: tuple(s // a.itemsize if s % a.itemsize == 0 else None for s in a.strides))
    is_contiguous = staticmethod(lambda a: a.flags.c_contiguous)
    device = staticmethod(lambda a: None)
    ptr = staticmethod(lambda a: None if a is None else a.ctypes.data)
    dtype = staticmethod(lambda dtype, default, what: np.dtype(dtype))               # the host signatures default to float64
    new = staticmethod(lambda shape, dtype, device, zero=False: (np.zeros if zero else np.empty)(tuple(shape), dtype))
    contiguous = staticmethod(np.ascontiguousarray)                                  # array-likes too
    float64 = staticmethod(lambda x, what: np.ascontiguousarray(np.asarray(x, dtype=np.float64)))

    def call(self, name, anchor, *args):
        check(getattr(lib(), name)(*args), name)

    def workspace(self, nbytes, device):
        """the workspace arguments of a host twin: none (the host sums in place)"""
        return ()

    def scratch(self, nbytes, device):
        return np.empty(int(nbytes), np.uint8)

    def max_count(self, ws):
        return int(ws[ORDERED_MAX_COUNT_OFFSET:ORDERED_MAX_COUNT_OFFSET + 4].view(np.uint32)[0])


class DeviceOperands(_Operands):
    suffix, noun = "", "a device tensor"

    _one = None

    def __new__(cls):                                  # one instance, made at the first call that finds the GPU (require_gpu raises without)
        if cls._one is None:
            torch = require_gpu()
            cls._one = super().__new__(cls)
            cls._one.torch, cls._one.f32, cls._one.f64 = torch, torch.float32, torch.float64
            cls._one.key = torch.int64                 # the 64 bits of a raster key (numpy's side holds them as uint64)
            cls._one.i32 = torch.int32
        return cls._one

    strides = staticmethod(lambda t: t.stride())
    is_contiguous = staticmethod(lambda t: t.is_contiguous())
    device = staticmethod(lambda t: t.device)
    ptr = staticmethod(lambda t: None if t is None else t.data_ptr())

    def is_array(self, t):
        return isinstance(t, self.torch.Tensor) and t.is_cuda

    def dtype(self, dtype, default, what):
        dtype = default if dtype is None else dtype
        if dtype not in (self.f32, self.f64):
            raise ValueError("%s: dtype is torch.float32 or torch.float64" % what)
        return dtype

    def new(self, shape, dtype, device, zero=False):
        return (self.torch.zeros if zero else self.torch.empty)(tuple(shape), dtype=dtype, device=device)

    def contiguous(self, t):
        return t.detach().contiguous() if self.is_array(t) else t

    def float64(self, x, what):
        if not self.is_array(x) or x.dtype != self.f64:
            raise ValueError("%s: x (and y for atan2) must be float64 device tensors" % what)
        return self.contiguous(x)

    def call(self, name, anchor, *args):
        """the launch on `anchor`'s device and its current stream"""
        with on_device(anchor):
            check(getattr(lib(), name)(*args, current_stream(anchor.device)), name)

    def workspace(self, nbytes, device):
        """(pointer, bytes) of the per-stream scratch the adjoints share (ops._cached_workspace); nbytes 0: (None, 0)"""
        if not nbytes:
            return None, 0
        from . import ops
        ws = ops._cached_workspace(nbytes, device)
        return ws.data_ptr(), ws.numel()

    def scratch(self, nbytes, device):
        """a device byte tensor of at least nbytes: the per-stream scratch of workspace()"""
        from . import ops
        return ops._cached_workspace(nbytes, device)

    def max_count(self, ws):
        """the header's largest count: a 4-byte copy to the host, which waits for the stream"""
        return int(ws[ORDERED_MAX_COUNT_OFFSET:ORDERED_MAX_COUNT_OFFSET + 4].view(self.torch.int32).item()) & 0xffffffff


def coords_model_count(model, n, what):
    """ValueError unless `model` is known and takes n parameters"""
    if model not in COORDS_MODELS:
        raise ValueError("unknown coordinate-map model %r (known: %s)" % (model, ", ".join(COORDS_MODELS)))
    if int(n) != COORDS_MODEL_PARAMS[model]:
        raise ValueError("%s: unknown parameter layout for model %r: it takes %d parameters, not %d" % (what, model, COORDS_MODEL_PARAMS[model], n))


def coords_model_params(model, params, what="lerf_coords_build"):
    """(model code, float64 parameter vector) of a coordinate-map model"""
    p = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(-1))
    coords_model_count(model, p.size, what)
    return COORDS_MODELS[model], p


def mesh_interp_code(interp):
    if interp not in MESH_INTERPS:
        raise ValueError("interp is 'bilinear' or 'bicubic', not %r" % (interp,))
    return MESH_INTERPS[interp]


_HOST = HostOperands()


# The eight operations that exist on both sides, over X = HostOperands() or DeviceOperands(): ops.coords_* and coords_*_host below
# bind them and carry the documentation.  Mesh, compose, invert, invert_raster and the two adjoints take a leading B on their maps
# ([B, h, w, 2]) and then make ONE call of the batched entry point (lerf_coords_*_batched); a 3-D operand beside a batch is shared
# where the C contract allows it.  Reproject and its adjoint (coords_reproject_on, coords_reproject_bwd_on) are on both sides too: their
# batch is the entry point's own n_sets, one parameter set per depth plane.
def coords_build_on(X, model, params, out_hw, dtype, out, origin, device=None):
    what = "lerf_coords_build" + X.suffix
    code, p = coords_model_params(model, params, what)
    out, stride = X.out(out, out_hw, dtype, X.f64, device, what)
    X.call(what, out, code, p.ctypes.data, int(p.size), *X.operand(out, stride), int(out_hw[0]), int(out_hw[1]), int(origin[0]), int(origin[1]))
    return out


def coords_mesh_on(X, ctrl, out_hw, interp, dtype, out, origin, full_hw):
    what = "lerf_coords_mesh" + X.suffix
    c = X.contiguous(ctrl)
    if not X.is_array(c) or c.ndim not in (3, 4) or c.shape[-1] != 2:
        raise ValueError("%s: ctrl must be %s [gh, gw, 2] or [B, gh, gw, 2]" % (what, X.noun))
    if not X.is_float(c):
        raise ValueError("%s: ctrl must be float32 or float64" % what)
    code = mesh_interp_code(interp)
    full_hw = out_hw if full_hw is None else full_hw
    B = c.shape[0] if c.ndim == 4 else 0
    if c.ndim == 4 and B < 1:
        raise ValueError("%s: an empty batch" % what)
    gh, gw = c.shape[-3], c.shape[-2]
    out, stride, set_stride = X.outs(out, B, out_hw, dtype, c.dtype, X.device(c), what)
    X.one_device(what, ("ctrl", "out"), c, out)
    X.run("lerf_coords_mesh", B, c, (X.ptr(c), X.code(c), gh, gw, code, int(full_hw[0]), int(full_hw[1]), *X.operand(out, stride),
                                     int(out_hw[0]), int(out_hw[1]), int(origin[0]), int(origin[1])), (2 * gh * gw, set_stride))
    return out


def _one_batch(what, names, *sizes):
    """the common B of operands that hold B (batched) or 0 (single, shared) maps"""
    B = max(sizes)
    if any(b and b != B for b in sizes):
        raise ValueError("%s: %s hold different numbers of maps" % (what, " and ".join(names)))
    return B


def coords_compose_on(X, outer, inner, dtype, out):
    what = "lerf_coords_compose" + X.suffix
    a, sa, ta, Ba = X.batch(outer, "outer")
    b, sb, tb, Bb = X.batch(inner, "inner")
    X.one_device(what, ("outer", "inner"), a, b)
    if Ba and not Bb:
        raise ValueError("%s: a batch of outer maps needs a batch of as many inner maps" % what)
    B = _one_batch(what, ("outer", "inner"), Ba, Bb)
    out, so, to = X.outs(out, B, b.shape[-3:-1], dtype, b.dtype, X.device(b), what)
    X.run("lerf_coords_compose", B, b, (*X.operand(a, sa), a.shape[-3], a.shape[-2], *X.operand(b, sb), *X.operand(out, so), b.shape[-3],
                                        b.shape[-2]), (ta, tb, to))
    return out


def coords_invert_on(X, f, out_hw, init, dtype, out, origin, max_iter, tol):
    what = "lerf_coords_invert" + X.suffix
    a, sa, ta, Ba = X.batch(f, "f")
    b, sb, tb, Bb = (None, 0, 0, 0) if init is None else X.batch(init, "init")
    B = _one_batch(what, ("f", "init"), Ba, Bb)
    out, so, to = X.outs(out, B, out_hw, dtype, a.dtype, X.device(a), what)
    X.one_device(what, ("f", "out", "init"), a, out, b)
    if b is not None and tuple(b.shape[-3:-1]) != tuple(out.shape[-3:-1]):
        raise ValueError("%s: init must have out's shape" % what)
    X.run("lerf_coords_invert", B, a, (*X.operand(a, sa), a.shape[-3], a.shape[-2], X.ptr(b), LERF_F64 if b is None else X.code(b), sb,
                                       *X.operand(out, so), out.shape[-3], out.shape[-2], int(origin[0]), int(origin[1]), int(max_iter),
                                       float(tol)), (ta, tb, to))
    return out


def coords_invert_raster_on(X, f, out_hw, depth, dtype, out, origin, max_span, orient, keys, return_keys):
    what = "lerf_coords_invert_raster" + X.suffix
    a, sa, ta, Ba = X.batch(f, "f")
    fhw = tuple(a.shape[-3:-1])
    Bd = a.shape[0] if Ba and depth is not None and getattr(depth, "ndim", 0) == 3 else 0        # depth [fH, fW]: one for every map
    B = _one_batch(what, ("f", "depth"), Ba, Bd)
    out, so, to = X.outs(out, B, out_hw, dtype, a.dtype, X.device(a), what)
    d = None if depth is None else X.dense(depth, ((Bd,) if Bd else ()) + fhw, X.f32, X.device(a), what + ": depth")
    k = X.dense(keys, tuple(out.shape[:-1]), X.key, X.device(a), what + ": keys")
    X.one_device(what, ("f", "out"), a, out)
    ohw = tuple(out.shape[-3:-1])
    X.run("lerf_coords_invert_raster", B, a, (*X.operand(a, sa), fhw[0], fhw[1], X.ptr(d), *X.operand(out, so), ohw[0], ohw[1], int(origin[0]),
                                              int(origin[1]), int(max_span), int(orient), X.ptr(k)),
          (ta, fhw[0] * fhw[1] if Bd > 1 else 0, to, ohw[0] * ohw[1] if B > 1 else 0))
    return (out, k) if return_keys else out


TRIMESH_TILE = (4, 16)          # kTileRows x kTileCols: the item tile of the rasteriser's hot path
TRIMESH_MAX_SPAN = 65536


def trimesh_max_items(F, n_sets, out_hw, max_span):
    """the size rule of lerf_coords_trimesh in Python: n_sets * F * b, b the most item tiles one face can have; the call is refused
    (LERF_EUNSUPPORTED) when this exceeds 2^32 - 1"""
    b = 1
    for n, tile in zip(out_hw, TRIMESH_TILE):
        plane = -(-int(n) // tile)
        b *= min(plane, (int(max_span) + tile - 2) // tile + 1) if max_span > 0 else plane
    return int(n_sets) * int(F) * b


def coords_trimesh_on(X, pos, attr, faces, out_hw, attr_faces, depth, w, dtype, out, origin, max_span, orient, keys, return_keys, return_depth):
    what = "lerf_coords_trimesh" + X.suffix
    for a, name in ((pos, "pos"), (attr, "attr")):
        if not X.is_array(a) or a.ndim not in (2, 3) or a.shape[-1] != 2 or min(a.shape) < 1 or not X.is_float(a):
            raise ValueError("%s: %s must be %s [V, 2] or [B, V, 2], float32 or float64" % (what, name, X.noun))
    p, a = X.contiguous(pos), X.contiguous(attr)
    dev = X.device(p)
    B = _one_batch(what, ("pos", "attr"), p.shape[0] if p.ndim == 3 else 0, a.shape[0] if a.ndim == 3 else 0)
    V, Va = p.shape[-2], a.shape[-2]

    def indices(f, name):
        if not X.is_array(f) or f.dtype != X.i32 or f.ndim not in (2, 3) or f.shape[-1] != 3 or min(f.shape) < 1:
            raise ValueError("%s: %s must be %s [F, 3] or [B, F, 3], int32" % (what, name, X.noun))
        if f.ndim == 3 and f.shape[0] != B:
            raise ValueError("%s: %s holds %d sets of faces for a batch of %d" % (what, name, f.shape[0], B))
        return X.contiguous(f)

    fc = indices(faces, "faces")
    F = fc.shape[-2]
    af = None if attr_faces is None else indices(attr_faces, "attr_faces")
    if af is not None and af.shape[-2] != F:
        raise ValueError("%s: attr_faces must hold one triple per face" % what)

    def per_vertex(v, name, dtypes):
        if v is None:
            return None
        if not X.is_array(v) or v.dtype not in dtypes or v.ndim not in (1, 2) or v.shape[-1] != V or (v.ndim == 2 and v.shape[0] != B):
            raise ValueError("%s: %s must be %s [V] or [B, V], float32%s" % (what, name, X.noun, " or float64" if len(dtypes) > 1 else ""))
        return X.contiguous(v)

    d, wv = per_vertex(depth, "depth", (X.f32,)), per_vertex(w, "w", (X.f32, X.f64))
    if return_depth and d is None:
        raise ValueError("%s: depth_out needs depth" % what)
    if not 0 <= int(max_span) <= TRIMESH_MAX_SPAN or not -1 <= int(orient) <= 1:
        raise ValueError("%s: max_span is 0 (no tear rule) or 1..%d, orient -1, 0 or 1" % (what, TRIMESH_MAX_SPAN))
    ohw = (int(out_hw[0]), int(out_hw[1]))
    n_sets = max(B, 1)
    if min(ohw) < 1:
        raise ValueError("%s: out_hw must be positive" % what)
    if trimesh_max_items(F, n_sets, ohw, int(max_span)) > 0xffffffff or n_sets * (F + 1) > 0xffffffff:
        raise LerfError("%s: %d faces x %d sets into %d x %d with max_span = %d may need more than 2^32 - 1 (face, tile) items; pass a "
                        "max_span (a face wider than that is skipped), or split the mesh" % (what, F, n_sets, ohw[0], ohw[1], max_span))
    out, so, to = X.outs(out, B, ohw, a.dtype if dtype is None else dtype, a.dtype, dev, what)
    k = X.dense(keys, tuple(out.shape[:-1]), X.key, dev, what + ": keys")
    zo = X.new(tuple(out.shape[:-1]), X.f32, dev) if return_depth else None
    X.one_device(what, ("pos", "attr", "faces", "attr_faces", "depth", "w", "out"), p, a, fc, af, d, wv, out)
    nbytes = int(lib().lerf_coords_trimesh_workspace_bytes(F, n_sets))
    ws = X.scratch(nbytes, dev)
    per = lambda t, base, n: 0 if t is None or t.ndim == base or B < 2 else n          # the set stride of a dense operand: 0 shares it
    X.run("lerf_coords_trimesh", B, p, (X.ptr(p), X.code(p), V, X.ptr(a), X.code(a), Va, X.ptr(fc), X.ptr(af), F, X.ptr(d), X.ptr(wv), LERF_F32 if wv is None else X.code(wv),
                                        *X.operand(out, so), ohw[0], ohw[1], int(origin[0]), int(origin[1]), int(max_span), int(orient), X.ptr(k),
                                        X.ptr(zo), X.ptr(ws), nbytes),
          (per(p, 2, 2 * V), per(a, 2, 2 * Va), per(fc, 2, 3 * F), per(af, 2, 3 * F), per(d, 1, V), per(wv, 1, V), to,
           ohw[0] * ohw[1] if B > 1 else 0, ohw[0] * ohw[1] if B > 1 else 0))
    res = (out,) + ((k,) if return_keys else ()) + ((zo,) if return_depth else ())
    return res if len(res) > 1 else out


def coords_trimesh_bwd_on(X, pos, attr, faces, out_hw, keys, grad_out, attr_faces, depth, w, origin, max_span, orient, need, grad_attr, grad_pos,
                          grad_w, max_adders, raise_over):
    """lerf_coords_trimesh_bwd over X: the mesh operands as coords_trimesh_on takes them, keys the forward's plane, grad_out float64 of the
    map's shape -> (grad_attr, grad_pos, grad_w, most): float64 of attr's, pos's and w's shapes with a leading B where the call is a batch
    (an operand shared by the batch gets one gradient PER SET), None where need[k] is false; most: the header's largest valence.
    raise_over: a count above max_adders raises LerfError (the vertices over the cap hold NaN)."""
    what = "lerf_coords_trimesh_bwd" + X.suffix
    for a, name in ((pos, "pos"), (attr, "attr")):
        if not X.is_array(a) or a.ndim not in (2, 3) or a.shape[-1] != 2 or min(a.shape) < 1 or not X.is_float(a):
            raise ValueError("%s: %s must be %s [V, 2] or [B, V, 2], float32 or float64" % (what, name, X.noun))
    p, a = X.contiguous(pos), X.contiguous(attr)
    dev = X.device(p)
    ohw = (int(out_hw[0]), int(out_hw[1]))
    if not X.is_array(keys) or keys.dtype != X.key or keys.ndim not in (2, 3) or tuple(keys.shape[-2:]) != ohw or not X.is_contiguous(keys):
        raise ValueError("%s: keys must be the forward's contiguous key plane [oH, oW] or [B, oH, oW]" % what)
    B = _one_batch(what, ("pos", "attr", "keys"), p.shape[0] if p.ndim == 3 else 0, a.shape[0] if a.ndim == 3 else 0, keys.shape[0] if keys.ndim == 3 else 0)
    if B and keys.ndim != 3:
        raise ValueError("%s: a batch needs one key plane per set" % what)
    V, Va = p.shape[-2], a.shape[-2]

    def indices(f, name):
        if not X.is_array(f) or f.dtype != X.i32 or f.ndim not in (2, 3) or f.shape[-1] != 3 or min(f.shape) < 1:
            raise ValueError("%s: %s must be %s [F, 3] or [B, F, 3], int32" % (what, name, X.noun))
        if f.ndim == 3 and f.shape[0] != B:
            raise ValueError("%s: %s holds %d sets of faces for a batch of %d" % (what, name, f.shape[0], B))
        return X.contiguous(f)

    fc = indices(faces, "faces")
    F = fc.shape[-2]
    af = None if attr_faces is None else indices(attr_faces, "attr_faces")
    if af is not None and af.shape[-2] != F:
        raise ValueError("%s: attr_faces must hold one triple per face" % what)

    def per_vertex(v, name, dtypes):
        if v is None:
            return None
        if not X.is_array(v) or v.dtype not in dtypes or v.ndim not in (1, 2) or v.shape[-1] != V or (v.ndim == 2 and v.shape[0] != B):
            raise ValueError("%s: %s must be %s [V] or [B, V], float32%s" % (what, name, X.noun, " or float64" if len(dtypes) > 1 else ""))
        return X.contiguous(v)

    d, wv = per_vertex(depth, "depth", (X.f32,)), per_vertex(w, "w", (X.f32, X.f64))
    need = tuple(bool(n) for n in need)
    if len(need) != 3 or not any(need):
        raise ValueError("%s: need = (attr, pos, w), at least one of them" % what)
    if need[2] and wv is None:
        raise ValueError("%s: a gradient for w needs w" % what)
    if not 0 <= int(max_span) <= TRIMESH_MAX_SPAN or not -1 <= int(orient) <= 1:
        raise ValueError("%s: max_span is 0 (no tear rule) or 1..%d, orient -1, 0 or 1" % (what, TRIMESH_MAX_SPAN))
    max_adders = int(max_adders)
    if max_adders < 1:
        raise ValueError("%s: max_adders must be at least 1" % what)
    n_sets = max(B, 1)
    lead = (B,) if B else ()
    nbytes = int(lib().lerf_coords_trimesh_bwd_workspace_bytes(F, V, Va, n_sets))
    if not nbytes or trimesh_max_items(F, n_sets, ohw, int(max_span)) > 0xffffffff:
        raise LerfError("%s: %d faces x %d sets into %d x %d are beyond the size rule (F <= 2^24 - 1 and the forward's)" % (what, F, n_sets, ohw[0], ohw[1]))
    g = X.grad(grad_out, lead + ohw + (2,), dev, what + ": grad_out")
    ga = X.grad(grad_attr, lead + (Va, 2), dev, what + ": grad_attr") if need[0] else None
    gp = X.grad(grad_pos, lead + (V, 2), dev, what + ": grad_pos") if need[1] else None
    gw = X.grad(grad_w, lead + (V,), dev, what + ": grad_w") if need[2] else None
    X.one_device(what, ("pos", "attr", "faces", "attr_faces", "depth", "w", "keys"), p, a, fc, af, d, wv, keys)
    ws = X.scratch(nbytes, dev)
    per = lambda t, base, n: 0 if t is None or t.ndim == base or B < 2 else n          # the set stride of a dense operand: 0 shares it
    own = lambda t, n: 0 if t is None or B < 2 else n
    X.run("lerf_coords_trimesh_bwd", B, p, (X.ptr(p), X.code(p), V, X.ptr(a), X.code(a), Va, X.ptr(fc), X.ptr(af), F, X.ptr(d), X.ptr(wv),
                                            LERF_F32 if wv is None else X.code(wv), ohw[0], ohw[1], int(origin[0]), int(origin[1]), int(max_span),
                                            int(orient), X.ptr(keys), X.ptr(g), X.ptr(ga), X.ptr(gp), X.ptr(gw), X.ptr(ws), nbytes, max_adders),
          (per(p, 2, 2 * V), per(a, 2, 2 * Va), per(fc, 2, 3 * F), per(af, 2, 3 * F), per(d, 1, V), per(wv, 1, V), own(keys, ohw[0] * ohw[1]),
           own(g, 2 * ohw[0] * ohw[1]), own(ga, 2 * Va), own(gp, 2 * V), own(gw, V)))
    most = X.max_count(ws)
    if raise_over and most > max_adders:
        raise LerfError("%s: %d face corners add into one vertex, more than max_adders = %d (that vertex holds NaN); raise max_adders"
                        % (what, most, max_adders))
    return ga, gp, gw, most


def _coords_bwd_operands(X, what, first, second, names, grad_out):
    """the two maps (or batches) of an adjoint and its upstream gradient, which has the second one's shape"""
    a, sa, ta, Ba = X.batch(first, names[0])
    b, sb, tb, Bb = X.batch(second, names[1])
    X.one_device(what, names, a, b)
    if Ba and not Bb:
        raise ValueError("%s: a batch of %s maps needs a batch of as many %s maps" % (what, names[0], names[1]))
    B = _one_batch(what, names, Ba, Bb)
    if grad_out is None:
        raise ValueError("%s: grad_out must be contiguous float64 [oH, oW, 2]" % what)
    return a, sa, ta, b, sb, tb, B, X.grad(grad_out, b.shape, X.device(b), what + ": grad_out")


def _dense_set(B, t):
    """the set stride of a contiguous float64 gradient: its maps are back to back (0: a single, shared one)"""
    return 0 if B < 2 or t is None or t.ndim == 3 else 2 * t.shape[-3] * t.shape[-2]


def coords_compose_bwd_on(X, outer, inner, grad_out, grad_outer, grad_inner, need, max_adders=None):
    """max_adders None: the atomic scatter; an int: the ORDERED scatter with that cap (run_ordered).  Ordered, with ONE outer map shared
    by a batch: every set scatters into a gradient of its own (a target has one owner) and grad_outer gains them one after the other,
    set 0 first -- a fixed order, so the result is reproducible (it is the host twin's sum only where that order does not matter)."""
    what = "lerf_coords_compose_bwd" + X.suffix
    a, sa, ta, b, sb, tb, B, g = _coords_bwd_operands(X, what, outer, inner, ("outer", "inner"), grad_out)
    if not (need[0] or need[1]):
        raise ValueError("%s: at least one of the two gradients is needed" % what)
    ga = X.grad(grad_outer, a.shape, X.device(b), what + ": grad_outer") if need[0] else None
    gb = X.grad(grad_inner, b.shape, X.device(b), what + ": grad_inner") if need[1] else None
    args = (*X.operand(a, sa), a.shape[-3], a.shape[-2], *X.operand(b, sb), X.ptr(g), b.shape[-3], b.shape[-2])
    if max_adders is None:
        X.run("lerf_coords_compose_bwd", B, b, args + (X.ptr(ga), X.ptr(gb)), (ta, tb, _dense_set(B, g), _dense_set(B, ga), _dense_set(B, gb)))
        return ga, gb
    per_set = ga is not None and B > 1 and a.ndim == 3
    gs = X.new((B,) + tuple(a.shape), X.f64, X.device(b), zero=True) if per_set else ga
    X.run_ordered("lerf_coords_compose_bwd", B, b, args + (X.ptr(gs), X.ptr(gb)), (ta, tb, _dense_set(B, g), _dense_set(B, gs), _dense_set(B, gb)),
                  b.shape[-3] * b.shape[-2], a.shape[-3] * a.shape[-2], max_adders)
    if per_set:
        for s in range(B):
            ga += gs[s]
    return ga, gb


def coords_invert_bwd_on(X, f, inverse, grad_out, grad_f, max_adders=None):
    what = "lerf_coords_invert_bwd" + X.suffix
    a, sa, ta, b, sb, tb, B, g = _coords_bwd_operands(X, what, f, inverse, ("f", "inverse"), grad_out)
    if B and a.ndim == 3:
        raise ValueError("%s: a batch of inverses needs a batch of as many maps f (grad_f has one writer per set)" % what)
    gf = X.grad(grad_f, a.shape, X.device(b), what + ": grad_f")
    args = (*X.operand(a, sa), a.shape[-3], a.shape[-2], *X.operand(b, sb), X.ptr(g), b.shape[-3], b.shape[-2], X.ptr(gf))
    if max_adders is None:
        X.run("lerf_coords_invert_bwd", B, b, args, (ta, tb, _dense_set(B, g), _dense_set(B, gf)))
    else:
        X.run_ordered("lerf_coords_invert_bwd", B, b, args, (ta, tb, _dense_set(B, g), _dense_set(B, gf)), b.shape[-3] * b.shape[-2],
                      a.shape[-3] * a.shape[-2], max_adders)
    return gf


DEPTH_KINDS = {"z": 0, "inverse": 1}          # LERF_DEPTH_Z, LERF_DEPTH_INVERSE
REPROJECT_PARAMS = 12                         # m[9] = K_dst . R . inv(K_src) row-major, q[3] = K_dst . t


def _reproject_operands(X, what, kind, params, depth):
    """(kind code, params, depth, B, depth's set stride, (H, W)): params float64 [12] with depth [H, W], or [B, 12] with depth [B, H, W] or
    one shared [H, W]; B = 0 for the single form"""
    if kind not in DEPTH_KINDS:
        raise ValueError("%s: kind is one of %s, not %r" % (what, ", ".join(DEPTH_KINDS), kind))
    if not X.is_array(params) or params.dtype != X.f64 or params.ndim not in (1, 2) or params.shape[-1] != REPROJECT_PARAMS or params.shape[0] < 1:
        raise ValueError("%s: params must be float64 %s [%d] or [B, %d]" % (what, X.noun, REPROJECT_PARAMS, REPROJECT_PARAMS))
    if not X.is_array(depth) or not X.is_float(depth) or depth.ndim not in (2, 3) or min(depth.shape) < 1:
        raise ValueError("%s: depth must be float32 or float64 %s [H, W] or [B, H, W]" % (what, X.noun))
    B = params.shape[0] if params.ndim == 2 else 0
    if depth.ndim == 3 and depth.shape[0] != B:
        raise ValueError("%s: a batch of depth planes [B, H, W] needs params [B, %d]" % (what, REPROJECT_PARAMS))
    X.one_device(what, ("params", "depth"), params, depth)
    hw = (int(depth.shape[-2]), int(depth.shape[-1]))
    return DEPTH_KINDS[kind], X.contiguous(params), X.contiguous(depth), B, (hw[0] * hw[1] if B > 1 and depth.ndim == 3 else 0), hw


def coords_reproject_on(X, kind, params, depth, dtype, out, origin, depth_out):
    what = "lerf_coords_reproject" + X.suffix
    code, p, d, B, d_set, hw = _reproject_operands(X, what, kind, params, depth)
    out, so, to = X.outs(out, B, hw, dtype, X.f64, X.device(d), what)
    X.one_device(what, ("depth", "out"), d, out)
    zo = None
    if depth_out is not None and depth_out is not False:
        zo = X.dense(None if depth_out is True else depth_out, ((B,) if B else ()) + hw, X.f32, X.device(d), what + ": depth_out")
    X.call(what, d, code, X.ptr(p), max(B, 1), X.ptr(d), X.code(d), d_set, X.ptr(out), X.code(out), to, so, X.ptr(zo),
           hw[0] * hw[1] if B > 1 else 0, hw[0], hw[1], int(origin[0]), int(origin[1]))
    return out if zo is None else (out, zo)


def coords_reproject_bwd_on(X, kind, params, depth, grad_map, grad_depth_out, grad_depth, grad_params, need, origin):
    what = "lerf_coords_reproject_bwd" + X.suffix
    code, p, d, B, d_set, hw = _reproject_operands(X, what, kind, params, depth)
    lead, dev = ((B,) if B else ()), X.device(d)
    if grad_map is None:
        raise ValueError("%s: grad_map must be contiguous float64 %s" % (what, list(lead + hw + (2,))))
    if not (need[0] or need[1]):
        raise ValueError("%s: at least one of the two gradients is needed" % what)
    g = X.grad(grad_map, lead + hw + (2,), dev, what + ": grad_map")
    gz = None if grad_depth_out is None else X.grad(grad_depth_out, lead + hw, dev, what + ": grad_depth_out")
    gd = X.grad(grad_depth, lead + hw, dev, what + ": grad_depth") if need[0] else None
    gp = X.grad(grad_params, tuple(p.shape), dev, what + ": grad_params") if need[1] else None
    ws = X.workspace(int(lib().lerf_coords_reproject_bwd_workspace_bytes(max(B, 1), hw[0], hw[1])) if need[1] else 0, dev)
    X.call(what, d, code, X.ptr(p), max(B, 1), X.ptr(d), X.code(d), d_set, X.ptr(g), X.ptr(gz), hw[0], hw[1], int(origin[0]), int(origin[1]),
           X.ptr(gd), X.ptr(gp), *ws)
    return gd, gp


def _splat_operands(X, what, src, fmap, weight):
    """(x, map, row stride, set stride, weight, B, C, (H, W), the call's leading arguments): src [C, H, W] or [B, C, H, W] float32 /
    float64, map [H, W, 2] (shared by the batch) or [B, H, W, 2], weight None or src's dtype [H, W] / [B, H, W]; B = 0 for the single form"""
    if not X.is_array(src) or not X.is_float(src) or src.ndim not in (3, 4) or min(src.shape) < 1:
        raise ValueError("%s: src must be float32 or float64 %s [C, H, W] or [B, C, H, W]" % (what, X.noun))
    x = X.contiguous(src)
    B = x.shape[0] if x.ndim == 4 else 0
    Cn, H, W = (int(v) for v in x.shape[-3:])
    f, sf, tf, Bf = X.batch(fmap, "map")
    if tuple(f.shape[-3:-1]) != (H, W) or (Bf and Bf != B):
        raise ValueError("%s: map must be [%d, %d, 2], one per sample or one for the batch" % (what, H, W))
    X.one_device(what, ("src", "map", "weight"), x, f, weight)
    m = None
    if weight is not None:
        if not X.is_array(weight) or weight.dtype != x.dtype or tuple(weight.shape) != ((B,) if B else ()) + (H, W):
            raise ValueError("%s: weight must be src's dtype, %s" % (what, list(((B,) if B else ()) + (H, W))))
        m = X.contiguous(weight)
    head = (X.ptr(x), X.code(x), Cn, H, W, Cn * H * W if B > 1 else 0, *X.operand(f, sf), tf if B > 1 else 0, X.ptr(m), H * W if B > 1 else 0)
    return x, f, m, B, Cn, (H, W), head


def splat_on(X, src, fmap, out_hw, weight=None, norm=False, acc=None, max_adders=None):
    """lerf_splat / lerf_splat_host: ADD src into acc [.., C (+ 1 with norm), oH, oW] along the forward map; acc None: a zeroed one.
    max_adders an int: lerf_splat_ordered / lerf_splat_ordered_host with that cap (run_ordered)"""
    what = "lerf_splat" + X.suffix
    x, f, m, B, Cn, hw, head = _splat_operands(X, what, src, fmap, weight)
    oH, oW = int(out_hw[0]), int(out_hw[1])
    if oH < 1 or oW < 1:
        raise ValueError("%s: out_hw must be positive" % what)
    planes = Cn + (1 if norm else 0)
    shape = ((B,) if B else ()) + (planes, oH, oW)
    if acc is None:
        acc = X.new(shape, x.dtype, X.device(x), zero=True)
    else:
        acc = X.dense(acc, shape, x.dtype, X.device(x), what + ": acc")
    args = (*head, X.ptr(acc), int(bool(norm)), oH, oW, planes * oH * oW if B > 1 else 0, max(B, 1))
    if max_adders is None:
        X.call(what, x, *args)
    else:
        X.run_ordered("lerf_splat", B, x, args, None, hw[0] * hw[1], oH * oW, max_adders)
    return acc


def splat_bwd_on(X, src, fmap, grad, weight=None, norm=False, need=(True, True, True)):
    """lerf_splat_bwd / lerf_splat_bwd_host: the adjoint of splat_on at grad [.., C (+ 1), oH, oW] (src's dtype, contiguous) ->
    (grad_src, grad_weight, grad_map): new buffers, None for a half that need[k] skips; grad_map float64 of the map's shape (a map
    shared by a batch: the sum over the samples)"""
    what = "lerf_splat_bwd" + X.suffix
    x, f, m, B, Cn, hw, head = _splat_operands(X, what, src, fmap, weight)
    planes, lead, dev = Cn + (1 if norm else 0), ((B,) if B else ()), X.device(x)
    if not X.is_array(grad) or grad.ndim != x.ndim or tuple(grad.shape[:-2]) != lead + (planes,) or min(grad.shape) < 1:
        raise ValueError("%s: grad must be %s ... [%d, oH, oW]" % (what, X.noun, planes))
    oH, oW = int(grad.shape[-2]), int(grad.shape[-1])
    g = X.dense(grad, lead + (planes, oH, oW), x.dtype, dev, what + ": grad")
    if not any(need):
        raise ValueError("%s: at least one of the three gradients is needed" % what)
    if need[1] and m is None:
        raise ValueError("%s: the weight's gradient needs a weight" % what)
    gx = X.new(tuple(x.shape), x.dtype, dev) if need[0] else None
    gm = X.new(lead + hw, x.dtype, dev) if need[1] else None
    gf = X.new(lead + hw + (2,), X.f64, dev) if need[2] else None
    n = hw[0] * hw[1]
    X.call(what, x, *head, X.ptr(g), int(bool(norm)), oH, oW, planes * oH * oW if B > 1 else 0, X.ptr(gx), Cn * n if B > 1 else 0, X.ptr(gm),
           n if B > 1 else 0, X.ptr(gf), 2 * n if B > 1 else 0, max(B, 1))
    if gf is not None and B and f.ndim == 3:
        gf = gf.sum(0)
    return gx, gm, gf


def coords_math_on(X, op, x, y):
    what = "lerf_coords_math" + X.suffix
    if op not in COORDS_MATH_OPS:
        raise ValueError("op is one of %s, not %r" % (", ".join(COORDS_MATH_OPS), op))
    if op == "atan2" and y is None:
        raise ValueError("%s: atan2 takes x and y" % what)
    a = X.float64(x, what)
    b = X.float64(y, what) if op == "atan2" else None
    if b is not None and (b.shape != a.shape or X.device(b) != X.device(a)):
        raise ValueError("%s: x and y must have one shape, on one device" % what)
    out = X.new(a.shape, X.f64, X.device(a))
    n = int(np.prod(a.shape, dtype=np.int64))
    if n:
        X.call(what, a, COORDS_MATH_OPS[op], X.ptr(a), X.ptr(b), n, X.ptr(out))
    return out


def coords_build_host(model, params, out_hw, dtype=np.float64, out=None, origin=(0, 0)):
    """lerf_coords_build_host: the map of a model built on the host by the kernels' own arithmetic (bit-equal to the device's)"""
    return coords_build_on(_HOST, model, params, out_hw, dtype, out, origin)


def coords_mesh_host(ctrl, out_hw, interp="bilinear", dtype=np.float64, out=None, origin=(0, 0), full_hw=None):
    """lerf_coords_mesh_host: ctrl [gh, gw, 2] float32 / float64 upsampled to the tile out_hw at `origin` of the map full_hw; a batch
    ctrl [B, gh, gw, 2] -> [B, oH, oW, 2] by one call of lerf_coords_mesh_batched_host"""
    return coords_mesh_on(_HOST, ctrl, out_hw, interp, dtype, out, origin, full_hw)


def coords_compose_host(outer, inner, dtype=np.float64, out=None):
    """lerf_coords_compose_host: C[i, j] = outer(inner[i, j]), host arrays under the strided map contract; a batch inner [B, oH, oW, 2]
    with outer [B, aH, aW, 2] or one shared [aH, aW, 2] -> [B, oH, oW, 2] by one call of lerf_coords_compose_batched_host"""
    return coords_compose_on(_HOST, outer, inner, dtype, out)


def coords_invert_host(f, out_hw, init=None, dtype=np.float64, out=None, origin=(0, 0), max_iter=16, tol=1e-9):
    """lerf_coords_invert_host: G[i, j] = the u with f(u) = origin + (i, j), f read bilinearly, by Newton's method from init[i, j]
    (None: the affine guess from three corners of f); NaN where f does not reach.  Host arrays under the strided map contract.  A batch
    f [B, fH, fW, 2] (init batched, shared or None) -> [B, oH, oW, 2] by one call of lerf_coords_invert_batched_host."""
    return coords_invert_on(_HOST, f, out_hw, init, dtype, out, origin, max_iter, tol)


def coords_invert_raster_host(f, out_hw, depth=None, dtype=np.float64, out=None, origin=(0, 0), max_span=16, orient=0, keys=None,
                              return_keys=False):
    """lerf_coords_invert_raster_host: the rasterising inverse of f [fH, fW, 2] into the tile out_hw at `origin` by the row-major host
    loop over the kernel's own per-triangle arithmetic (bit-equal to ops.coords_invert_raster in G and in keys).  depth: float32
    contiguous [fH, fW] or None; keys: a contiguous uint64 [oH, oW] workspace (None: a new one) -> G, or (G, keys) with
    return_keys=True: the winning keys, low 32 bits the triangle, all ones for a hole.  A batch f [B, fH, fW, 2] (depth [B, fH, fW], one
    shared [fH, fW] or None; keys [B, oH, oW], one plane per sample) -> [B, oH, oW, 2] by one call of lerf_coords_invert_raster_batched_host."""
    return coords_invert_raster_on(_HOST, f, out_hw, depth, dtype, out, origin, max_span, orient, keys, return_keys)


def coords_trimesh_host(pos, attr, faces, out_hw, attr_faces=None, depth=None, w=None, dtype=None, out=None, origin=(0, 0), max_span=0, orient=0,
                        keys=None, return_keys=False, return_depth=False):
    """lerf_coords_trimesh_host: the indexed triangle mesh (pos [V, 2], attr [Va, 2] float32 / float64; faces, attr_faces [F, 3] int32;
    depth [V] float32; w [V] float32 / float64) rasterised into the tile out_hw at `origin` by the plain loop over faces and their pixel boxes with the
    kernel's own per-face and per-pixel functions: bit-equal to ops.coords_trimesh in out, keys and depth.  -> out, or (out[, keys]
    [, depth_out]) with return_keys / return_depth.  dtype: out's, default attr's.  pos / attr [B, V, 2] (faces, attr_faces, depth, w
    batched alike or shared) -> [B, oH, oW, 2] by one call of lerf_coords_trimesh_batched_host."""
    return coords_trimesh_on(_HOST, pos, attr, faces, out_hw, attr_faces, depth, w, dtype, out, origin, max_span, orient, keys, return_keys,
                             return_depth)


def coords_trimesh_bwd_host(pos, attr, faces, out_hw, keys, grad_out, attr_faces=None, depth=None, w=None, origin=(0, 0), max_span=0, orient=0,
                            need=(True, True, False), grad_attr=None, grad_pos=None, grad_w=None, max_adders=4096, return_most=False):
    """lerf_coords_trimesh_bwd_host: the adjoint of coords_trimesh_host at fixed visibility by the kernel's own statement -- a
    256-slot array per face, the same tree, the same sorted lists per vertex: bit-equal to ops.coords_trimesh_bwd.  keys: the uint64 plane
    of the forward (return_keys=True); grad_out float64 of the map's shape; need = (attr, pos, w).  -> (grad_attr, grad_pos, grad_w)
    float64, ACCUMULATED INTO the ones given (None: zeroed ones), None where not needed; with return_most also the largest number of
    drawn face corners at one vertex.  A vertex above max_adders holds NaN in every component; nothing is raised here.  A batch:
    [B, ...] operands and keys [B, oH, oW]; every gradient then has the leading B, also for an operand the batch shares."""
    ga, gp, gw, most = coords_trimesh_bwd_on(_HOST, pos, attr, faces, out_hw, keys, grad_out, attr_faces, depth, w, origin, max_span, orient, need,
                                             grad_attr, grad_pos, grad_w, max_adders, False)
    return (ga, gp, gw, most) if return_most else (ga, gp, gw)


def coords_compose_bwd_host(outer, inner, grad_out, grad_outer=None, grad_inner=None, need=(True, True)):
    """lerf_coords_compose_bwd_host: ACCUMULATE the adjoint of compose(outer, inner) of the float64 grad_out [oH, oW, 2] into
    grad_outer [aH, aW, 2] and grad_inner [oH, oW, 2] (None: zeroed ones; need[k] False: that half is skipped and None is
    returned for it) -> (grad_outer, grad_inner).  A batch (inner and grad_out [B, oH, oW, 2]; outer [B, aH, aW, 2] or one shared
    [aH, aW, 2], whose gradient gains the sum over the samples in sample order) is one call of lerf_coords_compose_bwd_batched_host."""
    return coords_compose_bwd_on(_HOST, outer, inner, grad_out, grad_outer, grad_inner, need)


def coords_compose_bwd_ordered_host(outer, inner, grad_out, grad_outer=None, grad_inner=None, need=(True, True), max_adders=4096):
    """lerf_coords_compose_bwd_ordered_host: coords_compose_bwd_host by the four passes of the ordered scatter; the same bits"""
    return coords_compose_bwd_on(_HOST, outer, inner, grad_out, grad_outer, grad_inner, need, max_adders)


def coords_invert_bwd_host(f, inverse, grad_out, grad_f=None):
    """lerf_coords_invert_bwd_host: ACCUMULATE the implicit-function adjoint of inverse = invert(f) of the float64 grad_out
    [oH, oW, 2] into grad_f [fH, fW, 2] (None: a zeroed one).  A batch (every operand with a leading B) is one call of
    lerf_coords_invert_bwd_batched_host."""
    return coords_invert_bwd_on(_HOST, f, inverse, grad_out, grad_f)


def coords_invert_bwd_ordered_host(f, inverse, grad_out, grad_f=None, max_adders=4096):
    """lerf_coords_invert_bwd_ordered_host: coords_invert_bwd_host by the four passes of the ordered scatter; the same bits"""
    return coords_invert_bwd_on(_HOST, f, inverse, grad_out, grad_f, max_adders)


def coords_build_bwd_host(model, params, grad_map, origin=(0, 0)):
    """lerf_coords_build_bwd_host: the adjoint of the model builders on the host, in the device's summation order (bit-equal to it).
    params float64 [n] or [B, n] (n = COORDS_MODEL_PARAMS[model]), grad_map float64 [oH, oW, 2] or [B, oH, oW, 2] -> a NEW zeroed
    gradient of params' shape with the sums added (pre-filled buffers: the C entry point accumulates)."""
    if model not in COORDS_MODELS:
        raise ValueError("unknown coordinate-map model %r (known: %s)" % (model, ", ".join(COORDS_MODELS)))
    p = np.ascontiguousarray(np.asarray(params, dtype=np.float64))
    g = np.asarray(grad_map)
    if p.ndim not in (1, 2) or g.ndim != p.ndim + 2 or g.shape[-1] != 2 or (p.ndim == 2 and g.shape[0] != p.shape[0]):
        raise ValueError("lerf_coords_build_bwd_host: params is [n] with grad_map [oH, oW, 2], or [B, n] with [B, oH, oW, 2]")
    coords_model_count(model, p.shape[-1], "lerf_coords_build_bwd_host")
    if g.dtype != np.float64 or not g.flags.c_contiguous:
        raise ValueError("lerf_coords_build_bwd_host: grad_map must be a C-contiguous float64 array")
    out = np.zeros(p.shape, np.float64)
    check(lib().lerf_coords_build_bwd_host(COORDS_MODELS[model], p.ctypes.data, 1 if p.ndim == 1 else p.shape[0], p.shape[-1], g.ctypes.data,
                                           g.shape[-3], g.shape[-2], int(origin[0]), int(origin[1]), out.ctypes.data),
          "lerf_coords_build_bwd_host")
    return out


def coords_reproject_host(kind, params, depth, dtype=np.float64, out=None, origin=(0, 0), depth_out=None):
    """lerf_coords_reproject_host: the map that carries a view with a depth per pixel into another view, by the host loop over the
    kernel's own statements (bit-equal to ops.coords_reproject).  kind "z" (depth) or "inverse" (1 / depth); params float64 [12] =
    (K_dst . R . inv(K_src))[9], (K_dst . t)[3] with depth [H, W] float32 / float64, or [B, 12] with depth [B, H, W] or one shared
    [H, W] -> the map [H, W, 2] or [B, H, W, 2], (NaN, NaN) where the entry is not valid.  out: an array or a strided tile view, whose
    depth plane is the TILE's, at `origin` of the whole map.  depth_out: True or a float32 array of depth's shape -> (map, zo), zo the
    depth in the other view, what coords_invert_raster_host takes as depth."""
    return coords_reproject_on(_HOST, kind, params, depth, dtype, out, origin, depth_out)


def coords_reproject_bwd_host(kind, params, depth, grad_map, grad_depth_out=None, grad_depth=None, grad_params=None, need=(True, True),
                              origin=(0, 0)):
    """lerf_coords_reproject_bwd_host: ACCUMULATE the adjoint of coords_reproject_host of grad_map (float64 contiguous, the map's
    shape) and grad_depth_out (float64, zo's shape, or None) into grad_depth (float64, depth's batch shape) and grad_params (float64,
    params' shape); None: zeroed ones; need[k] False skips that half and returns None for it -> (grad_depth, grad_params).  The sums
    run in the device's order: bit-equal to ops.coords_reproject_bwd."""
    return coords_reproject_bwd_on(_HOST, kind, params, depth, grad_map, grad_depth_out, grad_depth, grad_params, need, origin)


def splat_host(src, map, out_hw, weight=None, norm=False, acc=None):
    """lerf_splat_host: the forward warp by summation splatting on the host, by the row-major loop over the kernel's own statements
    (csrc/lerf_splat_point.h).  src [C, H, W] or [B, C, H, W] float32 / float64; map [H, W, 2] (shared) or [B, H, W, 2], float32 / float64,
    map[i, j] = the (row, col) in the out_hw frame at which source pixel (i, j) lands; weight None or src's dtype [H, W] / [B, H, W]
    -> acc [.., C (+ 1 with norm: the plane of the weights), oH, oW] of src's dtype.  acc given: ACCUMULATED INTO and returned."""
    return splat_on(_HOST, src, map, out_hw, weight, norm, acc)


def splat_ordered_host(src, map, out_hw, weight=None, norm=False, acc=None, max_adders=4096):
    """lerf_splat_ordered_host: splat_host by the four passes of the ordered scatter (count, scan, fill, sort and sum); the same bits.
    LerfError when more than max_adders source pixels add into one output pixel (that pixel holds NaN in every plane)."""
    return splat_on(_HOST, src, map, out_hw, weight, norm, acc, max_adders)


def splat_bwd_host(src, map, grad, weight=None, norm=False, need=(True, True, True)):
    """lerf_splat_bwd_host: the adjoint of splat_host at grad [.., C (+ 1), oH, oW] -> (grad_src, grad_weight, grad_map), bit-equal to
    ops.splat_bwd; need[k] False skips that half (None); grad_map is float64"""
    return splat_bwd_on(_HOST, src, map, grad, weight, norm, need)


def coords_math_host(op, x, y=None):
    """lerf_coords_math_host: sqrt_pm(x), atan_pm(x) or atan2_pm(x, y) (op "sqrt", "atan", "atan2") of float64 arrays, element by element,
    by the HOST twin of the helpers the fisheye and equirect models are built on (csrc/lerf_coords_models.h: + - * / only, bit-equal to
    the device's ops.coords_math, a few ulp from numpy's) -> a new float64 array of x's shape"""
    return coords_math_on(_HOST, op, x, y)


# ------------------------------------------------------------------ device plumbing
_GPU_SEEN = None


def require_gpu():
    global _GPU_SEEN
    if _GPU_SEEN is not None:                       # a GPU that was there stays there: the hot call sites ask 200 times per frame
        return _GPU_SEEN
    import torch
    if not torch.cuda.is_available():
        raise LerfError("lerf-pytorch_amd needs an MI355X (gfx950) GPU: torch.cuda.is_available() is False "
                        "and there is no CPU fallback.")
    _GPU_SEEN = torch
    return torch


_TORCH_DT = None


def _dt(t):
    global _TORCH_DT
    import torch
    if _TORCH_DT is None:
        _TORCH_DT = {torch.uint8: LERF_U8, torch.float32: LERF_F32, torch.float64: LERF_F64, torch.int16: LERF_I16}
    return _TORCH_DT[t.dtype]


def plane(t, sy, sx, sc, offset=0):
    """Plane descriptor of torch tensor `t` (element strides)."""
    return Plane(t.data_ptr() + offset * t.element_size(), _dt(t), int(sy), int(sx), int(sc))


def current_stream(device=None):
    """torch's current stream of `device` (default: the current device) as a hipStream_t"""
    import torch
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)       # the handle without a Stream object (7 us less per launch)
    if raw is not None:
        if device is None:
            idx = torch.cuda.current_device()
        else:
            idx = torch.device(device).index
            idx = torch.cuda.current_device() if idx is None else idx
        return C.c_void_p(raw(idx))
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class on_device:
    """`with on_device(t):` -- the tensor's device is the current one for the launches inside (the library resolves
    per-device kernel attributes with hipGetDevice, and current_stream() then is the stream of THAT device); no-op for
    host tensors (pinned frames of stream.StreamingSR run on the caller's current device)."""

    def __init__(self, t):
        import torch
        self._g = None
        if getattr(t, "is_cuda", False) and t.device.index != torch.cuda.current_device():    # already current: nothing to switch
            self._g = torch.cuda.device(t.device)

    def __enter__(self):
        if self._g is not None:
            self._g.__enter__()
        return self

    def __exit__(self, *exc):
        if self._g is not None:
            return self._g.__exit__(*exc)
        return False
