"""Device operators: thin wrappers that hand torch-owned HBM buffers to the
C ABI on the current HIP stream.  torch is plumbing here (memory, streams);
all arithmetic happens in liblerf_hip.so.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import KINDS


def _torch():
    return _lib.require_gpu()


# --------------------------------------------------------------------------- geometry
class SrGeometry:
    """Separable SR geometry (Resize2dNumpy.set_shape, resize_right2d_numpy.py:18-140)
    as two 1-D tables per axis, resident on the device."""

    def __init__(self, in_hw, scale_factors=None, out_hw=None, support=2, device=None, arithmetic="f64", dis_scale=1.0,
                 pad_mode=0):
        """arithmetic: "f64" = the numpy classes' float64 tables (normative for the eval path); "torch32" = the
        float32 tables of the reference's torch classes (resize_right2d_torch.py:48-103), bit-equal to theirs.
        dis_scale: factor applied to the distances the weights see -- the anti-aliasing of the numpy Gaussian class
        for down-sampling (`min_scale_factor * dis`, resize_right2d_numpy.py:186-193); `support` is then the enlarged
        ceil(support / min_scale_factor) of :51-55 (the caller computes it, like the reference's set_scale_and_out_sz)."""
        torch = _torch()
        H, W = int(in_hw[0]), int(in_hw[1])
        if out_hw is not None and scale_factors is None:
            scale_factors = [out_hw[0] / H, out_hw[1] / W]                 # :28-31
        if not isinstance(scale_factors, (list, tuple)):
            scale_factors = [scale_factors, scale_factors]                 # :33-37
        sh, sw = float(scale_factors[0]), float(scale_factors[1])
        if not (sh > 0.0 and sw > 0.0):
            raise ValueError("scale factors must be positive")
        if not 1 <= int(support) <= _lib.LERF_MAX_SUPPORT:
            raise NotImplementedError("support size {} (after anti-aliasing enlargement) exceeds the kernels' maximum of {}"
                                      .format(support, _lib.LERF_MAX_SUPPORT))
        if out_hw is None:
            out_hw = (_lib.out_size(H, sh), _lib.out_size(W, sw))          # :41-45
        self.in_hw, self.out_hw, self.scales, self.S = (H, W), (int(out_hw[0]), int(out_hw[1])), (sh, sw), int(support)
        self.device = torch.device(device if device is not None else "cuda")
        self.pad_mode = int(pad_mode)                                        # LERF_PAD_* of the image operand (:208)
        tables = {"f64": _lib.sr_axis_tables, "torch32": _lib.sr_axis_tables_f32}[arithmetic]
        lr, dr64, dr32, pr = tables(H, self.out_hw[0], sh, self.S)
        lc, dc64, dc32, pc = tables(W, self.out_hw[1], sw, self.S)
        if float(dis_scale) != 1.0:
            dr64, dc64 = float(dis_scale) * dr64, float(dis_scale) * dc64
            dr32, dc32 = dr64.astype(np.float32), dc64.astype(np.float32)
        self.pad_vec = ((0, 0), pr, pc)                                     # :129
        self.host = dict(left_r=lr, dis_r=dr64, dis_r32=dr32, left_c=lc, dis_c=dc64, dis_c32=dc32)
        # exact x2 tables of lerf_sr_axis_tables on both axes: rows / columns pair up on their taps, distances have period 2 --
        # lets lerf_sr_fused_u8 take the persistent kernel (LERF_GEO_X2_TABLES; slices of these tables keep the property)
        if sh == 2.0 and sw == 2.0 and arithmetic == "f64" and float(dis_scale) == 1.0 and self.S == 2 \
                and self.out_hw == (2 * H, 2 * W):
            self.flags = _lib.GEO_X2_TABLES
        # the native builder's verdict on the tables just built: exact x2 of the WHOLE frame, any even support -- the promise
        # (LERF_GEO_EXACT_X2) that lets lerf_sr_fused_u8 take the X2 flavour of the tile-fused kernels.  Slices (row_slice,
        # block_slice) drop it: their owned ranges start at arbitrary origins and keep the table path.
        if arithmetic == "f64":
            self.flags = int(getattr(self, "flags", 0)) | _lib.sr_geometry_flags(self.in_hw, self.out_hw, self.scales, self.S,
                                                                                 lr, dr64, dr32, lc, dc64, dc32)
        self._upload()

    def _upload(self):
        torch = _torch()
        h = self.host
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self.t = dict(left_r=up(h["left_r"]), dis_r=up(h["dis_r32"]), left_c=up(h["left_c"]), dis_c=up(h["dis_c32"]),
                      dis_r64=up(h["dis_r"]), dis_c64=up(h["dis_c"]))
        g = _lib.SrGeo()
        g.S, g.out_h, g.out_w = self.S, self.out_hw[0], self.out_hw[1]
        g.pad_mode = getattr(self, "pad_mode", 0)
        g.tie_queue_cap = int(getattr(self, "tie_queue_cap", 0))
        g.roi_y, g.roi_x, g.roi_h, g.roi_w = getattr(self, "roi", (0, 0, 0, 0))
        g.flags = int(getattr(self, "flags", 0))
        for k in ("left_r", "dis_r", "left_c", "dis_c", "dis_r64", "dis_c64"):
            setattr(g, k, self.t[k].data_ptr())
        self.struct = g

    def with_tie_queue_cap(self, cap):
        """Test hook (lerf_sr_geo_t.tie_queue_cap): a copy of this geometry whose launches queue at most `cap` rounding
        ties per tile (0 entries: cap < 0 in the ABI; None restores the default) -- drives the in-loop fallback."""
        g = object.__new__(SrGeometry)
        g.__dict__.update(self.__dict__)
        g.tie_queue_cap = 0 if cap is None else (-1 if int(cap) == 0 else int(cap))
        g._upload()
        return g

    def with_flags(self, flags):
        """a copy of this geometry with `flags` added to lerf_sr_geo_t.flags (_lib.GEO_*: diagnostic A/B of the kernel families)"""
        g = object.__new__(SrGeometry)
        g.__dict__.update(self.__dict__)
        g.flags = int(getattr(self, "flags", 0)) | int(flags)
        g._upload()
        return g

    def _check_partition_pad(self):
        # a slice pads at the LOCAL frame borders: wrap padding would wrap inside the strip / block, and the far side of
        # the frame lives on another rank.  constant / edge / reflect / symmetric only reach pixels next to the global border,
        # which a slice that touches that border holds itself.
        if self.pad_mode == _lib.PAD_MODES["wrap"]:
            raise ValueError("strip / block partitions do not support pad_mode 'wrap' (the far side of the frame is on another rank)")

    def row_slice(self, lr_row0, lr_rows, out_row0, out_row1):
        """Geometry of a horizontal strip: the LR rows [lr_row0, lr_row0 + lr_rows) held locally
        (owned rows plus halo) produce the global output rows [out_row0, out_row1).  The row tables
        are the global ones, rebased to the strip -- the kernels never see the strip as a frame of
        its own, so non-integer scales partition exactly like integer ones."""
        self._check_partition_pad()
        g = object.__new__(SrGeometry)
        g.in_hw = (int(lr_rows), self.in_hw[1])
        g.out_hw = (int(out_row1 - out_row0), self.out_hw[1])
        g.scales, g.S, g.device, g.pad_vec = self.scales, self.S, self.device, self.pad_vec
        g.pad_mode = self.pad_mode
        g.flags = int(getattr(self, "flags", 0)) & ~_lib.GEO_EXACT_X2      # a slice is not the whole frame's tables
        h = self.host
        g.host = dict(left_r=(h["left_r"][out_row0:out_row1] - lr_row0).astype(np.int32),
                      dis_r=h["dis_r"][out_row0:out_row1], dis_r32=h["dis_r32"][out_row0:out_row1],
                      left_c=h["left_c"], dis_c=h["dis_c"], dis_c32=h["dis_c32"])
        g._upload()
        return g

    def block_slice(self, lr_row0, lr_rows, out_row0, out_row1, lr_col0, lr_cols, out_col0, out_col1, roi=None):
        """Geometry of a 2-D block: the LR rows [lr_row0, +lr_rows) x columns [lr_col0, +lr_cols) held locally (owned block
        plus halo) produce the global output rows [out_row0, out_row1) x columns [out_col0, out_col1).  Both axes' tables
        are the global ones rebased to the block.  roi = (y, x, h, w) of the OWNED block inside the local frame: the
        tile-fused kernel lays its tiles over it, so halo pixels only ever serve as tile halos."""
        g = self.row_slice(lr_row0, lr_rows, out_row0, out_row1)
        h = self.host
        g.in_hw = (int(lr_rows), int(lr_cols))
        g.out_hw = (int(out_row1 - out_row0), int(out_col1 - out_col0))
        g.host.update(left_c=(h["left_c"][out_col0:out_col1] - lr_col0).astype(np.int32),
                      dis_c=h["dis_c"][out_col0:out_col1], dis_c32=h["dis_c32"][out_col0:out_col1])
        if roi is not None:
            g.roi = tuple(int(v) for v in roi)
        g._upload()
        return g

    def ref(self):
        return C.byref(self.struct)


class WarpGeometry:
    """Homography geometry (Warp2dNumpy.set_shape, resize_right2d_numpy.py:292-407)."""

    def __init__(self, in_hw, matrix, out_hw, support=2, pad_mode=0, out_rect=None, src_y0=0):
        """out_rect = (i0, i1, j0, j1): the geometry of that rectangle of the output alone (`out_hw` stays the WHOLE output's: the
        pads come from its corner pixels); src_y0: the source operands hold the frame's rows from src_y0 on (a rank's band of a
        partitioned warp, dist.WarpRowPlan).  Same float64 arithmetic as the whole frame's, bit for bit."""
        m = np.asarray(matrix.detach().cpu().numpy() if hasattr(matrix, "detach") else matrix, dtype=np.float64)
        if m.shape != (3, 3):
            raise ValueError("matrix must be 3x3")
        self.matrix = m
        self.minv = np.linalg.inv(m)                                       # :327
        self.in_hw, self.out_hw, self.S = (int(in_hw[0]), int(in_hw[1])), (int(out_hw[0]), int(out_hw[1])), int(support)
        pads = _lib.warp_pads(self.minv, self.in_hw, self.out_hw, self.S)
        self.pad_vec = ((0, 0), (pads[0], pads[1]), (pads[2], pads[3]))    # :392
        g = _lib.WarpGeo()
        g.S, g.out_h, g.out_w = self.S, self.out_hw[0], self.out_hw[1]
        for i, v in enumerate(self.minv.reshape(9)):
            g.minv[i] = float(v)
        g.pad_r_lo, g.pad_r_hi, g.pad_c_lo, g.pad_c_hi = pads
        g.pad_mode = self.pad_mode = int(pad_mode)                          # LERF_PAD_* of the image operand (:560)
        self.full_out_hw = self.out_hw
        if out_rect is not None:
            i0, i1, j0, j1 = (int(v) for v in out_rect)
            if not (0 <= i0 < i1 <= self.out_hw[0] and 0 <= j0 < j1 <= self.out_hw[1]):
                raise ValueError("out_rect outside the output")
            g.out_y0, g.out_x0, g.out_h, g.out_w = i0, j0, i1 - i0, j1 - j0
            self.out_hw = (i1 - i0, j1 - j0)
        g.src_y0 = self.src_y0 = int(src_y0)
        self.struct = g

    def ref(self):
        return C.byref(self.struct)

    def tile_boxes(self, device):
        """int32 [tiles][4] on `device`: the output rows x columns that bound what each 64 x 64 source tile owns in the
        tile-fused warp (lerf_warp_tile_boxes: one host pass over the output per homography, kept with the geometry)"""
        torch = _torch()
        key = str(device)
        cache = self.__dict__.setdefault("_boxes", {})
        if key not in cache:
            H, W = self.in_hw
            nt = ((H + 63) // 64) * ((W + 63) // 64)
            b = np.zeros((nt, 4), dtype=np.int32)
            _lib.check(_lib.lib().lerf_warp_tile_boxes(self.ref(), H, W, b.ctypes.data), "lerf_warp_tile_boxes")
            cache[key] = (torch.from_numpy(b).to(device), b)
        return cache[key][0]


class RemapGeometry:
    """Dense-coordinate-map geometry (lerf_remap_geo_t): the warp with its projected grid read from `coords` instead of
    projected through a matrix.  coords: float64 / float32 [oH, oW, 2], entry (i, j) = (row, col) of the source position of
    output pixel (i, j), unclipped, integers = pixel indices (coords.py builds such maps).  A numpy array (or a host tensor)
    is uploaded once per device and kept with the geometry; a device tensor is used in place -- its last dimension must be
    contiguous and its column stride 2, its row stride is free (a tile of a larger map is a view of it).

    ONE MAP PER SAMPLE: coords [B, oH, oW, 2] (`batched`, `n_maps` = B) -- the planes or frames of a call are dealt to the maps
    in order, planes-per-map at a time, and the call returns what B calls with one map each return (lerf_remap*_batched: one
    launch).  The batch stride of a device tensor is free like the row stride: even, and for B > 1 at least one map's extent
    (oH - 1) * row stride + 2 * oW.  Each map has its own derived low pads."""

    def __init__(self, in_hw, coords, support=2, pad_mode=0, pads=None):
        """pads = (pad_r_lo, pad_c_lo): explicit low pads -- a tile of a larger map passes the WHOLE map's (whole.pads());
        None: the reference's, derived on the device from coords[0, 0] (calc_pad_sz, resize_right2d_numpy.py:363-369), of
        every map its own.  Explicit pads apply to every map of a batch."""
        self.in_hw, self.S, self.pad_mode = (int(in_hw[0]), int(in_hw[1])), int(support), int(pad_mode)
        if self.in_hw[0] < 1 or self.in_hw[1] < 1:
            raise ValueError("in_hw must be positive")
        dev = getattr(coords, "is_cuda", False)
        c = coords if dev else np.asarray(coords.detach().numpy() if hasattr(coords, "detach") else coords)
        if c.ndim not in (3, 4) or c.shape[-1] != 2 or any(n < 1 for n in c.shape[:-1]):
            raise ValueError("coords must be [oH, oW, 2] or [B, oH, oW, 2]")
        self.batched = c.ndim == 4
        self.n_maps = int(c.shape[0]) if self.batched else 1
        if dev:
            torch = _torch()
            c = c.detach()                   # the geometry reads the map's memory; its graph, if any, is the caller's (_RemapFn)
            if c.dtype not in (torch.float32, torch.float64):
                raise ValueError("coords must be float32 or float64")
            if c.stride(-1) != 1 or c.stride(-2) != 2 or c.stride(-3) % 2 or c.stride(-3) < 2 * c.shape[-2] \
                    or c.data_ptr() % (2 * c.element_size()):
                raise ValueError("device coords: contiguous (row, col) pairs, column stride 2, even row stride, entry-aligned")
            if self.batched and (c.stride(0) % 2 or c.stride(0) < 0 or
                                 (self.n_maps > 1 and c.stride(0) < (c.shape[1] - 1) * c.stride(1) + 2 * c.shape[2])):
                raise ValueError("device coords: even batch stride of at least one map's extent")
            self._host, self._dev = None, {str(c.device): c}
        else:
            if c.dtype not in (np.float32, np.float64):
                c = c.astype(np.float64)
            self._host, self._dev = np.ascontiguousarray(c), {}
        self.out_hw = (int(c.shape[-3]), int(c.shape[-2]))
        self.explicit_pads = None if pads is None else (int(pads[0]), int(pads[1]))
        if self.explicit_pads is not None and not all(0 <= p <= _lib.LERF_MAX_SUPPORT for p in self.explicit_pads):
            raise ValueError("pads must be non-negative low pads")

    def device_coords(self, device):
        key = str(device)
        if key not in self._dev:
            if self._host is None:
                raise ValueError("the coordinate map lives on %s, the operands on %s" % (next(iter(self._dev)), key))
            self._dev[key] = _torch().from_numpy(self._host).to(device)
        return self._dev[key]

    def struct(self, device):
        """(lerf_remap_geo_t of the map -- of map 0 of a batch --, the device tensor it points into)"""
        c = self.device_coords(device)
        g = _lib.RemapGeo()
        g.S, g.out_h, g.out_w = self.S, self.out_hw[0], self.out_hw[1]
        g.coords, g.coords_dtype, g.row_stride = c.data_ptr(), _lib._dt(c), c.stride(-3)
        g.pad_mode = self.pad_mode
        g.pad_r_lo, g.pad_c_lo = self.explicit_pads if self.explicit_pads is not None else (_lib.REMAP_PADS_FROM_MAP,) * 2
        return g, c

    def map_stride(self, device):
        """elements between consecutive maps of a batch on `device` (what lerf_remap*_batched take beside struct())"""
        if not self.batched:
            raise ValueError("one map: no batch stride")
        return int(self.device_coords(device).stride(0))

    def _first_entry(self):
        """the first entry of the map, [1, 1, 2] (of every map of a batch: [B, 1, 1, 2]), on the host"""
        if self._host is not None:
            return self._host[..., :1, :1, :]
        return next(iter(self._dev.values()))[..., :1, :1, :].cpu().numpy()

    def pads(self):
        """(pad_r_lo, pad_c_lo) the kernels use: the explicit ones, else derived from coords[0, 0] (host mirror of the kernels' rule).
        A batch: int32 [B, 2], one row per map."""
        if not self.batched:
            if self.explicit_pads is not None:
                return self.explicit_pads
            return _lib.remap_host_geometry(self._first_entry(), self.in_hw, self.S)[4]
        if self.explicit_pads is not None:
            return np.array([self.explicit_pads] * self.n_maps, dtype=np.int32)
        return np.array([_lib.remap_host_geometry(e, self.in_hw, self.S)[4] for e in self._first_entry()], dtype=np.int32)

    def host_geometry(self):
        """host mirror of the kernels' per-pixel geometry: (gr, gc, lr, lc, pads), see _lib.remap_host_geometry.  A batch: the
        per-map results stacked on a leading axis ([B, oH, oW] each, pads int32 [B, 2])."""
        c = self._host if self._host is not None else next(iter(self._dev.values())).cpu().numpy()
        if not self.batched:
            return _lib.remap_host_geometry(c, self.in_hw, self.S, self.explicit_pads)
        per = [_lib.remap_host_geometry(m, self.in_hw, self.S, self.explicit_pads) for m in c]
        return tuple(np.stack([p[k] for p in per]) for k in range(4)) + (np.array([p[4] for p in per], dtype=np.int32),)

    def rows(self, i0, i1):
        """the geometry of output rows [i0, i1) alone, with THIS map's pads (a view of the map, nothing is copied)"""
        if self.batched:
            raise ValueError("rows() of a batched map: every map has its own pads, and explicit pads apply to all maps of a call")
        if not 0 <= i0 < i1 <= self.out_hw[0]:
            raise ValueError("rows outside the map")
        src = self._host if self._host is not None else next(iter(self._dev.values()))
        return RemapGeometry(self.in_hw, src[i0:i1], self.S, self.pad_mode, pads=self.pads())


# --------------------------------------------------------------------------- helpers
def _planes_chw(t):
    """[N,H,W] contiguous-ish tensor -> Plane with channel = leading dim."""
    return _lib.plane(t, t.stride(1), t.stride(2), t.stride(0))


def _planes_hwc(t):
    return _lib.plane(t, t.stride(0), t.stride(1), t.stride(2))


def _out_dtype(name):
    torch = _torch()
    return {"u8": torch.uint8, "f32": torch.float32, "f64": torch.float64}[name]


# --------------------------------------------------------------------------- A1
def lut_interp_i16(img_u8_chw, h, w, dy, dx, lut_i8, interval=4):
    """int16 numerators [C,oC,h,w] (value * 2^interval) of one LUT pass (FourSimplexInterpFaster core)."""
    torch = _torch()
    if img_u8_chw.dtype != torch.uint8 or img_u8_chw.dim() != 3:
        raise ValueError("img must be uint8 [C,H,W]")
    if not 1 <= int(interval) <= 7:
        raise ValueError("interval must be 1..7")
    if lut_i8.dtype != torch.int8 or lut_i8.dim() != 2 or lut_i8.shape[0] != (2 ** (8 - int(interval)) + 1) ** 4:
        raise ValueError("lut must be int8 [L^4,oC] with L = 2^(8-interval) + 1")
    img = img_u8_chw.contiguous()
    lut = lut_i8.contiguous()
    Cn, Hp, Wp = img.shape
    oC = lut.shape[1]
    out = torch.empty((Cn, oC, h, w), dtype=torch.int16, device=img.device)
    dy = np.ascontiguousarray(dy, dtype=np.int8)
    dx = np.ascontiguousarray(dx, dtype=np.int8)
    p = _planes_chw(img)
    _lib.check(_lib.lib().lerf_lut_interp_i16(C.byref(p), Hp, Wp, Cn, int(h), int(w), dy.ctypes.data, dx.ctypes.data,
                                              lut.data_ptr(), oC, int(interval), out.data_ptr(), _lib.current_stream()),
               "lerf_lut_interp_i16")
    return out


INTERP_ACCUMULATE, INTERP_LDS, INTERP_DIRECT, INTERP_TILE64, INTERP_TILE32, INTERP_LUT_PLANAR = 1, 2, 4, 8, 16, 32     # LERF_INTERP_*
LUT_PLANE_BYTES = 83584                                                                             # LERF_LUT_PLANE_BYTES


def lut_planes(lut_i8):
    """[17^4, oC] int8 -> the LDS kernel's own layout, [oC, 83584] (LERF_INTERP_LUT_PLANAR): a workgroup then copies its plane
    alone instead of reading all oC interleaved bytes of every entry"""
    torch = _torch()
    n, oC = lut_i8.shape
    planes = torch.zeros((oC, LUT_PLANE_BYTES), dtype=torch.int8, device=lut_i8.device)
    planes[:, :n] = lut_i8.t()
    return planes



def lut_interp(img_chw, h, w, dy, dx, lut_i8, interval=4, rot=0, out_dtype=None, out=None, accumulate=False, kernel=None, planes=None):
    """One LUT pass with the reference's epilogue in the store (lerf_lut_interp_ex, ABI 7): img uint8 or float32 [C,Hp,Wp] (any
    strides) -> [C*oC, h', w'] = np.rot90(values, rot, [1, 2]) as float64 (default) / float32 VALUES (numerator / 2^interval),
    or the int16 numerators.  The rotation costs nothing: the kernel stores through the strides of the rotated view.
    out: a contiguous [C*oC, h', w'] tensor to write into; accumulate=True: out += result (the call sites' `pred += ...`).
    kernel: None (the library chooses), "lds", "lds64", "lds32" (the LDS kernel, its tile forced) or "direct" (tests, A/B runs).
    planes: lut_planes(lut_i8), handed to the LDS kernel when it takes the call (interval 4)."""
    torch = _torch()
    if img_chw.dtype not in (torch.uint8, torch.float32) or img_chw.dim() != 3:
        raise ValueError("img must be uint8 or float32 [C,H,W]")
    if not 1 <= int(interval) <= 7:
        raise ValueError("interval must be 1..7")
    if lut_i8.dtype != torch.int8 or lut_i8.dim() != 2 or lut_i8.shape[0] != (2 ** (8 - int(interval)) + 1) ** 4:
        raise ValueError("lut must be int8 [L^4,oC] with L = 2^(8-interval) + 1")
    out_dtype = out_dtype or (out.dtype if out is not None else torch.float64)
    if out_dtype not in (torch.float64, torch.float32, torch.int16):
        raise ValueError("out_dtype must be float64, float32 or int16")
    lut = lut_i8.contiguous()
    Cn, Hp, Wp = img_chw.shape
    oC = lut.shape[1]
    h, w, rot = int(h), int(w), int(rot) % 4
    oh, ow = (h, w) if rot % 2 == 0 else (w, h)
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs the tensor to add into (out=)")
        out = torch.empty((Cn * oC, oh, ow), dtype=out_dtype, device=img_chw.device)
    elif tuple(out.shape) != (Cn * oC, oh, ow) or out.dtype != out_dtype or not out.is_contiguous() or out.device != img_chw.device:
        raise ValueError("out must be a contiguous %s tensor of shape %r on the image's device" % (out_dtype, (Cn * oC, oh, ow)))
    flags = (INTERP_ACCUMULATE if accumulate else 0) | {None: 0, "lds": INTERP_LDS, "lds64": INTERP_LDS | INTERP_TILE64, "lds32": INTERP_LDS | INTERP_TILE32,
                                                      "direct": INTERP_DIRECT}[kernel]
    # element (y, x) of the un-rotated result lands at R = rot90(A, rot): rot 1: R[w-1-x, y]; 2: R[h-1-y, w-1-x]; 3: R[x, h-1-y]
    sy, sx, off = {0: (ow, 1, 0), 1: (1, -ow, (w - 1) * ow), 2: (-ow, -1, h * w - 1), 3: (-1, ow, ow - 1)}[rot]
    po = _lib.plane(out, sy, sx, oh * ow, offset=off)
    dy = np.ascontiguousarray(dy, dtype=np.int8)
    dx = np.ascontiguousarray(dx, dtype=np.int8)
    p = _planes_chw(img_chw)
    with _lib.on_device(out):
        if planes is not None and int(interval) == 4 and kernel != "direct" and oC > 1:
            if planes.dtype != torch.int8 or tuple(planes.shape) != (oC, LUT_PLANE_BYTES) or not planes.is_contiguous():
                raise ValueError("planes must be lut_planes(lut_i8)")
            rc = _lib.lib().lerf_lut_interp_ex(C.byref(p), Hp, Wp, Cn, h, w, dy.ctypes.data, dx.ctypes.data, planes.data_ptr(), oC,
                                               4, C.byref(po), flags | INTERP_LUT_PLANAR, _lib.current_stream())
            if rc != -2 or kernel is not None:             # LERF_EUNSUPPORTED: the direct kernel serves the call from the interleaved table
                _lib.check(rc, "lerf_lut_interp_ex")
                return out
        _lib.check(_lib.lib().lerf_lut_interp_ex(C.byref(p), Hp, Wp, Cn, h, w, dy.ctypes.data, dx.ctypes.data, lut.data_ptr(), oC,
                                                 int(interval), C.byref(po), flags, _lib.current_stream()), "lerf_lut_interp_ex")
    return out


EPI_DIV, EPI_MUL, EPI_ADD, EPI_CLIP, EPI_ROUND = 0, 1, 2, 3, 4     # LERF_EPI_* of include/lerf_hip.h


def numer_epilogue(acc_i16, interval, steps):
    """int16 numerators (value * 2^interval) -> float32, through a program of float64 steps [(EPI_*, a, b), ...] in numpy's
    order (lerf_numer_epilogue_f32): np.round(np.clip(pred / n + bias, 0, norm)).astype(np.float32) of the call sites"""
    torch = _torch()
    if acc_i16.dtype != torch.int16 or not acc_i16.is_contiguous() or len(steps) > 8:
        raise ValueError("acc must be a contiguous int16 tensor, at most 8 steps")
    out = torch.empty(acc_i16.shape, dtype=torch.float32, device=acc_i16.device)
    prog = (_lib.EpiOp * max(len(steps), 1))()
    for k, st in enumerate(steps):
        prog[k].op, prog[k].a, prog[k].b = int(st[0]), float(st[1]) if len(st) > 1 else 0.0, float(st[2]) if len(st) > 2 else 0.0
    with _lib.on_device(out):
        _lib.check(_lib.lib().lerf_numer_epilogue_f32(acc_i16.data_ptr(), acc_i16.numel(), int(interval), C.addressof(prog), len(steps),
                                                      out.data_ptr(), _lib.current_stream()), "lerf_numer_epilogue_f32")
    return out


# --------------------------------------------------------------------------- A2/A3
def lut_stages(img_u8_hwc, luts):
    """uint8 [H,W,C] -> (feat uint8 [H,W,C], hq uint8 [H,W,C,oC])."""
    torch = _torch()
    if img_u8_hwc.dtype != torch.uint8 or img_u8_hwc.dim() != 3:
        raise ValueError("img must be uint8 [H,W,C]")
    img = img_u8_hwc.contiguous()
    H, W, Cn = img.shape
    feat = torch.empty_like(img)
    hq = torch.empty((H, W, Cn, luts.oC), dtype=torch.uint8, device=img.device)
    pi = _planes_hwc(img)
    pf = _planes_hwc(feat)
    ph = _lib.plane(hq, hq.stride(0), hq.stride(1), hq.stride(2))
    _lib.check(_lib.lib().lerf_lut_stages_u8(C.byref(pi), H, W, Cn, luts.ref(), C.byref(pf), C.byref(ph),
                                             _lib.current_stream()), "lerf_lut_stages_u8")
    return feat, hq


def stages_packed(img_u8, luts, workspace=None):
    """uint8 [H,W,3] / [N,H,W,3] -> int32 [.., H,W,3] packed (hq0 | hq1<<8 | hq2<<16 | feat<<24) by the tile-fused
    stages kernel.  Raises LerfError(unsupported) for configurations it does not cover."""
    torch = _torch()
    if img_u8.dtype != torch.uint8:
        raise ValueError("img must be uint8")
    squeeze = img_u8.dim() == 3
    img = (img_u8.unsqueeze(0) if squeeze else img_u8).contiguous()
    N, H, W, Cn = img.shape
    packed = torch.empty((N, H, W, Cn), dtype=torch.int32, device=img.device)
    need = int(_lib.lib().lerf_sr_fused_workspace_bytes(H, W, Cn, N))
    if workspace is None:
        workspace = fused_workspace(H, W, Cn, N, img.device if img.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    elif workspace.dtype != torch.uint8 or workspace.numel() < need or not workspace.is_cuda or not workspace.is_contiguous():
        raise ValueError("workspace must be a contiguous uint8 device tensor of at least %d bytes" % need)
    with _lib.on_device(packed):
        _lib.check(_lib.lib().lerf_stages_packed_u8(img.data_ptr(), img.stride(0), N, H, W, Cn, luts.ref(),
                                                    packed.data_ptr(), packed.stride(0), workspace.data_ptr(), workspace.numel(),
                                                    _lib.current_stream()), "lerf_stages_packed_u8")
    return packed[0] if squeeze else packed


def stages_packed_ragged(imgs_u8, luts, workspace=None):
    """Frames of DIFFERENT sizes, one launch pair (lerf_stages_packed_ragged_u8): list of uint8 [H_i,W_i,C] device tensors
    -> list of int32 [H_i,W_i,C] packed stage outputs."""
    torch = _torch()
    if not imgs_u8:
        return []
    xs = [x.contiguous() for x in imgs_u8]
    Cn = xs[0].shape[-1]
    for x in xs:
        if x.dtype != torch.uint8 or x.dim() != 3 or x.shape[-1] != Cn or not x.is_cuda or x.device != xs[0].device:
            raise ValueError("ragged stages take uint8 [H,W,C] tensors of ONE device with one channel count")
    outs = [torch.empty(tuple(x.shape), dtype=torch.int32, device=x.device) for x in xs]
    items = (_lib.StageItem * len(xs))()
    for it, x, o in zip(items, xs, outs):
        it.img, it.packed, it.H, it.W = x.data_ptr(), o.data_ptr(), x.shape[0], x.shape[1]
    need = int(_lib.lib().lerf_stages_ragged_workspace_bytes(items, len(xs), Cn))
    if workspace is None:
        workspace = _cached_workspace(need, xs[0].device)
    elif workspace.dtype != torch.uint8 or workspace.numel() < need or not workspace.is_cuda or not workspace.is_contiguous():
        raise ValueError("workspace must be a contiguous uint8 device tensor of at least %d bytes" % need)
    with _lib.on_device(xs[0]):
        _lib.check(_lib.lib().lerf_stages_packed_ragged_u8(items, len(xs), Cn, luts.ref(), workspace.data_ptr(), workspace.numel(),
                                                           _lib.current_stream()), "lerf_stages_packed_ragged_u8")
    return outs


def unpack_stages(packed, oC):
    torch = _torch()
    feat = torch.empty(tuple(packed.shape), dtype=torch.uint8, device=packed.device)
    hq = torch.empty(tuple(packed.shape) + (oC,), dtype=torch.uint8, device=packed.device)
    p = packed.contiguous()
    _lib.check(_lib.lib().lerf_unpack_stages(p.data_ptr(), p.numel(), int(oC), feat.data_ptr(), hq.data_ptr(),
                                             _lib.current_stream()), "lerf_unpack_stages")
    return feat, hq


def _hyper_count(kind):
    """hyper-parameter maps of a kind: the fixed kernels (cubic, bilinear, ...) take none"""
    return {"gauss": 3, "linear": 1}.get(kind, 0)


def _packed_frames(packed):
    """packed int32 [H,W,C] or [N,H,W,C] -> ([N,H,W,C] with dense frames, whether the result drops the batch axis again)"""
    squeeze = packed.dim() == 3
    p = packed.unsqueeze(0) if squeeze else packed
    if not p[0].is_contiguous():
        p = p.contiguous()
    return p, squeeze


def _batched_out(out, oshape, squeeze, device):
    """`out` of the packed warps as [N,oH,oW,C]: "u8" / "f32" (a fresh tensor) or the caller's own, [oH,oW,C] for a 3-D input"""
    torch = _torch()
    if isinstance(out, str):
        return torch.empty(oshape, dtype=_out_dtype(out), device=device)
    o = out.unsqueeze(0) if (squeeze and out.dim() == 3) else out
    if tuple(o.shape) != oshape or o.dtype not in (torch.uint8, torch.float32) or o.device != device or o.stride(3) != 1:
        raise ValueError("out must be a uint8/float32 tensor of shape %s on the input's device" % (oshape[1:] if squeeze else oshape,))
    return o


def warp_packed(packed, geo: "WarpGeometry", kind="gauss", max_sigma=10.0, out="u8"):
    """packed: int32 [H,W,C] or a batch [N,H,W,C] sharing the homography (ONE launch for the batch).
    out: "u8" / "f32" (a fresh tensor) or a caller-owned uint8 / float32 tensor of the output shape to write into."""
    p, squeeze = _packed_frames(packed)
    N, Hb, W, Cn = p.shape
    H = geo.in_hw[0]                                        # the frame's height; `packed` may hold its rows from geo.src_y0 on only
    if W != geo.in_hw[1] or geo.src_y0 + Hb > H:
        raise ValueError("packed maps do not match the geometry's frame")
    o = _batched_out(out, (N, geo.out_hw[0], geo.out_hw[1], Cn), squeeze, p.device)
    po = _lib.plane(o, o.stride(1), o.stride(2), o.stride(3))
    _lib.check(_lib.lib().lerf_warp_packed(p.data_ptr(), p.stride(0), N, H, W, Cn, geo.ref(), KINDS[kind], float(max_sigma),
                                           C.byref(po), o.stride(0), _lib.current_stream()), "lerf_warp_packed")
    return o[0] if squeeze else o


def remap_packed(packed, geo: "RemapGeometry", kind="gauss", max_sigma=10.0, out="u8"):
    """warp_packed by a coordinate map (lerf_remap_packed): packed int32 [H,W,C] or a batch [N,H,W,C] sharing the map (ONE launch
    for the batch).  A batched geometry (one map per frame, lerf_remap_packed_batched): frame f reads map f, N == geo.n_maps, still
    one launch.  out: "u8" / "f32" (a fresh tensor) or a caller-owned uint8 / float32 tensor of the output shape."""
    p, squeeze = _packed_frames(packed)
    N, H, W, Cn = p.shape
    if (H, W) != geo.in_hw:
        raise ValueError("packed maps do not match the geometry's frame")
    if geo.batched and N != geo.n_maps:
        raise ValueError("%d frames for %d maps: a batched geometry takes one frame per map" % (N, geo.n_maps))
    o = _batched_out(out, (N, geo.out_hw[0], geo.out_hw[1], Cn), squeeze, p.device)
    po = _lib.plane(o, o.stride(1), o.stride(2), o.stride(3))
    g, _keep = geo.struct(p.device)
    if geo.batched:
        _lib.check(_lib.lib().lerf_remap_packed_batched(p.data_ptr(), p.stride(0), N, H, W, Cn, C.byref(g), geo.n_maps,
                                                        geo.map_stride(p.device), KINDS[kind], float(max_sigma), C.byref(po),
                                                        o.stride(0), _lib.current_stream()), "lerf_remap_packed_batched")
    else:
        _lib.check(_lib.lib().lerf_remap_packed(p.data_ptr(), p.stride(0), N, H, W, Cn, C.byref(g), KINDS[kind], float(max_sigma),
                                                C.byref(po), o.stride(0), _lib.current_stream()), "lerf_remap_packed")
    return o[0] if squeeze else o


def warp_fused_supported(img_u8, luts, geo: "WarpGeometry", kind="gauss", max_sigma=10.0):
    H, W, Cn = img_u8.shape[-3:]
    return bool(_lib.lib().lerf_warp_fused_supported(Cn, luts.ref(), geo.ref(), H, W, KINDS[kind], float(max_sigma)))


def warp_fused_u8(img_u8, luts, geo: "WarpGeometry", kind="gauss", max_sigma=10.0, out=None, workspace=None):
    """The whole warp path tile-fused (lerf_warp_fused_u8): uint8 [H,W,3] or a batch [N,H,W,3] sharing the homography ->
    uint8 [.., oH, oW, 3]; stage 1 into the workspace, then stage 2 + the warp per source tile -- no packed maps in HBM."""
    torch = _torch()
    if img_u8.dtype != torch.uint8:
        raise ValueError("img must be uint8")
    squeeze = img_u8.dim() == 3
    img = (img_u8.unsqueeze(0) if squeeze else img_u8).contiguous()
    N, H, W, Cn = img.shape
    oshape = (N, geo.out_hw[0], geo.out_hw[1], Cn)
    if out is None:
        o = torch.empty(oshape, dtype=torch.uint8, device=img.device)
    else:
        o = out.unsqueeze(0) if (squeeze and out.dim() == 3) else out
        if tuple(o.shape) != oshape or o.dtype != torch.uint8 or not o.is_contiguous() or o.device != img.device:
            raise ValueError("out must be a contiguous uint8 tensor of shape %s on the input's device" % (oshape,))
    need = int(_lib.lib().lerf_sr_fused_workspace_bytes(H, W, Cn, N))
    if workspace is None:
        workspace = fused_workspace(H, W, Cn, N, img.device)
    elif workspace.dtype != torch.uint8 or workspace.numel() < need or not workspace.is_cuda or not workspace.is_contiguous():
        raise ValueError("workspace must be a contiguous uint8 device tensor of at least %d bytes" % need)
    boxes = geo.tile_boxes(img.device)
    with _lib.on_device(o):
        _lib.check(_lib.lib().lerf_warp_fused_u8(img.data_ptr(), img.stride(0), N, H, W, Cn, luts.ref(), geo.ref(), boxes.data_ptr(),
                                                 KINDS[kind], float(max_sigma), o.data_ptr(), o.stride(0), workspace.data_ptr(),
                                                 workspace.numel(), _lib.current_stream()), "lerf_warp_fused_u8")
    return o[0] if squeeze else o


# --------------------------------------------------------------------------- A5/A6/A8
def _hyper_planes(hyper, layout, nh):
    arr = (_lib.Plane * 3)()
    keep = []
    if layout == "hwck":          # one uint8 tensor [H,W,C,oC]
        hq = hyper
        for k in range(3):
            arr[k] = _lib.plane(hq, hq.stride(0), hq.stride(1), hq.stride(2), offset=(k if k < nh else 0) * hq.stride(3))
        keep.append(hq)
    else:                          # separate planar [N,H,W] tensors with identical strides
        for k in range(3):
            t = hyper[k if k < nh else 0]
            arr[k] = _planes_chw(t)
        keep.extend(hyper)
    return arr, keep


def _stage3_hwc(call, feat, hq_u8, kind, geo, out, match=False):
    """One stage-3 launch on the uint8 stage outputs: feat [H,W,C] (contiguous), hq [H,W,C,oC] -> a fresh [oH,oW,C].  `call` takes
    the image, hyper and output planes; the operands live until it returns.  match: hq must have feat's shape (the SR contract)"""
    torch = _torch()
    nh = _hyper_count(kind)
    o = torch.empty((geo.out_hw[0], geo.out_hw[1], feat.shape[2]), dtype=_out_dtype(out), device=feat.device)
    pf = _planes_hwc(feat)
    ph = None
    if nh:
        hq = hq_u8.contiguous()
        if match and (hq.shape[:3] != feat.shape or hq.shape[3] < nh):
            raise ValueError("hyper shape mismatch")
        ph, _keep = _hyper_planes(hq, "hwck", nh)
    call(pf, ph, _planes_hwc(o))
    return o


def _stage3_planar(call, feat, hypers, kind, geo, out, match=False):
    """The same on planar float32 maps: feat [N,H,W] (contiguous float32), hypers = list of [N,H,W] -> a fresh [N,oH,oW]"""
    torch = _torch()
    nh = _hyper_count(kind)
    o = torch.empty((feat.shape[0], geo.out_hw[0], geo.out_hw[1]), dtype=_out_dtype(out), device=feat.device)
    pf = _planes_chw(feat)
    ph = None
    if nh:
        hypers = [h.contiguous().float() for h in hypers[:nh]]
        for h in hypers:
            if match and h.shape != feat.shape:
                raise ValueError("hyper maps must have the shape of the input")
        ph, _keep = _hyper_planes(hypers, "planar", nh)
    call(pf, ph, _planes_chw(o))
    return o


def _resize_call(geo, H, W, planes, kind, max_sigma):
    return lambda pf, ph, po: _lib.check(_lib.lib().lerf_resize(C.byref(pf), ph, H, W, planes, geo.ref(), KINDS[kind], float(max_sigma),
                                                                C.byref(po), _lib.current_stream()), "lerf_resize")


def _warp_call(geo, H, W, planes, kind, max_sigma):
    return lambda pf, ph, po: _lib.check(_lib.lib().lerf_warp(C.byref(pf), ph, H, W, planes, geo.ref(), KINDS[kind], float(max_sigma),
                                                              C.byref(po), _lib.current_stream()), "lerf_warp")


def resize_hwc_u8(feat_u8, hq_u8, geo: SrGeometry, kind="gauss", max_sigma=10.0, out="u8"):
    """stage 3 on the uint8 stage outputs: feat [H,W,C], hq [H,W,C,oC] -> [oH,oW,C]."""
    feat = feat_u8.contiguous()
    H, W, Cn = feat.shape
    return _stage3_hwc(_resize_call(geo, H, W, Cn, kind, max_sigma), feat, hq_u8, kind, geo, out, match=True)


def resize_planar(feat, hypers, geo: SrGeometry, kind="gauss", max_sigma=10.0, out="f32"):
    """stage 3 on planar float32 maps: feat [N,H,W], hypers = list of [N,H,W] in [0,1] -> [N,oH,oW]."""
    feat = feat.contiguous().float()
    N, H, W = feat.shape
    return _stage3_planar(_resize_call(geo, H, W, N, kind, max_sigma), feat, hypers, kind, geo, out, match=True)


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else None)


def _bwd_inputs(feat, hypers, kind, grad_out, double):
    """the tensors a stage-3 backward reads: contiguous float32 planes and the upstream gradient in the forward's output type"""
    feat = feat.contiguous().float()
    hs = [h.contiguous().float() for h in hypers[:_hyper_count(kind)]]
    g = grad_out.contiguous()
    return feat, hs, g.double() if double else g.float()


def _bwd_buffers(feat, hs, g, geo, grads):
    """checks grad_out and the gradient buffers of a stage-3 backward -> (grads padded to four, operands, gradients): the two
    argument runs every lerf_*_bwd prototype shares, in its order --
    operands = (feat, h0, h1, h2, N, H, W), before the geometry; gradients = (grad_out, grad_feat, grad_h0, grad_h1, grad_h2),
    after kind and max_sigma"""
    N, H, W = feat.shape
    if tuple(g.shape) != (N, geo.out_hw[0], geo.out_hw[1]):
        raise ValueError("grad_out must be [N, out_h, out_w] of the geometry")
    grads = list(grads) + [None] * (4 - len(grads))
    for t in grads:
        if t is not None and (t.dtype != feat.dtype or tuple(t.shape) != (N, H, W) or not t.is_contiguous()):
            raise ValueError("gradient buffers must be contiguous float32 [N, H, W]")
    hp = [_ptr(h) for h in hs] + [C.c_void_p(None)] * (3 - len(hs))
    return grads, (_ptr(feat), hp[0], hp[1], hp[2], N, H, W), (_ptr(g),) + tuple(_ptr(t) for t in grads)


def resize_bwd_planar(feat, hypers, geo: SrGeometry, kind, max_sigma, grad_out, grads):
    """lerf_resize_bwd_f32: accumulate the gradients of resize_planar(feat, hypers, geo, kind, max_sigma, out="f32") for the
    float32 upstream gradient `grad_out` [N, oH, oW] into `grads` = [grad_feat, grad_h0, grad_h1, grad_h2] (float32
    [N, H, W] contiguous tensors, or None to skip a map; the fixed kinds have grad_feat alone).  feat / hypers: float32
    [N, H, W].  The image gradient follows geo.pad_mode."""
    feat, hs, g = _bwd_inputs(feat, hypers, kind, grad_out, double=False)
    grads, operands, gradients = _bwd_buffers(feat, hs, g, geo, grads)
    _lib.check(_lib.lib().lerf_resize_bwd_f32(*operands, geo.ref(), KINDS[kind], float(max_sigma), *gradients, _lib.current_stream()),
               "lerf_resize_bwd_f32")
    return grads


def resize_planar_u8(feat_u8, hq_u8, geo: SrGeometry, kind="gauss", max_sigma=10.0):
    """stage 3 on planar uint8 maps: feat [N,H,W] (any strides), hq = list of uint8 numerator maps [N,H,W] with identical
    strides (hyper = hq / 255) -> uint8 [oH,oW,N] = clip(rne(value), 0, 255): the production arithmetic of the fused path"""
    torch = _torch()
    nh = {"gauss": 3, "linear": 1}[kind]
    N, H, W = feat_u8.shape
    hq = [h.contiguous() for h in hq_u8[:nh]]
    if feat_u8.dtype != torch.uint8 or any(h.dtype != torch.uint8 or h.shape != feat_u8.shape for h in hq):
        raise ValueError("uint8 maps of the input's shape")
    o = torch.empty((geo.out_hw[0], geo.out_hw[1], N), dtype=torch.uint8, device=feat_u8.device)
    pf = _planes_chw(feat_u8)
    ph, _keep = _hyper_planes(hq, "planar", nh)
    po = _planes_hwc(o)
    with _lib.on_device(o):
        _resize_call(geo, H, W, N, kind, max_sigma)(pf, ph, po)
    return o


def warp_hwc_u8(feat_u8, hq_u8, geo: WarpGeometry, kind="gauss", max_sigma=10.0, out="u8"):
    feat = feat_u8.contiguous()
    Hb, W, Cn = feat.shape
    H = geo.in_hw[0]                                        # (a band of the frame from geo.src_y0 on: see WarpGeometry)
    if W != geo.in_hw[1] or geo.src_y0 + Hb > H:
        raise ValueError("the maps do not match the geometry's frame")
    return _stage3_hwc(_warp_call(geo, H, W, Cn, kind, max_sigma), feat, hq_u8, kind, geo, out)


def warp_planar(feat, hypers, geo: WarpGeometry, kind="gauss", max_sigma=10.0, out="f32"):
    feat = feat.contiguous().float()
    N, H, W = feat.shape
    return _stage3_planar(_warp_call(geo, H, W, N, kind, max_sigma), feat, hypers, kind, geo, out)


def _remap_call(geo, device, H, W, planes, kind, max_sigma):
    """lerf_remap, or lerf_remap_batched for a geometry with one map per sample (`planes` = n_maps * planes per map), on the image,
    hyper and output planes"""
    def call(pf, ph, po):
        g, _keepc = geo.struct(device)
        if geo.batched:
            if planes % geo.n_maps:
                raise ValueError("%d planes for %d maps: every map takes the same number of planes" % (planes, geo.n_maps))
            _lib.check(_lib.lib().lerf_remap_batched(C.byref(pf), ph, H, W, planes, C.byref(g), geo.n_maps, geo.map_stride(device),
                                                     planes // geo.n_maps, KINDS[kind], float(max_sigma), C.byref(po),
                                                     _lib.current_stream()), "lerf_remap_batched")
        else:
            _lib.check(_lib.lib().lerf_remap(C.byref(pf), ph, H, W, planes, C.byref(g), KINDS[kind], float(max_sigma),
                                             C.byref(po), _lib.current_stream()), "lerf_remap")
    return call


def remap_hwc_u8(feat_u8, hq_u8, geo: RemapGeometry, kind="gauss", max_sigma=10.0, out="u8"):
    """warp_hwc_u8 by a coordinate map (lerf_remap).  A batched geometry (one map per frame, lerf_remap_batched): feat
    [N,H,W,C], hq [N,H,W,C,oC], N == geo.n_maps -> [N,oH,oW,C] in ONE launch.  The C ABI strides planes by one step, so the
    frames are interleaved for it ([H,W,N,C]: plane n * C + c) and the output is copied back to frame-major."""
    torch = _torch()
    if geo.batched:
        nh = _hyper_count(kind)
        if feat_u8.dim() != 4 or feat_u8.shape[0] != geo.n_maps:
            raise ValueError("a batched geometry takes [N,H,W,C] frames, one per map (N = %d)" % geo.n_maps)
        N, H, W, Cn = feat_u8.shape
        if (H, W) != geo.in_hw:
            raise ValueError("the maps do not match the geometry's frame")
        feat = feat_u8.permute(1, 2, 0, 3).contiguous().view(H, W, N * Cn)
        o = torch.empty((geo.out_hw[0], geo.out_hw[1], N * Cn), dtype=_out_dtype(out), device=feat.device)
        if nh:
            if hq_u8.dim() != 5 or tuple(hq_u8.shape[:4]) != (N, H, W, Cn) or hq_u8.shape[4] < nh:
                raise ValueError("hyper shape mismatch")
            hq = hq_u8.permute(1, 2, 0, 3, 4).contiguous().view(H, W, N * Cn, hq_u8.shape[4])
            ph, _keep = _hyper_planes(hq, "hwck", nh)
        else:
            ph = None
        _remap_call(geo, feat.device, H, W, N * Cn, kind, max_sigma)(_planes_hwc(feat), ph, _planes_hwc(o))
        return o.view(geo.out_hw[0], geo.out_hw[1], N, Cn).permute(2, 0, 1, 3).contiguous()
    feat = feat_u8.contiguous()
    H, W, Cn = feat.shape
    if (H, W) != geo.in_hw:
        raise ValueError("the maps do not match the geometry's frame")
    return _stage3_hwc(_remap_call(geo, feat.device, H, W, Cn, kind, max_sigma), feat, hq_u8, kind, geo, out)


def remap_planar(feat, hypers, geo: RemapGeometry, kind="gauss", max_sigma=10.0, out="f32"):
    """warp_planar by a coordinate map (lerf_remap): float32 [N,H,W] planes -> [N,oH,oW].  A batched geometry (lerf_remap_batched):
    N = geo.n_maps * P, planes [b * P, (b + 1) * P) read map b."""
    feat = feat.contiguous().float()
    N, H, W = feat.shape
    if (H, W) != geo.in_hw:
        raise ValueError("the maps do not match the geometry's frame")
    if geo.batched and N % geo.n_maps:
        raise ValueError("%d planes for %d maps: every map takes the same number of planes" % (N, geo.n_maps))
    return _stage3_planar(_remap_call(geo, feat.device, H, W, N, kind, max_sigma), feat, hypers, kind, geo, out)


def warp_bwd_planar(feat, hypers, geo: WarpGeometry, kind, max_sigma, grad_out, grads):
    """lerf_warp_bwd: accumulate the gradients of warp_planar(feat, hypers, geo, kind, max_sigma, out="f64") for the
    float64 upstream gradient `grad_out` [N, oH, oW] into `grads` = [grad_feat, grad_h0, grad_h1, grad_h2] (float32
    [N, H, W] contiguous tensors, or None to skip a map).  feat / hypers: float32 [N, H, W]."""
    feat, hs, g = _bwd_inputs(feat, hypers, kind, grad_out, double=True)
    grads, operands, gradients = _bwd_buffers(feat, hs, g, geo, grads)
    _lib.check(_lib.lib().lerf_warp_bwd(*operands, geo.ref(), KINDS[kind], float(max_sigma), *gradients, _lib.current_stream()),
               "lerf_warp_bwd")
    return grads


def remap_bwd_planar(feat, hypers, geo: RemapGeometry, kind, max_sigma, grad_out, grads, grad_coords=None):
    """lerf_remap_bwd: accumulate the gradients of remap_planar(feat, hypers, geo, kind, max_sigma, out="f64") for the
    float64 upstream gradient `grad_out` [N, oH, oW] into `grads` = [grad_feat, grad_h0, grad_h1, grad_h2] (float32
    [N, H, W] contiguous tensors, or None to skip a map) and, when given, the map gradient into `grad_coords` (float64
    [N, oH, oW, 2] contiguous, PER PLANE: the caller sums over the planes that share the map).  feat / hypers: float32
    [N, H, W].  A batched geometry (lerf_remap_bwd_batched): N = geo.n_maps * P, planes [b * P, (b + 1) * P) read map b."""
    torch = _torch()
    feat, hs, g = _bwd_inputs(feat, hypers, kind, grad_out, double=True)
    N, H, W = feat.shape
    if (H, W) != geo.in_hw:
        raise ValueError("the maps do not match the geometry's frame")
    if geo.batched and N % geo.n_maps:
        raise ValueError("%d planes for %d maps: every map takes the same number of planes" % (N, geo.n_maps))
    grads, operands, gradients = _bwd_buffers(feat, hs, g, geo, grads)
    if grad_coords is not None and (grad_coords.dtype != torch.float64 or tuple(grad_coords.shape) != (N,) + tuple(geo.out_hw) + (2,)
                                    or not grad_coords.is_contiguous()):
        raise ValueError("grad_coords must be contiguous float64 [N, out_h, out_w, 2]")
    gs, _keepc = geo.struct(feat.device)
    if geo.batched:
        _lib.check(_lib.lib().lerf_remap_bwd_batched(*operands, C.byref(gs), geo.n_maps, geo.map_stride(feat.device), N // geo.n_maps,
                                                     KINDS[kind], float(max_sigma), *gradients, _ptr(grad_coords),
                                                     _lib.current_stream()), "lerf_remap_bwd_batched")
    else:
        _lib.check(_lib.lib().lerf_remap_bwd(*operands, C.byref(gs), KINDS[kind], float(max_sigma), *gradients, _ptr(grad_coords),
                                             _lib.current_stream()), "lerf_remap_bwd")
    return grads


# --------------------------------------------------------------------------- fused SR
_WS = {}
_WS_MAX = 8


def _cached_workspace(need, device):
    """Scratch of at least `need` bytes, cached per (device, stream): launches on ONE stream are ordered, so the previous call
    on that stream has consumed the buffer; another stream (or thread with its own stream) gets a buffer of its own instead
    of racing for this one."""
    torch = _torch()
    need = max(int(need), 1)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    # the stream the launch will use: every launch below runs inside `_lib.on_device(tensor)` and passes
    # _lib.current_stream() of that device -- the same call that forms this key
    key = (device.index, int(torch.cuda.current_stream(device).cuda_stream))
    ws = _WS.pop(key, None)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=device)
    _WS[key] = ws                      # most recently used last
    while len(_WS) > _WS_MAX:          # streams come and go (stream handles are recycled): keep the cache bounded
        _WS.pop(next(iter(_WS)))
    return ws


def fused_workspace(H, W, Cn, N, device):
    """Device scratch of lerf_sr_fused_workspace_bytes() bytes for the two-launch fused path (stage-1 output of the
    batch between s1_kernel and the stage-2/3 launch), cached per device AND stream and grown on demand."""
    return _cached_workspace(int(_lib.lib().lerf_sr_fused_workspace_bytes(H, W, Cn, N)), device)


def _gpu_visible(t):
    """device memory, or pinned host memory (the kernels read / write it over PCIe: stream.StreamingSR)"""
    return t.is_cuda or t.is_pinned()


def _check_out_u8(out, shape, device, what, pitched=False):
    """frames may be strided (dim 0); each frame is dense HWC -- or, with pitched=True, HWC rows at a pitch >= W * C bytes
    (a view [:, :, :W] of a wider tensor: lerf_sr_geo_t.out_row_pitch)"""
    torch = _torch()
    if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != tuple(shape):
        raise ValueError("%s must be a uint8 tensor of shape %s" % (what, tuple(shape)))
    if not _gpu_visible(out):
        raise ValueError("%s must live in device memory or pinned host memory" % what)
    exp = 1
    for d in range(out.dim() - 1, 0, -1):
        if out.shape[d] != 1 and out.stride(d) != exp:
            if pitched and d == out.dim() - 3 and out.stride(d) > exp:
                exp = out.stride(d)                     # the row pitch
            else:
                raise ValueError("%s: every frame must be contiguous [H,W,C]%s" % (what, " (rows may be pitched)" if pitched else ""))
        exp *= out.shape[d]


def sr_fused_u8(img_u8, luts, geo: SrGeometry, kind="gauss", max_sigma=10.0, out=None, workspace=None):
    """uint8 [H,W,C] or [N,H,W,C] -> uint8 [oH,oW,C] / [N,oH,oW,C].  Two launches per call (stage 1 over the batch into
    the workspace, then stages 2+3 per tile); `out` (same rank as the input) and `workspace` may be caller-owned.
    workspace=False: ONE launch, every tile recomputes stage 1 on its halo -- the better choice for a single frame or
    block that fills the chip once (no workspace, no second launch)."""
    torch = _torch()
    if img_u8.dtype != torch.uint8:
        raise ValueError("img must be uint8")
    squeeze = img_u8.dim() == 3
    img = (img_u8.unsqueeze(0) if squeeze else img_u8)
    if img.dim() != 4:
        raise ValueError("img must be [H,W,C] or [N,H,W,C]")
    if not img[0].is_contiguous():
        img = img.contiguous()
    N, H, W, Cn = img.shape
    if (H, W) != geo.in_hw:
        raise ValueError("geometry was built for another input size")
    oshape = (N, geo.out_hw[0], geo.out_hw[1], Cn)
    if not _gpu_visible(img):
        raise ValueError("img must live in device memory or pinned host memory")
    dev = img.device if img.is_cuda else torch.device("cuda", torch.cuda.current_device())
    if out is None:
        o4 = torch.empty(oshape, dtype=torch.uint8, device=dev)
    else:
        o4 = out.unsqueeze(0) if (squeeze and out.dim() == 3) else out
        _check_out_u8(o4, oshape, img.device, "out", pitched=True)
    need = int(_lib.lib().lerf_sr_fused_workspace_bytes(H, W, Cn, N))
    if workspace is False:
        ws_ptr, ws_n = None, 0
    else:
        if workspace is None:
            workspace = fused_workspace(H, W, Cn, N, dev)
        elif workspace.dtype != torch.uint8 or workspace.numel() < need or not workspace.is_cuda or not workspace.is_contiguous():
            raise ValueError("workspace must be a contiguous uint8 device tensor of at least %d bytes" % need)
        ws_ptr, ws_n = workspace.data_ptr(), workspace.numel()
    # where the frames live travels with the call (no hipPointerGetAttributes per launch)
    gs = _lib.SrGeo.from_buffer_copy(geo.struct)
    gs.flags |= _lib.GEO_INPUT_DEVICE if img.is_cuda else _lib.GEO_INPUT_HOST
    if o4.shape[1] > 1 and o4.stride(1) != oshape[2] * Cn:
        gs.out_row_pitch = int(o4.stride(1))         # rows of a wider tensor (dist.sr_block pads a block's rows to 16 bytes)
    with _lib.on_device(o4):
        _lib.check(_lib.lib().lerf_sr_fused_u8(img.data_ptr(), img.stride(0), N, H, W, Cn, luts.ref(), C.byref(gs),
                                               KINDS[kind], float(max_sigma), o4.data_ptr(), o4.stride(0),
                                               ws_ptr, ws_n, _lib.current_stream()), "lerf_sr_fused_u8")
    return o4[0] if squeeze else o4


def sr_fused_supported(Cn, luts, geo: SrGeometry, kind="gauss", max_sigma=10.0):
    """True when lerf_sr_fused_u8 takes the tile-fused kernels for this configuration (else: the three direct kernels)."""
    return bool(_lib.lib().lerf_sr_fused_supported(int(Cn), luts.ref(), geo.ref(), geo.in_hw[0], geo.in_hw[1], KINDS[kind],
                                                   float(max_sigma)))


def sr_fused_ragged_u8(imgs_u8, luts, geos, kind="gauss", max_sigma=10.0, workspace=None):
    """Frames of DIFFERENT sizes through one launch pair (lerf_sr_fused_ragged_u8): lists of uint8 [H_i,W_i,C] device
    tensors and their SrGeometry -> list of uint8 [oH_i,oW_i,C].  What the reference's harness does image by image over a
    benchmark folder (eval_lut_sr.py:489-512)."""
    torch = _torch()
    if len(imgs_u8) != len(geos) or not imgs_u8:
        raise ValueError("one geometry per image")
    xs = [x.contiguous() for x in imgs_u8]
    Cn = xs[0].shape[-1]
    for x, g in zip(xs, geos):
        if x.dtype != torch.uint8 or x.dim() != 3 or x.shape[-1] != Cn or not x.is_cuda or x.device != xs[0].device:
            raise ValueError("ragged SR takes uint8 [H,W,C] tensors of ONE device with one channel count")
        if g.device != xs[0].device and (g.device.index is not None or xs[0].device.index != torch.cuda.current_device()):
            raise ValueError("the geometry tables live on another device than the frames")
        if tuple(x.shape[:2]) != g.in_hw:
            raise ValueError("geometry was built for another input size")
    outs = [torch.empty((g.out_hw[0], g.out_hw[1], Cn), dtype=torch.uint8, device=x.device) for x, g in zip(xs, geos)]
    items = (_lib.SrItem * len(xs))()
    for it, x, o, g in zip(items, xs, outs, geos):
        it.img, it.out, it.H, it.W, it.geo = x.data_ptr(), o.data_ptr(), x.shape[0], x.shape[1], g.struct
    need = int(_lib.lib().lerf_sr_ragged_workspace_bytes(items, len(xs), Cn))
    if workspace is None:
        workspace = _cached_workspace(need, xs[0].device)
    elif workspace.dtype != torch.uint8 or workspace.numel() < need or not workspace.is_cuda or not workspace.is_contiguous():
        raise ValueError("workspace must be a contiguous uint8 device tensor of at least %d bytes" % need)
    with _lib.on_device(xs[0]):
        _lib.check(_lib.lib().lerf_sr_fused_ragged_u8(items, len(xs), Cn, luts.ref(), KINDS[kind], float(max_sigma),
                                                      workspace.data_ptr(), workspace.numel(), _lib.current_stream()),
                   "lerf_sr_fused_ragged_u8")
    return outs


def rect_copy(frames_u8, staging_u8, rects, to_staging):
    """lerf_rect_copy_u8: rectangles (y, x, h, w, byte offset in staging) of a dense uint8 batch [N,fh,fw,C] <-> one
    contiguous staging tensor, ONE launch (halo pack / unpack of dist.BlockBuffer)."""
    torch = _torch()
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or not frames_u8.is_contiguous() or not staging_u8.is_contiguous():
        raise ValueError("frames must be a dense uint8 [N,fh,fw,C] tensor, staging contiguous")
    if not 1 <= len(rects) <= _lib.LERF_MAX_RECTS:
        raise ValueError("1..%d rectangles" % _lib.LERF_MAX_RECTS)
    N, fh, fw, Cn = frames_u8.shape
    arr = (_lib.Rect * len(rects))()
    for a, (y, x, h, w, off) in zip(arr, rects):
        a.y, a.x, a.h, a.w, a.off = int(y), int(x), int(h), int(w), int(off)
        if off + N * h * w * Cn > staging_u8.numel():
            raise ValueError("staging buffer too small")
    with _lib.on_device(frames_u8):
        _lib.check(_lib.lib().lerf_rect_copy_u8(frames_u8.data_ptr(), N, fh, fw, Cn, staging_u8.data_ptr(), arr, len(rects),
                                                1 if to_staging else 0, _lib.current_stream()), "lerf_rect_copy_u8")


def patch_batch(pool_u8, desc, C_out, sz, hsz, noise=None, desc_dev=None, im=None, lb=None):
    """lerf_patch_batch_u8: the DIV2K training batch (im [B,C,sz,sz], lb [B,C,hsz,hsz], float32) cut from a device pool of
    uint8 HWC images in ONE launch.  `desc`: a numpy record array of _lib.PATCH_DESC_DTYPE, checked on the host and uploaded
    here (or already on the device as `desc_dev`, uint8 [B * 72]); `noise`: device float32 [B,C,sz,sz] added to im."""
    torch = _torch()
    if pool_u8.dtype != torch.uint8 or not pool_u8.is_cuda or not pool_u8.is_contiguous():
        raise ValueError("the pool must be a contiguous uint8 tensor on the GPU")
    desc = np.ascontiguousarray(desc, dtype=_lib.PATCH_DESC_DTYPE).reshape(-1)
    B = int(desc.shape[0])
    dev = pool_u8.device
    if desc_dev is None:
        desc_dev = torch.from_numpy(desc.view(np.uint8)).to(dev)
    if noise is not None and (noise.dtype != torch.float32 or noise.device != dev or not noise.is_contiguous()
                              or tuple(noise.shape) != (B, C_out, sz, sz)):
        raise ValueError("noise must be a contiguous float32 [B,C,sz,sz] tensor on the pool's device")
    if im is None:
        im = torch.empty((B, C_out, sz, sz), dtype=torch.float32, device=dev)
    if lb is None:
        lb = torch.empty((B, C_out, hsz, hsz), dtype=torch.float32, device=dev)
    with _lib.on_device(pool_u8):
        _lib.check(_lib.lib().lerf_patch_batch_u8(pool_u8.data_ptr(), pool_u8.numel(), desc_dev.data_ptr(), desc.ctypes.data, B,
                                                  int(C_out), int(sz), int(hsz), noise.data_ptr() if noise is not None else None,
                                                  im.data_ptr(), lb.data_ptr(), _lib.current_stream()), "lerf_patch_batch_u8")
    return im, lb


# --------------------------------------------------------------------------- coordinate maps on the device
def coords_build(model, params, out_hw, dtype=None, out=None, origin=(0, 0), device=None):
    """lerf_coords_build: the map [oH, oW, 2] of `model` ("homography": the 9 entries of the INVERSE matrix; "radial": cr, cc,
    no, ni, hr, hc, k1, k2; "brown": inv(new_K . R)[9], fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6; "fisheye": inv(new_K . R)[9],
    fx, fy, cx, cy, k1, k2, k3, k4; "equirect": inv(K_view . R)[9], sx, sy, cxp, cyp) written by the kernel.
    out: a device tensor or a strided tile view of a larger map, built in place at `origin` = (i0, j0) of the whole map; else a
    new tensor of `dtype` (default float64) on `device` (default: the current one)."""
    X = _lib.DeviceOperands()
    dev = out.device if out is not None else X.torch.device("cuda", X.torch.cuda.current_device()) if device is None else X.torch.device(device)
    return _lib.coords_build_on(X, model, params, out_hw, dtype, out, origin, dev)


def _params_tensor(model, params, what):
    """(model code, detached contiguous float64 device tensor [n] or [B, n]) of a model's parameters held on the device"""
    torch = _torch()
    if model not in _lib.COORDS_MODELS:
        raise ValueError("unknown coordinate-map model %r (known: %s)" % (model, ", ".join(_lib.COORDS_MODELS)))
    n = _lib.COORDS_MODEL_PARAMS[model]
    if not isinstance(params, torch.Tensor) or not params.is_cuda or params.dtype != torch.float64 or params.ndim not in (1, 2) \
            or params.shape[-1] != n or params.shape[0] < 1:
        raise ValueError("%s: params must be a float64 device tensor [%d] or [B, %d] for model %r" % (what, n, n, model))
    return _lib.COORDS_MODELS[model], params.detach().contiguous()


def coords_build_params(model, params, out_hw, dtype=None, out=None, origin=(0, 0)):
    """lerf_coords_build_dev: coords_build with the parameters read from DEVICE memory -- params float64 [n] -> the map
    [oH, oW, 2], or [B, n] -> [B, oH, oW, 2], one map per parameter set in ONE launch; no host round trip, no sync.  Map b is
    bit-equal to coords_build of the same doubles.  Non-finite parameters are not refused (the host does not see them).  out: a
    device tensor of that shape or a strided tile view of a larger buffer, built in place at `origin`; else a new tensor of
    `dtype` (default float64) on params' device."""
    torch = _torch()
    code, p = _params_tensor(model, params, "lerf_coords_build_dev")
    oH, oW = int(out_hw[0]), int(out_hw[1])
    B = 1 if p.ndim == 1 else int(p.shape[0])
    if out is None:
        dtype = torch.float64 if dtype is None else dtype
        if oH < 1 or oW < 1:
            raise ValueError("lerf_coords_build_dev: out_hw must be positive")
        if dtype not in (torch.float32, torch.float64):
            raise ValueError("lerf_coords_build_dev: dtype is torch.float32 or torch.float64")
        out = torch.empty(((oH, oW, 2) if p.ndim == 1 else (B, oH, oW, 2)), dtype=dtype, device=p.device)
    elif not isinstance(out, torch.Tensor) or out.ndim != p.ndim + 2 or tuple(out.shape[-3:]) != (oH, oW, 2) or (p.ndim == 2 and out.shape[0] != B):
        raise ValueError("lerf_coords_build_dev: out must be %s" % ("[%d, %d, 2]" % (oH, oW) if p.ndim == 1 else "[%d, %d, %d, 2]" % (B, oH, oW)))
    elif out.device != p.device:
        raise ValueError("lerf_coords_build_dev: params and out live on different devices")
    _, stride = _lib.DeviceOperands().map(out if p.ndim == 1 else out[0], "out")
    set_stride = 0 if p.ndim == 1 else int(out.stride(0))
    with _lib.on_device(out):
        _lib.check(_lib.lib().lerf_coords_build_dev(code, p.data_ptr(), B, int(p.shape[-1]), out.data_ptr(), _lib._dt(out), set_stride, stride,
                                                    oH, oW, int(origin[0]), int(origin[1]), _lib.current_stream(out.device)),
                   "lerf_coords_build_dev")
    return out


def coords_build_bwd(model, params, grad_map, grad_params=None, origin=(0, 0)):
    """lerf_coords_build_bwd: ACCUMULATE the adjoint of coords_build_params(model, params) of grad_map (float64 contiguous
    [oH, oW, 2], or [B, oH, oW, 2] for params [B, n]) into grad_params (float64 contiguous, params' shape; None: a zeroed one):
    d loss / d every entry of the parameter vector.  An entry whose forward point is not finite contributes nothing.  Two
    launches, fixed summation order, no atomics: two calls on the same input are bit-equal, and equal to
    _lib.coords_build_bwd_host."""
    torch = _torch()
    code, p = _params_tensor(model, params, "lerf_coords_build_bwd")
    g = grad_map
    if not isinstance(g, torch.Tensor) or not g.is_cuda or g.dtype != torch.float64 or g.ndim != p.ndim + 2 or g.shape[-1] != 2 \
            or not g.is_contiguous() or g.shape[-3] < 1 or g.shape[-2] < 1 or (p.ndim == 2 and g.shape[0] != p.shape[0]):
        raise ValueError("lerf_coords_build_bwd: grad_map must be a contiguous float64 device tensor [oH, oW, 2] ([B, oH, oW, 2] for "
                         "params [B, n])")
    if g.device != p.device:
        raise ValueError("lerf_coords_build_bwd: params and grad_map live on different devices")
    if grad_params is None:
        grad_params = torch.zeros(tuple(p.shape), dtype=torch.float64, device=g.device)
    elif not isinstance(grad_params, torch.Tensor) or grad_params.dtype != torch.float64 or tuple(grad_params.shape) != tuple(p.shape) \
            or not grad_params.is_contiguous() or grad_params.device != g.device:
        raise ValueError("lerf_coords_build_bwd: grad_params must be contiguous float64 of params' shape on grad_map's device")
    B, n, oH, oW = (1 if p.ndim == 1 else int(p.shape[0])), int(p.shape[-1]), int(g.shape[-3]), int(g.shape[-2])
    need = int(_lib.lib().lerf_coords_build_bwd_workspace_bytes(n, B, oH, oW))
    with _lib.on_device(g):
        ws = _cached_workspace(need, g.device)
        _lib.check(_lib.lib().lerf_coords_build_bwd(code, p.data_ptr(), B, n, g.data_ptr(), oH, oW, int(origin[0]), int(origin[1]),
                                                    grad_params.data_ptr(), ws.data_ptr(), ws.numel(), _lib.current_stream(g.device)),
                   "lerf_coords_build_bwd")
    return grad_params


def coords_math(op, x, y=None):
    """lerf_coords_math: sqrt_pm(x), atan_pm(x) or atan2_pm(x, y) (op "sqrt", "atan", "atan2") of float64 device tensors, one thread per
    element: the helpers the fisheye and equirect models are built on, bit-equal to _lib.coords_math_host -> a new float64 tensor of
    x's shape on x's device"""
    return _lib.coords_math_on(_lib.DeviceOperands(), op, x, y)


def coords_mesh(ctrl, out_hw, interp="bilinear", dtype=None, out=None, origin=(0, 0), full_hw=None):
    """lerf_coords_mesh: the control mesh ctrl [gh, gw, 2] (device, float32 / float64, absolute source positions at vertices
    placed align-corners over the map full_hw, default out_hw) upsampled to the tile out_hw at `origin`; interp "bilinear" or
    "bicubic" (Keys A = -0.75, clamped border taps).  dtype: the map's, default ctrl's.  A batch ctrl [B, gh, gw, 2] gives
    [B, oH, oW, 2] in one launch (lerf_coords_mesh_batched), map s bit-equal to the single call on ctrl[s]; out may be a strided
    batch view (its batch stride becomes the set stride)."""
    return _lib.coords_mesh_on(_lib.DeviceOperands(), ctrl, out_hw, interp, dtype, out, origin, full_hw)


def coords_mesh_bwd(grad_map, ctrl_hw, interp="bilinear", grad_ctrl=None):
    """lerf_coords_mesh_bwd: ACCUMULATE the adjoint of coords_mesh (whole map) of the float64 contiguous grad_map [oH, oW, 2] into
    grad_ctrl (float64 contiguous [gh, gw, 2]; None: a zeroed one).  Deterministic: two calls on the same input are bit-equal.
    A batch grad_map [B, oH, oW, 2] gives grad_ctrl [B, gh, gw, 2] in ONE call of lerf_coords_mesh_bwd_batched (its two launches
    cover every sample; the workspace holds B row passes), sample s bit-equal to the single-map call."""
    torch = _torch()
    gh, gw = int(ctrl_hw[0]), int(ctrl_hw[1])
    code = _lib.mesh_interp_code(interp)
    g = grad_map
    if not isinstance(g, torch.Tensor) or not g.is_cuda or g.ndim not in (3, 4) or g.shape[-1] != 2 or g.dtype != torch.float64 \
            or not g.is_contiguous() or g.shape[0] < 1:
        raise ValueError("lerf_coords_mesh_bwd: grad_map must be a contiguous float64 device tensor [oH, oW, 2] or [B, oH, oW, 2]")
    if gh < 2 or gw < 2:
        raise ValueError("lerf_coords_mesh_bwd: the control mesh is at least 2 x 2")
    lead = tuple(g.shape[:-3])
    if grad_ctrl is None:
        grad_ctrl = torch.zeros(lead + (gh, gw, 2), dtype=torch.float64, device=g.device)
    elif grad_ctrl.dtype != torch.float64 or tuple(grad_ctrl.shape) != lead + (gh, gw, 2) or not grad_ctrl.is_contiguous() \
            or grad_ctrl.device != g.device:
        raise ValueError("lerf_coords_mesh_bwd: grad_ctrl must be contiguous float64 %s on grad_map's device" % (list(lead + (gh, gw, 2)),))
    oH, oW = int(g.shape[-3]), int(g.shape[-2])
    B = lead[0] if lead else 1
    need = B * int(_lib.lib().lerf_coords_mesh_bwd_workspace_bytes(gh, gw, oH, oW))
    with _lib.on_device(g):
        ws = _cached_workspace(need, g.device)
        if lead:
            _lib.check(_lib.lib().lerf_coords_mesh_bwd_batched(g.data_ptr(), oH, oW, code, gh, gw, grad_ctrl.data_ptr(), ws.data_ptr(), ws.numel(),
                                                               B, 2 * oH * oW if B > 1 else 0, 2 * gh * gw if B > 1 else 0,
                                                               _lib.current_stream(g.device)), "lerf_coords_mesh_bwd_batched")
        else:
            _lib.check(_lib.lib().lerf_coords_mesh_bwd(g.data_ptr(), oH, oW, code, gh, gw, grad_ctrl.data_ptr(), ws.data_ptr(), ws.numel(),
                                                       _lib.current_stream(g.device)), "lerf_coords_mesh_bwd")
    return grad_ctrl


def coords_compose(outer, inner, dtype=None, out=None):
    """lerf_coords_compose: C[i, j] = outer(inner[i, j]) -- the outer map sampled bilinearly at the positions the inner map
    holds, so remap(remap(img, outer), inner) and remap(img, C) describe the same geometry.  Device maps under the strided
    contract, any mix of float32 / float64; dtype: C's, default inner's.  A batch inner [B, oH, oW, 2] with outer [B, aH, aW, 2] or
    one shared [aH, aW, 2] gives [B, oH, oW, 2] in one launch (lerf_coords_compose_batched)."""
    return _lib.coords_compose_on(_lib.DeviceOperands(), outer, inner, dtype, out)


def coords_invert(f, out_hw, init=None, dtype=None, out=None, origin=(0, 0), max_iter=16, tol=1e-9):
    """lerf_coords_invert: G[i, j] = the position u with f(u) = origin + (i, j), f [fH, fW, 2] read as its bilinear interpolant
    (compose's rule), by Newton's method per entry from init[i, j] (None: the affine guess from three corners of f), at most
    max_iter passes, stopped at max |f(u) - target| <= tol; (NaN, NaN) where f does not reach, folds, or holds a NaN in the cell
    read.  out_hw: the size of the frame f points into.  Device maps under the strided contract (tile views of f, init and out
    with `origin` = the tile's place in the whole inverse), any mix of float32 / float64; dtype: G's, default f's.  One launch on
    the current stream, no sync.  A batch f [B, fH, fW, 2] (init [B, oH, oW, 2], one shared [oH, oW, 2] or None; a single f with a
    batch of inits is shared too) gives [B, oH, oW, 2] in the same one launch (lerf_coords_invert_batched)."""
    return _lib.coords_invert_on(_lib.DeviceOperands(), f, out_hw, init, dtype, out, origin, max_iter, tol)


def coords_invert_raster(f, out_hw, depth=None, dtype=None, out=None, origin=(0, 0), max_span=16, orient=0, keys=None, return_keys=False):
    """lerf_coords_invert_raster: the inverse of f [fH, fW, 2] read as its PIECEWISE-LINEAR interpolant over two triangles a cell, by
    rasterising every triangle into the tile out_hw at `origin` with a depth test: for maps that fold or tear, where coords_invert
    gives NaN.  Where several triangles cover a pixel the smallest depth wins (depth: float32 contiguous [fH, fW] on f's device;
    None: the lowest triangle); a triangle whose pixel box is wider than max_span (1..64) is a tear and fills nothing; orient +1 /
    -1 culls triangles of the other orientation (+1: the identity's), 0 keeps both; (NaN, NaN) where nothing lands.  keys: an int64
    contiguous [oH, oW] workspace on f's device (None: a new one), which holds the winning 64-bit keys afterwards -- low 32 bits the
    triangle, -1 (all ones) for a hole.  -> G, or (G, keys) with return_keys=True.  Device maps under the strided contract, any mix
    of float32 / float64; dtype: G's, default f's.  Three launches on the current stream, no sync; bit-equal from run to run and to
    _lib.coords_invert_raster_host.  A batch f [B, fH, fW, 2] (depth [B, fH, fW], one shared [fH, fW] or None) gives [B, oH, oW, 2] in
    the same three launches (lerf_coords_invert_raster_batched); keys is then [B, oH, oW]: ONE KEY PLANE PER SAMPLE, 8 bytes per
    output pixel per sample."""
    return _lib.coords_invert_raster_on(_lib.DeviceOperands(), f, out_hw, depth, dtype, out, origin, max_span, orient, keys, return_keys)


def coords_trimesh(pos, attr, faces, out_hw, attr_faces=None, depth=None, w=None, dtype=None, out=None, origin=(0, 0), max_span=0, orient=0,
                   keys=None, return_keys=False, return_depth=False):
    """lerf_coords_trimesh: an indexed triangle mesh rasterised into the tile out_hw at `origin` of a coordinate map.  pos [V, 2]:
    the (row, col) of every vertex in the output frame; attr [Va, 2]: what the map holds there (the source position), float32 or
    float64 each; faces [F, 3] int32 indices into pos; attr_faces [F, 3] int32 indices into attr (None: faces); depth [V] float32:
    the smallest interpolated depth wins a pixel (None: the lowest face); w [V] float32 or float64: perspective-correct interpolation of attr
    (a face with a w <= 0 is skipped: no near-plane clipping); max_span 0 = no tear rule, else a face whose pixel box is wider is
    skipped; orient +1 / -1 culls, 0 keeps both; (NaN, NaN) where no face lands.  keys: an int64 contiguous [oH, oW] workspace on the
    mesh's device (None: a new one) that holds the winning 64-bit keys afterwards, low 32 bits the face, -1 for a hole.  -> out, or
    (out[, keys][, depth_out]) with return_keys / return_depth (depth_out float32 [oH, oW], NaN in holes; needs depth).  dtype:
    out's, default attr's.  Five launches on the current stream (fill, count, scan, raster, resolve), no sync; bit-equal from run to
    run and to _lib.coords_trimesh_host.  The (face, tile) items of one call are numbered in 32 bits: n_sets * F * b <= 2^32 - 1 with
    b the 4 x 16 pixel tiles of the frame, or of a box max_span wide when max_span > 0 -- about 33 000 faces into 2160 x 3840 with
    max_span = 0; a finer mesh passes a max_span.  pos / attr [B, V, 2] (faces, attr_faces [B, F, 3], depth, w [B, V] batched alike,
    or one shared) give [B, oH, oW, 2] in the same five launches (lerf_coords_trimesh_batched); keys is then [B, oH, oW]."""
    return _lib.coords_trimesh_on(_lib.DeviceOperands(), pos, attr, faces, out_hw, attr_faces, depth, w, dtype, out, origin, max_span, orient, keys,
                                  return_keys, return_depth)


def coords_trimesh_bwd(pos, attr, faces, out_hw, keys, grad_out, attr_faces=None, depth=None, w=None, origin=(0, 0), max_span=0, orient=0,
                       need=(True, True, False), grad_attr=None, grad_pos=None, grad_w=None, max_adders=4096):
    """lerf_coords_trimesh_bwd: ACCUMULATE the adjoint of coords_trimesh at FIXED VISIBILITY of grad_out (float64
    contiguous, the map's shape) into grad_attr [Va, 2], grad_pos [V, 2] and grad_w [V] (float64 contiguous; None: zeroed ones);
    need = (attr, pos, w): a false one is skipped and returned as None; w's needs w.  The mesh operands, origin, max_span and orient are
    the forward's; keys is the int64 plane the forward wrote (return_keys=True).  Every pixel belongs to the face its key names;
    coverage and the depth test get no gradient; grad_out is read at won pixels only.  A face pass (one workgroup per face, a fixed
    tree) and a vertex pass (the ordered scatter's four passes, the faces as entries) on the current stream over the stream's cached
    scratch: bit-equal from run to run and to _lib.coords_trimesh_bwd_host.  Afterwards the largest number of drawn face corners at one
    vertex is read back (ONE 4-byte copy and a synchronisation of the stream); above max_adders: LerfError -- that vertex holds NaN.
    A batch ([B, V, 2] operands, keys [B, oH, oW]) is one call; every gradient then has the leading B, also for an operand the batch
    shares (the caller sums those) -> (grad_attr, grad_pos, grad_w)."""
    return _lib.coords_trimesh_bwd_on(_lib.DeviceOperands(), pos, attr, faces, out_hw, keys, grad_out, attr_faces, depth, w, origin, max_span,
                                      orient, need, grad_attr, grad_pos, grad_w, max_adders, True)[:3]


def coords_compose_bwd(outer, inner, grad_out, grad_outer=None, grad_inner=None, need=(True, True), deterministic=False, max_adders=4096):
    """lerf_coords_compose_bwd: ACCUMULATE the adjoint of coords_compose(outer, inner) of grad_out (float64 contiguous [oH, oW, 2])
    into grad_outer (float64 contiguous [aH, aW, 2]: a bilinear scatter by float64 atomic adds, reproducible up to the rounding of
    a reordered sum) and grad_inner (float64 contiguous [oH, oW, 2]: one writer per entry, bit-reproducible); None: zeroed ones;
    need[k] False skips that half and returns None for it.  The maps are device tensors under the strided contract, the outer
    map at least 2 x 2.  One launch on the current stream, no sync -> (grad_outer, grad_inner).  A batch: inner, grad_out and
    grad_inner [B, oH, oW, 2] with outer and grad_outer [B, aH, aW, 2], or ONE shared outer [aH, aW, 2] whose grad_outer [aH, aW, 2]
    gains the sum over the samples -- still one launch (lerf_coords_compose_bwd_batched).
    deterministic=True: lerf_coords_compose_bwd_ordered -- grad_outer is summed in the host twin's order and equals
    _lib.coords_compose_bwd_host bit for bit, from run to run; the workspace is the stream's cached scratch.  After the launches the
    largest number of entries adding into one element is read back (ONE 4-byte copy and a synchronisation of the stream); above
    max_adders: LerfError, that element holds NaN.  One shared outer map in a batch: every sample scatters into a gradient of its own
    and grad_outer gains them one after the other, sample 0 first."""
    return _lib.coords_compose_bwd_on(_lib.DeviceOperands(), outer, inner, grad_out, grad_outer, grad_inner, need,
                                      int(max_adders) if deterministic else None)


def coords_invert_bwd(f, inverse, grad_out, grad_f=None, deterministic=False, max_adders=4096):
    """lerf_coords_invert_bwd: ACCUMULATE the adjoint of inverse = coords_invert(f, ...) of grad_out (float64 contiguous
    [oH, oW, 2]) into grad_f (float64 contiguous [fH, fW, 2]; None: a zeroed one) by the implicit function theorem: the bilinear
    scatter of -J^-T grad_out at the cell of every entry of the inverse (float64 atomic adds); NaN entries of the inverse, NaN
    corners and folded cells contribute nothing.  Device maps under the strided contract.  One launch on the current stream, no
    sync.  A batch: f and grad_f [B, fH, fW, 2], inverse and grad_out [B, oH, oW, 2], one launch (lerf_coords_invert_bwd_batched).
    deterministic=True: lerf_coords_invert_bwd_ordered, bit-equal to _lib.coords_invert_bwd_host and from run to run;
    then the largest count is read back (one 4-byte copy and a synchronisation); above max_adders: LerfError."""
    return _lib.coords_invert_bwd_on(_lib.DeviceOperands(), f, inverse, grad_out, grad_f, int(max_adders) if deterministic else None)


def coords_reproject(kind, params, depth, dtype=None, out=None, origin=(0, 0), depth_out=None):
    """lerf_coords_reproject: the map that carries a view with a depth per pixel into another view.  kind "z" (depth) or "inverse"
    (1 / depth); params float64 device [12] = (K_dst . R . inv(K_src))[9], (K_dst . t)[3] with depth [H, W] (device, float32 /
    float64), or [B, 12] with depth [B, H, W] or one shared [H, W] -> the map [H, W, 2] or [B, H, W, 2] of `dtype` (default float64):
    entry (i, j) is (row, col) of pixel (i, j) in the other view, (NaN, NaN) where the depth is not positive (inverse: negative), not
    finite, or the point lies behind the other camera.  out: a device tensor or a strided tile view (its depth plane is the TILE's)
    at `origin` of the whole map.  depth_out: True or a float32 device tensor of depth's batch shape -> (map, zo), zo the depth in the
    other view, what coords_invert_raster takes as depth.  ONE launch on the current stream whatever B, no sync; bit-equal to
    _lib.coords_reproject_host."""
    return _lib.coords_reproject_on(_lib.DeviceOperands(), kind, params, depth, dtype, out, origin, depth_out)


def coords_reproject_bwd(kind, params, depth, grad_map, grad_depth_out=None, grad_depth=None, grad_params=None, need=(True, True),
                         origin=(0, 0)):
    """lerf_coords_reproject_bwd: ACCUMULATE the adjoint of coords_reproject of grad_map (float64 contiguous, the map's shape) and
    grad_depth_out (float64 contiguous, zo's shape; None: no upstream) into grad_depth (float64, [H, W] or [B, H, W]: one writer per
    entry) and grad_params (float64, params' shape: the build adjoint's two fixed-order passes, no atomics); None: zeroed ones;
    need[k] False skips that half and returns None for it -> (grad_depth, grad_params).  An entry that is not valid contributes
    nothing, whatever the upstreams hold.  One launch (two with grad_params) on the current stream, no sync; two calls are bit-equal,
    and equal to _lib.coords_reproject_bwd_host."""
    return _lib.coords_reproject_bwd_on(_lib.DeviceOperands(), kind, params, depth, grad_map, grad_depth_out, grad_depth, grad_params, need,
                                        origin)


def splat(src, map, out_hw, weight=None, norm=False, acc=None, deterministic=False, max_adders=4096):
    """lerf_splat: the forward warp by summation splatting -- every pixel of src is ADDED into the out_hw frame at the position the
    forward map gives it, bilinearly over up to four pixels; mass that leaves the frame is lost, a non-finite entry contributes nothing.
    src [C, H, W] or [B, C, H, W] (device, float32 / float64); map [H, W, 2] (shared by the batch) or [B, H, W, 2], float32 / float64;
    weight None or src's dtype [H, W] / [B, H, W] -> acc [.., C (+ 1 with norm: the plane of the weights), oH, oW] of src's dtype; acc
    given: ACCUMULATED INTO (several frames into one canvas).  ONE launch on the current stream whatever B, no sync; one no-return float
    atomic add per tap and plane, so two runs agree up to the rounding of a reordered sum (exactly, where every partial sum is exact).
    deterministic=True: lerf_splat_ordered -- count, scan, fill, then one thread per output pixel sorts its source pixels
    and adds them in row-major order: bit-equal to _lib.splat_host and from run to run, into a pre-filled acc too.  Six launches and a
    memset on the current stream over the stream's cached scratch; afterwards the largest number of source pixels adding into one
    output pixel is read back (ONE 4-byte copy and a synchronisation of the stream).  Above max_adders: LerfError -- that pixel holds
    NaN in every plane, every other pixel is exact."""
    return _lib.splat_on(_lib.DeviceOperands(), src, map, out_hw, weight, norm, acc, int(max_adders) if deterministic else None)


def scan_exclusive_u32(data):
    """lerf_scan_exclusive_u32: the exclusive prefix sums (modulo 2^32) of a contiguous int32 device vector (its bits read as
    uint32), in place, by multi-kernel passes on the current stream -- pass 2 of the ordered scatter on its own"""
    torch = _torch()
    if not (isinstance(data, torch.Tensor) and data.is_cuda and data.dtype == torch.int32 and data.dim() == 1 and data.is_contiguous()
            and data.numel() >= 1):
        raise ValueError("lerf_scan_exclusive_u32: data must be a contiguous int32 device vector")
    L = _lib.lib()
    need = int(L.lerf_scan_exclusive_u32_workspace_bytes(data.numel()))
    ws = _cached_workspace(need, data.device) if need else None
    with _lib.on_device(data):
        _lib.check(L.lerf_scan_exclusive_u32(data.data_ptr(), data.numel(), None if ws is None else ws.data_ptr(), need,
                                             _lib.current_stream(data.device)), "lerf_scan_exclusive_u32")
    return data


def splat_bwd(src, map, grad, weight=None, norm=False, need=(True, True, True)):
    """lerf_splat_bwd: the adjoint of splat at grad [.., C (+ 1), oH, oW] (src's dtype) -> (grad_src, grad_weight, grad_map), None for a
    half that need[k] skips; grad_map float64 of the map's shape.  A gather with one writer per source pixel: one launch, no atomics,
    bit-equal from run to run and to _lib.splat_bwd_host."""
    return _lib.splat_bwd_on(_lib.DeviceOperands(), src, map, grad, weight, norm, need)
