"""Reference side of the remap tests: the oracle's warp geometry restated for a dense coordinate map.

oracle.lerf_oracle._warp_core reaches the geometry only through the module global `warp_geometry`; a test replaces it
(monkeypatch.setattr) with `map_geometry` below and hands the MAP to warp_params_f32 / warp_u8 in their `matrix` argument.
The restatement is warp_geometry's own lines from the clip on (oracle/lerf_oracle.py:365-374, the reference's
resize_right2d_numpy.py:338-369): nothing about the taps, the weights or the pads' use is restated."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)


def map_geometry(coords, in_hw, out_hw, S):
    """warp_geometry(matrix, in_hw, out_hw, S) with the projected grid read from `coords` [oH, oW, 2] = (row, col), unclipped
    (float32 maps are promoted exactly)"""
    c = np.asarray(coords).astype(np.float64)
    H, W = in_hw
    assert c.shape == (out_hw[0], out_hw[1], 2)
    gx = c[..., 0].clip(0, H)                   # row coordinate
    gy = c[..., 1].clip(0, W)                   # col coordinate
    lx = np.int_(np.ceil(gx - S / 2 - EPS32))
    ly = np.int_(np.ceil(gy - S / 2 - EPS32))
    plx = max(-int(lx[0, 0]), 0)
    phx = max(int(lx[-1, -1]) + S - 1 - H + 1, 0)
    ply = max(-int(ly[0, 0]), 0)
    phy = max(int(ly[-1, -1]) + S - 1 - W + 1, 0)
    return dict(gx=gx + plx, gy=gy + ply, lx=lx + plx, ly=ly + ply, pad=(plx, phx, ply, phy))


def sinus_flow(in_hw, out_hw):
    """row = i H/oH + 2.5 sin(j/7) - 3, col = j W/oW + 2 cos(i/5) + 4: leaves the frame on two sides, non-zero low pads"""
    (H, W), (oH, oW) = in_hw, out_hw
    ii, jj = np.meshgrid(np.arange(oH), np.arange(oW), indexing="ij")
    return np.ascontiguousarray(np.stack([ii * H / oH + 2.5 * np.sin(jj / 7) - 3, jj * W / oW + 2 * np.cos(ii / 5) + 4], axis=-1))


def folded(in_hw, out_hw):
    """a map with a fold (the columns run forth, back and forth again: non-monotone) and a constant region (the lower right
    quarter reads one source position)"""
    (H, W), (oH, oW) = in_hw, out_hw
    ii, jj = np.meshgrid(np.arange(oH), np.arange(oW), indexing="ij")
    t = jj / (oW - 1.0)
    col = (W - 1) * np.abs(np.abs(3 * t - 1) - 1) * 0.97 + 0.31
    row = ii * (H - 1.0) / (oH - 1.0) + 0.25 * np.sin(jj / 3.0)
    m = np.stack([row, col], axis=-1)
    m[oH // 2:, oW // 2:] = (H * 0.37, W * 0.61)
    return np.ascontiguousarray(m)
