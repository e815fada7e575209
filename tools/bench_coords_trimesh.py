"""Times the triangle-mesh rasteriser (lerf_coords_trimesh behind ops.coords_trimesh) on the MI355X, into a 2160 x 3840 map:

  grid      (a) the grid triangulation (coords.grid_faces) of the 2160 x 3840 radial map of tools/bench_coords.py -- 16.6 M faces a
            pixel or two wide, max_span = 16 -- against lerf_coords_invert_raster on the same map IN THE SAME RUN (the two draw the same
            triangles and return the same bits; one thread per cell against one wave per (face, tile) item), float64;
  jittered  (b) a jittered 17 x 30 vertex grid -- 928 triangles some 130 pixels wide, which invert_raster cannot draw at all (its
            max_span ends at 64) -- with and without depth and w, float32 and float64 operands, max_span = 0.

Device times: device events around `--iters` calls after `--warmup` calls, median of `--repeats` windows; the calls that are compared
are timed in INTERLEAVED windows (one window of each per repeat), so clock and thermal drift meet both alike.  With every time go the
(face, tile) items of the call (the count pass's own rule, restated in torch), the items and the inside-test passes per output pixel
-- the 64-bit atomics the raster pass issues when no load lets one be skipped; the skip only lowers it -- and the share of covered
pixels.  Both legs compare a 135 x 240 crop with the host twin by bits.  Prints ONE JSON line; there is no speed gate -- the in-run
check is the bit equality.

    python tools/bench_coords_trimesh.py [--iters 10] [--warmup 3] [--repeats 5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TILE = (4, 16)


def interleaved_ms(fns, iters, warmup, repeats):
    """{name: (median, min, max) ms per call}: every repeat times one window of each fn in turn"""
    import torch
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / iters)
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ms.items()}


def mesh_statistics(pos, faces, hw, origin, max_span):
    """(items, inside-test passes) of a call, in torch on pos's device: the boxes by the set-up's rule (orient 0, no depth or w test),
    the inside test with plain edge functions -- a statistic, not the kernel's canonical endpoint order"""
    import torch
    P = pos.double()[faces.long()]                                       # [F, 3, 2]
    A, B, C = P[:, 0], P[:, 1], P[:, 2]

    def edge(P_, Q_, qr, qc):
        return (Q_[:, 1, None, None] - P_[:, 1, None, None]) * (qr - P_[:, 0, None, None]) - (Q_[:, 0, None, None] - P_[:, 0, None, None]) * (qc - P_[:, 1, None, None])
    area2 = (B[:, 1] - A[:, 1]) * (C[:, 0] - A[:, 0]) - (B[:, 0] - A[:, 0]) * (C[:, 1] - A[:, 1])
    ok = torch.isfinite(P).all(dim=(1, 2)) & torch.isfinite(area2) & (area2 != 0)
    lo, hi = torch.ceil(P.min(dim=1).values), torch.floor(P.max(dim=1).values)
    if max_span > 0:
        ok &= (((hi - lo) + 1.0) <= max_span).all(dim=1)
    first = torch.tensor([float(origin[0]), float(origin[1])], dtype=torch.float64, device=pos.device)
    last = first + torch.tensor([hw[0] - 1.0, hw[1] - 1.0], dtype=torch.float64, device=pos.device)
    lo, hi = torch.maximum(lo, first), torch.minimum(hi, last)
    ok &= (lo <= hi).all(dim=1)
    lo, hi = torch.where(ok[:, None], lo, first), torch.where(ok[:, None], hi, first)
    tile = torch.tensor([float(TILE[0]), float(TILE[1])], dtype=torch.float64, device=pos.device)
    tiles = torch.floor((hi - first) / tile) - torch.floor((lo - first) / tile) + 1.0
    items = int((tiles[:, 0] * tiles[:, 1])[ok].sum())
    span = (hi - lo + 1.0)[ok].max(dim=0).values if bool(ok.any()) else torch.zeros(2)
    block = 64
    passes = 0
    off = torch.arange(block, dtype=torch.float64, device=pos.device)
    chunk = max(1, (1 << 22) // (block * block))                        # faces a step: 4 M evaluations
    for f0 in range(0, len(faces), chunk):
        s = slice(f0, f0 + chunk)
        for br in range(0, int(span[0]), block):
            for bc in range(0, int(span[1]), block):
                qr = (lo[s, 0, None, None] + br) + off[None, :, None]
                qc = (lo[s, 1, None, None] + bc) + off[None, None, :]
                e = (edge(A[s], B[s], qr, qc), edge(B[s], C[s], qr, qc), edge(C[s], A[s], qr, qc))
                pos_area = (area2[s] > 0)[:, None, None]
                inside = torch.where(pos_area, (e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0), (e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0))
                inside &= ok[s, None, None] & (qr <= hi[s, 0, None, None]) & (qc <= hi[s, 1, None, None])
                passes += int(inside.sum())
    return items, passes


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out-hw", type=int, nargs=2, default=[2160, 3840])
    ap.add_argument("--grid-hw", type=int, nargs=2, default=[17, 30])
    a = ap.parse_args()
    import torch
    from lerf_pytorch_amd import _lib, coords, ops
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    hw, ghw = tuple(a.out_hw), tuple(a.grid_hw)
    entries = hw[0] * hw[1]
    res = {"tool": "bench_coords_trimesh", "out_hw": list(hw), "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats,
           "tile": list(TILE)}
    equal = True

    def row(t):
        return {"ms": round(t[0], 4), "ms_min": round(t[1], 4), "ms_max": round(t[2], 4)}

    def same_as_host(dev_res, host_res):
        ok = True
        for g, h in zip(dev_res, host_res):
            g = g.cpu().numpy()
            ok = ok and bool(np.array_equal(g.view(np.uint64) if g.dtype in (np.int64, np.float64) else g.view(np.uint32),
                                            h.view(np.uint64) if h.dtype in (np.uint64, np.float64) else h.view(np.uint32)))
        return ok

    ch, cw = min(135, hw[0]), min(240, hw[1])
    # ---- (a) the grid mesh of the radial map against invert_raster
    F = coords.radial(hw, hw, 0.08, -0.02, device=dev)
    faces = torch.from_numpy(coords.grid_faces(*hw)).to(dev)
    ii, jj = torch.meshgrid(torch.arange(hw[0], dtype=torch.float64, device=dev), torch.arange(hw[1], dtype=torch.float64, device=dev), indexing="ij")
    attr = torch.stack([ii, jj], dim=-1).reshape(-1, 2).contiguous()
    pos = F.reshape(-1, 2)
    out, keys = torch.empty(hw + (2,), dtype=torch.float64, device=dev), torch.empty(hw, dtype=torch.int64, device=dev)
    out2, keys2 = torch.empty_like(out), torch.empty_like(keys)
    t = interleaved_ms({"trimesh": lambda: ops.coords_trimesh(pos, attr, faces, hw, out=out, max_span=16, keys=keys),
                        "invert_raster": lambda: ops.coords_invert_raster(F, hw, out=out2, max_span=16, keys=keys2)}, a.iters, a.warmup, a.repeats)
    grid = {"faces": int(len(faces)), "max_span": 16, "trimesh": row(t["trimesh"]), "invert_raster": row(t["invert_raster"]),
            "ratio_to_invert_raster": round(t["trimesh"][0] / t["invert_raster"][0], 3),
            "equals_invert_raster": bool(torch.equal(keys, keys2)) and bool(torch.equal(torch.nan_to_num(out, nan=-1.0), torch.nan_to_num(out2, nan=-1.0))),
            "covered_fraction": round(float((keys != -1).double().mean()), 4)}
    equal = equal and grid["equals_invert_raster"]
    ci, cj = max(hw[0] // 2 - ch // 2, 0), max(hw[1] // 2 - cw // 2, 0)
    crop = F[ci:ci + ch, cj:cj + cw].contiguous()
    mid = crop[ch // 2, cw // 2].cpu().numpy()
    origin = (max(int(mid[0]) - ch // 2, 0), max(int(mid[1]) - cw // 2, 0))
    cfaces = coords.grid_faces(ch, cw)
    cattr = np.stack(np.meshgrid(np.arange(ch, dtype=np.float64), np.arange(cw, dtype=np.float64), indexing="ij"), axis=-1).reshape(-1, 2)
    d_res = ops.coords_trimesh(crop.reshape(-1, 2), torch.from_numpy(cattr).to(dev), torch.from_numpy(cfaces).to(dev), (ch, cw), origin=origin,
                               max_span=16, return_keys=True)
    h_res = _lib.coords_trimesh_host(crop.reshape(-1, 2).cpu().numpy(), cattr, cfaces, (ch, cw), origin=origin, max_span=16, return_keys=True)
    grid["equals_host_on_crop"] = same_as_host(d_res, h_res)
    equal = equal and grid["equals_host_on_crop"]
    items, passes = mesh_statistics(crop.reshape(-1, 2), torch.from_numpy(cfaces).to(dev), (ch, cw), origin, 16)
    grid.update(crop={"hw": [ch, cw], "origin": list(origin)}, items_per_pixel_on_crop=round(items / (ch * cw), 3),
                atomics_per_pixel_max_on_crop=round(passes / (ch * cw), 3))
    res["grid"] = grid
    del F, faces, attr, pos, out2, keys2

    # ---- (b) a jittered vertex grid: faces some 130 pixels wide
    rng = np.random.default_rng(0)
    gy, gx = np.meshgrid(np.linspace(0, hw[0] - 1, ghw[0]), np.linspace(0, hw[1] - 1, ghw[1]), indexing="ij")
    base = np.stack([gy, gx], axis=-1).reshape(-1, 2)
    step = min((hw[0] - 1) / (ghw[0] - 1), (hw[1] - 1) / (ghw[1] - 1))
    pos_np = base + rng.uniform(-0.2 * step, 0.2 * step, base.shape)
    attr_np = 0.5 * base + 3.0
    depth_np = rng.uniform(1.0, 2.0, len(base)).astype(np.float32)
    w_np = (1.0 + 0.25 * rng.uniform(size=len(base))).astype(np.float32)
    faces_np = coords.grid_faces(*ghw)
    jit = {"vertices": list(ghw), "faces": int(len(faces_np)), "max_span": 0}
    fd, dd, wd = (torch.from_numpy(x).to(dev) for x in (faces_np, depth_np, w_np))
    calls = {}
    for name, dt in (("float64", np.float64), ("float32", np.float32)):
        pd, ad = torch.from_numpy(pos_np.astype(dt)).to(dev), torch.from_numpy(attr_np.astype(dt)).to(dev)
        o = torch.empty(hw + (2,), dtype=pd.dtype, device=dev)
        calls[name] = (lambda pd=pd, ad=ad, o=o: ops.coords_trimesh(pd, ad, fd, hw, out=o, keys=keys))
        calls[name + "_depth_w"] = (lambda pd=pd, ad=ad, o=o: ops.coords_trimesh(pd, ad, fd, hw, depth=dd, w=wd, out=o, keys=keys))
    t = interleaved_ms(calls, a.iters, a.warmup, a.repeats)
    for name in calls:
        jit[name] = row(t[name])
        jit[name]["ratio_to_invert_raster_of_the_grid_leg"] = round(t[name][0] / grid["invert_raster"]["ms"], 3)
    calls["float64"]()
    jit["covered_fraction"] = round(float((keys != -1).double().mean()), 4)
    items, passes = mesh_statistics(torch.from_numpy(pos_np).to(dev), fd, hw, (0, 0), 0)
    jit.update(items=items, items_per_pixel=round(items / entries, 4), atomics_per_pixel_max=round(passes / entries, 3))
    origin = (hw[0] // 2 - ch // 2, hw[1] // 2 - cw // 2)
    ok = True
    for dt in (np.float64, np.float32):
        for kw in ({}, {"depth": depth_np, "w": w_np}):
            P, A = pos_np.astype(dt), attr_np.astype(dt)
            d_res = ops.coords_trimesh(torch.from_numpy(P).to(dev), torch.from_numpy(A).to(dev), fd, (ch, cw), origin=origin, return_keys=True,
                                       return_depth=bool(kw), **{k: torch.from_numpy(v).to(dev) for k, v in kw.items()})
            h_res = _lib.coords_trimesh_host(P, A, faces_np, (ch, cw), origin=origin, return_keys=True, return_depth=bool(kw), **kw)
            ok = ok and same_as_host(d_res, h_res)
    jit["equals_host_on_crop"] = ok
    jit["crop"] = {"hw": [ch, cw], "origin": list(origin)}
    equal = equal and ok
    res["jittered"] = jit
    res["device_equals_host"] = equal
    print(json.dumps(res))
    if not equal:
        raise SystemExit("a device-built map differs from its host form")


if __name__ == "__main__":
    main()
