"""Times the coordinate-map builders on the MI355X for a 2160 x 3840 float64 map (133 MB):

  build     every model (homography, radial, brown, fisheye, equirect) written by lerf_coords_build, against the SAME map built by the
            numpy builder of coords.py (fisheye, equirect: the host twin, the only host form bit-equal to the kernel) plus
            torch.from_numpy(...).to(device) (wall clock, median of --host-repeats); fisheye and equirect add a chain of divisions
            (sqrt_pm's six Heron passes, atan_pm's reduction) to a kernel that otherwise only writes: their time over brown's, measured in
            the same run, is the number of interest (ratio_to_brown)
  mesh      a 33 x 61 control mesh upsampled (bilinear, bicubic) and the adjoint of each (lerf_coords_mesh_bwd)
  compose   an outer 2160 x 3840 map sampled at an inner 2160 x 3840 map
  invert    a 2160 x 3840 radial map (over a 2160 x 3840 source) inverted into a 2160 x 3840 inverse (lerf_coords_invert), as a
            float64 and as a float32 map, from the affine start; beside it, in the same run, compose of the map with its inverse
            (the same sizes) and the host twin (wall clock); the mean and the largest number of Newton passes
  invert_raster   the same radial map inverted by rasterisation (lerf_coords_invert_raster: fill, one thread per cell with a 64-bit
            integer atomic min per covered pixel, resolve), float64 and float32, max_span = 16, with and without a depth plane, next to
            invert and compose in the same run: its time over invert's, the share of pixels reached, device against host twin (G and
            keys) on a 135 x 240 crop from the middle of the map, and the atomics per output pixel -- the (triangle, pixel) pairs that
            pass the inside test on that crop, counted in numpy; the kernel's skip of an atomic behind a smaller key only lowers it

Device times: device events around `--iters` calls after `--warmup` calls, median of `--repeats` windows (tools/bench_remap.py's
scheme).  With each device time go the bytes the call must move at least once and the share of the HBM peak they imply:
16 B per entry written; the adjoint reads the map gradient once per tap row (2 or 4 times); compose reads 16 B of the inner map,
writes 16 B and reads the outer map once (its taps are neighbours' taps); invert writes 16 B (8 B) per entry and reads the map
once.  One pass of invert moves what compose moves -- four dependent 16-byte gathers -- so invert's time over compose's should sit
near the mean number of passes; the passes are counted without touching the kernel: an entry that needs p passes is NaN with
max_iter < p, so the count of non-NaN entries at max_iter = 1, 2, ... gives the histogram (entries still NaN at --max-iter ran all
of them).  Prints ONE JSON line; no speed gate -- the in-run
check is that every device map equals its host form bit for bit.

    python tools/bench_coords.py [--iters 20] [--warmup 5] [--repeats 7] [--host-repeats 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

M_ISC = [[2.05, 0.12, 15.0], [-0.08, 1.95, 40.0], [1.5e-5, -1.0e-5, 1.0]]     # bench.py config 4
HBM_PEAK = 8.0e12
FISH_DIST = [0.05, -0.012, 0.004, -0.0009]
PANO_HW = (4096, 8192)
VIEW_R = [[0.8660254037844387, 0.0, 0.5], [0.0, 1.0, 0.0], [-0.5, 0.0, 0.8660254037844387]]      # the view turned 30 degrees about y


def device_ms(fn, iters, warmup, repeats):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def host_ms(fn, repeats):
    import torch
    ms, out = [], None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ms)), out


def raster_candidates(F, out_hw, origin, max_span):
    """The (triangle, pixel) pairs that pass lerf_coords_invert_raster's inside test on a small float64 map, counted in numpy (orient 0;
    a statistic: the edge functions are not evaluated in the kernel's canonical endpoint order, so a pixel exactly on an edge may
    round the other way): the 64-bit atomics the raster pass issues when no load lets one be skipped -- the skip only lowers it."""
    def edge(P, Q, qr, qc):
        return (Q[..., 1] - P[..., 1]) * (qr - P[..., 0]) - (Q[..., 0] - P[..., 0]) * (qc - P[..., 1])
    P00, P01, P10, P11 = F[:-1, :-1], F[:-1, 1:], F[1:, :-1], F[1:, 1:]
    total = 0
    for A, B, C in ((P00, P01, P10), (P11, P10, P01)):
        with np.errstate(all="ignore"):
            area2 = edge(A, B, C[..., 0], C[..., 1])
            ok = np.isfinite(A).all(-1) & np.isfinite(B).all(-1) & np.isfinite(C).all(-1) & np.isfinite(area2) & (area2 != 0.0)
            box = []
            for k, (first, n) in enumerate(zip(origin, out_hw)):
                v = np.stack([A[..., k], B[..., k], C[..., k]])
                lo, hi = np.ceil(v.min(0)), np.floor(v.max(0))
                ok &= ~((hi - lo) + 1.0 > max_span)
                box.append((np.maximum(lo, first), np.minimum(hi, first + n - 1)))
            for dr in range(max_span):
                for dc in range(max_span):
                    qr, qc = box[0][0] + dr, box[1][0] + dc
                    e = (edge(A, B, qr, qc), edge(B, C, qr, qc), edge(C, A, qr, qc))
                    inside = np.where(area2 > 0.0, (e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0), (e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0))
                    total += int((ok & (qr <= box[0][1]) & (qc <= box[1][1]) & inside).sum())
    return total


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--in-hw", type=int, nargs=2, default=[1080, 1920])
    ap.add_argument("--out-hw", type=int, nargs=2, default=[2160, 3840])
    ap.add_argument("--mesh-hw", type=int, nargs=2, default=[33, 61])
    ap.add_argument("--max-iter", type=int, default=16)
    ap.add_argument("--tol", type=float, default=1e-9)
    a = ap.parse_args()
    import torch
    from lerf_pytorch_amd import _lib, coords, ops
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    in_hw, hw, ghw = tuple(a.in_hw), tuple(a.out_hw), tuple(a.mesh_hw)
    entries = hw[0] * hw[1]
    K = np.array([[0.9 * in_hw[1], 0.0, (in_hw[1] - 1) / 2.0], [0.0, 0.9 * in_hw[1], (in_hw[0] - 1) / 2.0], [0.0, 0.0, 1.0]])
    new_K = K * np.array([[2.0], [2.0], [1.0]])
    dist = [-0.12, 0.03, 0.001, -0.0005, 0.002]
    builders = {
        "homography": lambda d: coords.from_homography(np.array(M_ISC), hw, device=d),
        "radial": lambda d: coords.radial(in_hw, hw, 0.08, -0.02, device=d),
        "brown": lambda d: coords.undistort_rectify(K, dist, None, new_K, hw, device=d),
        "fisheye": lambda d: coords.fisheye_undistort_rectify(K, FISH_DIST, None, new_K, hw, device=d),
        "equirect": lambda d: coords.equirect_view(PANO_HW, new_K, VIEW_R, hw, device=d),
    }

    def row(t, nbytes):
        return {"ms": round(t[0], 4), "ms_min": round(t[1], 4), "ms_max": round(t[2], 4), "bytes": int(nbytes),
                "hbm_fraction": round(nbytes / (t[0] * 1e-3) / HBM_PEAK, 4)}

    res = {"tool": "bench_coords", "in_hw": list(in_hw), "out_hw": list(hw), "mesh_hw": list(ghw), "dtype": "float64",
           "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats, "host_repeats": a.host_repeats, "map_bytes": 16 * entries}
    equal = True
    build = {}
    for name, fn in builders.items():
        out = torch.empty(hw + (2,), dtype=torch.float64, device=dev)
        code, p = _lib.coords_model_params(name, {
            "homography": np.linalg.inv(np.array(M_ISC)).reshape(9),
            "radial": [(in_hw[0] - 1) / 2.0, (in_hw[1] - 1) / 2.0, np.hypot(*hw) / 2.0, np.hypot(*in_hw) / 2.0, (hw[0] - 1) / 2.0, (hw[1] - 1) / 2.0, 0.08, -0.02],
            "brown": coords.brown_params(K, dist, None, new_K), "fisheye": coords.fisheye_params(K, FISH_DIST, None, new_K),
            "equirect": coords.equirect_params(PANO_HW, new_K, VIEW_R)}[name])
        t = device_ms(lambda: ops.coords_build(name, p, hw, out=out), a.iters, a.warmup, a.repeats)
        h_ms, h_map = host_ms(lambda: torch.from_numpy(fn(None)).to(dev), a.host_repeats)
        same = bool(torch.equal(fn(dev), h_map))
        equal = equal and same
        build[name] = dict(row(t, 16 * entries), host_numpy_plus_upload_ms=round(h_ms, 2), speedup=round(h_ms / t[0], 1), equals_host=same)
    for name in ("fisheye", "equirect"):
        build[name]["ratio_to_brown"] = round(build[name]["ms"] / build["brown"]["ms"], 2)
    res["build"] = build

    rng = np.random.default_rng(0)
    gy, gx = np.meshgrid(np.linspace(0, in_hw[0] - 1, ghw[0]), np.linspace(0, in_hw[1] - 1, ghw[1]), indexing="ij")
    ctrl_np = np.stack([gy, gx], axis=-1) + rng.normal(0, 2.0, ghw + (2,))
    ctrl = torch.from_numpy(ctrl_np).to(dev)
    G = torch.randn(hw + (2,), dtype=torch.float64, device=dev)
    gctrl = torch.zeros(ghw + (2,), dtype=torch.float64, device=dev)
    out = torch.empty(hw + (2,), dtype=torch.float64, device=dev)
    mesh = {}
    for interp, taps in (("bilinear", 2), ("bicubic", 4)):
        t = device_ms(lambda: ops.coords_mesh(ctrl, hw, interp, out=out), a.iters, a.warmup, a.repeats)
        mesh[interp] = row(t, 16 * entries + ctrl.numel() * 8)
        tb = device_ms(lambda: ops.coords_mesh_bwd(G, ghw, interp, grad_ctrl=gctrl), a.iters, a.warmup, a.repeats)
        mesh[interp + "_adjoint"] = row(tb, taps * 16 * entries + 2 * 16 * ghw[0] * hw[1] + 2 * 16 * ghw[0] * ghw[1])
        same = bool(torch.equal(ops.coords_mesh(ctrl, hw, interp), torch.from_numpy(coords.from_mesh(ctrl_np, hw, interp)).to(dev)))
        equal = equal and same
        mesh[interp]["equals_host"] = same
    res["mesh"] = mesh

    outer = coords.radial(in_hw, hw, 0.08, -0.02, device=dev)
    inner = coords.from_homography(np.array([[1.01, 0.004, 3.0], [-0.003, 0.99, 5.0], [1e-6, -1e-6, 1.0]]), hw, device=dev)
    t = device_ms(lambda: ops.coords_compose(outer, inner, out=out), a.iters, a.warmup, a.repeats)
    res["compose"] = row(t, 3 * 16 * entries)

    # invert: F = a radial map over a source of the inverse's size, so most targets are reached; compose(F, G) beside it
    F = coords.radial(hw, hw, 0.08, -0.02, device=dev)
    inv = {"max_iter": a.max_iter, "tol": a.tol}
    G = None
    for name, Fm in (("float64", F), ("float32", F.float())):
        o = torch.empty(hw + (2,), dtype=Fm.dtype, device=dev)
        t = device_ms(lambda: ops.coords_invert(Fm, hw, out=o, max_iter=a.max_iter, tol=a.tol), a.iters, a.warmup, a.repeats)
        eb = 16 if name == "float64" else 8
        inv[name] = row(t, 2 * eb * entries)
        done = [int((~torch.isnan(ops.coords_invert(Fm, hw, out=o, max_iter=k, tol=a.tol)[..., 0])).sum()) for k in range(1, a.max_iter + 1)]
        hist = [done[0]] + [done[k] - done[k - 1] for k in range(1, len(done))]
        passes = sum((k + 1) * n for k, n in enumerate(hist)) + a.max_iter * (entries - done[-1])
        inv[name].update(reached_fraction=round(done[-1] / entries, 4), mean_passes=round(passes / entries, 3),
                         mean_passes_reached=round(sum((k + 1) * n for k, n in enumerate(hist)) / max(done[-1], 1), 3),
                         max_passes_reached=max(k + 1 for k, n in enumerate(hist) if n) if done[-1] else 0)
        if name == "float64":
            G = o.clone()
    t = device_ms(lambda: ops.coords_compose(F, G, out=out), a.iters, a.warmup, a.repeats)
    inv["compose_same_size"] = row(t, 3 * 16 * entries)
    inv["float64"]["ratio_to_compose"] = round(inv["float64"]["ms"] / inv["compose_same_size"]["ms"], 2)
    inv["float32"]["ratio_to_compose"] = round(inv["float32"]["ms"] / inv["compose_same_size"]["ms"], 2)
    F_np = F.cpu().numpy()
    h_ms, h_map = host_ms(lambda: torch.from_numpy(_lib.coords_invert_host(F_np, hw, max_iter=a.max_iter, tol=a.tol)).to(dev), 1)
    same = bool(torch.equal(torch.nan_to_num(G, nan=-1.0), torch.nan_to_num(h_map, nan=-1.0)))
    equal = equal and same
    inv["host_twin_plus_upload_ms"] = round(h_ms, 1)
    inv["equals_host"] = same
    res["invert"] = inv

    # invert_raster: the same radial map drawn triangle by triangle (lerf_coords_invert_raster), next to invert in the same run
    ras = {"max_span": 16}
    depth = (1.0 + 1e-3 * torch.arange(hw[0], device=dev)[:, None] + 5e-4 * torch.arange(hw[1], device=dev)[None, :]).float().contiguous()
    keys = torch.empty(hw, dtype=torch.int64, device=dev)
    ci, cj, ch, cw = hw[0] // 2 - 67, hw[1] // 2 - 120, min(135, hw[0]), min(240, hw[1])
    ci, cj = max(ci, 0), max(cj, 0)
    for name, Fm in (("float64", F), ("float32", F.float())):
        o = torch.empty(hw + (2,), dtype=Fm.dtype, device=dev)
        eb = 16 if name == "float64" else 8
        crop = Fm[ci:ci + ch, cj:cj + cw].contiguous()
        mid = crop[ch // 2, cw // 2].double().cpu().numpy()
        origin = (max(int(mid[0]) - ch // 2, 0), max(int(mid[1]) - cw // 2, 0))
        for dname, d in (("", None), ("_depth", depth)):
            t = device_ms(lambda: ops.coords_invert_raster(Fm, hw, depth=d, out=o, max_span=16, keys=keys), a.iters, a.warmup, a.repeats)
            # F and depth read once, keys filled, touched by the atomics and read, the inverse written
            r = row(t, (eb + (4 if d is not None else 0) + 24 + eb) * entries)
            r["ratio_to_invert"] = round(t[0] / inv[name]["ms"], 2)
            r["reached_fraction"] = round(float((keys != -1).double().mean()), 4)
            dc = None if d is None else d[ci:ci + ch, cj:cj + cw].contiguous()
            g_dev, k_dev = ops.coords_invert_raster(crop, (ch, cw), depth=dc, origin=origin, max_span=16, return_keys=True)
            crop_np = crop.cpu().numpy()
            g_host, k_host = _lib.coords_invert_raster_host(crop_np, (ch, cw), depth=None if dc is None else dc.cpu().numpy(), dtype=crop_np.dtype,
                                                            origin=origin, max_span=16, return_keys=True)
            same = bool(np.array_equal(k_dev.cpu().numpy().view(np.uint64), k_host)) and \
                bool(torch.equal(torch.nan_to_num(g_dev, nan=-1.0), torch.nan_to_num(torch.from_numpy(g_host).to(dev), nan=-1.0)))
            equal = equal and same
            r["equals_host_on_crop"] = same
            ras[name + dname] = r
    ras["crop"] = {"hw": [ch, cw], "origin": list(origin)}
    ras["atomics_per_pixel_max"] = round(raster_candidates(F[ci:ci + ch, cj:cj + cw].cpu().numpy(), (ch, cw), origin, 16) / (ch * cw), 3)
    res["invert_raster"] = ras
    res["device_equals_host"] = equal
    print(json.dumps(res))
    if not equal:
        raise SystemExit("a device-built map differs from its host form")


if __name__ == "__main__":
    main()
