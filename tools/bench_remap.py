"""Times the remap (warp by a dense coordinate map) against the homographic warp of the same run on the MI355X:
LeRF-G, 1920x1080 -> 3840x2160 RGB uint8, S = 2, the config-4 matrix of bench.py (M_ISC).

  warp        LerfEngine.warp(frame, M, out_hw), unfused packed path (stages_packed + lerf_warp_packed)
  remap f64   LerfEngine.remap(frame, geo) with the float64 map coords.from_homography(M, out_hw)
  remap f32   the same map rounded to float32

Each through the engine without the validity mask (`engine`: stages 1+2 + stage 3) and as stage 3 alone on packed maps that are
already there (`stage3`: lerf_warp_packed / lerf_remap_packed).  The frame, the packed maps and the coordinate map are on the
device before the clock starts; device events around `--iters` calls after `--warmup` calls, median of `--repeats` windows, the
three variants interleaved window by window so that they share whatever the machine does meanwhile.

Bytes per output pixel of stage 3 (what must cross HBM at least once): 3 written, the packed maps read once (12 B per SOURCE
pixel), and the map: 16 B (float64) or 8 B (float32) -- the remap moves 3.7x / 2.3x the warp's bytes at this scale, which is the
ratio to hold the measured time ratio against.  Prints ONE JSON line; the in-run check is that the float64-map remap returns the
warp's bytes exactly (the float32 map rounds the coordinates: the differing bytes are counted, not asserted).

    python tools/bench_remap.py [--iters 20] [--warmup 5] [--repeats 7]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

M_ISC = [[2.05, 0.12, 15.0], [-0.08, 1.95, 40.0], [1.5e-5, -1.0e-5, 1.0]]     # bench.py config 4
HBM_PEAK = 8.0e12


def time_interleaved(fns, iters, warmup, repeats):
    """{name: median ms per call}, the functions timed in turn inside every repeat"""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--in-hw", type=int, nargs=2, default=[1080, 1920])
    ap.add_argument("--out-hw", type=int, nargs=2, default=[2160, 3840])
    a = ap.parse_args()
    import torch
    import lerf_pytorch_amd as L
    from lerf_pytorch_amd import _lib, coords, ops
    _lib.require_gpu()
    (H, W), out_hw = a.in_hw, tuple(a.out_hw)
    M = np.array(M_ISC)
    eng = L.LerfEngine.shipped("lerf-g")
    # a natural-statistics frame (smooth + texture): the LUT gathers of stages 1+2 depend on the content, stage 3 does not
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 128 + 60 * np.sin(yy / 37.0)[..., None] * np.cos(xx / 53.0)[..., None] + rng.normal(0, 12, (H, W, 3))
    frame = torch.from_numpy(np.clip(base, 0, 255).astype(np.uint8)).cuda()
    cm = coords.from_homography(M, out_hw)
    wgeo = ops.WarpGeometry((H, W), M, out_hw, eng.support)
    geos = {"f64": ops.RemapGeometry((H, W), torch.from_numpy(cm).cuda(), eng.support),
            "f32": ops.RemapGeometry((H, W), torch.from_numpy(cm.astype(np.float32)).cuda(), eng.support)}
    packed = ops.stages_packed(frame, eng.luts)
    out = torch.empty(out_hw + (3,), dtype=torch.uint8, device=frame.device)

    # in-run check: the float64 map reproduces the warp's bytes
    want = eng.warp(frame, M, out_hw, return_mask=False)[0]
    got64 = eng.remap(frame, geos["f64"], return_mask=False)[0]
    got32 = eng.remap(frame, geos["f32"], return_mask=False)[0]
    equal = bool(torch.equal(got64, want))
    differ32 = int((got32 != want).sum())

    engine = time_interleaved({
        "warp": lambda: eng.warp(frame, M, out_hw, return_mask=False),
        "remap_f64": lambda: eng.remap(frame, geos["f64"], return_mask=False),
        "remap_f32": lambda: eng.remap(frame, geos["f32"], return_mask=False)}, a.iters, a.warmup, a.repeats)
    stage3 = time_interleaved({
        "warp": lambda: ops.warp_packed(packed, wgeo, eng.kind, eng.max_sigma, out=out),
        "remap_f64": lambda: ops.remap_packed(packed, geos["f64"], eng.kind, eng.max_sigma, out=out),
        "remap_f32": lambda: ops.remap_packed(packed, geos["f32"], eng.kind, eng.max_sigma, out=out)}, a.iters, a.warmup, a.repeats)

    opix = out_hw[0] * out_hw[1]
    src_per_out = 12.0 * H * W / opix                      # packed dwords, read once
    bytes_px = {"warp": 3 + src_per_out, "remap_f64": 3 + src_per_out + 16, "remap_f32": 3 + src_per_out + 8}

    def rows(t):
        return {k: {"ms": round(v[0], 4), "ms_min": round(v[1], 4), "ms_max": round(v[2], 4), "gpix_per_s": round(opix / v[0] / 1e6, 3)}
                for k, v in t.items()}
    res = {"tool": "bench_remap", "model": "lerf-g", "in_hw": [H, W], "out_hw": list(out_hw), "S": eng.support,
           "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats,
           "engine": rows(engine), "stage3": rows(stage3),
           "ratio_engine": {k: round(engine[k][0] / engine["warp"][0], 3) for k in ("remap_f64", "remap_f32")},
           "ratio_stage3": {k: round(stage3[k][0] / stage3["warp"][0], 3) for k in ("remap_f64", "remap_f32")},
           "stage3_bytes_per_out_px": {k: round(v, 2) for k, v in bytes_px.items()},
           "stage3_bytes_ratio": {k: round(bytes_px[k] / bytes_px["warp"], 2) for k in ("remap_f64", "remap_f32")},
           "stage3_hbm_fraction": {k: round(bytes_px[k] * opix / (stage3[k][0] * 1e-3) / HBM_PEAK, 4) for k in bytes_px},
           "map_bytes_per_out_px": {"remap_f64": 16, "remap_f32": 8}, "written_bytes_per_out_px": 3,
           "remap_f64_equals_warp": equal, "remap_f32_bytes_differing": differ32, "out_bytes": 3 * opix}
    print(json.dumps(res))
    if not equal:
        raise SystemExit("remap of the homography's float64 map does not reproduce the warp's bytes")


if __name__ == "__main__":
    main()
