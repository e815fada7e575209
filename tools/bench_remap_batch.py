"""Times the remap of a batch with ONE COORDINATE MAP PER FRAME on the MI355X: LeRF-G, 8 frames 1920x1080 -> 3840x2160 RGB
uint8, S = 2, float64 maps, everything device-resident before the clock starts.

  (a) batched   eight per-frame maps in ONE launch         (lerf_remap_packed_batched: the frame on the grid)
  (b) loop      the same eight as eight single-map calls   (lerf_remap_packed, n = 1)
  (c) shared    eight frames sharing one map                (lerf_remap_packed, n = 8: one thread walks the frames -- the existing path)

Each as stage 3 alone on packed maps that are already there (`stage3`) and through LerfEngine.remap without the validity mask
(`engine`: stages 1+2 + stage 3).  The eight maps are the config-4 homography of bench.py with a different shift per frame, so
every frame's map is distinct memory and distinct values.  The method of tools/bench_remap.py: device events around `--iters`
calls after `--warmup` calls, the variants interleaved window by window, median of `--repeats` windows, [min, max] beside it.

Bytes of stage 3 per output pixel (what must cross HBM at least once): (a) and (b) 3 written + the packed maps + 16 of map;
(c) reads ONE map for the eight frames: 2 B of map per output pixel -- (a) against (c) is what per-frame maps cost, (a) against
(b) what the single launch saves.  Prints ONE JSON line; the in-run check is that (a) returns the bytes of (b).

    python tools/bench_remap_batch.py [--iters 10] [--warmup 3] [--repeats 7] [--frames 8]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_remap import M_ISC, time_interleaved            # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--in-hw", type=int, nargs=2, default=[1080, 1920])
    ap.add_argument("--out-hw", type=int, nargs=2, default=[2160, 3840])
    a = ap.parse_args()
    import torch
    import lerf_pytorch_amd as L
    from lerf_pytorch_amd import _lib, coords, ops
    _lib.require_gpu()
    (H, W), out_hw, N = a.in_hw, tuple(a.out_hw), a.frames
    eng = L.LerfEngine.shipped("lerf-g")
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 128 + 60 * np.sin(yy / 37.0)[..., None] * np.cos(xx / 53.0)[..., None]
    frames = torch.from_numpy(np.stack([np.clip(base + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8) for _ in range(N)])).cuda()
    # one homography per frame (a stabiliser's): the config-4 matrix, shifted by a few pixels per frame; built on the device
    maps = torch.empty((N,) + out_hw + (2,), dtype=torch.float64, device=frames.device)
    for f in range(N):
        M = np.array(M_ISC)
        M[0, 2] += 3.0 * f
        M[1, 2] -= 2.0 * f
        maps[f] = coords.from_homography(M, out_hw, device=frames.device)
    geo_b = ops.RemapGeometry((H, W), maps, eng.support)
    geo_1 = [ops.RemapGeometry((H, W), maps[f], eng.support) for f in range(N)]
    packed = ops.stages_packed(frames, eng.luts)
    out = torch.empty((N,) + out_hw + (3,), dtype=torch.uint8, device=frames.device)

    def s3_loop():
        for f in range(N):
            ops.remap_packed(packed[f], geo_1[f], eng.kind, eng.max_sigma, out=out[f])

    def eng_loop():
        for f in range(N):
            eng.remap(frames[f], geo_1[f], return_mask=False)

    # in-run check: the batched launch returns the loop's bytes
    got = ops.remap_packed(packed, geo_b, eng.kind, eng.max_sigma, out="u8")
    s3_loop()
    equal = bool(torch.equal(got, out))
    got_e = eng.remap(frames, geo_b, return_mask=False)[0]
    equal = equal and all(bool(torch.equal(got_e[f], eng.remap(frames[f], geo_1[f], return_mask=False)[0])) for f in range(N))
    del got, got_e

    stage3 = time_interleaved({
        "batched": lambda: ops.remap_packed(packed, geo_b, eng.kind, eng.max_sigma, out=out),
        "loop": s3_loop,
        "shared": lambda: ops.remap_packed(packed, geo_1[0], eng.kind, eng.max_sigma, out=out)}, a.iters, a.warmup, a.repeats)
    engine = time_interleaved({
        "batched": lambda: eng.remap(frames, geo_b, return_mask=False),
        "loop": eng_loop,
        "shared": lambda: eng.remap(frames, geo_1[0], return_mask=False)}, a.iters, a.warmup, a.repeats)

    opix = out_hw[0] * out_hw[1] * N

    def rows(t):
        return {k: {"ms": round(v[0], 4), "min_max": [round(v[1], 4), round(v[2], 4)], "gpix_per_s": round(opix / v[0] / 1e6, 3)}
                for k, v in t.items()}
    res = {"tool": "bench_remap_batch", "model": "lerf-g", "frames": N, "in_hw": [H, W], "out_hw": list(out_hw), "S": eng.support,
           "map_dtype": "float64", "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats,
           "stage3": rows(stage3), "engine": rows(engine),
           "ratio_batched_over_loop": {"stage3": round(stage3["batched"][0] / stage3["loop"][0], 3),
                                       "engine": round(engine["batched"][0] / engine["loop"][0], 3)},
           "ratio_batched_over_shared": {"stage3": round(stage3["batched"][0] / stage3["shared"][0], 3),
                                         "engine": round(engine["batched"][0] / engine["shared"][0], 3)},
           "batched_equals_loop": equal}
    print(json.dumps(res))
    if not equal:
        raise SystemExit("the batched remap does not reproduce the per-frame loop's bytes")


if __name__ == "__main__":
    main()
