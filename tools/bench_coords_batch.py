"""Times the BATCHED chained coordinate-map operations on the MI355X (lerf_coords_*_batched: one launch for B maps, the sample on the
grid's third axis) against the per-sample loop of single-map calls into the slices of one output -- what coords.py did before the
batched entry points existed -- in the same run, at two shapes:

  train   B = 16 maps of 192 x 192 with a 13 x 13 control mesh: the shape of a spatial-transformer head or of scaling and squaring in a
          training loop, where a launch covers 37 k entries and the loop is bound by its launches
  hd      B = 8 maps of 1080 x 1920 with a 33 x 61 control mesh: every launch fills the device, so the loop has little to lose

Per shape and operation (mesh and its adjoint, bicubic; compose of a diffeomorphism with itself and its adjoint, both halves; invert
from the affine start and its adjoint; invert_raster, max_span 16): the median of `--repeats` windows of `--iters` calls with
[min, max], device events around each window, the two variants' windows INTERLEAVED after `--warmup` calls of each, and
loop / batched of the medians.  The rasteriser's batched call holds B key planes (8 B per output pixel per sample) where the loop
reuses one.

In-run check: the batched outputs equal the loop's -- by bits for mesh, compose, invert, invert_raster (G and keys), grad_inner and the
mesh adjoint; within 1e-9 max(max|ref|, 1) (the ADJ_TOL of tests/test_gpu_coords_grad.py) for the two atomic scatters grad_outer and
grad_f.  Prints ONE JSON line; no speed gate.

    python tools/bench_coords_batch.py [--iters 20] [--warmup 5] [--repeats 7] [--shapes train hd]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"train": (16, (192, 192), (13, 13)), "hd": (8, (1080, 1920), (33, 61))}
ADJ_TOL = 1e-9


def interleaved_ms(fns, iters, warmup, repeats):
    """{name: (median, min, max)} of the per-call device time of each variant, window k of every variant before window k + 1 of any"""
    import torch
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / iters)
    return {name: (float(np.median(v)), float(min(v)), float(max(v))) for name, v in ms.items()}


def same_bits(torch, a, b):
    return bool(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b))


def close(torch, got, ref):
    scale = max(float(ref.abs().max()), 1.0)
    return float((got - ref).abs().max()) / scale


def bench_shape(torch, ops, name, a):
    B, hw, ghw = SHAPES[name]
    dev = torch.device("cuda", torch.cuda.current_device())
    f64 = dict(dtype=torch.float64, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    ii = torch.arange(hw[0], **f64)[:, None].expand(hw)
    jj = torch.arange(hw[1], **f64)[None, :].expand(hw)
    ident = torch.stack([ii, jj], dim=-1)
    # B smooth diffeomorphisms of the frame: identity + a few pixels of sinusoidal displacement, another phase per sample
    phase = torch.arange(B, **f64)[:, None, None]
    phi = torch.stack([ident[..., 0] + 2.5 * torch.sin(jj / 19.0 + ii / 31.0 + phase), ident[..., 1] + 3.0 * torch.cos(ii / 23.0 - jj / 29.0 + phase)],
                      dim=-1).contiguous()
    gy, gx = torch.meshgrid(torch.linspace(0, hw[0] - 1, ghw[0], **f64), torch.linspace(0, hw[1] - 1, ghw[1], **f64), indexing="ij")
    ctrl = (torch.stack([gy, gx], dim=-1)[None] + torch.randn((B,) + ghw + (2,), generator=gen, **f64)).contiguous()
    g = torch.randn((B,) + hw + (2,), generator=gen, **f64)
    out_b, out_l = torch.empty_like(phi), torch.empty_like(phi)
    keys_b = torch.empty((B,) + hw, dtype=torch.int64, device=dev)
    keys_l = torch.empty(hw, dtype=torch.int64, device=dev)
    gc_b, gc_l = torch.zeros((B,) + ghw + (2,), **f64), torch.zeros((B,) + ghw + (2,), **f64)
    ga_b, ga_l, gb_b, gb_l = (torch.zeros_like(phi) for _ in range(4))
    inv = ops.coords_invert(phi, hw)
    g_inv = torch.where(torch.isnan(inv), torch.zeros_like(g), g)

    def loop(one):
        def run():
            for n in range(B):
                one(n)
        return run

    def raster_loop(n):
        ops.coords_invert_raster(phi[n], hw, out=out_l[n], keys=keys_l)

    legs = {
        "mesh": (lambda: ops.coords_mesh(ctrl, hw, "bicubic", out=out_b), loop(lambda n: ops.coords_mesh(ctrl[n], hw, "bicubic", out=out_l[n]))),
        "mesh_bwd": (lambda: ops.coords_mesh_bwd(g, ghw, "bicubic", grad_ctrl=gc_b),
                     loop(lambda n: ops.coords_mesh_bwd(g[n], ghw, "bicubic", grad_ctrl=gc_l[n]))),
        "compose": (lambda: ops.coords_compose(phi, phi, out=out_b), loop(lambda n: ops.coords_compose(phi[n], phi[n], out=out_l[n]))),
        "compose_bwd": (lambda: ops.coords_compose_bwd(phi, phi, g, ga_b, gb_b), loop(lambda n: ops.coords_compose_bwd(phi[n], phi[n], g[n], ga_l[n], gb_l[n]))),
        "invert": (lambda: ops.coords_invert(phi, hw, out=out_b), loop(lambda n: ops.coords_invert(phi[n], hw, out=out_l[n]))),
        "invert_bwd": (lambda: ops.coords_invert_bwd(phi, inv, g_inv, ga_b), loop(lambda n: ops.coords_invert_bwd(phi[n], inv[n], g_inv[n], ga_l[n]))),
        "invert_raster": (lambda: ops.coords_invert_raster(phi, hw, out=out_b, keys=keys_b), loop(raster_loop)),
    }
    res = {"B": B, "hw": list(hw), "mesh_hw": list(ghw), "entries_per_map": hw[0] * hw[1], "raster_key_bytes_batched": 8 * B * hw[0] * hw[1],
           "raster_key_bytes_loop": 8 * hw[0] * hw[1]}
    equal = True
    for leg, (batched, looped) in legs.items():
        # the check first, on zeroed accumulators
        for t in (gc_b, gc_l, ga_b, ga_l, gb_b, gb_l):
            t.zero_()
        batched()
        looped()
        if leg in ("mesh", "compose", "invert"):
            check = {"bits": same_bits(torch, out_b, out_l)}
        elif leg == "invert_raster":
            last = ops.coords_invert_raster(phi[B - 1], hw, return_keys=True)[1]
            check = {"bits": same_bits(torch, out_b, out_l) and bool(torch.equal(keys_b[B - 1], keys_l)) and bool(torch.equal(keys_b[B - 1], last)),
                     "reached_fraction": round(float((keys_b != -1).double().mean()), 4)}
        elif leg == "mesh_bwd":
            check = {"bits": same_bits(torch, gc_b, gc_l)}
        elif leg == "compose_bwd":
            err = close(torch, ga_b, ga_l)
            check = {"bits": same_bits(torch, gb_b, gb_l), "grad_outer_rel_err": err, "within_tol": err <= ADJ_TOL}
        else:
            err = close(torch, ga_b, ga_l)
            check = {"grad_f_rel_err": err, "within_tol": err <= ADJ_TOL}
        equal = equal and check.get("bits", True) and check.get("within_tol", True)
        t = interleaved_ms({"batched": batched, "loop": looped}, a.iters, a.warmup, a.repeats)
        res[leg] = {"batched_ms": round(t["batched"][0], 4), "batched_ms_min": round(t["batched"][1], 4), "batched_ms_max": round(t["batched"][2], 4),
                    "loop_ms": round(t["loop"][0], 4), "loop_ms_min": round(t["loop"][1], 4), "loop_ms_max": round(t["loop"][2], 4),
                    "loop_over_batched": round(t["loop"][0] / t["batched"][0], 2), "launches_batched": {"mesh_bwd": 2, "invert_raster": 3}.get(leg, 1),
                    "launches_loop": {"mesh_bwd": 2, "invert_raster": 3}.get(leg, 1) * B, "check": check}
    res["reached_fraction_invert"] = round(float((~torch.isnan(inv[..., 0])).double().mean()), 4)
    return res, equal


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--shapes", nargs="+", default=["train", "hd"], choices=sorted(SHAPES))
    a = ap.parse_args()
    import torch
    from lerf_pytorch_amd import _lib, ops
    _lib.require_gpu()
    res = {"tool": "bench_coords_batch", "dtype": "float64", "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats}
    equal = True
    for name in a.shapes:
        res[name], ok = bench_shape(torch, ops, name, a)
        equal = equal and ok
    res["batched_equals_loop"] = equal
    print(json.dumps(res))
    if not equal:
        raise SystemExit("a batched output differs from the per-sample loop's")


if __name__ == "__main__":
    main()
