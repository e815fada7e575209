"""Times the ORDERED scatter against the atomic kernels it is the deterministic form of, on the MI355X, in one run:

  splat_atomic / splat_ordered       lerf_splat against lerf_splat_ordered: 1080 x 1920 -> 1080 x 1920, float32, C = 3 + the norm plane, a
                                     float32 map (a smooth flow of a few pixels), one frame and a batch of 8 -- bench_splat.py's shape
  compose_atomic / compose_ordered   lerf_coords_compose_bwd against lerf_coords_compose_bwd_ordered, both gradients, float64 maps, 2160 x 3840
                                     into 2160 x 3840
  invert_atomic / invert_ordered     lerf_coords_invert_bwd against lerf_coords_invert_bwd_ordered at the same shape

The ordered calls are the library's entry points themselves over a workspace allocated once: the launches, without the wrapper's
read-back of the largest count (one 4-byte copy and a synchronisation per call, which a training step pays once).  Device events
around windows of `--iters` calls, the variants' windows INTERLEAVED after `--warmup` calls of each (bench_splat.py's method); median
of `--repeats` windows with [min, max], and the ratio ordered / atomic of the medians of the same run.  The per-pass split (count,
scan, fill, sum, memset) comes from one torch.profiler window of the ordered call, kernel times summed by name; null where the
profiler does not deliver kernel records.  Prints ONE JSON line; no speed gate -- the in-run check is that the ordered result is the
same bits in two runs and agrees with the atomic one to the rounding of a reordered sum.

    python tools/bench_splat_ordered.py [--iters 10] [--warmup 2] [--repeats 5] [--hw 1080 1920] [--map-hw 2160 3840] [--batch 8]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_coords_build_grad import interleaved_ms          # noqa: E402  (the same timing loop)

PASSES = (("count", "CountPass"), ("scan", "scan_"), ("fill", "FillPass"), ("sum", "ordered_sum_kernel"), ("memset", "emset"))


def pass_split(torch, fn, iters):
    """{pass: ms per call} of the kernels one call of fn launches, or None"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
        out = {name: 0.0 for name, _ in PASSES}
        out["other"] = 0.0
        seen = 0
        for ev in prof.events():
            if str(getattr(ev, "device_type", "")).endswith("CUDA") or getattr(ev, "device_time", 0):
                t = float(getattr(ev, "device_time", 0) or getattr(ev, "cuda_time", 0))
                if not t:
                    continue
                seen += 1
                key = next((name for name, tag in PASSES if tag in ev.name), "other")
                out[key] += t / 1e3 / iters
        return {k: round(v, 4) for k, v in out.items()} if seen else None
    except Exception as e:                                    # the split is a figure, not a check
        return {"error": repr(e)[:200]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hw", type=int, nargs=2, default=[1080, 1920])
    ap.add_argument("--map-hw", type=int, nargs=2, default=[2160, 3840])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--max-adders", type=int, default=4096)
    a = ap.parse_args()
    import torch
    from lerf_pytorch_amd import _lib, ops
    _lib.require_gpu()
    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = _lib.current_stream(dev)
    res = {"tool": "bench_splat_ordered", "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats, "max_adders": a.max_adders, "cases": {}}
    ok = True

    def report(ms, pair, split):
        at, od = ms[pair + "_atomic"], ms[pair + "_ordered"]
        return {"atomic_ms": round(at[0], 4), "atomic_ms_min_max": [round(at[1], 4), round(at[2], 4)], "ordered_ms": round(od[0], 4),
                "ordered_ms_min_max": [round(od[1], 4), round(od[2], 4)], "ordered_over_atomic": round(od[0] / at[0], 3), "passes_ms": split}

    # ---- the splat forward
    hw, C = tuple(a.hw), 3
    n = hw[0] * hw[1]
    ii, jj = np.meshgrid(np.arange(hw[0], dtype=np.float64), np.arange(hw[1], dtype=np.float64), indexing="ij")
    for B in (1, a.batch):
        flow = np.stack([np.stack([2.7 * np.sin(jj / 97.0 + 0.3 * s) + 1.1 * np.cos(ii / 61.0), 3.4 * np.cos(ii / 131.0 + 0.2 * s) + 0.9 * np.sin(jj / 43.0)], -1)
                         for s in range(B)])
        f = torch.from_numpy((np.stack([ii, jj], -1)[None] + flow).astype(np.float32)).to(dev)
        x = torch.rand((B, C) + hw, dtype=torch.float32, device=dev)
        m = torch.rand((B,) + hw, dtype=torch.float32, device=dev) + 0.5
        acc = torch.zeros((B, C + 1) + hw, dtype=torch.float32, device=dev)
        ws = torch.empty(_lib.ordered_workspace_bytes(n, n, B), dtype=torch.uint8, device=dev)
        sets = (C * n, 2 * n, n, (C + 1) * n) if B > 1 else (0, 0, 0, 0)

        def ordered(acc=acc):
            rc = L.lerf_splat_ordered(x.data_ptr(), _lib.LERF_F32, C, hw[0], hw[1], sets[0], f.data_ptr(), _lib.LERF_F32, 2 * hw[1], sets[1], m.data_ptr(),
                                      sets[2], acc.data_ptr(), 1, hw[0], hw[1], sets[3], B, ws.data_ptr(), ws.numel(), a.max_adders, stream)
            assert rc == 0, rc

        fns = {"splat_atomic": lambda: ops.splat(x, f, hw, m, True, acc=acc), "splat_ordered": ordered}
        ms = interleaved_ms(fns, {k: a.iters for k in fns}, a.warmup, a.repeats)
        case = report(ms, "splat", pass_split(torch, ordered, 3))
        case["workspace_mb"] = round(ws.numel() / 2 ** 20, 1)
        one, two = torch.zeros_like(acc), torch.zeros_like(acc)
        ordered(one)
        ordered(two)
        ref = ops.splat(x, f, hw, m, True)
        case["largest_count"] = int(ws[4:8].view(torch.int32).item())
        case["two_runs_bit_equal"] = bool(torch.equal(one.view(torch.int32), two.view(torch.int32)))
        case["max_difference_to_atomic"] = float((one - ref).abs().max())
        ok = ok and case["two_runs_bit_equal"] and case["max_difference_to_atomic"] <= 1e-4 * max(float(ref.abs().max()), 1.0)
        res["cases"]["splat_B%d" % B] = case
        del f, x, m, acc, ws, one, two, ref
        torch.cuda.empty_cache()

    # ---- the two adjoints: a smooth outer map, positions that wander a few cells
    mh, mw = tuple(a.map_hw)
    ii, jj = np.meshgrid(np.arange(mh, dtype=np.float64), np.arange(mw, dtype=np.float64), indexing="ij")
    A = torch.from_numpy(np.stack([ii + 1.3 * np.sin(jj / 71.0), jj + 1.7 * np.cos(ii / 53.0)], -1)).to(dev)
    Bm = torch.from_numpy(np.stack([ii + 2.1 * np.cos(jj / 89.0) + 0.37, jj + 2.9 * np.sin(ii / 67.0) + 0.61], -1)).to(dev)
    g = torch.randn((mh, mw, 2), dtype=torch.float64, device=dev)
    ga, gb, gf = (torch.zeros((mh, mw, 2), dtype=torch.float64, device=dev) for _ in range(3))
    ws = torch.empty(_lib.ordered_workspace_bytes(mh * mw, mh * mw, 1), dtype=torch.uint8, device=dev)
    head = (A.data_ptr(), _lib.LERF_F64, 2 * mw, mh, mw, Bm.data_ptr(), _lib.LERF_F64, 2 * mw, g.data_ptr(), mh, mw)

    def compose_ordered(ga=ga):
        assert L.lerf_coords_compose_bwd_ordered(*head, ga.data_ptr(), gb.data_ptr(), ws.data_ptr(), ws.numel(), a.max_adders, stream) == 0

    def invert_ordered(gf=gf):
        assert L.lerf_coords_invert_bwd_ordered(*head, gf.data_ptr(), ws.data_ptr(), ws.numel(), a.max_adders, stream) == 0

    fns = {"compose_atomic": lambda: ops.coords_compose_bwd(A, Bm, g, ga, gb), "compose_ordered": compose_ordered,
           "invert_atomic": lambda: ops.coords_invert_bwd(A, Bm, g, gf), "invert_ordered": invert_ordered}
    ms = interleaved_ms(fns, {k: a.iters for k in fns}, a.warmup, a.repeats)
    for pair, fn, atomic in (("compose", compose_ordered, lambda t: ops.coords_compose_bwd(A, Bm, g, t, None, (True, False))),
                             ("invert", invert_ordered, lambda t: ops.coords_invert_bwd(A, Bm, g, t))):
        case = report(ms, pair, pass_split(torch, fn, 3))
        one, two, ref = (torch.zeros_like(ga) for _ in range(3))
        fn(one)
        fn(two)
        atomic(ref)
        case["largest_count"] = int(ws[4:8].view(torch.int32).item())
        case["two_runs_bit_equal"] = bool(torch.equal(one.view(torch.int64), two.view(torch.int64)))
        case["max_difference_to_atomic"] = float((one - ref).abs().max())
        ok = ok and case["two_runs_bit_equal"] and case["max_difference_to_atomic"] <= 1e-9 * max(float(ref.abs().max()), 1.0)
        res["cases"]["%s_bwd_%dx%d" % (pair, mh, mw)] = case
    res["workspace_mb_adjoints"] = round(ws.numel() / 2 ** 20, 1)
    res["ordered_is_reproducible_and_agrees"] = ok
    print(json.dumps(res))
    if not ok:
        raise SystemExit("the ordered scatter is not reproducible or differs from the atomic one")


if __name__ == "__main__":
    main()
