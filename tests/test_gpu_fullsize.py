"""Full-size GPU parity: every BASELINE.json configuration at its real size against the C restatement of the oracle
(oracle/lerf_oracle.c, pinned to the reference's golden vectors in tests/test_oracle_c.py), plus the size-independent
properties at 4K -> 8K and a 2-rank RCCL halo exchange.  Run with `-m gpu` on an MI355X.

  config 2  LeRF-G x2, 1080p -> 4K, S=2 ............ tests/test_gpu_parity.py::test_full_frame_bytes_equal_cpu_oracle
            and S=4 (the class default) ............. here
  config 3  LeRF-L, 1080p, x1.5/x2.0 and x2/x2 ..... here, byte-exact
  config 4  LeRF-G warp 1080p -> 4K, isc / osc ..... here, bytes + validity mask
  config 5  LeRF-G x2, 2160x3840 -> 4320x7680 ...... here: byte-exact vs the port, fused == unfused, crop-with-halo
            invariance, 8 emulated strips == full frame; 2-process RCCL halo exchange + stitch (needs 2 GPUs)

The float32 outputs are evaluated in float64 and rounded once (north_star: 1e-4 for fp32, read as ABSOLUTE on the
0..255 scale); the measured maximum per case is printed and asserted.
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu
PERF = os.environ.get("LERF_TEST_PERF") == "1"        # opt-in: throughput / wall-clock assertions

M_ISC = np.array([[2.05, 0.12, 15.0], [-0.08, 1.95, 40.0], [1.5e-5, -1.0e-5, 1.0]])
M_OSC = np.array([[4.1, 0.4, 30.0], [0.5, 3.8, 25.0], [8e-5, 1.2e-4, 1.0]])
F32_ABS_TOL = 1e-4


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


@pytest.fixture(scope="module")
def co():
    from oracle import c_oracle
    c_oracle.lib()
    return c_oracle


@pytest.fixture(scope="module")
def eng_g(torch):
    import lerf_pytorch_amd as L
    return L.LerfEngine.shipped("lerf-g")


@pytest.fixture(scope="module")
def eng_g4(torch):
    import lerf_pytorch_amd as L
    return L.LerfEngine.shipped("lerf-g", support=4)


@pytest.fixture(scope="module")
def eng_l(torch):
    import lerf_pytorch_amd as L
    return L.LerfEngine.shipped("lerf-l")


def _frame(kind, H, W, seed):
    sys.path.insert(0, REPO)
    import bench
    return bench.synth_frames(kind, 1, seed, H, W)[0]


def _bytes_equal(out, ref, what):
    d = np.abs(out.astype(np.int16) - ref.astype(np.int16))
    n = int((d != 0).sum())
    print("%s: %d of %d bytes differ, max |diff| %d" % (what, n, d.size, int(d.max())))
    assert d.max() <= 1, what                                   # north_star: <= 1 LSB
    assert n == 0, "%s: %d of %d bytes differ" % (what, n, d.size)


@pytest.mark.parametrize("kind", ["noise", "natural"])
@pytest.mark.parametrize("scale", [(1.5, 2.0), (2.0, 2.0)])
def test_config3_lerf_l_1080p_bytes_equal_port(torch, co, eng_l, luts_l, kind, scale):
    img = _frame(kind, 1080, 1920, 31)
    out = eng_l.sr(img, scale)
    ref = co.sr_u8(img, luts_l, scale[0], scale[1], linear=True)
    assert out.shape == ref.shape == (int(np.ceil(1080 * scale[0])), 3840, 3)
    _bytes_equal(out, ref, "LeRF-L 1080p x%s %s" % (scale, kind))


@pytest.mark.parametrize("name,M", [("isc", M_ISC), ("osc", M_OSC)])
def test_config4_warp_1080p_to_4k_bytes_and_mask_equal_port(torch, co, eng_g, luts_g, name, M):
    img = _frame("natural", 1080, 1920, 41)
    out, mask = eng_g.warp(img, M, (2160, 3840))
    ref, rmask = co.warp_u8(img, luts_g, M, (2160, 3840))
    assert np.array_equal(mask, rmask), "validity masks differ in %d places" % int((mask != rmask).sum())
    print("warp %s: valid fraction %.4f" % (name, mask.mean()))
    _bytes_equal(out * mask, ref * rmask, "LeRF-G warp 1080p->4K %s (valid region)" % name)
    _bytes_equal(out, ref, "LeRF-G warp 1080p->4K %s (whole frame)" % name)


def test_config4_warp_lerf_l_1080p(torch, co, eng_l, luts_l):
    img = _frame("noise", 1080, 1920, 43)
    out, mask = eng_l.warp(img, M_ISC, (2160, 3840))
    ref, rmask = co.warp_u8(img, luts_l, M_ISC, (2160, 3840), linear=True)
    assert np.array_equal(mask, rmask)
    _bytes_equal(out, ref, "LeRF-L warp 1080p->4K isc")


@pytest.mark.parametrize("kind", ["noise", "natural"])
def test_config2_support4_1080p_bytes_equal_port(torch, co, eng_g4, luts_g, kind):
    img = _frame(kind, 1080, 1920, 51)
    out = eng_g4.sr(img, 2)
    ref = co.sr_u8(img, luts_g, 2, 2, S=4)
    _bytes_equal(out, ref, "LeRF-G S=4 1080p x2 %s" % kind)


@pytest.mark.parametrize("cap", [0, 8])
def test_tie_queue_full_falls_back_in_loop(torch, co, eng_g, eng_g4, eng_l, luts_g, luts_l, cap):
    """Stage 3 queues the outputs that sit on a rounding tie (about 15 per 64x64 tile) and re-evaluates them in float64
    behind the task loop; with the queue capacity lowered to 0 / 8 entries nearly all of them take the in-loop fallback
    instead.  Both routes must give the reference's bytes (2x2 and 4x4 Gaussian, linear)."""
    from lerf_pytorch_amd import ops
    img = _frame("noise", 540, 960, 77)
    x = torch.from_numpy(img).cuda()

    def run(eng, scale):
        geo = eng.sr_geometry((540, 960), scale).with_tie_queue_cap(cap)      # lerf_sr_geo_t.tie_queue_cap: carried per call
        assert geo.struct.tie_queue_cap == (-1 if cap == 0 else cap)
        return ops.sr_fused_u8(x, eng.luts, geo, eng.kind, eng.max_sigma).cpu().numpy()

    _bytes_equal(run(eng_g, 2), co.sr_u8(img, luts_g, 2, 2), "LeRF-G S=2, tie queue of %d" % cap)
    _bytes_equal(run(eng_g4, 2), co.sr_u8(img, luts_g, 2, 2, S=4), "LeRF-G S=4, tie queue of %d" % cap)
    _bytes_equal(run(eng_l, (1.5, 2.0)), co.sr_u8(img, luts_l, 1.5, 2.0, linear=True), "LeRF-L, tie queue of %d" % cap)
    assert eng_g.sr_geometry((540, 960), 2).struct.tie_queue_cap == 0          # the engine's cached geometry is untouched


_COLUMN_TASK_CASES = {                     # name -> (engine fixture, scale, support, linear): tiles that run the dword-column tasks
    "g-s2-x3": ("eng_g", 3, 2, False),     # row groups of three: gsame = 3
    "g-s2-x2.4": ("eng_g", 2.4, 2, False), # groups of 2, 3, 2, 2, 3: the per-group size
    "g-s4-x3": ("eng_g4", 3, 4, False),    # 4 x 4 support, tie bits instead of distances
    "l-x3": ("eng_l", 3, 2, True),         # groups of three: the LeRF-L block tasks decline
}


@pytest.fixture(scope="module")
def column_task_refs(co, luts_g, luts_l):
    """the 70 x 80 noise frame of the column-task cases and, per case, the oracle's bytes and its count of outputs within
    1.5e-4 of a rounding tie (float64 stage 3 on the oracle's stage outputs) among the outputs that tile (0, 0) of a launch
    with 64-row tiles owns: those whose first tap, by the library's own axis tables, lies above row and left of column
    64 - S / 2 (the bound of the kernel's ownership search)"""
    from lerf_pytorch_amd import _lib
    img = np.random.default_rng(77).integers(0, 256, (70, 80, 3), dtype=np.uint8)
    refs = {}
    for name, (_, s, S, linear) in _COLUMN_TASK_CASES.items():
        luts = luts_l if linear else luts_g
        feat, hq = co.lut_stages(img, luts, 1 if linear else 3)
        x = co.resize(feat, hq, s, s, S=S, max_sigma=1.0 if linear else 10.0, kind="linear" if linear else "gauss")
        left_r = _lib.sr_axis_tables(70, x.shape[0], s, S)[0]
        left_c = _lib.sr_axis_tables(80, x.shape[1], s, S)[0]
        owned = (np.abs(x - np.rint(x)) > 0.5 - 1.5e-4)[left_r < 64 - S // 2][:, left_c < 64 - S // 2]
        near = int(owned.sum())
        refs[name] = (co.sr_u8(img, luts, s, s, S=S, linear=linear).copy(), near)
    return img, refs


@pytest.mark.parametrize("cap", [0, 8, None])
@pytest.mark.parametrize("name", list(_COLUMN_TASK_CASES))
def test_tie_queue_full_on_column_tasks(request, torch, column_task_refs, name, cap):
    """The dword-column tasks (scales whose row groups are not pairs) with the tie queue lowered to 0 / 8 entries: every
    undecided output past the capacity is resolved on the spot, inside the task loop, and patched into the packed dword
    before it is stored.  The launch is forced onto 64-row tiles (by default a 70 x 80 frame takes the 16-row instances, whose
    tiles hold a handful of near ties each): tile (0, 0) then owns 191 x 191 (152 x 152 at x2.4) outputs and more undecided
    ones than the queue holds -- counted on the CPU over exactly those outputs: 25 / 20 / 24 / 19 for the four cases, asserted
    to be at least 9 -- so at cap = 8 both the queue and the on-the-spot branch run in one tile; cap = None is the shipped
    capacity.  Bytes equal the oracle's on every route."""
    from lerf_pytorch_amd import _lib, ops
    img, refs = column_task_refs
    eng = request.getfixturevalue(_COLUMN_TASK_CASES[name][0])
    scale = _COLUMN_TASK_CASES[name][1]
    ref, near = refs[name]
    print("%s: %d outputs of tile (0, 0) within 1.5e-4 of a tie" % (name, near))
    assert near >= 9, "the input no longer overflows a queue of 8 in tile (0, 0)"
    geo = eng.sr_geometry((70, 80), scale).with_flags(_lib.GEO_TILE_ROWS_64)
    assert geo.struct.flags & _lib.GEO_TILE_ROWS_64
    if cap is not None:
        geo = geo.with_tie_queue_cap(cap)
        assert geo.struct.flags & _lib.GEO_TILE_ROWS_64
        assert geo.struct.tie_queue_cap == (-1 if cap == 0 else cap)
    out = ops.sr_fused_u8(torch.from_numpy(img).cuda(), eng.luts, geo, eng.kind, eng.max_sigma).cpu().numpy()
    _bytes_equal(out, ref, "%s, tie queue of %s" % (name, cap))


def test_repeated_launches_give_the_same_bytes(torch, eng_g, eng_g4, eng_l):
    """the same launch three times: a kernel that reads a register before its producer has finished (round 3: an inline-asm
    consumer right behind v_exp_f32, which the compiler's hazard recogniser cannot see) gives the right bytes on a fresh box
    and different ones afterwards"""
    from lerf_pytorch_amd import ops
    img = _frame("noise", 540, 960, 78)
    x = torch.from_numpy(img).cuda()
    for eng, scale in ((eng_g, 2), (eng_g4, 2), (eng_l, (1.5, 2.0)), (eng_g, 3)):
        geo = eng.sr_geometry((540, 960), scale)
        first = ops.sr_fused_u8(x, eng.luts, geo, eng.kind, eng.max_sigma).clone()
        for _ in range(2):
            assert torch.equal(ops.sr_fused_u8(x, eng.luts, geo, eng.kind, eng.max_sigma), first)


def test_config5_4k_to_8k_properties(torch, co, eng_g, luts_g):
    """2160x3840 -> 4320x7680: (a) the frame equals the float64 port byte for byte; (b) fused == unfused; (c) any
    interior crop with a 7-px halo reproduces the frame's bytes; (d) 8 strips with 7-row halos, ranks emulated one
    after the other on this GPU, stitch to the frame."""
    from lerf_pytorch_amd import dist as ldist
    img = _frame("noise", 2160, 3840, 61)
    x = torch.from_numpy(img).cuda()
    full = eng_g.sr(x, 2)
    assert tuple(full.shape) == (4320, 7680, 3)
    _bytes_equal(full.cpu().numpy(), co.sr_u8(img, luts_g, 2, 2), "LeRF-G 4K->8K noise")
    assert torch.equal(full, eng_g.sr(x, 2, fused=False))
    for (y0, x0, h, w) in ((64, 64, 128, 192), (1000, 2000, 33, 47), (2090, 3700, 60, 100)):
        crop = x[y0 - 7:y0 + h + 7, x0 - 7:x0 + w + 7].contiguous()
        oc = eng_g.sr(crop, 2)
        assert torch.equal(oc[14:-14, 14:-14], full[2 * y0:2 * (y0 + h), 2 * x0:2 * (x0 + w)])
    geo = eng_g.sr_geometry((2160, 3840), 2)
    parts = []
    for r in range(8):
        plan = ldist.StripPlan(2160, 8, r, eng_g.support, geo.host["left_r"])
        assert plan.y1 - plan.y0 == 270 and plan.halo == 7 and plan.check_support(geo.host["left_r"])
        parts.append(ldist.sr_strip(eng_g, x[plan.ylo:plan.yhi].contiguous(), plan, geo))
    assert torch.equal(torch.cat(parts, dim=0), full)


def test_config5_batch_of_frames(torch, eng_g):
    """a batch launch equals its frames one by one (4K frames, 3 of them to bound memory)"""
    rng = np.random.default_rng(62)
    x = torch.from_numpy(rng.integers(0, 256, (3, 2160, 3840, 3), dtype=np.uint8)).cuda()
    out = eng_g.sr(x, 2)
    for b in range(3):
        assert torch.equal(out[b], eng_g.sr(x[b], 2))


@pytest.mark.parametrize("n,hw", [(3, (1080, 1920)), (7, (600, 1100)), (19, (300, 700)), (4, (300, 700))])
def test_batches_through_the_xcd_tile_order(torch, co, eng_g, luts_g, n, hw):
    """Launches of >= 1024 workgroups hand every XCD a contiguous eighth of the (frame, tile) sequence (xcd_order); the
    grid sizes here (3 x 510 = 1530, 7 x 180 = 1260, 19 x 55 = 1045: remainders 2, 4, 5 modulo 8; 4 x 55 stays on the linear
    order below the threshold) exercise its remainder handling: a batch equals its frames one by one, and the C port on one of them."""
    rng = np.random.default_rng(63 + n)
    x = torch.from_numpy(rng.integers(0, 256, (n,) + hw + (3,), dtype=np.uint8)).cuda()
    out = eng_g.sr(x, 2)
    for b in range(n):
        assert torch.equal(out[b], eng_g.sr(x[b], 2)), "frame %d of %d" % (b, n)
    _bytes_equal(out[n - 1].cpu().numpy(), co.sr_u8(x[n - 1].cpu().numpy(), luts_g, 2, 2), "last frame of a batch of %d" % n)


# ------------------------------------------------------------------------------------------------ float32 outputs
@pytest.mark.parametrize("model,scale", [("lerf-g", (2.0, 2.0)), ("lerf-g", (3.0, 3.0)), ("lerf-l", (1.5, 2.0))])
def test_float32_outputs_abs_error_sr(torch, co, eng_g, eng_l, luts_g, luts_l, model, scale):
    """float32 SR outputs of the class/engine path against the float64 oracle at 540p (ABSOLUTE error, 0..255)."""
    eng, luts, lin = (eng_g, luts_g, False) if model == "lerf-g" else (eng_l, luts_l, True)
    img = _frame("noise", 540, 960, 71)
    o32 = eng.sr_float(img, scale)
    feat, hq = co.lut_stages(img, luts, 1 if lin else 3)
    ref = co.resize(feat, hq, scale[0], scale[1], 2, 1.0 if lin else 10.0, "linear" if lin else "gauss")
    err = float(np.max(np.abs(o32.astype(np.float64) - ref)))
    print("float32 SR %s x%s: max abs error %.3e (0..255 scale)" % (model, scale, err))
    assert err <= F32_ABS_TOL, err


@pytest.mark.parametrize("name,M", [("isc", M_ISC), ("osc", M_OSC)])
def test_float32_outputs_abs_error_warp(torch, co, eng_g, luts_g, name, M):
    img = _frame("natural", 540, 960, 72)
    Mh = M.copy()
    o32, _ = eng_g.warp(img, Mh, (1080, 1920), out="f32")
    feat, hq = co.lut_stages(img, luts_g, 3)
    ref = co.warp(feat, hq, Mh, (1080, 1920), 2, 10.0, "gauss")
    assert np.array_equal(np.isnan(o32), np.isnan(ref))
    ok = ~np.isnan(ref)
    err = float(np.max(np.abs(o32.astype(np.float64)[ok] - ref[ok])))
    print("float32 warp %s: max abs error %.3e (0..255 scale)" % (name, err))
    assert err <= F32_ABS_TOL, err


# ------------------------------------------------------------------------------------------------ RCCL, 2 ranks
_NCCL_WORKER = r"""
import os, sys
import numpy as np
import torch
import torch.distributed as dist
sys.path.insert(0, os.environ["LERF_REPO"])
import lerf_pytorch_amd as L
from lerf_pytorch_amd import dist as ldist

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(rank)
dist.init_process_group("nccl", device_id=torch.device("cuda", rank))
H, W, N = 2160, 3840, 2
rng = np.random.default_rng(77)
img = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)            # the same frames on every rank
eng = L.LerfEngine.shipped("lerf-g")
for scale in (2.0, 1.5):
    geo = eng.sr_geometry((H, W), scale)
    plan = ldist.StripPlan(H, world, rank, eng.support, geo.host["left_r"])
    buf = ldist.StripBuffer(plan, N, W, 3, torch.uint8, torch.device("cuda"))
    buf.own.copy_(torch.from_numpy(img[:, plan.y0:plan.y1]).cuda())
    for rep in range(2):                                             # the persistent buffer is reused across steps
        ext = buf.exchange()
    torch.cuda.synchronize()
    assert np.array_equal(ext.cpu().numpy(), img[:, plan.ylo:plan.yhi]), "halo rows differ"
    mine = ldist.sr_strip(eng, ext, plan, geo)                       # [N, rows, oW, 3]
    counts = [ldist.StripPlan(H, world, r, eng.support, geo.host["left_r"]).out_rows() for r in range(world)]
    full = eng.sr(torch.from_numpy(img).cuda(), scale)
    for b in range(N):
        whole = ldist.gather_strips(mine[b], counts)
        assert torch.equal(whole, full[b]), "stitched strips differ from the full frame (scale %s)" % scale
        single = ldist.sr_frame_strips(eng, torch.from_numpy(img[b, plan.y0:plan.y1]).cuda(), H, scale, gather=True)
        assert torch.equal(single, full[b])
# 2-D blocks over the same ranks (8 ranks: 2 x 4; 2 ranks: 1 x 2): edges + corners in one batch_isend_irecv, one pack and
# one unpack launch, tiles over the owned block, one launch per frame batch
grid = ldist.block_grid(world)
for scale in (2.0, 1.5):
    geo = eng.sr_geometry((H, W), scale)
    lr, lc = geo.host["left_r"], geo.host["left_c"]
    plan = ldist.BlockPlan(H, W, grid, rank, eng.support, lr, lc)
    buf = ldist.BlockBuffer(plan, N, 3, torch.uint8, torch.device("cuda"), lr, lc)
    for rep in range(2):
        buf.ext.zero_()
        buf.own.copy_(torch.from_numpy(np.ascontiguousarray(img[:, plan.y0:plan.y1, plan.x0:plan.x1])).cuda())
        ext = buf.exchange()
    torch.cuda.synchronize()
    assert np.array_equal(ext.cpu().numpy(), img[:, plan.ylo:plan.yhi, plan.xlo:plan.xhi]), "block halo differs"
    mine = ldist.sr_block(eng, ext, plan, geo)                       # [N, h, w, 3]
    rects = [ldist.BlockPlan(H, W, grid, r, eng.support, lr, lc).out_rect() for r in range(world)]
    full = eng.sr(torch.from_numpy(img).cuda(), scale)
    whole = ldist.gather_blocks(mine, rects, geo.out_hw)
    assert torch.equal(whole, full), "stitched blocks differ from the full frames (scale %s)" % scale
    single = ldist.sr_frame_blocks(eng, torch.from_numpy(np.ascontiguousarray(img[0, plan.y0:plan.y1, plan.x0:plan.x1])).cuda(), H, W, scale,
                                   gather=True)
    assert torch.equal(single, full[0])
dist.barrier()
dist.destroy_process_group()
print("rank %d ok" % rank)
"""


def test_rccl_two_rank_halo_exchange_and_stitch(torch, tmp_path):
    """min(device_count, 8) processes (at least 2), one GPU each, backend nccl (= RCCL): halo rows (strips) and halo
    rectangles (2-D blocks, edges + corners) arrive in place, the stitched strips / blocks equal the full frame at x2
    and x1.5 (unequal parts).  Skipped on a 1-GPU box."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs (this box has %d)" % torch.cuda.device_count())
    world = min(torch.cuda.device_count(), 8)
    script = tmp_path / "nccl_worker.py"
    script.write_text(_NCCL_WORKER)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0", LERF_REPO=REPO)
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=900)
        except subprocess.TimeoutExpired:
            p.kill()
            o, _ = p.communicate()
        outs.append(o.decode())
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, outs[r][-3000:])


@pytest.mark.parametrize("launcher,extra", [("bare", []), ("torchrun", []), ("bare", ["--config", "5", "--mode", "strips", "--frames", "2"]),
                                            ("torchrun", ["--config", "5", "--mode", "blocks", "--frames", "2"])])
def test_bench_two_ranks_on_one_shared_gpu(torch, launcher, extra):
    """bench.py's multi-rank code (rank -> device, barriers around the timed region, MAX over the ranks, rank 0 prints the one
    line, weak-scaling aggregate; config 5: the strip / block partition with its pack, exchange and unpack every step) run for
    real on a one-GPU box: LERF_BENCH_SHARE_GPU=1 puts both ranks on GPU 0 and the collectives on gloo (RCCL refuses two ranks
    on one device).  Both ways the driver may start it: bare (the GPU-free parent spawns the ranks) and under torch.distributed.run."""
    import json
    env = dict(os.environ, LERF_BENCH_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    args = [os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--sustained", "0"] + extra
    if launcher == "bare":
        cmd = [sys.executable] + args
    else:
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
               "--master-port", str(port)] + args
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["steps"] == 3 and j["value"] > 0 and j["config"]["backend"].startswith("gloo")
    assert j["config"]["ranks_reported_by_rccl"] == 0          # the hook's label; a real N-GPU line carries N (bench.py asserts it)
    if not extra:
        assert j["scaling"] == "weak" and j["config"]["frames_per_step_per_gpu"] == 8
        # the aggregate counts both ranks' frames: 2 x 8 frames of 3840 x 2160 per step
        assert abs(j["value"] - 2 * 8 * 3840 * 2160 / (j["ms_per_step"] * 1e-3) / 1e6) < 1e-3 * j["value"]
    else:
        assert j["scaling"] == "strong" and j["config"]["mode"] == extra[3]
        # strong scaling: the batch of whole 8K frames once, whatever the number of ranks
        assert abs(j["value"] - 2 * 7680 * 4320 / (j["ms_per_step"] * 1e-3) / 1e6) < 1e-3 * j["value"]


def test_bench_plain_line_is_the_headline_alone(torch):
    """A plain `bench.py --gpus 1 --steps N --warmup W` sets up, times its steps and prints the line: the headline fields and
    none of the secondary legs of --full; with LERF_TEST_PERF=1, at most 30 s of the whole run outside its steps."""
    import json
    import time
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "LERF_BENCH_SHARE_GPU"):
        env.pop(k, None)
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    j = json.loads([l for l in r.stdout.decode().splitlines() if l.startswith("{")][-1])
    assert j["steps"] == 20 and j["warmup"] == 5 and j["value"] > 0 and j["ms_per_step"] > 0 and j["higher_is_better"] is True
    assert j["unit"] == "Mpix/s" and j["metric"].startswith("Mpix/s LeRF-G x2 SR") and j["dtype"] == "i32+f32 (u8 io)"
    moved = {"sustained", "mpix_s_other_input", "latency_one_frame_per_launch", "end_to_end", "psnr_delta_vs_ref_db", "roofline_lds",
             "cpu_baseline", "cpu_baseline_single_thread", "cpu_baseline_half_budget", "parity_vs_cpu_port", "other_configs"}
    assert not moved & set(j), sorted(moved & set(j))
    assert not PERF or wall - (20 + 5) * j["ms_per_step"] * 1e-3 < 30.0, wall


def test_bench_default_line_carries_every_baseline_config(torch):
    """the `python bench.py --full` line holds a leg for configs 3, 4, 5 (one GPU) and S = 4, each with its own
    in-run byte parity against the C port and a roofline block; and `--config 5 --frames 4` (the N = 1 point of a scaling run
    in frames mode) agrees with the config-5 leg."""
    import json
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "LERF_BENCH_SHARE_GPU"):
        env.pop(k, None)
    base = [sys.executable, os.path.join(REPO, "bench.py"), "--steps", "10", "--warmup", "3", "--sustained", "0"]
    r = subprocess.run(base + ["--full", "--no-end-to-end", "--no-cpu-baseline"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    j = json.loads([l for l in r.stdout.decode().splitlines() if l.startswith("{")][-1])
    assert j["n_gpus"] == 1 and j["config"]["ranks_reported_by_rccl"] == 1 and j["config"]["library"].endswith("liblerf_hip.so")
    legs = j["other_configs"]
    assert sorted(legs) == ["config1_256x256_tile", "config2_support4", "config3_lerf_l_x1.5x2.0", "config4_warp_isc", "config5_4k_to_8k_one_gpu"]
    for name, leg in legs.items():
        assert "error" not in leg, (name, leg)
        assert leg["parity_vs_cpu_port"]["mismatches"] == 0 and leg["parity_vs_cpu_port"].get("mask_mismatches", 0) == 0
        # wall-clock expectations only on request (LERF_TEST_PERF=1): a shared or throttled box must not fail a correctness suite
        if name == "config1_256x256_tile":
            assert leg["mpix_s"] > 0 and leg["cpu_port_one_thread_mpix_s"] > 0
            assert not PERF or leg["mpix_s"] > 1000
            continue
        assert leg["mpix_s"] > 0 and (not PERF or leg["mpix_s"] > 5000)
        assert leg["roofline"]["bound"] == "hbm" and leg["roofline"]["achieved"] > 0 and "traffic" in leg["roofline"]
    assert not PERF or sum(leg["leg_seconds"] for leg in legs.values()) < 30.0
    tol = 0.03 if PERF else 0.10                               # the same workload through two entry points of bench.py
    ratios = []
    for attempt in range(2):                                   # (two runs of a 4.6-ms step on a shared box: one retry before it counts)
        r5 = subprocess.run(base + ["--config", "5", "--frames", "4", "--mode", "frames", "--no-cpu-baseline", "--no-other-input"], env=env,
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
        assert r5.returncode == 0, r5.stderr.decode()[-3000:]
        j5 = json.loads([l for l in r5.stdout.decode().splitlines() if l.startswith("{")][-1])
        assert j5["config"]["ranks_reported_by_rccl"] == 1 and j5["config"]["frames_per_step_per_gpu"] == 4
        ratios.append(j5["value"] / legs["config5_4k_to_8k_one_gpu"]["mpix_s"])
        if abs(ratios[-1] - 1.0) < tol:
            break
    assert abs(ratios[-1] - 1.0) < tol, (ratios, legs["config5_4k_to_8k_one_gpu"]["mpix_s"])
