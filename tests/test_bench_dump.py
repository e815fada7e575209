"""bench.py --dump-outputs: what the timed path computed in its last step, written as float32 .npy files under DIR (a seeded
sample of a large output, at most 64 MB in all), identical from run to run and equal to the C port of the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, REPO)
import bench  # noqa: E402


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_outputs_full_and_sampled(tmp_path):
    import torch
    g = torch.Generator().manual_seed(0)
    small = torch.randint(0, 256, (1, 40, 56, 3), generator=g, dtype=torch.uint8)
    big = torch.randint(0, 256, (2, 1100, 1500, 3), generator=g, dtype=torch.uint8)          # 9.9 M elements: sampled
    d = str(tmp_path / "a")
    desc = bench.dump_outputs(torch, d, {"small": small, "out": big})
    assert desc["arrays"]["small"]["written"] == "full" and desc["arrays"]["out"]["shape"] == [2, 1100, 1500, 3]
    assert sorted(os.listdir(d)) == ["out_sample.npy", "out_sample_index.npy", "small.npy"]
    assert _dir_bytes(d) <= 64 << 20
    s = np.load(os.path.join(d, "small.npy"))
    assert s.dtype == np.float32 and np.array_equal(s, small.numpy().astype(np.float32))
    v, i = np.load(os.path.join(d, "out_sample.npy")), np.load(os.path.join(d, "out_sample_index.npy"))
    assert v.dtype == np.float32 and i.dtype == np.float64 and v.shape == i.shape == (bench.DUMP_SAMPLE,)
    assert np.all(np.diff(i) > 0) and i[-1] < big.numel()
    assert np.array_equal(v, big.numpy().reshape(-1)[i.astype(np.int64)].astype(np.float32))
    # the sample depends on the output's shape only
    d2 = str(tmp_path / "b")
    bench.dump_outputs(torch, d2, {"out": torch.zeros_like(big)})
    assert np.array_equal(np.load(os.path.join(d2, "out_sample_index.npy")), i)


@pytest.mark.parametrize("extra", [["--steps", "0"], ["--warmup", "-1"], ["--dump-outputs", "x", "--config", "1"],
                                   ["--dump-outputs", "x", "--path", "callsite"]])
def test_bench_refuses_bad_arguments(extra):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + extra, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "error" in r.stderr


@pytest.mark.gpu
def test_bench_dump_is_repeatable_and_equals_the_cpu_port(tmp_path):
    from oracle import c_oracle
    steps = 3
    runs = []
    for k in range(2):
        d = str(tmp_path / ("run%d" % k))
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", str(steps), "--warmup", "1", "--frames", "1",
                            "--sustained", "0", "--no-cpu-baseline", "--no-other-input", "--no-end-to-end", "--no-psnr",
                            "--dump-outputs", d], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert j["steps"] == steps and j["dump_outputs"]["arrays"]["out"]["shape"] == [1, 2160, 3840, 3]
        assert _dir_bytes(d) <= 64 << 20
        runs.append((np.load(os.path.join(d, "out_sample.npy")), np.load(os.path.join(d, "out_sample_index.npy"))))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    # the same seeded frame through the C port of the oracle: the sampled bytes are its bytes
    frame = bench.synth_frames("noise", 1, 1000, 1080, 1920, channels=3)[0]
    c_oracle.set_threads(bench.host_cpu_budget()[0])
    want = c_oracle.sr_u8(frame, bench._oracle_luts("lerf-g"), 2.0, 2.0, S=2)
    v, i = runs[0]
    assert np.array_equal(v, want.reshape(-1)[i.astype(np.int64)].astype(np.float32))
