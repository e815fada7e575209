"""The LeRF-Net backward (lerf_imdn_bwd.hip) where a workgroup of imdn_wgrad_kernel walks several tiles -- more than
MAX_SLABS = 256 tiles, which train_model.py's default batch (16 crops of 48 x 48, 288 tiles) meets on every step -- and
on exact ties of the LeakyReLU derivative and of the clamp mask.

The batches are imdn_tile_cases.py's: many tiny images, screened in float64 so that no float32 run can flip a LeakyReLU
sign or the clamp mask (test_imdn_hazard_cpu.py checks that on the CPU: float32 autograd within 1e-5 of float64).

Tolerances.
  float64: test_gpu_imdn_train.py's rule, unchanged: per parameter tensor and for grad_x e = max |t - t64| / max |t64|
    against float64 CPU autograd, e_stock the same figure for stock float32 autograd on the GPU, e_stock <= 1e-3 and
    e_hip <= 4 e_stock + 1e-6.  A lost, doubled or overwritten tile among 257 to 600 moves a weight gradient by about
    1 / sqrt(tiles), 4 to 6 %.
  census: exact.  The gradient is a small integer at one pixel per tile, so the upsampler's bias gradient is a sum of
    integers below 2^24 in any order.
  split runs: grad_x bitwise (dgrad has no slabs).
  ties: the rule above, and the upsampler's bias gradient of the two channels at y == +-1 against the float64 sum
    factor * sum G[:, n] within 1e-6 * factor * sum |G[:, n]|, about 3e-4 * factor: a float32 sum of 360 normal terms
    whose partial sums stay near sqrt(360) = 19 collects about 19 roundings of 6e-8 * 19, 2e-5 * factor.  A strict
    comparison gives 0 instead of the sum, which the test requires to exceed 100 bounds."""
import numpy as np
import pytest

import imdn_grad_ref as GR
import imdn_tile_cases as T
from test_gpu_imdn_train import _flat, _run, _unflat, torch  # noqa: F401 (torch is the module fixture)

pytestmark = pytest.mark.gpu

_stock = {}


def _stock_grads(torch, key, sd, x, G, post):
    """stock float32 autograd on the GPU, once per batch"""
    if key not in _stock:
        _stock[key] = GR.net_grads(torch, sd, T.PREFIX, x, G, post, torch.float32, "cuda")[1:]
    return _stock[key]


def _check_rule(label, gh, gx, gs, gxs, g64, gx64):
    """the float64 rule on every tensor and grad_x; prints the worst pair"""
    worst = (-1.0, 0.0, "")
    fails = []
    for k, t, ts, t64 in [(k, gh[k], gs[k], g64[k]) for k in g64] + [("grad_x", gx, gxs, gx64)]:
        e_hip, e_stock = GR.rel_err(t, t64), GR.rel_err(ts, t64)
        assert e_stock <= 1e-3, (k, e_stock)
        if e_hip > worst[0]:
            worst = (e_hip, e_stock, k)
        if not e_hip <= 4 * e_stock + 1e-6:
            fails.append((k, e_hip, e_stock))
    print("%s: worst e_hip %.3g (e_stock %.3g) at %s" % (label, worst[0], worst[1], worst[2]))
    assert not fails, fails


@pytest.mark.parametrize("name", list(T.CASES))
def test_multi_tile_backward_matches_float64(torch, name):
    nf, in_nc, out_nc, B, H, W, post = T.CASES[name]
    sd, x, G, kept = T.batch(name)
    _, g64, gx64 = T.reference(name)
    gs, gxs = _stock_grads(torch, name, sd, x, G, post)
    _, gw, gx = _run(torch, sd, nf, in_nc, out_nc, x, G, post)
    gh = _unflat(sd, T.PREFIX, gw.cpu().numpy())
    _check_rule("%s %s, %d tiles, kept %.3f" % (name, T.CASES[name], T.n_tiles(B, H, W), kept), gh, gx.cpu().numpy(), gs, gxs,
                g64, gx64)


@pytest.mark.parametrize("name", ["a", "c", "e"])
def test_tile_census_is_exact(torch, name):
    nf, in_nc, out_nc, B, H, W, _ = T.CASES[name]
    sd, x, _, _ = T.batch(name)
    G, sums = T.census(out_nc, B, H, W)
    assert int((G != 0).sum()) == T.n_tiles(B, H, W) and sums.sum() < 1 << 24
    _, gw, _ = _run(torch, sd, nf, in_nc, out_nc, x, G, 0, want_gx=False)
    got = _unflat(sd, T.PREFIX, gw.cpu().numpy())[T.PREFIX + "model.2.bias"]
    assert got.dtype == np.float32 and np.array_equal(got, sums.astype(np.float32)), (got, sums)


def test_split_runs_localise_the_walk(torch):
    """the whole of batch c (600 tiles) against its three thirds (200 tiles each, no walk): a failure of e_whole with a
    sound e_split lies in the walk"""
    name = "c"
    nf, in_nc, out_nc, B, H, W, post = T.CASES[name]
    sd, x, G, _ = T.batch(name)
    _, g64, gx64 = T.reference(name)
    gs, gxs = _stock_grads(torch, name, sd, x, G, post)
    _, gw, gx = _run(torch, sd, nf, in_nc, out_nc, x, G, post)
    parts = []
    for i in range(0, B, 100):
        assert T.n_tiles(100, H, W) <= T.MAX_SLABS
        parts.append(_run(torch, sd, nf, in_nc, out_nc, x[i:i + 100], G[i:i + 100], post)[1:])
    assert torch.equal(gx, torch.cat([p[1] for p in parts])), "grad_x of the whole batch differs from its thirds"
    gh = _unflat(sd, T.PREFIX, gw.cpu().numpy())
    split = _unflat(sd, T.PREFIX, sum(p[0].cpu().numpy().astype(np.float64) for p in parts))
    k = max(g64, key=lambda k: GR.rel_err(gh[k], g64[k]))
    print("c whole against thirds: worst e_whole %.3g, e_split %.3g there, worst e_split %.3g (e_stock %.3g) at %s"
          % (GR.rel_err(gh[k], g64[k]), GR.rel_err(split[k], g64[k]), max(GR.rel_err(split[j], g64[j]) for j in g64),
             GR.rel_err(gs[k], g64[k]), k))
    _check_rule("c whole", gh, gx.cpu().numpy(), gs, gxs, g64, gx64)


@pytest.mark.parametrize("post", [1, 2])
def test_exact_ties_take_the_inclusive_side(torch, post):
    """pre-activations of exactly 0 (slope 0.05, as torch's leaky_relu) and raw outputs of exactly +-1 (inside the clamp,
    as torch.clamp's derivative)"""
    nf, in_nc, out_nc, B, H, W = T.TIED
    sd, x, G, kept = T.tied_batch(post)
    y64, g64, gx64 = T.reference("tied", post)
    assert np.all(y64[:, 0] == 1) and np.all(y64[:, 2] == -1)
    gs, gxs = _stock_grads(torch, ("tied", post), sd, x, G, post)
    out, gw, gx = _run(torch, sd, nf, in_nc, out_nc, x, G, post)
    edge = {1: (254.0, 0.0), 2: (1.0, 0.0)}[post]
    assert bool((out[:, 0] == edge[0]).all()) and bool((out[:, 2] == edge[1]).all())
    gh = _unflat(sd, T.PREFIX, gw.cpu().numpy())
    for e in T.tied_exempt(nf):
        if isinstance(e, tuple):                                    # the zeroed rows are reached through the 0.05 slope
            assert g64[T.PREFIX + e[0] + ".bias"][e[1]] != 0
    _check_rule("ties post %d, kept %.3f" % (post, kept), gh, gx.cpu().numpy(), gs, gxs, g64, gx64)
    factor = 127.0 if post == 1 else 0.5
    gb = gh[T.PREFIX + "model.2.bias"]
    for n in (0, 2):
        g = G[:, n].astype(np.float64)
        bound = 1e-6 * factor * np.abs(g).sum()
        assert g.size == 360 and abs(factor * g.sum()) > 100 * bound    # a masked-out channel reads 0: far outside the bound
        assert abs(float(gb[n]) - factor * g.sum()) <= bound, (n, gb[n], factor * g.sum())
