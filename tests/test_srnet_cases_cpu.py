"""CPU pins of srnet_cases.py: what test_gpu_srnet_paths.py relies on when it compares lerf_srnet.hip with float64
autograd bit for bit.  Nothing here touches the GPU.

For every integer case: float32 autograd equals float64 autograd in every tensor; for every gradient entry the sum of the
absolute values of its terms, taken through the absolute network, is below 2^24 (so any summation order is exact); the
gradients are dense enough to notice a lost block (>= 20 % of every weight tensor, >= half of the reached image);
every hidden layer has open and closed gates; in each of layers 1..5 at least 1 % of all (position, neuron) pairs sit on
a pre-activation of exactly 0 with a non-zero incoming gradient; and relu'(0) = 1 changes an integer in every gated
tensor, in all gates at once (float64 autograd) and in each gate alone.  W6 and b6 pass no gate and cannot differ.

For the random and the zero-bias batches: every pre-activation that is not an exact zero keeps |z| > Z_WIDTH in float64
and float32 autograd stays within Z_WIDTH / 4 of it, so no float32 run flips a gate; the case list reaches every class of
the host rule (test_case_list_reaches_every_path)."""
import numpy as np
import pytest
import torch

import srnet_cases as S


def test_host_rule_restated():
    assert (S.n_tiles(1, 181, 182), S.n_slabs(1, 181, 182), S.last_rows(1, 181, 182)) == (1030, 512, 14)
    assert [S.walk(g, 1, 181, 182) for g in (0, 5, 6, 511)] == [3, 3, 2, 2]
    assert (S.n_tiles(1, 128, 128), S.n_slabs(1, 128, 128), S.last_rows(1, 128, 128)) == (512, 512, 32)
    assert [S.walk(g, 2, 59, 139) for g in (0, 1, 511)] == [2, 1, 1] and S.n_tiles(2, 59, 139) == 513
    assert (S.n_tiles(1, 1, 1), S.n_slabs(1, 1, 1), S.last_rows(1, 1, 1)) == (1, 1, 1)
    assert S.last_rows(1, 1, 31) == 31 and S.n_tiles(1, 1, 33) == 2
    assert S.straddles(3, 5, 7) and not S.straddles(2, 8, 8) and not S.straddles(1, 5, 7)
    for P, h, w in ((1, 181, 182), (3, 90, 122), (2, 59, 139), (3, 5, 7)):
        assert sum(S.walk(g, P, h, w) for g in range(S.n_slabs(P, h, w))) == S.n_tiles(P, h, w)


def test_case_list_reaches_every_path():
    """the coverage table: every class of the host rule has an integer case; the three-tile walk has one per outC"""
    table = {c: [] for c in S.CLASSES}
    for name, (mode, outC, P, h, w, extra, _) in S.INT_CASES.items():
        for c in S.classes(P, h, w):
            table[c].append(name)
    missing = [c for c, v in table.items() if not v]
    assert not missing, missing
    for c, v in table.items():
        print("%-42s %s" % (c, " ".join(v)))
    cases = list(S.INT_CASES.values())
    assert {c[0] for c in cases} >= set("sct")
    assert {c[1] for c in cases} == {1, 3, 4}
    assert {c[5] == 0 for c in cases} == {True, False}                    # bd equal to and above the reach
    assert {S.INT_CASES[n][1] for n in table["tiles >= 1025: walks of three and of two"]} == {1, 3, 4}
    assert {S.INT_CASES[n][1] for n in table["one position"] + table["one partial tile of 31"]} >= {3, 4}
    for name, (mode, outC, P, h, w, extra) in S.RAND_CASES.items():
        assert "tiles >= 1025: walks of three and of two" in S.classes(P, h, w), name
    assert {c[1] for c in S.RAND_CASES.values()} == {3, 4}
    # the split runs of walk3-t: each plane of the integer case, each third of the random one stays below the walk
    _, _, P, h, w, _, _ = S.INT_CASES["walk3-t"]
    assert P > 1 and S.n_tiles(1, h, w) < S.MAX_SLABS
    _, _, P, h, w, _ = S.RAND_CASES["walk3-t"]
    assert P % 3 == 0 and S.n_tiles(P // 3, h, w) < S.MAX_SLABS and (P // 3 * h * w) % S.ROWS      # other tiles than the whole
    # the accumulation check needs pixels no tap reaches
    for name in ("walk3-t", "t513", "straddle"):
        mode, _, P, h, w, extra, _ = S.INT_CASES[name]
        assert extra > 0 and not S.reached(mode, P, h, w, S.REACH[mode] + extra).all()


@pytest.mark.parametrize("outC", [1, 3, 4])
def test_integer_weights_are_what_the_docstring_says(outC):
    d = S.integer_weights(outC, 3)
    t = S.tensors_of(d)
    assert all(np.array_equal(a, np.round(a)) for a in t)
    assert np.abs(t[0]).max() <= 2 and all(a.min() >= -2 and a.max() <= 1 for a in t[1:10:2])
    assert not np.any(t[11])
    for li in range(5):
        W, b = t[2 * li], t[2 * li + 1]
        assert np.array_equal(b[0::2], b[1::2])
        diff = W[0::2] - W[1::2]
        assert np.all(np.any(diff != 0, axis=1)), "a pair with identical rows"
        # what moves stays inside an input pair: the two channels of every pair sum alike in both rows
        assert np.array_equal(W[0::2, 0::2] + W[0::2, 1::2], W[1::2, 0::2] + W[1::2, 1::2])
        if li:
            assert set(np.unique(W)) == {-1, 0, 1} and np.all(np.abs(W).sum(1) == 6)
    W6 = t[10]
    assert np.array_equal(W6[:, 0::2], -W6[:, 1::2]) and set(np.unique(W6[:, 0::2])) == {0, 1, 2}
    assert np.all((W6[:, 0::2] != 0).sum(1) == (48 if outC >= 3 else 104))


@pytest.mark.parametrize("mode", list("sctd"))
def test_integer_image_makes_the_pixel_pairs_equal(mode):
    bd = S.REACH[mode] + 1
    img = S.integer_image(mode, 2, 19, 23, bd, 5)
    x = S.tuples(img, mode, 19, 23)
    assert np.array_equal(x[:, 0], x[:, 1]) and np.array_equal(x[:, 2], x[:, 3])
    assert set(np.unique(img)) == {0, 1, 2, 3}
    black = ~x.any(1)
    # the band (a sixth of the lines; the middle diagonals of mode t are the long ones) and, where one line decides all
    # four pixels, the quarter of the lines that drew a 0
    assert 0.05 < black.mean() < 0.6
    assert len(np.unique(x, axis=0)) >= 4


@pytest.mark.parametrize("name", list(S.INT_CASES))
def test_integer_case_is_exact_and_telling(name):
    d, img, G, geo = S.int_case(name)
    assert set(np.unique(G)) <= set(range(-3, 4)) and img.min() >= 0 and img.max() <= 3
    c = S.census(d, img, G, geo)
    print(name, {k: (np.round(v, 3).tolist() if isinstance(v, list) and isinstance(v[0], float) else v) for k, v in c.items()})
    assert c["float32 equals float64"]
    assert c["forward is zero"] and c["integers"] and c["unreached grad_img is zero"]
    assert c["largest sum of absolute terms"] < 2 ** 24
    assert min(c["non-zero share"]) >= 0.2, c["non-zero share"]
    assert c["non-zero share of the reached grad_img"] >= 0.5
    assert all(c["gates open and closed"])
    assert min(c["tie share"]) >= 0.01, c["tie share"]
    assert all(c["open at zero differs"][:10]), c["open at zero differs"]
    assert not any(c["open at zero differs"][10:])                        # W6 and b6 pass no gate
    assert all(c["open_alone"]), c["open_alone"]
    assert S.census_ok(c) == []
    # the shared reference is the same float64 autograd
    y, gs, gx = S.int_reference(name)
    y2, gs2, gx2 = S.autograd(d, geo[0], img, G, geo[3], geo[4])
    assert np.array_equal(gx, gx2) and all(np.array_equal(a, b) for a, b in zip(gs, gs2))


def test_pack_and_unpack_agree_with_the_layout():
    d = S.integer_weights(4, 3)
    flat = S.pack(d)
    assert flat.size == 64 * 4 + 64 + 64 * (64 + 128 + 192 + 256) + 4 * 64 + 4 * 320 + 4
    assert all(np.array_equal(a, b) for a, b in zip(S.unpack(flat, 4), S.tensors_of(d)))


@pytest.mark.parametrize("name", list(S.RAND_CASES))
def test_random_batches_are_screened(name):
    """no float32 run can flip a gate: every |z| above Z_WIDTH in float64, float32 within Z_WIDTH / 4 of it"""
    d, img, G, (mode, outC, P, h, w, bd), kept = S.rand_case(name)
    assert img.shape == (P, h + bd, w + bd) and kept > 0.25
    _, _, _, z64, _ = S.autograd(d, mode, img, G, h, w, internals=True)
    _, _, _, z32, _ = S.autograd(d, mode, img, G, h, w, dtype=torch.float32, internals=True)
    print(name, "kept %.3f" % kept, "min |z| %.3g" % min(np.abs(a).min() for a in z64),
          "max |z32 - z64| %.3g" % max(np.abs(a - b).max() for a, b in zip(z64, z32)))
    for a, b in zip(z64, z32):
        assert np.abs(a).min() > S.Z_WIDTH and np.abs(a - b).max() < S.Z_WIDTH / 4
        assert (a > 0).any() and (a < 0).any()


def test_tied_batch_is_screened():
    """zero biases and a black band: the ties are exact zeros in float32 too, and no other pre-activation of a float32
    run comes near a sign flip (float32 within Z_WIDTH / 4 of float64, every other |z| above Z_WIDTH)"""
    d, img, G, (mode, outC, P, h, w, bd), tied, kept = S.tied_batch()
    assert all(not np.any(a) for a in S.tensors_of(d)[1::2])
    assert 0.25 < tied.mean() < 0.5 and kept > 0.25
    _, _, _, z64, da64 = S.autograd(d, mode, img, G, h, w, internals=True)
    _, _, _, z32, _ = S.autograd(d, mode, img, G, h, w, dtype=torch.float32, internals=True)
    for a, b, da in zip(z64, z32, da64):
        assert not np.any(a[tied]) and not np.any(b[tied])
        assert np.abs(a[~tied]).min() > S.Z_WIDTH and np.abs(a - b).max() < S.Z_WIDTH / 4
        assert np.any(da[tied] != 0)                                      # the ties carry gradient: >= would let it through
    # relu'(0) = 1 moves every bias gradient of layers 1..5 by far more than the tolerance of the GPU test (1e-3 at most)
    _, gs, _ = S.tied_reference()
    _, gso, _ = S.autograd(d, mode, img, G, h, w, open_at_zero=True)
    for i in range(1, 10, 2):
        assert S.rel_err(gso[i], gs[i]) > 0.05, (S.TENSORS[i], S.rel_err(gso[i], gs[i]))
