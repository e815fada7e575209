"""The SWF2LUT LUT pass (lerf_train.hip: lerf_swf2lut_interp_f32 / _bwd_f32) on every launch path of its backward,
through the C ABI, against the float64 oracle (oracle.swf2lut_interp) with a per-entry error bound.

The backward's host side picks the path from the shape (restated in `launch` below): a workgroup owns a band of
rows_per_band = clamp(4096 // w, 1, h) rows of one plane; a plane of one band flushes its image gradient with a plain
`+=`, several bands flush with atomics (halo rows are shared); when (rows_per_band + bd) * (w + bd) * 4 bytes exceed
40 KB the image gradient bypasses LDS and goes to global atomics; w > 4096 gives one-row bands.  LUT-row gradients go
through a 4096-slot LDS hash table; a row whose slot is held by another row adds to global memory directly.  The case
list is checked against the rule (test_case_list_reaches_every_path), so a change of the rule that leaves a path
unreached fails here.

Forward: integer products and sums below 2^24, so float32 is exact -- bit for bit against the oracle.

Backward, per entry.  Let t_1..t_N be the float64 terms the oracle sums into one entry (N = 'count', S = sum |t_i|
= 'abs' of oracle.swf2lut_interp(..., bounds=True)) and p the buffer's prior content.  The kernel forms each term
with at most two float32 roundings (grad_weight: (g * w_n) * 127, grad_img: g * (P_{n+1} - P_n); g = G / 16 and the
integer factors are exact), so |t^_i - t_i| <= gamma_2 |t_i|.  It then adds the N rounded terms and p in some order
(per output channel in registers, per band in LDS, one flush per band, global atomics) -- a binary tree of float32
additions with N + 1 leaves, N additions, and no leaf passes more than N of them.  Each addition rounds once
(relative 2^-24), so

    |result - (p + sum t_i)| <= gamma_{N+2} * (S + |p|),    gamma_n = n u / (1 - n u),  u = 2^-24

(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., lemma 3.1 and section 4.2).  The test allows
gamma_{N + oC + 2}: oC more roundings than the derivation needs.  An entry with N = 0 is never written: it must hold p
exactly.  The bound is per entry, so a dropped halo row or a lost collision share on a small entry is seen."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TS_LOG = 12                                     # interp_bwd_kernel<OC, 12>: 4096 hash slots
PAD = {"s": 1, "d": 2, "y": 2, "c": 3, "t": 3}
LUT_ROWS = 17 ** 4
PATHS = ("one_band", "halo_bands", "gim_lds", "gim_global", "row_bands")


def launch(h, w, bd):
    """the host rule of lerf_swf2lut_interp_bwd_f32 (grad_img non-NULL): (rows_per_band, bands, gim_lds)"""
    rpb = min(max(4096 // w, 1), h)
    bands = -(-h // rpb)
    return rpb, bands, (rpb + bd) * (w + bd) * 4 <= 40 * 1024


def paths(h, w, bd):
    rpb, bands, lds = launch(h, w, bd)
    p = {"one_band" if bands == 1 else "halo_bands", "gim_lds" if lds else "gim_global"}
    if w > 4096:
        p.add("row_bands")
    return p


def hash_slot(row):
    return ((np.asarray(row, np.uint64) * np.uint64(2654435761)) % np.uint64(2 ** 32)) >> np.uint64(32 - TS_LOG)


# 2x2-periodic image (MSBs only) for mode s: its four pixel classes land on LUT rows 36395, 31771, 78155, 78139, and
# 31771 / 78139 share hash slot 2284 -- in every band one of them claims the slot and the other goes to global atomics
COLLIDE_2X2 = np.array([[15, 15], [7, 6]]) * 16
COLLIDE_ROWS = (31771, 78139)

# (mode, oC, (B, C), h, w, bd, image kind)
CASES = []
for _oc in (1, 3):
    CASES += [(m, _oc, (16, 1), 48, 48, PAD[m], "noise") for m in "sdyct"]          # the reference's training crop
    CASES += [
        ("s", _oc, (2, 1), 40, 300, 1, "noise"),            # several bands + halo rows, LDS; 2 planes, forward grid.x = 2
        ("c", _oc, (1, 2), 30, 700, 4, "noise"),            # bd beyond the pattern reach, several bands
        ("t", _oc, (1, 1), 4, 2600, 3, "noise"),            # one-row bands, image gradient in global memory
        ("t", _oc, (1, 1), 1, 2600, 3, "smooth"),           # h = 1: one band, global image gradient
        ("s", _oc, (1, 1), 3, 5200, 1, "noise"),            # w > 4096, global
        ("s", _oc, (2, 1), 2, 4200, 1, "smooth"),           # w > 4096, LDS
        ("d", _oc, (1, 1), 1, 10, 2, "const"),              # h = 1, every pixel on the same corners
        ("y", _oc, (3, 1), 20, 260, 5, "const"),            # several bands, bd > reach, 3 planes
        ("t", _oc, (4, 1), 48, 48, 3, "smooth"),
        ("s", _oc, (1, 1), 64, 64, 1, "collide"),           # hash collision, one band
        ("s", _oc, (2, 1), 130, 96, 1, "collide"),          # hash collision, several bands
        ("s", _oc, (1, 1), 2, 6000, 1, "collide"),          # hash collision, one-row bands, global
    ]
IDS = ["%s%d-%dx%dx%dx%d-bd%d-%s" % (m, oc, B, Cn, h, w, bd, k) for m, oc, (B, Cn), h, w, bd, k in CASES]


def make_inputs(case):
    mode, oC, (B, Cn), h, w, bd, kind = case
    rng = np.random.default_rng(CASES.index(case) + 1)
    hp, wp = h + bd, w + bd
    if kind == "noise":                     # more distinct LUT rows per band than hash slots
        img = rng.integers(0, 256, (B, Cn, hp, wp))
        img[0, 0, :, : min(4, wp)] = 255
    elif kind == "const":                   # one LUT cell for every pixel: the same 2 weighted corners hammered
        img = np.full((B, Cn, hp, wp), 100)
    elif kind == "smooth":
        yy, xx = np.meshgrid(np.arange(hp), np.arange(wp), indexing="ij")
        img = np.broadcast_to(40 + (yy * 3 + xx // 37) % 180, (B, Cn, hp, wp)).copy()
    else:
        img = np.tile(COLLIDE_2X2, (B, Cn, -(-hp // 2), -(-wp // 2)))[:, :, :hp, :wp]
    wt = np.clip(rng.standard_normal((LUT_ROWS, oC)) * 0.7, -1.3, 1.3).astype(np.float32)
    on_gate = rng.random(wt.shape) < 0.02
    wt[on_gate] = np.where(rng.random(int(on_gate.sum())) < 0.5, 1.0, -1.0)          # rint(127 w) = +-127: the gate's edge
    if kind == "collide":
        wt[COLLIDE_ROWS[0]] = 0.3
        wt[COLLIDE_ROWS[1]] = -0.6
        wt[COLLIDE_ROWS[1], 0] = 1.1 if oC > 1 else -0.6                            # one channel behind the gate (oC = 3)
    G = rng.standard_normal((B, Cn * oC, h, w)).astype(np.float32)
    return img.astype(np.float32), wt, G


_ORACLE = {}


def oracle_of(oracle, case):
    if case not in _ORACLE:
        img, wt, G = make_inputs(case)
        mode, oC, _, _, _, bd, _ = case
        _ORACLE[case] = (img, wt, G) + tuple(oracle.swf2lut_interp(wt, oC, mode, img, bd, G, bounds=True))
    return _ORACLE[case]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


@pytest.fixture(scope="module")
def lib(torch):
    from lerf_pytorch_amd import _lib
    return _lib


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else None)


def gpu_forward(torch, lib, case, img, wt):
    mode, oC, (B, Cn), h, w, bd, _ = case
    x, wd = torch.tensor(img, device="cuda"), torch.tensor(wt, device="cuda")
    out = torch.empty((B, Cn * oC, h, w), dtype=torch.float32, device="cuda")
    lib.check(lib.lib().lerf_swf2lut_interp_f32(_p(wd), oC, mode.encode(), _p(x), B * Cn, h, w, bd, _p(out),
                                                lib.current_stream()), "lerf_swf2lut_interp_f32")
    return out.cpu().numpy()


def gpu_backward(torch, lib, case, img, wt, G, gw_prior, gi_prior):
    """the ABI call with caller-owned gradient buffers holding gw_prior / gi_prior (None: pass NULL)"""
    mode, oC, (B, Cn), h, w, bd, _ = case
    x, wd, g = (torch.tensor(a, device="cuda") for a in (img, wt, G))
    gw = torch.tensor(gw_prior, device="cuda") if gw_prior is not None else None
    gi = torch.tensor(gi_prior, device="cuda") if gi_prior is not None else None
    lib.check(lib.lib().lerf_swf2lut_interp_bwd_f32(_p(wd), oC, mode.encode(), _p(x), _p(g), B * Cn, h, w, bd, _p(gw), _p(gi),
                                                    lib.current_stream()), "lerf_swf2lut_interp_bwd_f32")
    torch.cuda.synchronize()
    return (gw.cpu().numpy() if gw is not None else None), (gi.cpu().numpy() if gi is not None else None)


def prefill(shape):
    """a known pattern with no zero: (k - 2.5) * 0.375, k = 0..6 cycling"""
    return ((np.arange(int(np.prod(shape))) % 7 - 2.5) * 0.375).astype(np.float32).reshape(shape)


def assert_within(got, grad, count, absum, oC, prior, what):
    n = count + oC + 2
    bound = n * U / (1 - n * U) * (absum + np.abs(prior.astype(np.float64)))
    err = np.abs(got.astype(np.float64) - (prior.astype(np.float64) + grad))
    bad = err > bound
    if bad.any():
        i = np.argwhere(bad)[:5]
        raise AssertionError("%s: %d of %d entries outside the bound, e.g. %s: got %s want %s (bound %s, count %s)" % (
            what, int(bad.sum()), bad.size, i.tolist(), got[tuple(i.T)], (prior + grad)[tuple(i.T)], bound[tuple(i.T)],
            count[tuple(i.T)]))
    untouched = count == 0
    assert np.array_equal(got[untouched], prior[untouched]), "%s: an entry with no term changed" % what


def test_case_list_reaches_every_path():
    """the coverage table: every (oC, path) cell of the host rule is reached by some case"""
    table = {(oc, p): [] for oc in (1, 3) for p in PATHS}
    for case, cid in zip(CASES, IDS):
        mode, oC, _, h, w, bd, _ = case
        for p in paths(h, w, bd):
            table[(oC, p)].append(cid)
    missing = [k for k, v in table.items() if not v]
    assert not missing, missing
    for (oc, p), v in sorted(table.items()):
        print("oC=%d %-10s %2d cases" % (oc, p, len(v)))
    # the constructed image really collides: two touched rows, one slot
    assert hash_slot(COLLIDE_ROWS[0]) == hash_slot(COLLIDE_ROWS[1])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_and_backward_against_oracle(torch, lib, oracle, case):
    img, wt, G, ro, rgw, rgi, st = oracle_of(oracle, case)
    mode, oC = case[0], case[1]
    assert np.array_equal(gpu_forward(torch, lib, case, img, wt), ro)                 # bit for bit
    # zero-filled buffers (what the autograd wrapper passes)
    gw, gi = gpu_backward(torch, lib, case, img, wt, G, np.zeros_like(wt), np.zeros_like(img))
    assert_within(gw, rgw, st["gw_count"], st["gw_abs"], oC, np.zeros_like(wt), "grad_weight")
    assert_within(gi, rgi, st["gimg_count"], st["gimg_abs"], oC, np.zeros_like(img), "grad_img")
    rows = np.nonzero(np.any(gw != 0, axis=1))[0]
    want_rows = np.nonzero(np.any(st["gw_abs"] > 0, axis=1))[0]
    assert np.array_equal(rows, want_rows), "touched LUT rows differ"
    if case[-1] == "collide":
        # both colliding rows carry a real share of the gradient: one of them went through the global fallback
        share = st["gw_abs"][list(COLLIDE_ROWS)].sum(1) / st["gw_abs"].sum()
        assert np.all(share > 0.1), share
    # the ABI accumulates into the caller's buffers, on every path (the one-band image gradient with a plain +=)
    pw, pi = prefill(wt.shape), prefill(img.shape)
    gw, gi = gpu_backward(torch, lib, case, img, wt, G, pw, pi)
    assert_within(gw, rgw, st["gw_count"], st["gw_abs"], oC, pw, "grad_weight accumulated")
    assert_within(gi, rgi, st["gimg_count"], st["gimg_abs"], oC, pi, "grad_img accumulated")
    # either gradient pointer may be NULL; the other gradient is unchanged (grad_img NULL also moves the LUT-row pass off
    # the LDS image-gradient path, so it is a different launch)
    gw, none = gpu_backward(torch, lib, case, img, wt, G, pw, None)
    assert none is None
    assert_within(gw, rgw, st["gw_count"], st["gw_abs"], oC, pw, "grad_weight with grad_img = NULL")
    none, gi = gpu_backward(torch, lib, case, img, wt, G, None, pi)
    assert_within(gi, rgi, st["gimg_count"], st["gimg_abs"], oC, pi, "grad_img with grad_weight = NULL")


@pytest.mark.parametrize("case", [c for c in CASES if c[2:] == ((2, 1), 130, 96, 1, "collide")] +
                         [c for c in CASES if c[2:] == ((2, 1), 40, 300, 1, "noise")], ids=lambda c: "%s%d-%s" % (c[0], c[1], c[-1]))
def test_repeated_collision_heavy_runs_agree(torch, lib, oracle, case):
    """atomics are unordered, so repeated runs need not be bitwise equal -- but every run is within the bound"""
    img, wt, G, ro, rgw, rgi, st = oracle_of(oracle, case)
    oC = case[1]
    runs = [gpu_backward(torch, lib, case, img, wt, G, np.zeros_like(wt), np.zeros_like(img)) for _ in range(4)]
    for gw, gi in runs:
        assert_within(gw, rgw, st["gw_count"], st["gw_abs"], oC, np.zeros_like(wt), "grad_weight")
        assert_within(gi, rgi, st["gimg_count"], st["gimg_abs"], oC, np.zeros_like(img), "grad_img")
    for gw, gi in runs[1:]:
        assert_within(gw, runs[0][0].astype(np.float64), st["gw_count"], st["gw_abs"], oC, np.zeros_like(wt), "run to run")
