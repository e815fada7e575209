"""The SRNet forward and backward (lerf_srnet.hip: lerf_srnet_fwd_f32 / lerf_srnet_bwd_f32) on every class of the
backward's host rule -- one partial tile, whole tiles, a tile across two planes, 512 tiles, the first walk at 513..516 and
walks of three tiles at 1030 -- with srnet_cases.py's batches, and the autograd wrapper on top of it.

Tolerances.
  integer net: none.  Every term is an integer and every sum of absolute terms is below 2^24 (test_srnet_cases_cpu.py), so
    the 12 weight gradients, grad_img and the all-zero forward output equal the float32 cast of float64 autograd bit for
    bit, in any tile, slab or MFMA order; so do prior + gradient in a pre-filled accumulator (integers in +-1..8) and
    the sum of the per-plane runs.  The cases tie in every layer (>= 1 % of all pre-activations are exactly 0 with a
    non-zero incoming gradient), so relu'(0) = 0 is part of what is compared.
  random weights: test_gpu_imdn_train_tiles.py's rule, per parameter tensor and for grad_img: e = max |t - t64| / max |t64|
    against float64 CPU autograd, e_stock the same figure for stock float32 autograd of the restatement on the GPU,
    e_stock <= 1e-3 and e_hip <= 4 e_stock + 1e-6.  A lost or doubled tile among 1030 moves a weight gradient by about
    1 / sqrt(1030), 3 %.  The forward keeps test_gpu_srnet.py's first-order bound.  The batches are many small planes
    screened in float64 (srnet_cases.screened_planes): on one unscreened 181 x 182 image about ten of the 10 million
    pre-activations lie within 1e-6 of 0, float32 flips the gate of one or two of them (CPU autograd does too), and a
    single flip moved grad_img by 2e-2 and a weight gradient by 1e-3 of its largest entry, for the kernel and the
    restatement alike: such a batch measures the draw, not the kernel.
  split runs, repeats, accumulation: bitwise (grad_img has no slabs, each tile row is independent; the slab order is
    fixed; the accumulators take one float32 addition per entry).
  the wrapper: test_gpu_srnet.py's test_backward_against_float64, 1e-4 of the tensor's largest entry."""
import numpy as np
import pytest

import srnet_cases as S
from test_gpu_srnet import _bwd, _fwd, torch  # noqa: F401 (torch is the module fixture)

pytestmark = pytest.mark.gpu


def _dev(torch, a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda")


def _run_bwd(torch, flat, geo, img, G, gw0=None, gx0=None, want_gx=True, poison=False):
    """one lerf_srnet_bwd_f32 -> (grad_weights, grad_img or None) as numpy; gw0 / gx0 are the accumulators' prior content
    (zeros if None); poison fills the workspace with NaN bit patterns first"""
    mode, outC, P, h, w, bd = geo
    gw = torch.zeros_like(flat) if gw0 is None else _dev(torch, gw0)
    gx = None
    if want_gx:
        gx = torch.zeros_like(img) if gx0 is None else _dev(torch, gx0)
    if poison:
        L = __import__("lerf_pytorch_amd")._lib
        nbytes = L.lib().lerf_srnet_bwd_workspace_bytes(outC, P, h, w)
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
        assert _bwd(torch, flat, outC, mode, img, G, h, w, bd, gw, gx, ws, nbytes) == 0
    else:
        assert _bwd(torch, flat, outC, mode, img, G, h, w, bd, gw, gx) == 0
    return gw.cpu().numpy(), (gx.cpu().numpy() if want_gx else None)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _first_diff(got, ref, outC):
    """where a packed gradient differs from the 12 reference tensors, for the assertion message"""
    out = []
    for name, g, r in zip(S.TENSORS, S.unpack(got, outC), ref):
        bad = np.argwhere(g != r.astype(np.float32).reshape(g.shape))
        if len(bad):
            i = tuple(bad[0])
            out.append("%s: %d entries, first %s got %r want %r" % (name, len(bad), i, float(g[i]), float(r.reshape(g.shape)[i])))
    return out


# ---------------------------------------------------------------------------------- 1, 2: the integer net on every class
@pytest.mark.parametrize("name", list(S.INT_CASES))
def test_integer_net_bit_for_bit(torch, name):
    d, img_n, G_n, geo = S.int_case(name)
    mode, outC, P, h, w, bd = geo
    y64, gs64, gx64 = S.int_reference(name)
    want_w = np.concatenate([g.reshape(-1) for g in gs64]).astype(np.float32)
    want_x = gx64.astype(np.float32)
    assert np.array_equal(want_w, np.concatenate([g.reshape(-1) for g in gs64])) and not np.any(y64)     # the cast loses nothing
    flat, img, G = _dev(torch, S.pack(d)), _dev(torch, img_n), _dev(torch, G_n)
    rc, out = _fwd(torch, flat, outC, mode, img, h, w, bd)
    assert rc == 0 and not np.any(out.cpu().numpy()), "the forward output of the integer net is 0 everywhere"
    print("%s %s: %d tiles, %d slabs, walks %s, %d rows in the last tile" % (
        name, geo, S.n_tiles(P, h, w), S.n_slabs(P, h, w), sorted({S.walk(g, P, h, w) for g in range(S.n_slabs(P, h, w))}),
        S.last_rows(P, h, w)))
    # zero-filled accumulators, grad_img non-NULL and NULL
    gw, gx = _run_bwd(torch, flat, geo, img, G)
    assert np.array_equal(gw, want_w), _first_diff(gw, gs64, outC)
    assert np.array_equal(gx, want_x), (int((gx != want_x).sum()), np.argwhere(gx != want_x)[:3].tolist())
    gw, _ = _run_bwd(torch, flat, geo, img, G, want_gx=False)
    assert np.array_equal(gw, want_w), _first_diff(gw, gs64, outC)
    # pre-filled accumulators (integers without zeros): prior + gradient, and prior bytes where no tap reaches
    gw0, gx0 = S.prefill(want_w.shape, 7, True), S.prefill(want_x.shape, 8, True)
    gw, gx = _run_bwd(torch, flat, geo, img, G, gw0, gx0)
    assert np.array_equal(gw, gw0 + want_w)
    r = S.reached(mode, P, h, w, bd)
    assert np.array_equal(gx[r], (gx0 + want_x)[r]) and _same_bits(gx[~r], gx0[~r])
    gw, _ = _run_bwd(torch, flat, geo, img, G, gw0, want_gx=False)
    assert np.array_equal(gw, gw0 + want_w)


def test_workspace_follows_the_host_rule():
    """min(tiles, 512) slabs of the packed size rounded up to 64 floats, then 4 floats per position: the slab count the
    case classes are derived from is the library's"""
    lib = __import__("lerf_pytorch_amd")._lib.lib()
    shapes = [c[1:5] for c in S.INT_CASES.values()] + [(2, 1, 1, 32 * 511), (2, 1, 1, 32 * 511 + 1), (2, 7, 1, 32 * 512 + 1)]
    for outC, P, h, w in shapes:
        stride = (S.pack(S.integer_weights(outC, 3)).size + 63) // 64 * 64
        assert stride == (lib.lerf_srnet_weight_floats(outC) + 63) // 64 * 64
        want = 4 * (S.n_slabs(P, h, w) * stride + 4 * P * h * w)
        assert lib.lerf_srnet_bwd_workspace_bytes(outC, P, h, w) == want, (outC, P, h, w, S.n_slabs(P, h, w))


# ---------------------------------------------------------------------------------- 3: random weights, nothing exact
_stock = {}


def _stock_grads(torch, key, d, geo, img, G):
    """stock float32 autograd of the restatement on the GPU, once per batch"""
    if key not in _stock:
        _stock[key] = S.autograd(d, geo[0], img, G, geo[3], geo[4], dtype=torch.float32, device="cuda")[1:]
    return _stock[key]


def _check_rule(label, outC, gw, gx, stock, ref):
    """the float64 rule on the 12 tensors and grad_img; prints the worst pair"""
    (gs, gxs), (g64, gx64) = stock, ref
    worst, fails = (-1.0, 0.0, ""), []
    rows = list(zip(S.TENSORS, S.unpack(gw, outC), gs, g64)) + [("grad_img", gx, gxs, gx64)]
    for k, t, ts, t64 in rows:
        e_hip, e_stock = S.rel_err(np.asarray(t).reshape(t64.shape), t64), S.rel_err(ts, t64)
        assert e_stock <= 1e-3, (k, e_stock)
        if e_hip > worst[0]:
            worst = (e_hip, e_stock, k)
        if not e_hip <= 4 * e_stock + 1e-6:
            fails.append((k, e_hip, e_stock))
    print("%s: worst e_hip %.3g (e_stock %.3g) at %s" % (label, worst[0], worst[1], worst[2]))
    assert not fails, fails


@pytest.mark.parametrize("name", list(S.RAND_CASES))
def test_random_walk_matches_float64(torch, oracle, name):
    d, img_n, G_n, geo, kept = S.rand_case(name)
    mode, outC, P, h, w, bd = geo
    y64, g64, gx64 = S.rand_reference(name)
    flat, img, G = _dev(torch, S.pack(d)), _dev(torch, img_n), _dev(torch, G_n)
    rc, out = _fwd(torch, flat, outC, mode, img, h, w, bd)
    assert rc == 0
    yo, M6 = oracle.srnet_forward(d, S.KEY, S.tuples(img_n, mode, h, w), absolute=True)
    u = 2.0 ** -24
    got = out.cpu().numpy().transpose(0, 2, 3, 1).reshape(-1, outC)
    assert np.all(np.abs(got - yo) <= 969 * u / (1 - 969 * u) * M6 + 2.0 ** -22), float(np.max(np.abs(got - yo)))
    gw, gx = _run_bwd(torch, flat, geo, img, G)
    _check_rule("%s %s, %d tiles, kept %.3f" % (name, geo, S.n_tiles(P, h, w), kept), outC, gw, gx, _stock_grads(torch, name, d, geo, img_n, G_n),
                (g64, gx64))


def test_real_ties_zero_bias_black_band(torch):
    """_Conv's zero biases on planes with a black band: every pre-activation of the black positions is exactly 0, and
    relu'(0) = 0 keeps their cotangents out of every bias gradient (relu'(0) = 1 moves each of them by more than 5 %,
    test_srnet_cases_cpu.py) and out of the image: pixel row 3 is read by the black positions alone"""
    d, img_n, G_n, geo, tied, kept = S.tied_batch()
    mode, outC, P, h, w, bd = geo
    _, g64, gx64 = S.tied_reference()
    flat, img, G = _dev(torch, S.pack(d)), _dev(torch, img_n), _dev(torch, G_n)
    rc, out = _fwd(torch, flat, outC, mode, img, h, w, bd)
    assert rc == 0
    got = out.cpu().numpy().transpose(0, 2, 3, 1).reshape(-1, outC)
    assert not np.any(got[tied])
    gw, gx = _run_bwd(torch, flat, geo, img, G)
    _check_rule("ties %s, %d tiles, %.3f of the positions tied, kept %.3f" % (geo, S.n_tiles(P, h, w), tied.mean(), kept), outC,
                gw, gx, _stock_grads(torch, "tied", d, geo, img_n, G_n), (g64, gx64))
    assert not np.any(gx64[:, 3]) and np.any(gx64[:, 2]) and not np.any(gx[:, 3])


# ---------------------------------------------------------------------------------- 4: localisation and independence
@pytest.mark.parametrize("kind", ["integer", "random"])
def test_split_runs_localise_the_walk(torch, kind):
    """walk3-t whole (1030 tiles and more, every slab walks) against its parts alone (344 tiles, none walks; the planes
    of the integer case, the thirds of the random one, whose tiles are cut elsewhere than the whole's): the output and
    grad_img bitwise, the integer weight gradient bitwise the sum of the parts.  If the whole fails its float64
    comparison while this shows sound parts, the fault lies in the walk."""
    d, img_n, G_n, geo = S.int_case("walk3-t") if kind == "integer" else S.rand_case("walk3-t")[:4]
    mode, outC, P, h, w, bd = geo
    n = 1 if kind == "integer" else P // 3
    assert S.n_tiles(P, h, w) > 2 * S.MAX_SLABS and S.n_tiles(n, h, w) < S.MAX_SLABS and P % n == 0
    flat, img, G = _dev(torch, S.pack(d)), _dev(torch, img_n), _dev(torch, G_n)
    rc, out = _fwd(torch, flat, outC, mode, img, h, w, bd)
    gw, gx = _run_bwd(torch, flat, geo, img, G)
    parts = []
    for p in range(0, P, n):
        rc_p, out_p = _fwd(torch, flat, outC, mode, img[p:p + n].contiguous(), h, w, bd)
        assert rc == 0 and rc_p == 0
        gw_p, gx_p = _run_bwd(torch, flat, (mode, outC, n, h, w, bd), img[p:p + n].contiguous(), G[p:p + n].contiguous())
        parts.append((out_p.cpu().numpy(), gw_p, gx_p))
    assert _same_bits(out.cpu().numpy(), np.concatenate([p[0] for p in parts])), "the output of the batch differs from its planes"
    assert _same_bits(gx, np.concatenate([p[2] for p in parts])), "grad_img of the batch differs from its planes"
    split = sum(p[1].astype(np.float64) for p in parts)
    if kind == "integer":
        assert np.array_equal(gw, split.astype(np.float32)) and np.array_equal(split, split.astype(np.float32))
    else:
        _, g64, _ = S.rand_reference("walk3-t")
        e = [(S.rel_err(a.reshape(r.shape), r), S.rel_err(b.reshape(r.shape), r), k)
             for k, a, b, r in zip(S.TENSORS, S.unpack(gw, outC), S.unpack(split, outC), g64)]
        k = max(e)
        print("walk3-t whole against thirds: worst e_whole %.3g, e_split %.3g there (%s), worst e_split %.3g"
              % (k[0], k[1], k[2], max(x[1] for x in e)))
        assert all(x[0] <= 1e-4 and x[1] <= 1e-4 for x in e), e      # test_gpu_srnet.py's per-tensor bound, both ways


def test_walk_is_bitwise_repeatable(torch):
    """1030 tiles with random weights, four times: a workspace of its own, again, and one full of NaN bit patterns
    (a slab entry read before its first tile wrote it would show)"""
    d, img_n, G_n, geo, _ = S.rand_case("walk3-s")
    flat, img, G = _dev(torch, S.pack(d)), _dev(torch, img_n), _dev(torch, G_n)
    a = _run_bwd(torch, flat, geo, img, G)
    b = _run_bwd(torch, flat, geo, img, G)
    c = _run_bwd(torch, flat, geo, img, G, poison=True)
    assert np.all(np.isfinite(a[0])) and np.all(np.isfinite(a[1]))
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
    assert _same_bits(a[0], c[0]) and _same_bits(a[1], c[1])
    # and without grad_img the weight gradient is the same
    assert _same_bits(a[0], _run_bwd(torch, flat, geo, img, G, want_gx=False, poison=True)[0])


def test_accumulation_above_the_reach(torch):
    """bd = reach + 1 with random weights: pixels no tap reaches keep their prior bytes, the others and every weight take
    exactly one float32 addition of what a zero-filled run returns"""
    d, img_n, G_n, geo, _ = S.rand_case("walk3-t")
    mode, outC, P, h, w, bd = geo
    assert bd > S.REACH[mode]
    flat, img, G = _dev(torch, S.pack(d)), _dev(torch, img_n), _dev(torch, G_n)
    gw, gx = _run_bwd(torch, flat, geo, img, G)
    gw0, gx0 = S.prefill(gw.shape, 9, False), S.prefill(gx.shape, 10, False)
    assert np.all(gw0 != 0) and np.all(gx0 != 0)
    gw1, gx1 = _run_bwd(torch, flat, geo, img, G, gw0, gx0)
    r = S.reached(mode, P, h, w, bd)
    assert 0 < (~r).sum() and not np.any(gx[~r])
    assert _same_bits(gx1[~r], gx0[~r]) and _same_bits(gx1[r], (gx0 + gx)[r])
    assert _same_bits(gw1, gw0 + gw)


# ---------------------------------------------------------------------------------- 5: the autograd wrapper
def _net(torch, mode, outC, seed, bias=True):
    from lerf_pytorch_amd.resample.model import _SRNet
    torch.manual_seed(seed)
    net = _SRNet(mode, 64, outC)
    if bias:                                                      # _Conv's zeros would tie nothing here but hide a bias mix-up
        with torch.no_grad():
            for n, p in net.named_parameters():
                if n.endswith("bias"):
                    p.copy_(0.05 * torch.randn(p.shape))
    return net.cuda()


def _d_of(net):
    ps = [p.detach().float().cpu().numpy() for p in net.parameters()]
    return S.as_dict([p.reshape(p.shape[0], -1) if i % 2 == 0 else p for i, p in enumerate(ps)])


def _wrapper_case(torch, mode, outC, B, Cn, h, w, seed):
    bd = S.REACH[mode]
    rng = np.random.default_rng(seed)
    img = rng.random((B, Cn, h + bd, w + bd)).astype(np.float32)
    G = rng.standard_normal((B, Cn * outC, h, w)).astype(np.float32)
    return img, G


def _ref(net, mode, img, G, h, w):
    B, Cn = img.shape[:2]
    _, gs, gx = S.autograd(_d_of(net), mode, img.reshape((B * Cn,) + img.shape[2:]), G.reshape((B * Cn, -1, h, w)), h, w)
    return gs, gx.reshape(img.shape)


def _close(got, ref, what):
    got = got.detach().double().cpu().numpy().reshape(ref.shape)
    assert np.max(np.abs(got - ref)) <= 1e-4 * np.abs(ref).max(), (what, float(np.max(np.abs(got - ref)) / np.abs(ref).max()))


def test_wrapper_frozen_weights_and_image_without_grad(torch):
    mode, outC, B, Cn, h, w = "c", 3, 2, 2, 9, 11
    net = _net(torch, mode, outC, 11)
    img, G = _wrapper_case(torch, mode, outC, B, Cn, h, w, 12)
    gs, gx = _ref(net, mode, img, G, h, w)
    # the image without grad: the NULL grad_img path
    x = _dev(torch, img)
    (net(x) * _dev(torch, G)).sum().backward()
    assert x.grad is None
    for (n, p), g in zip(net.named_parameters(), gs):
        _close(p.grad, g, n)
    # the weights frozen, the image a leaf: the image gradient alone
    net.zero_grad(set_to_none=True)
    net.requires_grad_(False)
    x = _dev(torch, img).requires_grad_()
    (net(x) * _dev(torch, G)).sum().backward()
    assert all(p.grad is None for p in net.parameters())
    _close(x.grad, gx, "grad_img")


def test_wrapper_non_contiguous_grad_out(torch):
    mode, outC, B, Cn, h, w = "s", 3, 2, 1, 10, 7
    net = _net(torch, mode, outC, 21)
    img, G = _wrapper_case(torch, mode, outC, B, Cn, h, w, 22)
    gs, gx = _ref(net, mode, img, G, h, w)
    x = _dev(torch, img).requires_grad_()
    g = _dev(torch, np.ascontiguousarray(G.transpose(0, 2, 3, 1))).permute(0, 3, 1, 2)
    assert not g.is_contiguous() and tuple(g.shape) == G.shape
    net(x).backward(g)
    for (n, p), r in zip(net.named_parameters(), gs):
        _close(p.grad, r, n)
    _close(x.grad, gx, "grad_img")
    # and through a permuted loss
    net.zero_grad(set_to_none=True)
    x.grad = None
    (net(x).permute(0, 2, 3, 1) * g.permute(0, 2, 3, 1)).sum().backward()
    for (n, p), r in zip(net.named_parameters(), gs):
        _close(p.grad, r, n)
    _close(x.grad, gx, "grad_img")


def test_wrapper_one_net_twice_in_a_graph(torch):
    """as stage 2 uses net r0 for rotations 0 and 2: the parameter gradients of the two applications add"""
    mode, outC, B, Cn, h, w = "t", 3, 1, 2, 8, 8
    net = _net(torch, mode, outC, 31)
    img_a, G_a = _wrapper_case(torch, mode, outC, B, Cn, h, w, 32)
    img_b, G_b = _wrapper_case(torch, mode, outC, B, Cn, h, w, 33)
    gs_a, gx_a = _ref(net, mode, img_a, G_a, h, w)
    gs_b, gx_b = _ref(net, mode, img_b, G_b, h, w)
    xa, xb = _dev(torch, img_a).requires_grad_(), _dev(torch, img_b).requires_grad_()
    ((net(xa) * _dev(torch, G_a)).sum() + (net(xb) * _dev(torch, G_b)).sum()).backward()
    for (n, p), a, b in zip(net.named_parameters(), gs_a, gs_b):
        _close(p.grad, a + b, n)
    _close(xa.grad, gx_a, "grad_img a")
    _close(xb.grad, gx_b, "grad_img b")


def test_wrapper_double_model_gets_float64_gradients(torch):
    """SRNetsSWF2 after .double(): the nets still run in float32, the gradients arrive in the parameters' float64"""
    from lerf_pytorch_amd.resample.model import SRNetsSWF2
    from test_gpu_srnet import _opt
    torch.manual_seed(41)
    m = SRNetsSWF2(_opt(), inC=1, outC=3).cuda().double()
    mode, outC, B, Cn, h, w = "c", 3, 2, 1, 7, 12
    net = m.s2_cr1
    assert all(p.dtype == torch.float64 for p in m.parameters())
    img, G = _wrapper_case(torch, mode, outC, B, Cn, h, w, 42)
    gs, gx = _ref(net, mode, img, G, h, w)
    x = torch.tensor(img, dtype=torch.float64, device="cuda", requires_grad=True)
    y = m(x, 2, mode, 1)
    assert y.dtype == torch.float32
    (y * _dev(torch, G)).sum().backward()
    for (n, p), r in zip(net.named_parameters(), gs):
        assert p.grad.dtype == torch.float64, n
        _close(p.grad, r, n)
    assert x.grad.dtype == torch.float64
    _close(x.grad, gx, "grad_img")
    assert all(p.grad is None for n, p in m.named_parameters() if not n.startswith("s2_cr1."))
