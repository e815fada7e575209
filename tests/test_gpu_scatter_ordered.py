"""The ORDERED scatter on the device (entry_kernel<CountPass / FillPass>, scan_block_kernel / scan_add_kernel,
ordered_sum_kernel of csrc/lerf_coords.hip behind ops.splat / ops.coords_compose_bwd / ops.coords_invert_bwd with deterministic=True and
the torch twins of coords) against the PLAIN HOST twins -- lerf_splat_host, lerf_coords_compose_bwd_host, lerf_coords_invert_bwd_host.
The device adds in the host's order, so every comparison is made on the raw bits, and every case runs twice:

  1. the cases of tests/test_scatter_ordered_cpu.py: the splat forward (a pre-filled accumulator too), both adjoints, each half alone;
  2. the scan at its block seams;
  3. strided operands: a padded map and a padded accumulator set stride, the padding untouched, the operands unmodified;
  4. one workspace reused by two different calls without clearing it;
  5. the smallest shapes that can still go wrong: a target frame one element beyond one scan block, beyond three, beyond B * B (a third
     level); a 65 x 5 source (a ragged last block on both axes); segments of exactly max_adders and of max_adders + 1;
  6. the torch twins: deterministic=True, None under torch.use_deterministic_algorithms(True), False still the atomic kernel.
"""
import numpy as np
import pytest

from test_scatter_ordered_cpu import (ADJ_CASES, ADJ_IDS, CAP, POWER_CASE, SPLAT_CASES, SPLAT_IDS, adjoint_case, cap_case, prefilled, scan_input,
                                      scan_lengths, scan_ref)
from test_splat_cpu import f32, f64, make_case, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def _dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------- 1. the CPU file's cases
@pytest.mark.parametrize("case", SPLAT_CASES, ids=SPLAT_IDS)
def test_splat_ordered_is_the_host_twin_by_bit_pattern_twice(torch, case):
    from lerf_pytorch_amd import _lib, ops
    X, F, M = make_case(case)
    ohw, norm = case[1], case[7]
    ref = _lib.splat_host(X, F, ohw, M, norm)
    dX, dF, dM = (_dev(torch, a) for a in (X, F, M))
    keep = [t.clone() for t in (dX, dF)]
    for _ in range(2):
        got = ops.splat(dX, dF, ohw, dM, norm, deterministic=True, max_adders=CAP)
        assert same_bits(_np(got), ref)
    base = prefilled(ref.shape, ref.dtype)
    ref2 = _lib.splat_host(X, F, ohw, M, norm, acc=base.copy())
    for _ in range(2):
        got2 = ops.splat(dX, dF, ohw, dM, norm, acc=_dev(torch, base), deterministic=True, max_adders=CAP)
        assert same_bits(_np(got2), ref2)
    assert torch.equal(dX, keep[0]) and same_bits(_np(dF), _np(keep[1]))


@pytest.mark.parametrize("case", ADJ_CASES, ids=ADJ_IDS)
def test_compose_bwd_ordered_is_the_host_twin_by_bit_pattern_twice(torch, case):
    from lerf_pytorch_amd import _lib, ops
    outer, inner, g = adjoint_case(*case)
    base_a, base_b = prefilled(outer.shape, f64, 11), prefilled(inner.shape, f64, 12)
    dA, dB, dG = (_dev(torch, a) for a in (outer, inner, g))
    for need in ((True, True), (True, False), (False, True)):
        ra, rb = _lib.coords_compose_bwd_host(outer, inner, g, base_a.copy() if need[0] else None, base_b.copy() if need[1] else None, need)
        for _ in range(2):
            ga, gb = ops.coords_compose_bwd(dA, dB, dG, _dev(torch, base_a) if need[0] else None, _dev(torch, base_b) if need[1] else None, need,
                                            deterministic=True, max_adders=CAP)
            for got, ref in ((ga, ra), (gb, rb)):
                assert (got is None) == (ref is None) and (ref is None or same_bits(_np(got), ref))


@pytest.mark.parametrize("case", ADJ_CASES, ids=ADJ_IDS)
def test_invert_bwd_ordered_is_the_host_twin_by_bit_pattern_twice(torch, case):
    from lerf_pytorch_amd import _lib, ops
    fmap, inverse, g = adjoint_case(*case)
    base = prefilled(fmap.shape, f64, 13)
    ref = _lib.coords_invert_bwd_host(fmap, inverse, g, base.copy())
    dF, dI, dG = (_dev(torch, a) for a in (fmap, inverse, g))
    for _ in range(2):
        assert same_bits(_np(ops.coords_invert_bwd(dF, dI, dG, _dev(torch, base), deterministic=True, max_adders=CAP)), ref)


def test_a_shared_outer_map_in_a_batch_sums_its_sets_in_order(torch):
    from lerf_pytorch_amd import _lib, ops
    outer, inner, g = adjoint_case(3, f64, f64)
    shared = np.ascontiguousarray(outer[1])
    base = prefilled(shared.shape, f64, 14)
    want, _ = _lib.coords_compose_bwd_ordered_host(shared, inner, g, base.copy(), None, (True, False), max_adders=CAP)
    for _ in range(2):
        ga, _ = ops.coords_compose_bwd(_dev(torch, shared), _dev(torch, inner), _dev(torch, g), _dev(torch, base), None, (True, False),
                                       deterministic=True, max_adders=CAP)
        assert same_bits(_np(ga), want)


# ---------------------------------------------------------------------------------------------- 2. the scan
@pytest.mark.parametrize("k", range(5))
def test_scan_on_the_device(torch, k):
    from lerf_pytorch_amd import ops
    n = scan_lengths()[k]
    v = scan_input(n)
    want = scan_ref(v)
    for _ in range(2):
        t = torch.from_numpy(v.view(np.int32).copy()).cuda()
        got = _np(ops.scan_exclusive_u32(t)).view(np.uint32).astype(np.uint64)
        assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------- 3, 4. raw calls: strides, one workspace
def raw_splat_ordered(torch, x, f, f_row, f_set, acc, acc_set, norm, ohw, ws, cap, n_sets):
    """lerf_splat_ordered itself on the current stream: x [n_sets, C, H, W] dense, f and acc with the given strides (in elements)"""
    from lerf_pytorch_amd import _lib
    n_sets_, Cn, H, W = x.shape
    assert n_sets_ == n_sets
    with _lib.on_device(x):
        return _lib.lib().lerf_splat_ordered(x.data_ptr(), _lib.LERF_F32 if x.dtype == torch.float32 else _lib.LERF_F64, Cn, H, W, Cn * H * W,
                                             f.data_ptr(), _lib.LERF_F32 if f.dtype == torch.float32 else _lib.LERF_F64, f_row, f_set, None, 0,
                                             acc.data_ptr(), int(norm), ohw[0], ohw[1], acc_set, n_sets, ws.data_ptr(), ws.numel(), cap,
                                             _lib.current_stream(x.device))


def test_strided_map_and_accumulator_set_stride(torch):
    from lerf_pytorch_amd import _lib
    case = ((23, 31), (29, 37), 3, 3, True, f32, f64, True, False)
    X, F, _ = make_case(case)
    (H, W), ohw, B, P = case[0], case[1], 3, 4
    ref = _lib.splat_host(X, F, ohw, None, True)
    row, fset = 2 * (W + 3), (H * 2 * (W + 3)) + 10                       # padded rows, padded sets (both even)
    fbuf = torch.full((B * fset,), -7.0, dtype=torch.float64, device="cuda")
    fview = fbuf.as_strided((B, H, W, 2), (fset, row, 2, 1))
    fview.copy_(_dev(torch, F))
    aset = P * ohw[0] * ohw[1] + 13
    abuf = torch.full((B * aset,), -7.0, dtype=torch.float32, device="cuda")
    aview = abuf.as_strided((B, P) + ohw, (aset, ohw[0] * ohw[1], ohw[1], 1))
    dX = _dev(torch, X)
    ws = torch.empty(_lib.ordered_workspace_bytes(H * W, ohw[0] * ohw[1], B), dtype=torch.uint8, device="cuda")
    fkeep, xkeep = fbuf.clone(), dX.clone()
    for _ in range(2):
        aview.zero_()
        assert raw_splat_ordered(torch, dX, fbuf, row, fset, abuf, aset, True, ohw, ws, CAP, B) == 0
        torch.cuda.synchronize()
        assert same_bits(_np(aview.contiguous()), ref)
        pad = abuf.as_strided((B, 13), (aset, 1), P * ohw[0] * ohw[1])
        assert bool((pad == -7.0).all())
        assert same_bits(_np(fbuf), _np(fkeep)) and torch.equal(dX, xkeep)


def test_one_workspace_serves_two_different_calls_uncleared(torch):
    from lerf_pytorch_amd import _lib
    L = _lib.lib()
    X, F, _ = make_case(POWER_CASE)
    ref = _lib.splat_host(X, F, (8, 8), None, True)
    outer, inner, g = adjoint_case(0, f64, f64)
    rf = _lib.coords_invert_bwd_host(outer, inner, g)
    need = max(_lib.ordered_workspace_bytes(70 * 130, 64, 1), _lib.ordered_workspace_bytes(11 * 13, 63, 1))
    ws = torch.full((need,), 0xa5, dtype=torch.uint8, device="cuda")
    dX, dF, dA, dB, dG = (_dev(torch, a) for a in (X[None], F, outer, inner, g))
    for _ in range(2):
        acc = torch.zeros((1, 4, 8, 8), dtype=torch.float32, device="cuda")
        gf = torch.zeros((7, 9, 2), dtype=torch.float64, device="cuda")
        assert raw_splat_ordered(torch, dX, dF, 2 * 130, 0, acc, 0, True, (8, 8), ws, CAP, 1) == 0
        with _lib.on_device(dA):
            assert L.lerf_coords_invert_bwd_ordered(dA.data_ptr(), _lib.LERF_F64, 18, 7, 9, dB.data_ptr(), _lib.LERF_F64, 26, dG.data_ptr(), 11, 13,
                                                    gf.data_ptr(), ws.data_ptr(), ws.numel(), CAP, _lib.current_stream(dA.device)) == 0
        torch.cuda.synchronize()
        assert same_bits(_np(acc[0]), ref) and same_bits(_np(gf), rf)
        assert 0 < int(ws[4:8].view(torch.int32).item()) <= 4 * 143


# ---------------------------------------------------------------------------------------------- 5. the smallest shapes that can go wrong
def seam_frames():
    from lerf_pytorch_amd import _lib
    B = _lib.scan_block()
    frames = {B + 1: None, 3 * B + 1: None, B * B + 1: None}
    for n in frames:
        h = next(d for d in range(int(n ** 0.5), 0, -1) if n % d == 0)       # the squarest factorisation (a prime: one row)
        frames[n] = (h, n // h)
    return list(frames.values())


@pytest.mark.parametrize("k", range(3))
def test_target_frames_at_the_scan_seams_with_a_ragged_source(torch, k):
    """a 65 x 5 source (a ragged last block of the 64 x 4 entry grid on both axes) spread over a frame of B + 1, 3 B + 1 and B * B + 1
    elements -- one scan block and one element, several blocks, a third scan level -- with clusters on the first and last elements"""
    from lerf_pytorch_amd import _lib, ops
    oH, oW = seam_frames()[k]
    rng = np.random.default_rng(k)
    X = rng.standard_normal((2, 65, 5)).astype(f32)
    F = np.stack([rng.uniform(-1.0, oH, (65, 5)), rng.uniform(-1.0, oW, (65, 5))], -1)
    F[:20, 0] = (0.0, 0.0)
    F[20:40, 0] = (oH - 1.0, oW - 1.0)
    F[40:60, 0] = (oH - 1.0, oW - 1.5) if oW > 1 else (oH - 1.5, 0.0)
    ref = _lib.splat_host(X, F, (oH, oW), None, True)
    assert np.count_nonzero(ref) > 300 and ref[0, 0, 0] != 0 and ref[0, -1, -1] != 0
    dX, dF = _dev(torch, X), _dev(torch, F)
    for _ in range(2):
        assert same_bits(_np(ops.splat(dX, dF, (oH, oW), None, True, deterministic=True, max_adders=64)), ref)


def test_a_segment_of_exactly_the_cap_and_one_beyond(torch):
    from lerf_pytorch_amd import _lib, ops
    X, F = cap_case(f32)
    ohw = (5, 6)
    ref = _lib.splat_host(X, F, ohw, None, True)
    dX, dF = _dev(torch, X), _dev(torch, F)
    for _ in range(2):
        assert same_bits(_np(ops.splat(dX, dF, ohw, None, True, deterministic=True, max_adders=9)), ref)
    with pytest.raises(_lib.LerfError, match=r"9 .*max_adders = 8"):
        ops.splat(dX, dF, ohw, None, True, deterministic=True, max_adders=8)
    ws = torch.empty(_lib.ordered_workspace_bytes(12, 30, 1), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((1, 3) + ohw, dtype=torch.float32, device="cuda")
    assert raw_splat_ordered(torch, dX[None], dF, 8, 0, acc, 0, True, ohw, ws, 8, 1) == 0
    got = _np(acc[0])
    mask = np.zeros(got.shape, bool)
    mask[:, 2, 3] = True
    assert np.isnan(got[mask]).all() and np.array_equal(got[~mask].view(np.uint32), ref[~mask].view(np.uint32))
    assert int(ws[4:8].view(torch.int32).item()) == 9


# ---------------------------------------------------------------------------------------------- 6. the torch twins
def counted(monkeypatch, names):
    """count the library calls of `names` and pass them through"""
    from lerf_pytorch_amd import _lib
    L, calls = _lib.lib(), {n: 0 for n in names}
    for n in names:
        def through(*a, _n=n, _f=getattr(L, n)):
            calls[_n] += 1
            return _f(*a)
        monkeypatch.setattr(L, n, through)
    return calls


def test_splat_torch_follows_the_flag(torch, monkeypatch):
    from lerf_pytorch_amd import _lib, coords
    X, F, M = make_case(POWER_CASE)
    ref = _lib.splat_host(X, F, (8, 8), M, True)
    C = X.shape[0]
    dX, dF, dM = (_dev(torch, a) for a in (X, F, M))
    calls = counted(monkeypatch, ("lerf_splat", "lerf_splat_ordered"))
    out, norm = coords.splat_torch(dX, dF, (8, 8), dM, return_norm=True, deterministic=True)
    assert same_bits(_np(out), ref[:C]) and same_bits(_np(norm), ref[C]) and calls == {"lerf_splat": 0, "lerf_splat_ordered": 1}
    x = dX.clone().requires_grad_(True)
    out = coords.splat_torch(x, dF, (8, 8), dM, deterministic=True)
    assert same_bits(_np(out), ref[:C]) and calls["lerf_splat_ordered"] == 2
    out.sum().backward()
    assert bool(torch.isfinite(x.grad).all())
    was = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        out = coords.splat_torch(dX, dF, (8, 8), dM, return_norm=True)[0]
        assert same_bits(_np(out), ref[:C]) and calls == {"lerf_splat": 0, "lerf_splat_ordered": 3}
        coords.splat_torch(dX, dF, (8, 8), dM, deterministic=False)
        assert calls == {"lerf_splat": 1, "lerf_splat_ordered": 3}
    finally:
        torch.use_deterministic_algorithms(was)
    coords.splat_torch(dX, dF, (8, 8), dM)                       # the flag is off again: None is the atomic kernel
    coords.splat(dX, dF, (8, 8), dM)
    assert calls == {"lerf_splat": 3, "lerf_splat_ordered": 3}
    assert same_bits(_np(coords.splat(dX, dF, (8, 8), dM, deterministic=True)), ref[:C]) and calls["lerf_splat_ordered"] == 4


def test_compose_and_invert_torch_follow_the_flag(torch, monkeypatch):
    from lerf_pytorch_amd import _lib, coords
    outer, inner, g = adjoint_case(0, f64, f64)
    outer = np.nan_to_num(outer, nan=3.0)                        # the forward of invert wants a map without holes
    ra, rb = _lib.coords_compose_bwd_host(outer, inner, g)
    names = ("lerf_coords_compose_bwd", "lerf_coords_compose_bwd_ordered", "lerf_coords_invert_bwd", "lerf_coords_invert_bwd_ordered")
    calls = counted(monkeypatch, names)
    dG = _dev(torch, g)

    def compose(**kw):
        a, b = _dev(torch, outer).requires_grad_(True), _dev(torch, inner).requires_grad_(True)
        coords.compose_torch(a, b, **kw).backward(dG)
        return _np(a.grad), _np(b.grad)

    ga, gb = compose(deterministic=True)
    assert same_bits(ga, ra) and same_bits(gb, rb) and calls["lerf_coords_compose_bwd_ordered"] == 1 and calls["lerf_coords_compose_bwd"] == 0
    was = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        ga, gb = compose()
        assert same_bits(ga, ra) and same_bits(gb, rb) and calls["lerf_coords_compose_bwd_ordered"] == 2
    finally:
        torch.use_deterministic_algorithms(was)
    ga, gb = compose(deterministic=False)
    assert same_bits(gb, rb) and np.allclose(ga, ra, rtol=0, atol=1e-12, equal_nan=True)
    assert calls["lerf_coords_compose_bwd"] == 1 and calls["lerf_coords_compose_bwd_ordered"] == 2

    def invert(**kw):
        f = _dev(torch, outer).requires_grad_(True)
        G = coords.invert_torch(f, (11, 13), **kw)
        up = torch.where(torch.isnan(G), torch.zeros_like(G), dG)
        G.backward(up)
        return _np(f.grad), _np(G.detach()), _np(up)

    gf, G, up = invert(deterministic=True)
    assert same_bits(gf, _lib.coords_invert_bwd_host(outer, G, up)) and calls["lerf_coords_invert_bwd_ordered"] == 1
    try:
        torch.use_deterministic_algorithms(True)
        gf2, _, _ = invert()
        flow = _dev(torch, 0.05 * np.sin(np.arange(7 * 9 * 2, dtype=f64)).reshape(7, 9, 2)).requires_grad_(True)
        coords.invert_flow_torch(flow).nan_to_num().sum().backward()
    finally:
        torch.use_deterministic_algorithms(was)
    assert same_bits(gf2, gf) and calls["lerf_coords_invert_bwd_ordered"] == 3 and calls["lerf_coords_invert_bwd"] == 0
    invert(deterministic=False)
    assert calls["lerf_coords_invert_bwd"] == 1 and calls["lerf_coords_invert_bwd_ordered"] == 3
