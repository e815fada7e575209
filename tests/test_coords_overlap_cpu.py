"""CPU-only, exhaustive: WHICH OPERANDS OF A COORDINATE-MAP CALL MAY INTERSECT, on every host twin the argument generator of
tools/fuzz_coords_args.py knows (include/lerf_hip.h: "a refused call launches and writes nothing").

The policy the header states entry point by entry point is one sentence: an operand the call WRITES -- an output, keys, a gradient, a
workspace -- intersects no other operand of the call.  For every host twin, single and batched (n_sets = 2), the generator builds one
valid call with every optional operand present (Z.full_call), and

  * for every ordered pair (written operand, any other operand) the written operand's pointer is moved onto the other: the call
    returns LERF_EINVAL and leaves the arena as it found it;
  * for every pair of operands the call only reads, one is moved onto the other: the call is still accepted.

THE EXCEPTIONS, each stated and asserted below:
  1. lerf_coords_mesh_host         a single map may be written over its control mesh (the policy holds in a batch only)
  2. lerf_coords_compose_host      a single map may be written over either input (the policy holds in a batch only)
  3. lerf_coords_mesh_bwd          likewise for the single-map adjoint (device-only: asserted where there is no device, where an
                                   accepted call fails at its launch; the batched form refuses every pair)
  4. lerf_coords_compose_batched_host   out may BE b -- the same pointer, dtype, row stride and set stride: in place -- and nothing else
and one operand that is not an operand of the table at all:
  5. lerf_coords_build_host        params are host doubles copied BY VALUE before anything is written, so out may lie on them

Which pointers a call writes is marked in the generator from the header's text, not read from csrc/lerf_coords.hip.
"""
import os
import sys

import pytest

from conftest import REPO

from lerf_pytorch_amd import _lib

sys.path.insert(0, os.path.join(REPO, "tools"))
import fuzz_coords_args as Z  # noqa: E402

EINVAL = -1
# exceptions 1, 2 and 5: (entry point, written operand) -> the operands it may lie on
ALLOWED = {("lerf_coords_mesh_host", "out"): {"ctrl"}, ("lerf_coords_compose_host", "out"): {"a", "b"},
           ("lerf_coords_build_host", "out"): {"params"}}


def _variants():
    for name, (builder, batched) in sorted(Z.HOST.items()):
        for b in ([False, True] if name in Z.OWN_NSETS else [batched]):
            yield pytest.param(name, builder, b, id="%s-%d" % (name, 2 if b else 1))


class Moved:
    """the full call of one entry point, and what it returns and leaves with one pointer moved onto another"""

    def __init__(self, name, builder, batched):
        self.name, self.fn, self.arena = name, getattr(_lib.lib(), name), Z.Arena()
        self.call = Z.full_call(builder, batched)
        self.ptrs = [(i, a.meta["name"], a.meta["writes"]) for i, a in enumerate(self.call.args) if a.kind == "ptr"]
        assert all(self.call.args[i].v is not None for i, _, _ in self.ptrs)                # every optional operand is present
        assert len({self.call.args[i].v for i, _, _ in self.ptrs}) == len(self.ptrs)        # and in a slot of its own
        self.arena.reset()
        for off, values in self.call.planes:
            self.arena.put(off, values)
        self.clean = self.arena.digest()

    def run(self, moves=()):
        args = [("p", a.v) if a.kind == "ptr" else a.v for a in self.call.args]
        for i, j in moves:
            args[i] = args[j]
        return Z.run_case(self.fn, self.arena, args, self.call.tail, self.call.planes)


@pytest.mark.parametrize("name,builder,batched", _variants())
def test_a_written_operand_intersects_no_other_and_read_operands_may_alias(name, builder, batched):
    m = Moved(name, builder, batched)
    assert m.run()[0] == 0                                                   # the call itself is valid
    assert any(w for _, _, w in m.ptrs), name                                 # and writes something
    for i, x, x_writes in m.ptrs:
        for j, y, y_writes in m.ptrs:
            if i == j:
                continue
            rc, digest = m.run([(i, j)])
            if (x_writes and y in ALLOWED.get((name, x), ())) or (y_writes and x in ALLOWED.get((name, y), ())):
                assert rc == 0, (name, x, y)                                  # the stated exception
            elif x_writes or y_writes:
                assert rc == EINVAL and digest == m.clean, (name, x, "onto", y, rc)
            else:
                assert rc == 0, (name, x, "onto", y, rc)


def test_the_generator_knows_every_host_twin_with_two_operands():
    """every lerf_coords_*_host / lerf_splat*_host export that takes a map is in the generator's table (math has three plain vectors
    and its own checks: no operand table)"""
    hosts = {n for n in _lib.EXPORTS if n.endswith("_host") and (n.startswith("lerf_coords_") or n.startswith("lerf_splat"))}
    assert hosts - set(Z.HOST) == {"lerf_coords_math_host"}
    assert set(Z.HOST) <= hosts


def test_exception_compose_in_a_batch_out_may_be_b_in_place_and_nothing_else():
    """exception 4: out == b with equal dtype, row stride and set stride is the in-place form; with any of the three different, or
    out on a, the batched call is refused and writes nothing"""
    m = Moved("lerf_coords_compose_batched_host", Z.compose, True)
    a = m.call.args
    # a, a_dtype, a_stride, aH, aW, b, b_dtype, b_stride, out, out_dtype, out_stride, oH, oW, n_sets, a_set, b_set, out_set
    A, B, B_DT, B_RS, OUT, OUT_DT, OUT_RS, B_SET, OUT_SET = 0, 5, 6, 7, 8, 9, 10, 15, 16
    assert [a[k].kind for k in (A, B, OUT)] == ["ptr"] * 3 and a[OUT_SET].kind == "sstride" and len(a) == 17
    w = a[B_RS].meta["w"]
    a[B_RS].v = a[OUT_RS].v = 2 * w
    a[B_SET].v = a[OUT_SET].v = 200                                           # room for a padded 6 x 6 map: 5 * 16 + 12 elements
    a[OUT_DT].v = a[B_DT].v
    assert m.run([(OUT, B)])[0] == 0                                          # in place
    rc, digest = m.run([(OUT, A)])
    assert rc == EINVAL and digest == m.clean
    for k, other in ((OUT_DT, Z.F32 + Z.F64 - a[B_DT].v), (OUT_RS, 2 * w + 4), (OUT_SET, 202)):
        same, a[k].v = a[k].v, other
        assert m.run()[0] == 0, k                                             # a valid call apart from the overlap ...
        rc, digest = m.run([(OUT, B)])
        assert rc == EINVAL and digest == m.clean, k                          # ... which is then no longer "in place"
        a[k].v = same


def test_exception_mesh_bwd_refuses_every_overlap_in_a_batch_only():
    """exception 3.  The batched adjoint refuses its three pairs before it looks for a device (host pointers: a refused call never
    reads them).  The single-map form accepts them; an accepted call launches, so that half runs only where there is no device and the
    launch fails without touching anything."""
    m = Moved("lerf_coords_mesh_bwd_batched", Z.mesh_bwd, True)
    assert [n for _, n, _ in m.ptrs] == ["g", "gc", "ws"]
    for i, x, _ in m.ptrs:
        for j, y, _ in m.ptrs:
            if i != j:
                rc, digest = m.run([(i, j)])
                assert rc == EINVAL and digest == m.clean, (x, y)
    if _lib.lib().lerf_device_count() > 0:
        return
    m = Moved("lerf_coords_mesh_bwd", Z.mesh_bwd, False)
    for i, x, _ in m.ptrs:
        for j, y, _ in m.ptrs:
            if i != j:
                rc, digest = m.run([(i, j)])
                assert rc not in (0, EINVAL) and digest == m.clean, (x, y, rc)
