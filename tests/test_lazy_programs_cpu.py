"""CPU: the seeded program generator of tests/lazy_programs.py covers what tests/test_gpu_lazy_fuzz.py relies on.  The programs
run here on plain numpy with a stub pass (no library, no GPU); what is asserted are conditions on the fixed seed list -- every
statement kind and derive operator is there often enough, the two interleavings the generator places on purpose have their
shares -- so that a fuzz run that passes has passed on programs of the intended kind."""
import numpy as np

import lazy_programs as lp

PROGRAMS = [lp.generate(s) for s in lp.SEEDS]
FACTS = [lp.analyse(p) for p in PROGRAMS]


def test_generation_is_deterministic():
    assert len(set(lp.SEEDS)) == len(lp.SEEDS)
    for s, p in zip(lp.SEEDS, PROGRAMS):
        assert lp.generate(s) == p and lp.render(lp.generate(s)) == lp.render(p)
    assert len({lp.render(p) for p in PROGRAMS}) == len(PROGRAMS)


def test_no_program_is_empty():
    for s, p, f in zip(lp.SEEDS, PROGRAMS, FACTS):
        assert f["kinds"]["start"] >= 1 and f["kinds"]["accumulate"] >= 1 and f["kinds"]["derive"] >= 1, s
        assert lp.render(p).strip()


def test_every_statement_kind_and_derive_operator_occurs_20_times():
    for kind in lp.KINDS:
        assert sum(f["kinds"][kind] for f in FACTS) >= 20, kind
    for op in lp.DERIVE_OPS:
        assert sum(f["ops"][op] for f in FACTS) >= 20, op
    for group in ("start", "accumulate", "finish", "consume", "mutate"):          # and every variant of a kind at all
        for variant in FACTS[0]["detail"][group]:
            assert sum(f["detail"][group][variant] for f in FACTS) >= 1, (group, variant)


def test_interleaving_shares():
    n = len(PROGRAMS)
    assert 2 * sum(f["interleaved"] for f in FACTS) >= n                # derive from a pending sum, accumulate again, then read
    assert 10 * sum(f["fractional_feed"] for f in FACTS) >= n           # round / clip with fractional bounds feeding a pass or / 255
    assert any(f["crossed_int16_bound_with_reader"] for f in FACTS) and max(f["max_passes"] for f in FACTS) <= 18
    chains = [len(st[3]) for p in PROGRAMS for st in p if st[0] == "derive"]
    assert 8 in chains and 9 in chains                                  # the longest fused program and the step that must fall back


def test_every_program_runs_on_plain_numpy():
    for s, p in zip(lp.SEEDS, PROGRAMS):
        a = lp.execute(p, lp.stub_interp, lp.STUB_PADS, lp.STUB_LUTS, lambda x: x, (9, 13))
        b = lp.execute(p, lp.stub_interp, lp.STUB_PADS, lp.STUB_LUTS, lambda x: x, (9, 13))
        assert a and [n for n, _ in a] == [n for n, _ in b], s
        for (name, x), (_, y) in zip(a, b):
            x, y = np.asarray(x), np.asarray(y)
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=True), (s, name)
            assert x.dtype in (np.float32, np.float64), (s, name, x.dtype)


def test_the_stub_pass_stays_in_a_pass_value_range():
    img = lp.image(5, (9, 13))
    for r in range(4):
        for oC in (1, 3):
            out = lp.lut_pass(lp.stub_interp, lp.STUB_PADS, lp.STUB_LUTS, img, "s2_sr0", "c", r, oC)
            assert out.shape == (3 * oC, 9, 13) and out.dtype == np.float64
            assert np.abs(out).max() <= 127 and (out * 16 == np.round(out * 16)).all()
