"""The oracle's dump of a k-mer sketch in the layout of the exported state vector (orc_sketch_state, Oracle.sketch_state): tied to the
four numbers that tests/test_sketch_oracle.py already pins to the reference's kmerstream code, to StreamCounter::join, and — once —
the reason the GPU tests compare the words and not the estimates (tests/test_gpu_sketch_state.py)."""
import numpy as np
import pytest

from tests import sketch_state as ss


@pytest.fixture(scope="module")
def saturated():
    """The oracle over the three batches of the GPU file's test 1: its dump after each batch, and its four numbers at the end."""
    batches, ref_len = ss.saturation_batches()
    o = ss.oracle(ref_len, **ss.SAT)
    states = []
    for b in batches:
        assert o.process(b) == 0
        states.append(o.sketch_state(0, 0))
    return states, ss.results(o)[0]


@pytest.mark.parametrize("e", [0.2, 0.01])
def test_estimates_recomputed_from_the_dump(e):
    """sumCount, F2 and the per-level zero / one counts put through the F0 and f1 formulas, from the dump alone, are orc_sketch_results;
    several levels in use, two pairs with different tables (q 30 restarts k-mers at three bases in a hundred)."""
    cols, ref_len = ss.random_reads(7, np.full(3000, 150))
    low = np.random.default_rng(8).random(cols["qual"].size) < 0.03
    cols["qual"][low] = 20
    o = ss.oracle(ref_len, klist=[32], qlist=[17, 30], e=e, seed=3)
    assert o.process(cols) == 0
    dumps = [o.sketch_state(0, p) for p in range(2)]
    want = ss.results(o)
    used = [int((ss.parse(d, e)[2] != 0).any(axis=1).sum()) for d in dumps]
    assert min(used) >= 10, used
    for d, w in zip(dumps, want):
        assert d.dtype == np.uint64 and len(d) == ss.sizes(e)[2]
        got, (l0, l1) = ss.estimates(d, e)
        assert got == w and l0 is not None and l1 is not None, (got, w, l0, l1)
    assert want[0] != want[1] and want[0][0] > want[1][0] > 0


def test_join_is_the_saturating_sum():
    """StreamCounter::join (StreamCounter.hpp:95-112): min(15, a + b) per counter, F2 and sumCount added — against one oracle that
    took both inputs."""
    e = ss.SAT["e"]
    (a, na), (b, nb) = ss.random_reads(21, np.full(2000, 150)), ss.random_reads(22, np.full(1500, 100))
    dumps = []
    for parts in ((a,), (b,), (a, b)):
        o = ss.oracle(max(na, nb), **ss.SAT)
        for p in parts:
            assert o.process(p) == 0
        dumps.append(ss.parse(o.sketch_state(0, 0), e))
    (sa, fa, ca), (sb, fb, cb), (s, f, c) = dumps
    assert sa + sb == s and np.array_equal(fa + fb, f)
    assert np.array_equal(np.minimum(15, ca.astype(np.uint32) + cb), c)
    assert (ca[0] == 15).any() and (ca[0] < 15).any() and (c[3] > np.maximum(ca[3], cb[3])).any()  # (saturating and plain sums both occur)


def test_saturation_conditions(saturated):
    ss.assert_saturation_conditions(saturated[0])


def test_estimates_are_blind_to_what_the_words_show(saturated):
    """Three single changes to the table after batch 3, each one a table the kernels could produce: a level whose clamp is lost, a
    level whose increments were suppressed, a level whose counter index is off by one.  sumCount, F0, f1 and F2 stay what they are;
    the compared words change."""
    states, want = saturated
    e, base = ss.SAT["e"], states[2]
    s, f2, ctr = ss.parse(base, e)
    got, (l0, l1) = ss.estimates(base, e)
    assert got == want
    quiet = [w for w in range(8, 32) if w not in (l0, l1) and 0 < (ctr[w] != 0).sum() and len(np.unique(ctr[w])) > 1]
    assert (ctr[0] == 15).all() and len(quiet) >= 2, (l0, l1, quiet)

    def changed(level, row):
        c = ctr.astype(np.uint16)
        c[level] = row
        return ss.build(s, f2, c)

    R = ctr.shape[1]
    mutants = dict(clamp_lost=changed(0, 16 + np.arange(R) % 25),                # counters 16 .. 40 in a saturated level
                   level_cleared=changed(quiet[0], 0),                           # (its increments wrongly masked off)
                   index_rotated=changed(quiet[1], np.roll(ctr[quiet[1]], 1)))   # (hash >> w instead of hash >> (w + 1), say)
    for name, m in mutants.items():
        assert ss.estimates(m, e)[0] == want, name
        d = ss.describe(m, base, e)
        assert d is not None and "counters, level" in d, (name, d)
    assert "level 0, index 0: 16 != 15" in ss.describe(mutants["clamp_lost"], base, e)
    assert "level %d" % quiet[0] in ss.describe(mutants["level_cleared"], base, e)
