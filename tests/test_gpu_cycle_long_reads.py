"""GPU: k_qcyc and k_mbc on long reads (bamqc_amd/csrc/k_qcyc.hip, k_mbc.hip), in contexts with max_read_len raised.

1. k_qcyc behind its row cap: the launcher makes 64 rows of 256 cycles at the most, and the last row takes whatever lies behind its
   tile — reached only with a capacity above 16 384.  Reads of 16 129 .. 17 000 bases at N = 16 500 and 17 408: the loop over the
   bytes 256 and up of a read's part in the last row, its reverse-strand cycles and its clip L > N.
2. Rows with several workgroups: 600 reads of about 10 000 bases among 600 short ones, 40 rows, g1 >= 2, two read groups, a
   capacity that is no multiple of 256.
3. k_mbc's list of 768 runs refilled many times in one step: reads of 3080 runs each (an indel every few bases), in a step that holds
   three read groups, so the tile is flushed and retaken round after round.

The reference is the loop restatement of each statistic (tests/qbc_ref.py, tests/mbc_ref.py), computed once per batch at the larger
capacity: a bin's count does not depend on N (a base counts when its cycle is below N), so the table at a smaller N is the first N
cycles of the larger one.  Every launch shape is asserted from the restated arithmetic (tests/cycle_steps.py) for this card."""
import numpy as np
import pytest

from tests import cycle_steps as cs
from tests import mbc_ref, qbc_ref, synth
from tests import test_gpu_mismatch_by_cycle as tm
from tests import test_gpu_qual_by_cycle as tq
from tests.long_layout import dna_ref, reads_on_ref, records
from tests.parity import split
from tests.test_gpu_value_limits import n_cu

pytestmark = pytest.mark.gpu
P, PR, REV, FIRST, LAST, MAIN = cs.P, cs.PR, cs.REV, cs.FIRST, cs.LAST, cs.MAIN


def draw_quals(rng, n):
    return cs.QUALS[rng.integers(0, len(cs.QUALS), n)]


def both_modules(ref, n_lanes, N, max_read_len):
    return tm.context(ref, n_lanes, N, qual_by_cycle=N, max_read_len=max_read_len)


def check_both(a, counts, H, T, n_lanes, N):
    got_q, got_m = tq.module_words(a, n_lanes, N), tm.module_words(a, n_lanes, N, behind=n_lanes * 2 * N * 224)
    for name, got, want in (("k_qcyc", got_q, H), ("k_mbc", got_m, T)):
        assert np.array_equal(got, want), "%s: %d words differ, first at %s" % (name, (got != want).sum(), np.argwhere(got != want)[0].tolist())
    if counts is not None:
        tq.check_tables(a, counts, H)
        tm.check_tables(a, counts, T)
    return got_q, got_m


# ---------------------------------------------------------------------------------------------------------------------------
# 1. k_qcyc behind the row cap
# ---------------------------------------------------------------------------------------------------------------------------
CAP_LENGTHS = [16_129, 16_383, 16_384, 16_385, 16_640, 17_000]  # 1 .. 872 cycles behind 63 * 256
CAP_MAX = 17_408


@pytest.fixture(scope="module")
def cap():
    ref = dna_ref(51, 60_000)
    rng = np.random.default_rng(52)
    L = [(n, rev | mate) for n in CAP_LENGTHS for rev in (0, REV) for mate in (FIRST, LAST)]
    L += [(int(n), int(rng.choice([0, REV])) | int(rng.choice([FIRST, LAST]))) for n in rng.choice([1, 16, 40, 150, 255], 200)]
    order = rng.permutation(len(L))
    flag = np.array([P | PR | MAIN | L[i][1] for i in order], np.uint16)
    L = np.array([L[i][0] for i in order])
    pos = np.sort(rng.integers(0, len(ref) - 17_100, len(L)))
    cols = tm.plant(reads_on_ref(ref, pos, L, flag, draw_quals(rng, int(L.sum()))), rng, frac=0.01)
    cols["mapq"][:] = 30
    return cols, ref, qbc_ref.table(cols, 1, CAP_MAX), mbc_ref.table(cols, [ref], 1, 4096)


@pytest.mark.parametrize("N", [16_500, CAP_MAX])  # below the longest read (the reverse reads' clip L > N inside the last row) and above it
def test_qcyc_behind_the_64th_row(cap, N):
    cols, ref, H_max, _ = cap
    lay = cs.qcyc_launch(cols["l_seq"], N, n_cu())
    print("row cap N %d: n_cu %d, rows %d, g0 %d, g1 %d, per %d / %d, the last row holds %d cycles" % (
        N, n_cu(), lay["rows"], lay["g0"], lay["g1"], lay["per0"], lay["per1"], lay["last_width"]))
    assert lay["rows"] == cs.MAX_ROWS and lay["last_width"] == min(N, 17_000) - 63 * cs.ROW_CYCLES > 256
    H = H_max[:, :, :N]
    assert H[0, 0, 16_128:].any() and H[0, 1, 16_128:].any() and H[0, :, 16_384:].any()
    a = tq.context(ref, 1, N, max_read_len=CAP_MAX)
    a.submit(cols)
    counts = a.finalize()
    got = tq.module_words(a, 1, N)
    assert np.array_equal(got, H), "%d words differ, first at %s" % ((got != H).sum(), np.argwhere(got != H)[0].tolist())
    tq.check_tables(a, counts, H)
    a.close()


def test_mbc_on_the_same_reads(cap):
    """k_mbc on the 17 000-base reads at N = 4096: reverse reads with L far above N, runs of 4096 positions in 16 and 17 passes."""
    cols, ref, _, T = cap
    assert all(T[0, m, t, 256:].any() for m in range(2) for t in range(2))
    a = tm.context(ref, 1, 4096, max_read_len=CAP_MAX)
    a.submit(cols)
    counts = a.finalize()
    got = tm.module_words(a, 1, 4096)
    assert np.array_equal(got, T), "%d words differ, first at %s" % ((got != T).sum(), np.argwhere(got != T)[0].tolist())
    tm.check_tables(a, counts, T)
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. rows with several workgroups
# ---------------------------------------------------------------------------------------------------------------------------
ROWS_MAX = 10_496


@pytest.fixture(scope="module")
def many_rows():
    ref = dna_ref(61, 80_000)
    rng = np.random.default_rng(62)
    n = 1200
    L = np.where(np.arange(n) % 2 == 0, np.array([9984, 10_000, 10_240, 10_241])[(np.arange(n) // 2) % 4], rng.choice([1, 16, 40, 150, 255], n))
    lane = (np.arange(n) // 290) % 2  # runs of 290 reads
    flag = (P | PR | MAIN | np.where(rng.random(n) < 0.5, REV, 0) | np.where(rng.random(n) < 0.5, FIRST, LAST)).astype(np.uint16)
    pos = np.sort(rng.integers(0, len(ref) - 10_300, n))
    cols = tm.plant(reads_on_ref(ref, pos, L, flag, draw_quals(rng, int(L.sum())), lane=lane), rng, frac=0.01)
    cols["mapq"][:] = 30
    return cols, ref, qbc_ref.table(cols, 2, 10_240), mbc_ref.table(cols, [ref], 2, 10_240)


@pytest.mark.parametrize("N", [10_000, 10_240])
def test_rows_with_several_workgroups(many_rows, N):
    cols, ref, H_max, T_max = many_rows
    lay = cs.qcyc_launch(cols["l_seq"], N, n_cu())
    mb = cs.mbc_launch(len(cols["flag"]), n_cu())
    print("rows N %d: n_cu %d, k_qcyc rows %d, g0 %d, g1 %d, per %d / %d, steps %d / %d, the last row holds %d cycles; k_mbc grid %d per %d" % (
        N, n_cu(), lay["rows"], lay["g0"], lay["g1"], lay["per0"], lay["per1"], max(lay["steps0"]), max(lay["steps1"]), lay["last_width"], mb["grid"], mb["per"]))
    assert lay["g1"] >= 2 and lay["rows"] == 40
    H, T = H_max[:, :, :N], T_max[:, :, :, :N]
    assert all(H[l, m, N - 16:].any() and T[l, m, t, N - 256:].any() for l in range(2) for m in range(2) for t in range(2))
    a = both_modules(ref, 2, N, ROWS_MAX)
    a.submit(cols)
    check_both(a, a.finalize(), H, T, 2, N)
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. k_mbc's rounds
# ---------------------------------------------------------------------------------------------------------------------------
REPEAT = [(1, "M"), (1, "I"), (2, "M"), (1, "D"), (3, "M"), (1, "I"), (5, "M"), (1, "N")]  # 13 read bases, 13 genome positions, 4 runs
NINE = [(20, "M"), (3, "I"), (20, "M"), (2, "D"), (20, "M"), (3, "I"), (20, "M"), (2, "D"), (20, "M")]
ROUNDS_MAX = 10_240


@pytest.fixture(scope="module")
def rounds():
    """161 reads, one workgroup and one step of k_mbc, three read groups.  Eight reads of 770 repeats of REPEAT — 10 010 bases, 6160
    operations, 3080 runs of 1, 2, 3 and 5 positions that start at every alignment mod 4 — on both strands, as both mates, in read
    groups 0 and 2; 150 reads of nine operations (5 runs) in the three read groups; a read whose second run lies 2^28 positions
    behind the contig, one at 2^31 - 200 and one at -3."""
    ref = dna_ref(71, 60_000)
    rng = np.random.default_rng(72)
    cases = [(REPEAT * 770, 500 + 4001 * k + k % 4, P | PR | MAIN | (REV if k & 1 else 0) | (LAST if k & 2 else FIRST), 0 if k & 4 else 2) for k in range(8)]
    cases += [(NINE, 300 + 331 * k, P | PR | MAIN | (REV if k & 2 else 0) | (LAST if k & 1 else FIRST), k % 3) for k in range(150)]
    cases += [([(50, "M"), ((1 << 28) - 1, "N"), (50, "M")], 1000, P | PR | MAIN | FIRST, 1),
              ([(150, "M")], (1 << 31) - 200, P | PR | MAIN | LAST, 1),
              ([(150, "M")], -3, P | PR | MAIN | LAST | REV, 2)]
    recs = []
    for i in rng.permutation(len(cases)):  # (the long reads anywhere among the threads of the step)
        ops, pos, flag, lane = cases[i]
        codes = tm.on_ref(ref, pos, ops, rng)
        recs.append(dict(codes=codes.astype(np.int64), qual=draw_quals(rng, len(codes)), flag=flag, pos=pos, ops=ops, lane=lane,
                         nm=sum(n for n, op in ops if op in "ID")))
    cols = records(recs)
    cols["mapq"][:] = 30  # (no read is eligible for the triplet counters)
    tm.plant(cols, rng, frac=0.02)
    assert (cols["n_cigar"] == 6160).sum() == 8 and (cols["l_seq"] == 10_010).sum() == 8
    return cols, ref, qbc_ref.table(cols, 3, ROUNDS_MAX), mbc_ref.table(cols, [ref], 3, ROUNDS_MAX)


@pytest.mark.parametrize("N", [1024, ROUNDS_MAX])
def test_mbc_rounds_of_a_step_with_three_read_groups(rounds, N):
    cols, ref, H_max, T_max = rounds
    mb = cs.mbc_launch(len(cols["flag"]), n_cu())
    order = cs.processing_order(cols["lane"])
    runs = cs.mbc_runs(cols, [len(ref)], N)
    bound, model = cs.mbc_rounds(runs[order], cols["lane"][order])
    mixed = sum(len(g) >= 2 for g in model)
    print("rounds N %d: n_cu %d, k_mbc grid %d per %d steps %s; %d runs, the most of one thread %d: at least %d rounds; taking slots in turn %d rounds, %d of them with two read groups and more" % (
        N, n_cu(), mb["grid"], mb["per"], mb["steps"], runs.sum(), runs.max(), bound, len(model), mixed))
    assert mb["grid"] == 1 and mb["steps"] == [1] and bound >= 5 and mixed >= 3
    if N == ROUNDS_MAX:
        assert sorted(runs.tolist())[-8:] == [3080] * 8 and runs.max() > 4 * cs.MB_RUNS  # one thread fills the list four times over
    H, T = H_max[:, :, :N], T_max[:, :, :, :N]
    assert all(T[l, m, t].any() for l in range(3) for m in range(2) for t in range(2))
    a = both_modules(ref, 3, N, ROUNDS_MAX)
    a.submit(cols)
    got_q, got_m = check_both(a, a.finalize(), H, T, 3, N)
    a.close()
    b = both_modules(ref, 3, N, ROUNDS_MAX)  # read by read: what a read adds does not depend on its neighbours in the list
    for part in split(cols, list(range(1, len(cols["flag"])))):
        b.submit(part)
    b.finalize()
    again_q, again_m = check_both(b, None, H, T, 3, N)
    assert np.array_equal(again_q, got_q) and np.array_equal(again_m, got_m)
    b.close()
