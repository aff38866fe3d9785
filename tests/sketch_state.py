"""Test infrastructure for the k-mer sketch's exported tables (no GPU use): the sizes and the layout of a sketch in the flat state
vector, the estimators of StreamCounter.hpp restated over a dump, the word-by-word comparison with its message, and the inputs
that tests/test_sketch_state_cpu.py and tests/test_gpu_sketch_state.py share.

A sketch is [sumCount][F2 table, F2size words][32 levels x R counters]; a counter is a 16-bit field, four per word, counter j of
level w in field w * R + j (bits 16 (f & 3) of word f // 4).  oracle/sketch_oracle.c (orc_sketch_state) writes the reference's
StreamCounter in that layout; k_sketch_export (bamqc_amd/csrc/sketch.hip) writes the card's tables."""
import math

import numpy as np

from tests.adp_steps import FIRST, LAST, MAIN, P, REV, cols_of_nibbles
from tests.long_layout import dna_ref
from tests.oracle_lib import Oracle

LEVELS = 32
NAN_AS_SIZE_T = 9223372036854775808  # (size_t)(0.0 / 0) of the reference's build: no level in range
ACGT = np.array([1, 2, 4, 8], np.uint8)  # BAM 4-bit codes


def _pow2(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def sizes(e):
    """(F2size, R = counters per level, words per sketch) as the StreamCounter ctor sizes them (StreamCounter.hpp:25-46)."""
    f2 = _pow2(int(2.0 / (e * e) + 1))
    r = _pow2((max(8192, int(48.0 / (e * e) + 1)) + 15) // 16) * 16
    return f2, r, 1 + f2 + LEVELS * r // 4


def parse(words, e):
    """-> (sumCount, F2 table, counters[32][R]) of one sketch's words; the counters as np.uint16 (what the fields hold)."""
    f2, r, n = sizes(e)
    words = np.ascontiguousarray(words, np.uint64)
    assert words.shape == (n,), (words.shape, n)
    return int(words[0]), words[1:1 + f2], words[1 + f2:].view("<u2").reshape(LEVELS, r)


def build(sum_count, f2, ctr):
    """parse's inverse (counters of any integer type; values must fit a field)."""
    assert int(np.max(ctr)) <= 0xFFFF
    return np.concatenate([np.array([sum_count], np.uint64), np.asarray(f2, np.uint64),
                           np.ascontiguousarray(ctr, "<u2").reshape(-1).view(np.uint64)])


def estimates(words, e):
    """(sumCount, F0, f1, F2) from a sketch's words, by the formulas of StreamCounter::F0 / f1 / F2 (StreamCounter.hpp:114-172, 308-317;
    sc_F0, sc_f1, sc_F2 of the oracle), and the level F0 and f1 took (None: none).  Counters above 15 count as what they are: > 1."""
    s, f2, ctr = parse(words, e)
    R = ctr.shape[1]
    r0 = [int(x) for x in (ctr == 0).sum(axis=1)]
    r1 = [int(x) for x in (ctr == 1).sum(axis=1)]

    def scan(level_value, occupancy):
        limit = 0.2
        while limit > 1e-8:
            for i in range(LEVELS):
                t = occupancy(i)
                if t <= (1 - limit) * R and t >= limit * R:
                    return int(level_value(i)), i
            limit = limit / 1.5
        return NAN_AS_SIZE_T, None

    F0, l0 = scan(lambda i: (math.log(1.0 - (R - r0[i]) / float(R)) / math.log(1.0 - 1.0 / R)) * math.pow(2.0, i + 1), lambda i: R - r0[i])
    f1, l1 = scan(lambda i: float(R - 1) * (r1[i] / float(r0[i])) * math.pow(2.0, i + 1), lambda i: r0[i])
    c = f2.astype(np.float64)
    tot, sq = float(c.sum()), float((c * c).sum())  # (integers below 2^53: exact in any order)
    return (s, F0, f1, int(sq + (sq - tot * tot) / len(f2))), (l0, l1)


def results(o, lane=0):
    """orc_sketch_results of a read group as [(sumCount, F0, f1, F2), ...] in pair order (finalises the oracle)."""
    return [tuple(int(x) for x in s[2:]) for s in o.finalize()[lane]["sketch"]]


def describe(got, want, e):
    """None when the words are equal, else the first difference: section, level, index, both values, and how many words differ."""
    bad = np.flatnonzero(got != want)
    if not len(bad):
        return None
    f2, r, n = sizes(e)
    i = int(bad[0])
    if i == 0:
        where, g, w = "sumCount", int(got[0]), int(want[0])
    elif i <= f2:
        where, g, w = "F2[%d]" % (i - 1), int(got[i]), int(want[i])
    else:
        gf, wf = got[i:i + 1].view("<u2"), want[i:i + 1].view("<u2")
        k = int(np.flatnonzero(gf != wf)[0])
        f = 4 * (i - 1 - f2) + k
        where, g, w = "counters, level %d, index %d" % (f // r, f % r), int(gf[k]), int(wf[k])
    return "%d words differ, first: %s: %d != %d" % (len(bad), where, g, w)


def assert_block(block, o, n_lanes, n_pairs, e, what=""):
    """block: the sketch words of an exported state vector, [lane][pair] order; o: the oracle that took the same batches."""
    n = sizes(e)[2]
    assert block.shape == (n_lanes * n_pairs * n,), (block.shape, n_lanes, n_pairs, n)
    for lane in range(n_lanes):
        for pair in range(n_pairs):
            at = (lane * n_pairs + pair) * n
            d = describe(block[at:at + n], o.sketch_state(lane, pair), e)
            assert d is None, "%s: read group %d, pair %d: %s" % (what, lane, pair, d)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def random_reads(seed, L, lane=None, rev=None, qual=40):
    """Reads of independently random A/C/G/T (they fill the tables: reads drawn from a small reference repeat their k-mers), first and
    second mates in turn, strands as `rev` says (default: every third read reverse), one quality.  L: the lengths.  -> (cols, contig length)"""
    rng = np.random.default_rng(seed)
    L = np.asarray(L, np.int64)
    n = len(L)
    rev = (np.arange(n) % 3 == 2) if rev is None else np.asarray(rev, bool)
    flag = P | MAIN | np.where(np.arange(n) & 1, LAST, FIRST) | np.where(rev, REV, 0)
    cols, ref_len = cols_of_nibbles(ACGT[rng.integers(0, 4, int(L.sum()))], L, flag, lane)
    cols["qual"][:] = qual
    return cols, ref_len


CONTEXT = dict(n_refs=1, max_read_len=4096, isize=2000)  # what the library's context and the oracle are both made with


def oracle(ref, **opts):
    """An oracle context on one contig: `ref` is its Dna5 codes, or the length of tests.long_layout.dna_ref(77, .)."""
    return Oracle(**dict(CONTEXT, **opts)).reference(0, dna_ref(77, ref) if isinstance(ref, int) else ref)


SAT = dict(klist=[32], qlist=[17], e=0.2, seed=1, n_lanes=1)  # test 1 of the GPU file: 8192 counters per level, 64 F2 entries
SAT_READS = 6000                                              # x 150 bp, k 32: 714 000 hashes a batch


def saturation_batches():
    """Three batches that fill level 0 in the first, level 1 in the second and all but a few counters of level 2 in the third (a mean of
    33 increments per counter: 0 to 3 counters stay below 15, depending on the third batch's seed; with 308 it is three, and level 3 is
    half full either way) -> ([cols] * 3, contig length)"""
    made = [random_reads(seed, np.full(SAT_READS, 150)) for seed in (301, 302, 308)]
    return [c for c, n in made], max(n for c, n in made)


def assert_saturation_conditions(states):
    """states: the oracle's dump after each of the three batches (the conditions the GPU comparison rests on)."""
    e = SAT["e"]
    c1, c2, c3 = (parse(s, e)[2] for s in states)
    assert (c1[0] == 15).all() and not (c1[1] == 15).all(), "after batch 1: level 0 full, level 1 not yet"
    assert (c2[1] == 15).all(), "after batch 2: level 1 full"
    assert (c3[2] < 15).any() and (c3[2] == 15).any(), "after batch 3: level 2 holds counters below 15 and at 15"
    occ = (c3 != 0).mean(axis=1)
    assert ((occ[8:] >= 0.05) & (occ[8:] <= 0.5)).any(), "some level at or above 8 between 5 % and 50 % occupied: %s" % occ[8:16]
