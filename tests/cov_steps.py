"""The batches of the coverage depth tests (TEST INFRASTRUCTURE; tests/test_gpu_coverage_steps.py runs them on the card,
tests/test_coverage_steps_cpu.py asserts that each of them crosses the edge it is named for): hand-made reads placed window by window.

How a read gets its window (OverallNumbers.hpp:84-110, tests/anchor_recurrence.py): with `shift` the position of the first live
window's first base, a read at position b sits at p = b - shift; p > 2000 (or another contig) flushes both live windows — a reset,
the window index advances by 2 and shift = b; 1000 < p < 2000 flushes one — a slide, index + 1, shift + 1000; p <= 1000 and p = 2000
leave the windows alone.  k_cov works on tiles of 4 windows, numbered from the read group's first live window at batch entry.

No read is eligible for triplet counting (no read is a proper pair), so the contigs may come in any order and their bases are never
read; everything else of the count set is compared with the oracle all the same."""
import collections
import functools

import numpy as np

from tests import cov_ref, synth

P, REV, FIRST, LAST, UNMAPPED = 0x1, 0x10, 0x40, 0x80, 0x4
REF_LEN = 50_000
M10 = ((10, "M"),)
M50 = ((50, "M"),)

Case = collections.namedtuple("Case", "batches n_lanes n_refs opts head")  # head: the leading batches that make a shard's head


def refs_of(n_refs):
    return [np.random.default_rng(4100 + i).integers(0, 4, size=REF_LEN).astype(np.uint8) for i in range(n_refs)]


@functools.lru_cache(maxsize=None)
def _bases(L):
    return ("ACGT" * (L // 4 + 1))[:L]


def rd(pos, ops=M50, rid=0, lane=0, rev=False, last=False):
    """one mapped read that enters coverage(); NM = the inserted and deleted bases (no mismatches)"""
    ops = list(ops)
    L = sum(n for n, c in ops if c in "MIS=X")
    flag = P | (REV if rev else 0) | (LAST if last else FIRST)
    return synth.single_read(_bases(L), [30] * L, ops, flag, pos=pos, rid=rid, nm=sum(n for n, c in ops if c in "ID"), lane=lane)


def unmapped(lane=0):
    return synth.single_read(_bases(50), [30] * 50, [], P | FIRST | UNMAPPED | 0x8, pos=-1, rid=-1, mapq=0, nm=-1, as_=synth.BQC_AS_ABSENT, lane=lane)


def walkers(shift, k, **kw):
    """k reads of 10 bases that slide the windows by one each from `shift` on: positions shift + 1500, + 2500, ... (offset 500 in
    the window they open); behind them shift + 1000 k is the first live window's first base"""
    return [rd(shift + 1500 + 1000 * j, M10, **kw) for j in range(k)]


def case(batches, n_lanes=1, n_refs=1, head=1, **opts):
    return Case([synth.concat(b) if isinstance(b, list) else b for b in batches], n_lanes, n_refs, opts, head)


def one_read_per_batch(c):
    cols = synth.concat(c.batches)
    return c._replace(batches=[synth.slice_batch(cols, i, i + 1) for i in range(len(cols["flag"]))])


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the clamp at 100
# ---------------------------------------------------------------------------------------------------------------------------
CLAMP_K = [99, 100, 101, 102, 300]
CLAMP_STACK_WINDOWS = {"boundary": 0, "common": 4, "live at the end": 13}


def stack(pos, K, **kw):
    return [rd(pos, M50, rev=bool(i & 2), last=bool(i & 1), **kw) for i in range(K)]


def clamp(K):
    """Three stacks of K identical reads of 50 bases, over positions nothing else covers: in window 0 (tile 0: a boundary tile, the
    slow path), in window 4 (tile 1 with the reads going on to window 13: a common tile) and in window 13, which is live at the end
    of the stream (k_cov_final).  15 windows; the other 14 reads cover 10 positions once each.  By hand: 150 positions of depth K,
    140 of depth 1, 14 710 of depth 0."""
    reads = [rd(0, M10)] + stack(200, K) + walkers(0, 4) + stack(4600, K) + walkers(4000, 9) + stack(13_600, K)
    return case([reads])


def clamp_by_hand(K):
    want = np.zeros(cov_ref.COVSIZE + 1, np.uint64)
    want[0], want[1] = 15_000 - 150 - 140, 140
    want[min(K, cov_ref.COVSIZE)] += 150
    return want


def clamp_split():
    """a stack of 101 cut 60 + 41 by a batch end: depth 101 exists only as the second batch's run plus the carry-in"""
    return case([[rd(0, M10)] + stack(200, 60), stack(200, 41) + walkers(0, 3)])


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the window thresholds
# ---------------------------------------------------------------------------------------------------------------------------
THRESHOLD_P = [0, 1, 999, 1000, 1001, 1999, 2000, 2001]
GROUP = 5000  # positions between two anchoring reads: a reset whatever the group before left


def thresholds():
    """After an anchoring read (a reset: shift = its position A) reads at A + p.  Interval ends at 1999, 2000 and 2001 from the
    window start, from offset 0, 999 and 1000; p = 1001 and 1999 slide; p = 2000 stays at offset 2000 and covers nothing, with or
    without a leading clip; p = 2001 resets.  Then 2500M alone, and 100M 2500D 100M (one run of 2700, cut at 2000).  Eight groups on
    contig 0, the rest on contig 1."""
    reads = []
    for k, p in enumerate(THRESHOLD_P):
        A = GROUP * k
        reads.append(rd(A, M10))
        if p == 0:
            reads += [rd(A, ((n, "M"),)) for n in (1999, 2000, 2001)]
        elif p == 999:
            reads += [rd(A + p, ((n, "M"),), rev=True) for n in (1000, 1001, 1002)]
        elif p == 1000:
            reads += [rd(A + p, ((n, "M"),), last=True) for n in (999, 1000, 1001)]
        elif p == 2000:
            reads += [rd(A + p, ((100, "M"),)), rd(A + p, ((5, "S"), (100, "M")), rev=True)]
        else:
            reads.append(rd(A + p, ((100, "M"),)))
    reads += [rd(0, ((2500, "M"),), rid=1), rd(GROUP, M10, rid=1), rd(GROUP + 10, ((100, "M"), (2500, "D"), (100, "M")), rid=1),
              rd(GROUP + 600, M50, rid=1)]
    return case([reads], n_refs=2, max_read_len=4096)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. tile seams
# ---------------------------------------------------------------------------------------------------------------------------
def seams():
    """Two batches, one read group.  Batch 1: a read in window 3, the last of tile 0, that covers [500, 2000) — its own window and
    window 4, the first of tile 1, whose read range must begin at the first read of window 3 (list_begin = first_at(wlo - 1));
    reads of tile 1's own; in window 7, the last of tile 1, a read of 2620 positions from offset 500 (cut at 2000: windows 7 and 8,
    nothing of window 9) and one at offset 1000 exactly (window 8 only).  Window 7 is the batch's last: tile 2 holds nothing but
    that spill, all of it carried out.  Batch 2 numbers its windows from 7: a read over the carried-in depth, then resets to
    relative windows 2, 4, 6 and 8 — windows 3 and 7, the last of their tiles, are never a read's first window and stay at depth
    0 —, a read in window 8 that spills into 9, and two slides."""
    long_d = lambda n: ((10, "M"), (n, "D"), (10, "M"))
    b1 = [rd(0, M10)] + walkers(0, 2) + [rd(3500, long_d(1600), rev=True)] + walkers(3000, 4)[:1] + [rd(4700, M50), rd(4990, M50)] + walkers(4000, 3)[:2]
    # (windows 0 .. 6 so far: the walkers of shift 4000 open 5 and 6)
    b1 += [rd(7500, long_d(2600)), rd(8000, ((300, "M"),), last=True)]
    b2 = [rd(7600, M50), rd(12_000, M10), rd(16_000, M10), rd(20_000, M10), rd(24_000, M10), rd(24_900, ((200, "M"),))] + walkers(24_000, 2)
    return case([b1, b2])


# ---------------------------------------------------------------------------------------------------------------------------
# 4. read-range lengths
# ---------------------------------------------------------------------------------------------------------------------------
RANGE_N = [255, 256, 257, 511, 512, 513, 1025]  # around the two prefetched entries per thread (512) and the loop over the rest


def ranges(N, n_lanes):
    """Tile 1 (windows 4 .. 7) of read group 0 with a read range of exactly N entries: the read of window 3, the one that opens window
    4, a crowd in window 4, a reset to window 6; the reset to window 8 ends the range, and the tile is a common one.  Two read
    groups: both walk the same windows read by read, the crowd alternates between them (group 1: other offsets and lengths), so
    the range holds the other group's reads at the same window numbers and only the read-group filter keeps them out."""
    per = lambda f: [f(lane=l) for l in range(n_lanes)]
    reads = per(lambda lane: rd(0, M10, lane=lane))
    for j in range(4):  # windows 1 .. 4
        reads += per(lambda lane: rd(1500 + 1000 * j, M10, lane=lane))
    S = N - 3 * n_lanes
    for i in range(S):
        lane = i % n_lanes
        reads.append(rd(4100 + (i * 7) % 800, ((30, "M"),), rev=bool(i & 4)) if lane == 0 else rd(4150 + (i * 11) % 700, ((20, "M"),), lane=1, last=True))
    reads += per(lambda lane: rd(6500, M10, lane=lane)) + per(lambda lane: rd(9000, M10, lane=lane))
    return case([reads], n_lanes=n_lanes)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the same virtual coordinates in two read groups
# ---------------------------------------------------------------------------------------------------------------------------
CLIP3 = ((30, "M"), (5, "S"), (30, "M"), (5, "S"), (30, "M"))


def same_coordinates():
    """Two read groups walk windows 0 .. 6 read by read, so their windows carry the same numbers in one mixed batch.  Group 0: three
    plain reads per window.  Group 1: per window two reads with two clips between matches (two extra intervals each), one per
    strand, at other offsets.  Head: the two anchoring reads and one read each; the rest has no gap above 1000."""
    head = [rd(0, M10, lane=0), rd(0, M10, lane=1), rd(300, M50, lane=0), rd(350, CLIP3, lane=1)]
    body = []
    for j in range(6):
        at = 1500 + 1000 * j
        body += [rd(at, M10, lane=0), rd(at, M10, lane=1)]
        body += [rd(at + 100 + 20 * k, M50, lane=0, last=bool(k & 1)) for k in range(3)]
        body += [rd(at + 130, CLIP3, lane=1), rd(at + 160, CLIP3, lane=1, rev=True, last=True)]
    return case([head, body], n_lanes=2)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. more tiles than workgroups
# ---------------------------------------------------------------------------------------------------------------------------
K_COV_GRID = 2048  # bqc_launch_cov: persistent workgroups


def many_tiles():
    """5000 reads, two read groups alternating, each group's consecutive reads on alternating contigs: every read but a group's
    first is a reset (2 windows), 1250 tiles per group, 2500 in the batch — workgroup i < 452 does tile i of group 0, then tile
    i + 2048, which is group 1's.  5000 position breaks: below the 16 384 the card's chain takes."""
    reads = [rd((i * 13) % 4000, ((20, "M"),), rid=(i // 2) % 2, lane=i % 2, rev=bool(i & 4), last=bool(i & 8)) for i in range(5000)]
    return case([reads], n_lanes=2, n_refs=2)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. carry
# ---------------------------------------------------------------------------------------------------------------------------
def absent_group():
    """Three batches: read group 0 in batches 1 and 3, read group 1 in batches 2 and 3.  Group 0's live windows — depth in both —
    and its half of the carry array must survive batch 2, which owns none of its tiles; batch 3 goes on inside them."""
    b1 = [rd(0, M10), rd(300, ((200, "M"),)), rd(900, ((300, "M"),), rev=True), rd(950, M50, last=True)]
    b2 = [rd(100, M10, lane=1), rd(400, ((200, "M"),), lane=1), rd(1000, ((400, "M"),), lane=1, rev=True)] + walkers(0, 2, lane=1)
    b3 = [rd(950, ((100, "M"),)), rd(2700, ((100, "M"),), lane=1), rd(1000, ((150, "M"),)), rd(1500, ((100, "M"),)), rd(3100, M50, lane=1),
          rd(2100, M50)]
    return case([b1, b2, b3], n_lanes=2)


def unmapped_between():
    """a batch of unmapped reads only (no tile, k_cov is not launched) between two batches that share live windows"""
    return case([[rd(0, M10), rd(500, ((300, "M"),)), rd(600, ((300, "M"),)), rd(900, ((300, "M"),))], [unmapped() for _ in range(5)],
                 [rd(700, ((300, "M"),)), rd(1000, M50), rd(1500, ((100, "M"),))]])


# ---------------------------------------------------------------------------------------------------------------------------
# 8. clipped CIGARs, on both strands
# ---------------------------------------------------------------------------------------------------------------------------
def far(d, tail=30):
    return ((10, "M"), (d, "D"), (10, "S"), (tail, "M"))  # a second run that starts d + 20 behind the read's offset


CLIPPED = [
    ((10, "S"), (90, "M")),                                                              # the leading clip shifts the interval
    ((30, "M"), (5, "S"), (30, "M"), (5, "S"), (30, "M"), (5, "S"), (30, "M")),          # three extra intervals
    ((5, "S"), (50, "M"), (20, "S"), (30, "M")),                                         # asymmetric: the strands differ
    ((60, "M"), (40, "D"), (60, "M")),                                                   # M D M: one run
    ((40, "M"), (3, "D"), (7, "S"), (2, "D"), (40, "M")),                                # deletions on both sides of a clip
] + [((30, "M"), (5, c), (30, "M")) for c in "=XNIPH"] + [                                # neither advance nor cover: one run of 60
    far(970), far(980), far(1470), far(1480), far(1985), far(400, 700),                  # runs that cross 2000, start at it or beyond it
    ((500, "S"), (400, "M"), (100, "S"), (24, "M")),
    ((990, "S"), (34, "M")),
]


def clipped():
    """Every CIGAR of CLIPPED four times: on both strands at offset 1000 and on both strands at offset 500 (the positions step by
    500 from 1000 on: every other one slides).  Head: three reads from position 0 that leave live windows; no gap above 500."""
    head = [rd(0, M10), rd(300, M50), rd(600, M50, rev=True)]
    body, at = [], 1000
    for ops in CLIPPED:
        for _ in range(2):
            body += [rd(at, ops, last=True), rd(at, ops, rev=True)]
            at += 500
    return case([head, body])


def extras_200():
    """one read alone in its batch: 201 x 1M and 200 x 1S alternating — 200 extra intervals against a capacity of
    cigar_words / 2 + 1 = 201"""
    ops = tuple(((1, "M"), (1, "S"))[k & 1] for k in range(401))
    return case([[rd(0, M10), rd(300, M50)], [rd(600, ops)], [rd(650, M50), rd(1500, M10)]])


def all_clipped():
    """a batch in which every read is 1M 1S 1M: as many extra intervals as reads"""
    ops = ((1, "M"), (1, "S"), (1, "M"))
    return case([[rd(0, M10)], [rd(100 + (i * 37) % 850, ops, rev=bool(i & 1), last=bool(i & 2)) for i in range(600)], [rd(1500, M10)]])


# ---------------------------------------------------------------------------------------------------------------------------
CASES = {"clamp_%d" % K: functools.partial(clamp, K) for K in CLAMP_K}
CASES.update({"clamp_split": clamp_split, "thresholds": thresholds, "seams": seams})
CASES.update({"range_%d_one_group" % N: functools.partial(ranges, N, 1) for N in RANGE_N})
CASES.update({"range_%d_two_groups" % N: functools.partial(ranges, N, 2) for N in RANGE_N})
CASES.update({"same_coordinates": same_coordinates, "many_tiles": many_tiles,
              "clamp_101_read_by_read": lambda: one_read_per_batch(clamp(101)), "thresholds_read_by_read": lambda: one_read_per_batch(thresholds()),
              "seams_read_by_read": lambda: one_read_per_batch(seams()), "absent_group": absent_group, "unmapped_between": unmapped_between,
              "clipped": clipped, "extras_200": extras_200, "all_clipped": all_clipped})
ANCHORED = ["clamp_101", "thresholds", "seams", "clipped", "many_tiles"]  # also through the card-anchored path
SHARD_TAILS = ["clipped", "same_coordinates", "extras_200"]               # also as the tail of a shard


@functools.lru_cache(maxsize=None)
def get(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement's result for a case, computed once"""
    c = get(name)
    return cov_ref.coverage(c.batches, c.n_lanes, c.n_refs)
