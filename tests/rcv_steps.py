"""Test infrastructure for the depth over given regions (no GPU use): the constants of k_rcv.hip, read from its #define lines, and the
batches of tests/test_gpu_region_coverage.py, each with its regions.  A batch is built once and never changed.

k_rcv walks a read of at most RC_T operations by a thread and a longer one by a wave, 64 operations a pass; the first region of a base
comes from an index of buckets of BUCKET bases over the regions' ends.  k_rcv_final folds the B + R slots in tiles of RC_TILE.

As in tests/sac_steps.py, no batch puts a read on a main chromosome, sets the proper-pair flag or loads a contig."""
import os
import re

import numpy as np

from tests.sac_steps import D, EQ, FIRST, H, I, LAST, M, N_, OPMAX, P, P_, REV, S, X, cols_flat, cols_of, genome_len, mixed_cigar, query_len  # noqa: F401

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bamqc_amd", "csrc", "k_rcv.hip")


def define(name):
    m = re.search(r"^#define %s\s+(\d+)\b" % name, open(HIP).read(), re.M)
    assert m, name
    return int(m.group(1))


RC_T = define("RC_T")
RC_TILE = define("RC_TILE")
BUCKET = 1 << define("RC_BUCKET_SHIFT")
RC_STEP = define("RC_THREADS")
PASS = 64
END_MAX = (1 << 31) - 1
NO_QUAL = 0x8000


def regions_of(triples):
    """Sorted (rid, start, end) triples as the three arrays of the enable call."""
    t = sorted(triples)
    return tuple(np.array([x[i] for x in t], np.int32) for i in range(3))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the rule: three read groups, two contigs
# ---------------------------------------------------------------------------------------------------------------------------
RULE_REFS = 2
RULE_REGIONS = regions_of([(0, 0, 8), (0, 100, 120), (0, 120, 130), (0, 200, 210), (1, 50, 60)])


def rule_batch(MQ=20):
    """Hand-made reads around the regions of contig 0 (0-8, 100-120 abutting 120-130, 200-210) and contig 1 (50-60), in three read groups."""
    reads = []
    for lane in range(3):
        b = dict(flag=P | (FIRST if lane != 1 else LAST) | (REV if lane == 2 else 0), lane=lane, mapq=max(MQ, 1))

        def add(cigar, pos, b=b, **kw):
            reads.append(dict(b, cigar=cigar, pos=pos, **kw))

        add([(10, M)], 105)                                     # inside a region
        add([(50, M)], 90)                                      # starts before 100-120 and ends behind 120-130: both, whole
        add([(10, M)], 90)                                      # ends exactly at a start: no count
        add([(10, M)], 130)                                     # begins exactly at an end: no count
        add([(10, M)], 115)                                     # across the abutting border
        add([(5, M), (10, D), (5, M)], 100)                     # 105 ... 114 under the deletion
        add([(5, M), (10, N_), (5, M)], 100)                    # the same under a skip
        add([(5, M), (3, I), (5, M)], 110)                      # an insertion moves nothing on the genome
        add([(6, S), (4, M)], 118)                              # the soft clip lies in front of pos
        add([(3, H), (2, P_), (6, M), (2, P_), (4, M), (5, H)], 112)  # H and P move nothing
        add([(4, EQ), (2, X), (4, EQ)], 198)                    # = and X runs over a region's start
        add([(6, M)] + [(4, op) for op in range(9, 16)] + [(4, M)], 205)  # codes 9 ... 15 do nothing
        add([(30, M)], 100, L=6)                                # l_seq shorter than the CIGAR: 6 bases covered, A += 6
        add([(4, M), (4, I), (30, M)], 100, L=10)               # the cut inside the second run: 2 bases of it
        add([(4, M), (8, S), (30, M)], 100, L=10)               # j passes l_seq under the clip: the second run covers nothing
        add([(12, M)], 0)                                       # pos at 0, over the region's end
        add([(3, M)], 0, flag=b["flag"] | NO_QUAL)              # no qualities stored: counts
        add([(10, M)], 105, mapq=max(MQ, 1) - 1)                # below MQ (MQ = 0: mapq 0, which counts)
        add([(10, M)], 105, mapq=MQ)
        for extra in (0x4, 0x100, 0x200, 0x400, 0x800):         # each excluded flag bit alone
            add([(10, M)], 105, flag=b["flag"] | extra)
        add([(10, M)], 105, flag=b["flag"] | 0x20 | 0x8)        # the mate's flags are not looked at
        add([(10, M)], 105, rid=-1)
        add([(20, M)], 45, rid=1)                               # the other contig: the whole region
        add([(10, M)], 300)                                     # examined, on no region: E and A only
        add([(5, D), (10, M)], 95)                              # a leading deletion: the run starts at 100
    return cols_of(reads, 1), RULE_REGIONS


# ---------------------------------------------------------------------------------------------------------------------------
# 2. lookup edges
# ---------------------------------------------------------------------------------------------------------------------------
LOOKUP_REFS = 4
MB = 1 << 20


def lookup_batch():
    """Contig 0: regions that begin or end on bucket borders - 1, + 0, + 1 and a region of 1 Mb with reads only in its middle and its last
    bucket.  Contig 1: no region.  Contig 2: a region that ends at 2^31 - 1 with a read on its last base.  Contig 3: regions, and a read
    behind the last of them."""
    big0 = 40 * BUCKET + 17
    trip = [(0, 10, BUCKET - 1), (0, BUCKET, BUCKET + 5), (0, BUCKET + 6, 2 * BUCKET), (0, 2 * BUCKET + 1, 3 * BUCKET + 1), (0, 4 * BUCKET - 1, 4 * BUCKET),
            (0, 5 * BUCKET, 5 * BUCKET + 1), (0, big0, big0 + MB), (2, END_MAX - 50, END_MAX), (3, 5, 9), (3, 3 * BUCKET + 3, 3 * BUCKET + 30)]
    regions = regions_of(trip)
    reads = []
    for _, s, e in trip[:6]:
        for p in (s - 3, s - 2, s - 1, s, e - 3, e - 2, e - 1, e):
            if p >= 0:
                reads.append(dict(cigar=[(3, M)], pos=p))
                reads.append(dict(cigar=[(1, S), (2, M), (1, I), (1, M)], pos=p, flag=P | LAST | REV))
    reads.append(dict(cigar=[(6 * BUCKET, M)], pos=0))                                   # one operation over all six
    reads.append(dict(cigar=[(100, M)], pos=big0 + MB // 2))                             # the 1 Mb region: its middle
    reads.append(dict(cigar=[(100, M), (50, D), (30, M)], pos=big0 + MB // 2 + BUCKET))
    reads.append(dict(cigar=[(100, M)], pos=big0 + MB - 60))                             # its last bucket, over its end
    reads.append(dict(cigar=[(10, M)], pos=big0 + MB))                                   # directly behind it
    reads.append(dict(cigar=[(100, M)], pos=1000, rid=1))                                # the contig without regions
    reads.append(dict(cigar=[(1, M)], pos=END_MAX - 1, rid=2))                           # the last base there can be
    reads.append(dict(cigar=[(40, M)], pos=END_MAX - 60, rid=2))
    reads.append(dict(cigar=[(40, M)], pos=END_MAX - 20, rid=2))                         # runs past 2^31 - 1
    reads.append(dict(cigar=[(10, M), (OPMAX, D), (10, M)], pos=END_MAX - 55, rid=2))    # g passes 2^31: nothing wraps
    reads.append(dict(cigar=[(10, M)], pos=0, rid=3))
    reads.append(dict(cigar=[(10, M)], pos=3 * BUCKET + 10, rid=3))
    reads.append(dict(cigar=[(10, M)], pos=3 * BUCKET + 30, rid=3))                      # behind the last region, in its bucket
    reads.append(dict(cigar=[(10, M)], pos=9 * BUCKET, rid=3))                           # behind the contig's last bucket
    reads.append(dict(cigar=[(10, M)], pos=-4, rid=3))                                   # starts in front of the contig
    return cols_of(reads, 2), regions


# ---------------------------------------------------------------------------------------------------------------------------
# 3. many regions under one operation
# ---------------------------------------------------------------------------------------------------------------------------
def many_batch():
    """Regions of length 1 on every second base over 2 x BUCKET bases from 1000 on; one M of 10 kb over all of them, a read whose deletion
    jumps over half of them, the same two down the wave path."""
    regions = regions_of([(0, p, p + 1) for p in range(1000, 1000 + 2 * BUCKET, 2)])
    pad = [(0, M), (5, P_)] * (RC_T // 2 + 1)
    reads = [dict(cigar=[(10_000, M)], pos=900), dict(cigar=[(151, M), (BUCKET, D), (5000, M)], pos=950, lane=1)]
    reads += [dict(cigar=pad + [(10_000, M)], pos=900, lane=1), dict(cigar=pad + [(151, M), (BUCKET, N_), (5000, M)], pos=950)]
    return cols_of(reads, 3), regions


# ---------------------------------------------------------------------------------------------------------------------------
# 4. CIGAR lengths on both paths
# ---------------------------------------------------------------------------------------------------------------------------
PATH_NCIGARS = [1, RC_T, RC_T + 1, PASS, PASS + 1, 2 * PASS + 1, 1000]


def path_batch():
    """Per operation count a forward read, a reverse read and a read three bases shorter than its CIGAR, from pos 1000; regions of 7 bases
    every 10 bases, so that operations of every pass lie on regions and between them."""
    reads = []
    for nc in PATH_NCIGARS:
        one = nc == 1
        reads.append(dict(cigar=[(33, M)] if one else mixed_cigar(nc, 0), pos=1000))
        reads.append(dict(cigar=[(33, EQ)] if one else mixed_cigar(nc, 1), pos=1000, flag=P | LAST | REV))
        c = [(33, X)] if one else mixed_cigar(nc, 2)
        reads.append(dict(cigar=c, pos=1003, L=query_len(c) - 3))
    span = max(genome_len(r["cigar"]) for r in reads)
    return reads, regions_of([(0, p, p + 7) for p in range(990, 1000 + span + 20, 10)])


# ---------------------------------------------------------------------------------------------------------------------------
# 5. contention, 6. sums
# ---------------------------------------------------------------------------------------------------------------------------
def hot_batch(n=20_000):
    """n identical reads of 60 bases over 40 bases of one 100-base region, alternating between two read groups."""
    L = np.full(n, 60)
    return cols_flat(L, np.full(n, P | FIRST), np.ones(n), np.full(n, 60 << 4), np.full(n, 480), lane=np.arange(n) % 2), regions_of([(0, 400, 500)])


def groups_batch(seed=44, n=2600, n_lanes=4):
    """Read groups alternating and in runs, two contigs with regions of 1 to 60 bases, CIGARs of 1 to 19 operations, some reads shorter than
    their CIGAR, one read in ten not examined, mapq of every kind."""
    rng = np.random.default_rng(seed)
    lane = [i % n_lanes for i in range(80)]
    while len(lane) < n:  # (the read groups take turns, so that each gets its share)
        lane += [(lane[-1] + 1) % n_lanes] * int(rng.choice([1, 2, 150]))
    lane = lane[:n]
    reads = []
    for k, g in enumerate(lane):
        cig = [(int(rng.integers(1, 60)), M)]
        for _ in range(int(rng.choice([0, 0, 0, 1, 1, 2, 4, 9]))):
            cig += [(int(rng.integers(1, 40)), int(rng.choice([I, D, D, N_, S]))), (int(rng.integers(1, 60)), M)]
        kind = rng.random()
        f = P | (REV if rng.random() < 0.5 else 0) | (FIRST if rng.random() < 0.5 else LAST)
        f |= 0x100 if kind < 0.02 else 0x800 if kind < 0.04 else 0x4 if kind < 0.06 else 0x400 if kind < 0.08 else 0x200 if kind < 0.1 else 0
        ql = query_len(cig)
        reads.append(dict(cigar=cig, L=ql - (int(rng.integers(1, 10)) if rng.random() < 0.1 and ql > 12 else 0), flag=f, lane=g, rid=int(k % 5 == 0),
                          pos=k * 3, mapq=int(rng.choice([0, 19, 20, 60, 255]))))
    trip, p = [], 2
    while p < 3 * n + 600:
        ln = int(rng.integers(1, 61))
        trip += [(r, p, p + ln) for r in (0, 1)]
        p += ln + int(rng.integers(0, 40))  # (0: abutting)
    return cols_of(reads, seed), regions_of(trip)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. finalize seams
# ---------------------------------------------------------------------------------------------------------------------------
def seam_regions():
    """Lengths 1, RC_TILE - 1, RC_TILE, RC_TILE + 1 and 3 RC_TILE + 5, then length-1 regions up to a run of them whose closing slots fall
    on a tile's last and first slot (a length-1 region owns two slots; one region of length 2 shifts the parity)."""
    trip, p, slot = [], 10, 0
    for ln in (1, RC_TILE - 1, RC_TILE, RC_TILE + 1, 3 * RC_TILE + 5):
        trip.append((0, p, p + ln))
        p += ln + 3
        slot += ln + 1
    # the next tile border behind `slot`, with room for a run of ones in front of it
    closing = []
    border = (slot // RC_TILE + 2) * RC_TILE
    for first in (border - 20, border + RC_TILE - 19):  # a run of ten ones whose last closing slot is border - 1, one whose last is border + RC_TILE
        fill = first - slot - 1                         # one region up to the run
        trip.append((0, p, p + fill))
        p += fill + 3
        slot += fill + 1
        for i in range(10):
            trip.append((0, p, p + 1))
            p += 1 + (0 if i % 3 == 0 else 2)           # (some of them abut)
            slot += 2
            closing.append(slot - 1)
    assert border - 1 in closing and border + RC_TILE in closing, (border, closing)
    return regions_of(trip), border


def seam_batch(seed=7, n=3000):
    """Random reads over the seam regions into lane 1 of 2 (lane 0 stays empty), and 40 identical reads on the first regions, so that
    depths pass small histogram caps."""
    regions, border = seam_regions()
    rng = np.random.default_rng(seed)
    span = int(regions[2][-1]) + 50
    reads = []
    for _ in range(n):
        cig = [(int(rng.integers(20, 400)), M)]
        if rng.random() < 0.3:
            cig += [(int(rng.integers(1, 30)), int(rng.choice([I, D, N_]))), (int(rng.integers(20, 300)), M)]
        reads.append(dict(cigar=cig, pos=int(rng.integers(0, span)), lane=1))
    reads += [dict(cigar=[(300, M)], pos=0, lane=1)] * 40
    return cols_of(reads, seed), regions, border


# ---------------------------------------------------------------------------------------------------------------------------
# 8. another list of the same B + R
# ---------------------------------------------------------------------------------------------------------------------------
LIST_A = regions_of([(0, 100, 200), (0, 300, 400)])
LIST_B = regions_of([(0, 100, 250), (0, 300, 350)])


def list_batch():
    """Reads over 300 ... 400: under list A's slots, list B's first closing slot (150) is the depth at 349, which is not 0."""
    return cols_of([dict(cigar=[(80, M)], pos=p) for p in (290, 300, 320, 340)] + [dict(cigar=[(50, M)], pos=120)], 8)
