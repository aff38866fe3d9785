"""Test infrastructure for the depth in fixed genome windows (no GPU use): the constants of k_wdp.hip, read from its #define lines,
the processing order restated, and the batches of tests/test_gpu_window_depth.py, each with its window size and contig lengths.  A
batch is built once and never changed.

k_wdp walks a read of at most WD_T operations by a thread and a longer one by a wave, 64 operations a pass; thread t of a step of WD_STEP
reads takes read t of the step in the PROCESSING ORDER: stream order for a batch of one read group, otherwise the reads grouped by read
group (stable).  Neighbouring lanes of a wave that add to one word (read group, plane, window) are combined.

As in tests/sac_steps.py, no batch puts a read on a main chromosome, sets the proper-pair flag or loads a contig."""
import os
import re

import numpy as np

from tests.sac_steps import D, EQ, FIRST, H, I, LAST, M, N_, OPMAX, P, P_, REV, S, X, cols_flat, cols_of, genome_len, mixed_cigar, query_len  # noqa: F401

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bamqc_amd", "csrc", "k_wdp.hip")


def define(name):
    m = re.search(r"^#define %s\s+(\d+)\b" % name, open(HIP).read(), re.M)
    assert m, name
    return int(m.group(1))


WD_T = define("WD_T")
WD_STEP = define("WD_THREADS")
WD_ETA_LANES = define("WD_ETA_LANES")
PASS = 64
WAVE = 64
NO_QUAL = 0x8000
LEN_MAX = (1 << 31) - 1


def processing_order(cols, n_lanes):
    """The order in which the kernel's threads take the reads (bqc_pipeline.cpp: host_pass)."""
    lane = cols["lane"].astype(np.int64)
    if len(np.unique(lane)) <= 1:
        return np.arange(len(lane))
    return np.argsort(np.where(lane < n_lanes, lane + 1, 0), kind="stable")


def keys_in_order(cols, W, ref_len, n_lanes, MQ):
    """Per read of the processing order, the word its first covered base goes to as (lane, plane, global window), for reads of one
    operation that lie on their contig: what neighbouring lanes are compared by."""
    o = processing_order(cols, n_lanes)
    woff = np.concatenate([[0], np.cumsum((np.asarray(ref_len, np.int64) + W - 1) // W)])
    return np.stack([cols["lane"][o].astype(np.int64), (cols["mapq"][o].astype(np.int64) < MQ).astype(np.int64), woff[cols["rid"][o]] + cols["pos"][o].astype(np.int64) // W], axis=1)


def run_lengths(keys):
    """The lengths of the runs of equal rows."""
    change = np.flatnonzero((keys[1:] != keys[:-1]).any(axis=1)) + 1
    return np.diff(np.concatenate([[0], change, [len(keys)]]))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the rule: three read groups, three contigs (the second of length 0)
# ---------------------------------------------------------------------------------------------------------------------------
RULE_W = 100
RULE_LENS = [1000, 0, 250]


def rule_batch(MQ=20):
    reads = []
    for lane in range(3):
        b = dict(flag=P | (FIRST if lane != 1 else LAST) | (REV if lane == 2 else 0), lane=lane, mapq=max(MQ, 1))

        def add(cigar, pos, b=b, **kw):
            reads.append(dict(b, cigar=cigar, pos=pos, **kw))

        add([(10, M)], 105)                                     # inside a window
        add([(50, M)], 180)                                     # over a border: 20 + 30
        add([(250, M)], 90)                                     # over four windows
        add([(5, M), (10, D), (5, M)], 195)                     # the border under the deletion
        add([(5, M), (10, N_), (5, M)], 195)                    # the same under a skip
        add([(5, M), (3, I), (5, M)], 297)                      # an insertion moves nothing on the genome
        add([(6, S), (4, M)], 398)                              # the soft clip lies in front of pos
        add([(3, H), (2, P_), (6, M), (2, P_), (4, M), (5, H)], 495)  # H and P move nothing
        add([(4, EQ), (2, X), (4, EQ)], 598)                    # = and X runs over a border
        add([(6, M)] + [(4, op) for op in range(9, 16)] + [(4, M)], 695)  # codes 9 ... 15 do nothing
        add([(30, M)], 190, L=6)                                # l_seq shorter than the CIGAR: 6 bases covered
        add([(4, M), (4, I), (30, M)], 196, L=10)               # the cut inside the second run: 2 bases of it
        add([(4, M), (8, S), (30, M)], 196, L=10)               # j passes l_seq under the clip: the second run covers nothing
        add([(12, M)], 0)                                       # pos at 0
        add([(3, M)], 0, flag=b["flag"] | NO_QUAL)              # no qualities stored: counts
        add([(10, M)], 105, mapq=max(MQ, 1) - 1)                # below MQ (MQ = 0: mapq 0, which is good): low and good in one window
        add([(10, M)], 105, mapq=MQ)
        add([(10, M)], 105, mapq=0)
        add([(10, M)], 105, mapq=255)
        for extra in (0x4, 0x100, 0x200, 0x400, 0x800):         # each excluded flag bit alone
            add([(10, M)], 105, flag=b["flag"] | extra)
        add([(10, M)], 105, flag=b["flag"] | 0x20 | 0x8)        # the mate's flags are not looked at
        add([(10, M)], 105, rid=-1)
        add([(10, M)], 105, rid=3)                              # no contig of that number
        add([(10, M)], 990)                                     # ends on the contig's last base
        add([(10, M)], 991)                                     # one base past the end: X
        add([(20, M)], 240, rid=2)                              # the short last window and 10 bases past it
        add([(20, M)], 250, rid=2)                              # pos on no base of the contig: examined, no `reads` word, all X
        add([(20, M)], 5, rid=1)                                # the contig of length 0: all X
        add([(10, M)], -4)                                      # starts in front of the contig: 4 bases X, no `reads` word
        add([(5, D), (10, M)], 95)                              # a leading deletion: pos in window 0, the bases in window 1
    return cols_of(reads, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. window borders
# ---------------------------------------------------------------------------------------------------------------------------
BORDER_WS = [100, 1000, 1024, 999_983, 1 << 24]
EXACT_M_MAX = 1024   # an M of exactly k W bases needs a read of k W bases: built for W up to here (3 W <= 3072 bases)


def border_lens(W):
    """Contigs of length 1, W - 1, W, W + 1, 3 W and 2 W + 37 (a short last window)."""
    return [1, W - 1, W, W + 1, 3 * W, 2 * W + 37]


def border_batch(W):
    lens = border_lens(W)
    reads = []
    for rid, ln in enumerate(lens):
        for b in sorted({0, W, 2 * W, ln}):
            for p in range(b - 4, b + 2):  # runs of 3 bases that end at b - 1, b, b + 1 and begin at b - 1, b, b + 1
                if -3 <= p < ln + 2:
                    reads.append(dict(cigar=[(3, M)], pos=p, rid=rid, lane=rid % 2, mapq=60 if p % 2 else 3))
        if ln > 2 * W:  # the same runs reached through a deletion from the contig's first bases
            for p in (W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1):
                reads.append(dict(cigar=[(2, M), (p - 2, D), (3, M), (1, I), (2, M)], pos=0, rid=rid))
                reads.append(dict(cigar=[(2, M), (p - 4, N_), (3, M)], pos=0, rid=rid, lane=1))
    if W <= EXACT_M_MAX:
        for k in (1, 2, 3):
            for p in (0, W, W - 1, 1):
                reads.append(dict(cigar=[(k * W, M)], pos=p, rid=4))            # exactly k windows' bases, on the borders and off them
            reads.append(dict(cigar=[(k * W, M)], pos=0, rid=5, lane=1, mapq=0))  # into the short last window from k = 3 on
            reads.append(dict(cigar=[(k * W, EQ)], pos=W, rid=2, lane=1))         # the whole run off a contig of W bases from its end on
    return cols_of(reads, 2), lens


# ---------------------------------------------------------------------------------------------------------------------------
# 3. coordinates
# ---------------------------------------------------------------------------------------------------------------------------
COORD_WS = [1 << 20, 999_983]
COORD_LENS = [LEN_MAX, 5000]


def coord_batch(W):
    reads = [dict(cigar=[(1, M)], pos=LEN_MAX - 1),                                     # the contig's last base
             dict(cigar=[(10, M)], pos=LEN_MAX - 10),                                   # ends on it
             dict(cigar=[(10, M)], pos=LEN_MAX - 6, lane=1),                            # runs past 2^31 - 1
             dict(cigar=[(10, M), (OPMAX, D), (10, M)], pos=LEN_MAX - OPMAX - 25),      # a deletion of 2^28 - 1 in front of a match
             dict(cigar=[(10, M), (OPMAX, N_), (10, M)], pos=LEN_MAX - 15, lane=1),     # g passes 2^31: nothing wraps, the second run is X
             dict(cigar=[(4, M), (OPMAX, D), (OPMAX, D), (4, M)], pos=100, rid=1)]      # far off a short contig
    last = (LEN_MAX - 1) // W
    for k in (last - 1, last):
        for p in (k * W - 1, k * W, k * W + 1):
            reads.append(dict(cigar=[(3, M)], pos=p, mapq=0 if p & 1 else 60))
            reads.append(dict(cigar=[(2, M), (1, D), (2, EQ)], pos=p - 3, lane=1))
    far = last * W - 1 - 3                                                                # from the first window to the last border: deletions
    reads.append(dict(cigar=[(3, M)] + [(OPMAX, D)] * (far // OPMAX) + [(far % OPMAX, N_), (3, M)], pos=0))  # of 2^28 - 1 each (the wave path)
    return cols_of(reads, 3)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. many windows under one operation; CIGAR lengths on both paths
# ---------------------------------------------------------------------------------------------------------------------------
PATH_W = 100
PATH_NCIGARS = [1, WD_T, WD_T + 1, PASS, PASS + 1, 2 * PASS + 1, 1000]


def wide_cigar(nc, salt=0):
    """nc operations: matches of 30 ... 170 bases (longer than a window now and then) with short other operations between them."""
    kinds = (I, D, M, N_, EQ, S, X, D)
    return [(30 + 35 * ((k + salt) % 5), M) if k % 2 == 0 else (1 + (k + salt) % 4, kinds[(k // 2 + salt) % len(kinds)]) for k in range(nc)]


def path_batch():
    """One M of 10 kb down the thread path and, behind a pad of empty operations, down the wave path; per operation count a read of
    short and a read of wide operations and one three bases shorter than its CIGAR.  Contig 0 holds every read whole; contig 1 ends
    inside the longest of them, so both paths clip."""
    pad = [(0, M), (5, P_)] * (WD_T // 2 + 1)
    reads = [dict(cigar=[(10_000, M)], pos=950), dict(cigar=pad + [(10_000, M)], pos=950, mapq=0),
             dict(cigar=[(10_000, M)], pos=950, rid=1), dict(cigar=pad + [(10_000, M)], pos=950, rid=1)]
    for nc in PATH_NCIGARS:
        one = nc == 1
        reads.append(dict(cigar=[(33, M)] if one else mixed_cigar(nc, 0), pos=1000))
        wide = wide_cigar if nc <= 2 * PASS + 1 else mixed_cigar  # (1000 wide operations would be a read of 50 kb)
        reads.append(dict(cigar=[(133, EQ)] if one else wide(nc, 1), pos=1000, flag=P | LAST | REV))
        c = [(33, X)] if one else wide(nc, 2)
        reads.append(dict(cigar=c, pos=1003, L=query_len(c) - 3, rid=1, mapq=7 * (nc % 5)))
    span = max(genome_len(r["cigar"]) for r in reads)
    return reads, [1000 + span + 150, 6000]


# ---------------------------------------------------------------------------------------------------------------------------
# 5. combining
# ---------------------------------------------------------------------------------------------------------------------------
HOT_W, HOT_LENS = 1000, [5000]


def hot_batch(n=20_000):
    """n identical reads of 60 bases inside one window, alternating between two read groups in the stream."""
    L = np.full(n, 60)
    return cols_flat(L, np.full(n, P | FIRST), np.ones(n), np.full(n, 60 << 4), np.full(n, 1480), lane=np.arange(n) % 2)


RUNS = [1, 2, 63, 64, 65, 1, 1, 63, 2, 64, 65, 3]  # the lengths of the runs of reads in one window, in stream order
RUN_W, RUN_LENS = 1000, [20_000]


def runs_batch():
    """One read group, reads of 50 bases: RUNS[i] reads in window i + 1, one run behind the other, so that the runs begin and end at
    every place of a wave and cross the waves' borders."""
    pos = np.concatenate([np.full(n, 1000 * (i + 1) + 10 * i) for i, n in enumerate(RUNS)])
    n = len(pos)
    return cols_flat(np.full(n, 50), np.full(n, P | FIRST), np.ones(n), np.full(n, 50 << 4), pos)


def alternating_batch(what, n=200):
    """n reads of 50 bases in ONE window that alternate in read group (what == "group": lanes 0 and 1, grouped by the processing order,
    100 each, so that the seam lies inside the second wave) or in class (what == "class": mapq 0 and 60 in one read group, side by
    side in every wave)."""
    lane = np.arange(n) % 2 if what == "group" else np.zeros(n, np.int64)
    mapq = np.full(n, 60) if what == "group" else np.where(np.arange(n) % 2, 60, 0)
    return cols_flat(np.full(n, 50), np.full(n, P | FIRST), np.ones(n), np.full(n, 50 << 4), np.full(n, 1200), lane=lane, mapq=mapq)


GROUP_W, GROUP_LENS = 100, [8000, 3500]


def groups_batch(seed=44, n=2600, n_lanes=4):
    """Read groups alternating and in runs, two contigs, positions that run forward (a sorted file), CIGARs of 1 to 19 operations, some
    reads shorter than their CIGAR, one read in ten not examined, mapq of every kind, the last reads over the contigs' ends."""
    rng = np.random.default_rng(seed)
    lane = [i % n_lanes for i in range(80)]
    while len(lane) < n:
        lane += [(lane[-1] + 1) % n_lanes] * int(rng.choice([1, 2, 150]))
    lane = lane[:n]
    reads = []
    for k, g in enumerate(lane):
        cig = [(int(rng.integers(1, 160)), M)]
        for _ in range(int(rng.choice([0, 0, 0, 1, 1, 2, 4, 9]))):
            cig += [(int(rng.integers(1, 40)), int(rng.choice([I, D, D, N_, S]))), (int(rng.integers(1, 60)), M)]
        kind = rng.random()
        f = P | (REV if rng.random() < 0.5 else 0) | (FIRST if rng.random() < 0.5 else LAST)
        f |= 0x100 if kind < 0.02 else 0x800 if kind < 0.04 else 0x4 if kind < 0.06 else 0x400 if kind < 0.08 else 0x200 if kind < 0.1 else 0
        ql = query_len(cig)
        rid = int(k % 5 == 0)
        reads.append(dict(cigar=cig, L=ql - (int(rng.integers(1, 10)) if rng.random() < 0.1 and ql > 12 else 0), flag=f, lane=g, rid=rid,
                          pos=k * 3 if rid == 0 else int(k * 1.4), mapq=int(rng.choice([0, 19, 20, 60, 255]))))
    return cols_of(reads, seed)
