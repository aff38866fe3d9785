"""Test infrastructure for the allele counts at given sites (no GPU use): the constants and the launch arithmetic of k_sac.hip restated
(tests/test_site_alleles_cpu.py holds the constants against the kernel's #define lines), the builders of column dicts, and the batches
of tests/test_gpu_site_alleles.py, each with its sites.  A batch is built once and never changed.

k_sac uses about one workgroup per CU; a workgroup walks its share ceil(n_reads / grid) of the processing order in steps of SA_STEP
reads.  A read that may touch a site and has at most SA_T operations is walked by a thread, a longer one by a wave, 64 operations a
pass.  The first site of a read comes from an index of buckets of BUCKET bases per contig.

No batch puts a read on a main chromosome, sets the proper-pair flag or loads a contig: the per-read kernels then have nothing to
refuse in CIGARs with huge deletions, and the genome is not read."""
import numpy as np

from tests.cycle_steps import ceil_div, seams, shares, steps

SA_T = 8
SA_STEP = 1024
PASS = 64
WG_READS = 256
BUCKET = 4096
POS_MAX = (1 << 31) - 2
OPMAX = (1 << 28) - 1
M, I, D, N_, S, H, P_, EQ, X = 0, 1, 2, 3, 4, 5, 6, 7, 8
P, REV, FIRST, LAST = 0x1, 0x10, 0x40, 0x80
QUERY_OPS = (0, 1, 4, 7, 8)
GENOME_OPS = (0, 2, 3, 7, 8)
QUALS = np.array([0, 2, 19, 20, 21, 37, 63, 93, 222], np.uint8)
NIBS = np.array([1, 2, 4, 8], np.uint8)


def sac_launch(n_reads, n_cu):
    """bqc_launch_sac: dict(grid, per, shares, steps: the step count of every workgroup)."""
    grid = max(1, min(n_cu, ceil_div(n_reads, WG_READS)))
    per, sh = shares(n_reads, grid)
    return dict(grid=grid, per=per, shares=sh, steps=[len(steps(b, e, SA_STEP)) for b, e in sh])


def query_len(cigar):
    return sum(n for n, op in cigar if op in QUERY_OPS)


def genome_len(cigar):
    return sum(n for n, op in cigar if op in GENOME_OPS)


def pack(nib):
    """4-bit codes of one read -> its packed bytes (the first base in the high nibble)."""
    nib = np.asarray(nib, np.uint8)
    if len(nib) & 1:
        nib = np.concatenate([nib, np.zeros(1, np.uint8)])
    return (nib[0::2] << 4) | nib[1::2]


def cols_flat(L, flag, ncig, words, pos, rid=None, lane=None, mapq=None, seed=0, nib=None, qual=None):
    """Column dict of reads given by arrays; the bases are drawn from A, C, G, T and the qualities from QUALS unless given (nib: the
    4-bit codes of all reads back to back, every read of even length then; qual: all qualities back to back)."""
    rng = np.random.default_rng(seed)
    L = np.asarray(L, np.int64)
    n = len(L)
    total = int(L.sum())
    if nib is None:
        seq = (NIBS[rng.integers(0, 4, int(((L + 1) // 2).sum()))] << 4) | NIBS[rng.integers(0, 4, int(((L + 1) // 2).sum()))]
    else:
        assert not (L & 1).any()
        seq = pack(nib)
    return dict(flag=np.asarray(flag, np.uint16), mapq=np.full(n, 60, np.uint8) if mapq is None else np.asarray(mapq, np.uint8),
                lane=np.zeros(n, np.uint8) if lane is None else np.asarray(lane, np.uint8),
                rid=np.zeros(n, np.int32) if rid is None else np.asarray(rid, np.int32), pos=np.asarray(pos, np.int64).astype(np.int32),
                tlen=np.zeros(n, np.int32), nm=np.full(n, -1, np.int32), as_=np.full(n, 100, np.int32), l_seq=L.astype(np.uint32),
                n_cigar=np.asarray(ncig, np.uint16), seq=seq.astype(np.uint8),
                qual=QUALS[rng.integers(0, len(QUALS), total)] if qual is None else np.asarray(qual, np.uint8), cigar=np.asarray(words, np.uint32))


def cols_of(reads, seed=0):
    """cols_flat for reads given as dicts: cigar [(length, op), ...], pos and optionally L (default: the CIGAR's query length), flag
    (default: paired, first mate, forward), lane (0), rid (0), mapq (60), nib / qual (the read's codes / qualities: then of every read)."""
    words = [(n << 4) | op for r in reads for n, op in r["cigar"]]
    L = [r.get("L", query_len(r["cigar"])) for r in reads]
    nib = qual = None
    if reads and "nib" in reads[0]:
        nib = np.concatenate([np.asarray(r["nib"], np.uint8) for r in reads])
    if reads and "qual" in reads[0]:
        qual = np.concatenate([np.asarray(r["qual"], np.uint8) for r in reads])
    return cols_flat(L, [r.get("flag", P | FIRST) for r in reads], [len(r["cigar"]) for r in reads], words, [r["pos"] for r in reads],
                     [r.get("rid", 0) for r in reads], [r.get("lane", 0) for r in reads], [r.get("mapq", 60) for r in reads], seed, nib, qual)


def sites_of(pairs):
    """Sorted, distinct (rid, pos) pairs as the two arrays of the enable call."""
    pairs = sorted(set(pairs))
    return np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)


def buckets(sites, n_refs):
    """The index the library builds: per contig the number of sites of every bucket up to the one of its last site ([]: no site)."""
    out = []
    for r in range(n_refs):
        p = sites[1][sites[0] == r].astype(np.int64)
        out.append(np.bincount(p // BUCKET).tolist() if len(p) else [])
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the rule: three read groups, three contigs of which the middle one has no site
# ---------------------------------------------------------------------------------------------------------------------------
RULE_REFS = 3


def rule_batch(Q=20, MQ=20, refused=False):
    """Hand-made reads around sites of contig 0 at 100 ... 140 and of contig 2, each kind on both strands in three read groups.
    refused: with the reads whose batch the library refuses before any kernel runs (a contig or a read group out of range, a quality
    of 223): they are the restatement's alone."""
    sites = sites_of([(0, p) for p in (100, 109, 110, 115, 120, 121, 125, 130, 140, 141)] + [(2, p) for p in (5, 50, 51, 52, 5000)])
    reads = []
    q40 = lambda n: np.full(n, 40, np.uint8)
    A10 = [1, 2, 4, 8, 1, 2, 4, 8, 1, 2]
    for lane in range(3):
        for rev in (0, REV):
            b = dict(flag=P | (FIRST if lane != 1 else LAST) | rev, lane=lane, mapq=max(MQ, 1))

            def add(cigar, pos, b=b, **kw):
                Lr = kw.get("L", query_len(cigar) + (query_len(cigar) & 1))  # (even: the codes are given, see cols_flat)
                reads.append(dict(dict(b, nib=(A10 * 20)[:Lr], qual=q40(Lr), L=Lr), cigar=cigar, pos=pos, **kw))

            add([(10, M)], 100)                                     # sites on the first (100) and the last (109) base; 110 is one behind
            add([(4, M), (12, D), (6, M)], 105)                     # 109 one behind the run's last base; 109 ... 120 under the deletion; 121 its first base behind it
            add([(4, M), (12, N_), (6, M)], 105)                    # the same under a skip
            add([(5, M), (3, I), (2, M)], 115)                      # 120 and 121 beside the insertion: stored index 5 + 3
            add([(6, S), (4, M)], 120)                              # 115 would lie under the soft clip in front of pos
            add([(3, H), (2, P_), (6, M), (2, P_), (4, M), (5, H)], 120)  # H and P move nothing: 125 at stored index 5, 121 at 1
            add([(4, EQ), (2, X), (4, EQ)], 121)                    # = and X runs
            add([(30, M)], 120, L=6)                                # the CIGAR is longer than the read: 125 at index 5 counts, 130 at 10 does not
            add([(6, M)] + [(4, op) for op in range(9, 16)] + [(4, M)], 120)  # codes 9 ... 15 do nothing
            add([(10, M)], 136, mapq=max(MQ, 1) - 1)                # below MQ (MQ = 0: mapq 0, which counts)
            add([(10, M)], 136, mapq=MQ)
            for extra in (0x4, 0x100, 0x200, 0x400, 0x800):         # each excluded flag bit alone
                add([(10, M)], 100, flag=b["flag"] | extra)
            add([(10, M)], 100, flag=b["flag"] | 0x20 | 0x8)        # the mate's flags are not looked at
            add([(10, M)], 100, rid=1)                              # the contig without sites
            add([(10, M)], 100, rid=-1)
            if refused:
                add([(10, M)], 100, rid=3)
                add([(10, M)], 100, lane=3)
                add([(10, M)], 49, rid=2)                           # 50, 51, 52 at stored index 1, 2, 3: qualities 222, 223, 255 below
            add([(10, M)], 45, rid=2)                               # 50, 51, 52 at stored index 5, 6, 7: codes and qualities below
            add([(10, M)], 47, rid=2)                               # the same sites at index 3, 4, 5
            add([(4, M)], 4996, rid=2)                              # the contig's last site on the read's last base; nothing behind it
            add([(4, M)], 5001, rid=2)                              # behind the last site
    cols = cols_of(reads)
    so = np.cumsum((cols["l_seq"].astype(np.int64) + 1) // 2) - (cols["l_seq"].astype(np.int64) + 1) // 2
    qo = np.cumsum(cols["l_seq"].astype(np.int64)) - cols["l_seq"]
    for r in np.flatnonzero((cols["rid"] == 2) & (cols["pos"] == 45)):  # codes 0 (=), 15 (N) and 3 (M: A or C) on the three sites
        cols["seq"][so[r] + 2] = (cols["seq"][so[r] + 2] & 0xF0) | 0x0        # index 5
        cols["seq"][so[r] + 3] = 0xF3                                         # index 6 and 7
    for r in np.flatnonzero((cols["rid"] == 2) & (cols["pos"] == 47)):  # qualities Q - 1, Q, 222 on the three sites (223: the library refuses)
        cols["qual"][qo[r] + 3:qo[r] + 6] = [max(Q, 1) - 1, Q, 222]
    for r in np.flatnonzero((cols["rid"] == 2) & (cols["pos"] == 49)):
        cols["qual"][qo[r] + 1:qo[r] + 4] = [222, 223, 255]
    return cols, sites


# ---------------------------------------------------------------------------------------------------------------------------
# 2. index edges, 3. a full bucket, 4. behind the last contig with sites, 5. position arithmetic
# ---------------------------------------------------------------------------------------------------------------------------
def index_batch():
    """Sites at 0, 4095, 4096, 4097 and 2^31 - 2; reads of 3 bases whose pos is each of them - 1, + 0 and + 1 (where that is a
    position), a read of 9000 bases over three buckets from 0 and reads that end one in front of a bucket's first site."""
    edge = [0, BUCKET - 1, BUCKET, BUCKET + 1, POS_MAX]
    sites = sites_of([(0, p) for p in edge] + [(0, 3 * BUCKET + 7)])
    reads = []
    for p in edge:
        for d in (-3, -2, -1, 0, 1):
            if 0 <= p + d <= POS_MAX + 1:
                for rev in (0, REV):
                    reads.append(dict(cigar=[(3, M)], pos=p + d, flag=P | FIRST | rev))
                    reads.append(dict(cigar=[(1, S), (2, M), (1, I), (1, M)], pos=p + d, flag=P | LAST | rev))
    reads.append(dict(cigar=[(9000, M)], pos=0))
    reads.append(dict(cigar=[(4000, M), (100, D), (4900, M)], pos=0))
    reads.append(dict(cigar=[(200, M)], pos=2 * BUCKET + 100))   # in an empty bucket, in front of the next bucket's site
    reads.append(dict(cigar=[(200, M)], pos=5 * BUCKET))         # behind the contig's last bucket
    reads.append(dict(cigar=[(10, M)], pos=-4))                  # starts in front of the contig: site 0 at stored index 4
    return cols_of(reads, 2), sites


def region_batch():
    """Every position of bucket 3 of contig 0 is a site (a bucket with 4096 sites); reads of 10 000 bases across it down the thread
    path (1 and 3 operations) and the wave path (20 operations), reads that start inside it, and short reads at its edges."""
    sites = sites_of([(0, p) for p in range(3 * BUCKET, 4 * BUCKET)] + [(0, 40), (0, 6 * BUCKET + 1)])
    reads = [dict(cigar=[(10_000, M)], pos=3 * BUCKET - 3000),
             dict(cigar=[(4000, M), (7, D), (6000, M)], pos=3 * BUCKET - 3000, flag=P | LAST | REV),
             dict(cigar=[(500, M), (1, I), (499, M)] * 6 + [(4000, M), (1, D)], pos=3 * BUCKET - 2000, lane=1)]
    for p in (3 * BUCKET - 2, 3 * BUCKET, 3 * BUCKET + 1, 3 * BUCKET + 2047, 3 * BUCKET + 2048, 4 * BUCKET - 3, 4 * BUCKET - 1, 4 * BUCKET):
        reads.append(dict(cigar=[(5, M)], pos=p, lane=1))
    return cols_of(reads, 3), sites


def far_batch():
    """S = 1: one site on contig 1 of 4; reads on it, on the contigs in front and behind (2 and 3), and far behind the site."""
    sites = sites_of([(1, 77)])
    reads = [dict(cigar=[(20, M)], pos=70, rid=r, flag=P | FIRST | (REV if k & 1 else 0)) for r in range(4) for k in range(5)]
    reads += [dict(cigar=[(20, M)], pos=p, rid=1) for p in (57, 58, 77, 78, 4096, 1 << 30)]
    return cols_of(reads, 4), sites


def arith_batch():
    """pos = 2^31 - 300 with a deletion of 2^28 - 1 in front of a match: g passes 2^31 and nothing wraps; sites up to 2^31 - 2 under
    the first match, down the thread path and (padded with empty operations) down the wave path; and a read that ends on 2^31 - 2."""
    p0 = (1 << 31) - 300
    sites = sites_of([(0, q) for q in (5, 44, p0 - 1, p0, p0 + 9, p0 + 10, p0 + 200, POS_MAX - 1, POS_MAX)])
    pad = [(0, M), (5, P_)] * 6
    reads = []
    for extra in ([], pad):
        reads.append(dict(cigar=extra + [(10, M), (OPMAX, D), (50, M)], pos=p0))
        reads.append(dict(cigar=extra + [(10, M), (OPMAX, N_), (OPMAX, D), (50, M)], pos=p0, flag=P | LAST | REV))
        reads.append(dict(cigar=extra + [(299, M)], pos=p0))               # its last base lies on 2^31 - 2
        reads.append(dict(cigar=extra + [(400, M)], pos=p0))               # runs past 2^31 - 2
        reads.append(dict(cigar=extra + [(3, M), (OPMAX, S), (3, M)], pos=p0 - 1, L=60))  # j passes L: the second run counts nothing
        reads.append(dict(cigar=extra + [(10, M), (OPMAX, D)] * 3 + [(40, M)], pos=0))    # three deletions: g = 3 * 2^28 + 27 at the end
    return cols_of(reads, 5), sites


# ---------------------------------------------------------------------------------------------------------------------------
# 6. CIGAR lengths on both paths
# ---------------------------------------------------------------------------------------------------------------------------
PATH_NCIGARS = [SA_T - 1, SA_T, SA_T + 1, 63, 64, 65, 127, 128, 129, 1000, 65_535]


def mixed_cigar(nc, salt=0):
    """nc operations: matches of 1 ... 3 bases with an insertion, a deletion, a skip or a soft clip between them now and then."""
    kinds = (I, D, M, N_, M, S, M, D)
    return [(1 + (k + salt) % 3, M) if k % 2 == 0 else (1 + (k + salt) % 4, kinds[(k // 2 + salt) % len(kinds)]) for k in range(nc)]


def path_batch():
    """Per operation count of PATH_NCIGARS a forward read, a reverse read and a read three bases shorter than its CIGAR, all from
    pos 1000; a site every 5 bases from 990 on, so that operations of every pass lie on sites."""
    reads = []
    for nc in PATH_NCIGARS:
        reads.append(dict(cigar=mixed_cigar(nc, 0), pos=1000))
        reads.append(dict(cigar=mixed_cigar(nc, 1), pos=1000, flag=P | LAST | REV))
        c = mixed_cigar(nc, 2)
        reads.append(dict(cigar=c, pos=1003, L=query_len(c) - 3))
    span = max(genome_len(r["cigar"]) for r in reads)
    return reads, sites_of([(0, p) for p in range(990, 1000 + span + 20, 5)])


# ---------------------------------------------------------------------------------------------------------------------------
# 7. contention, 8. seams and read groups, 9. order
# ---------------------------------------------------------------------------------------------------------------------------
def hot_batch(n=70_000):
    """n identical reads of 16 bases on one site."""
    L = np.full(n, 16)
    return cols_flat(L, np.full(n, P | FIRST), np.ones(n), np.full(n, 16 << 4), np.full(n, 500), nib=np.tile(np.array([1, 2, 4, 8] * 4, np.uint8), n),
                     qual=np.full(n * 16, 37, np.uint8)), sites_of([(0, 505)])


def step_layout(n_cu):
    """The step batch for a card of n_cu CUs: more than 2 * SA_STEP * n_cu reads, so that every workgroup makes three steps; read
    groups 0 ... 3, non-decreasing, the first change exactly on a step seam, the others inside steps."""
    n = 2 * SA_STEP * n_cu + 977
    while min(sac_launch(n, n_cu)["steps"]) < 3:
        n += 1
    la = sac_launch(n, n_cu)
    sm = seams(n, la["grid"], SA_STEP)
    c1 = (n_cu // 3) * la["per"] + SA_STEP
    c2 = (2 * n_cu // 3) * la["per"] + SA_STEP + 333
    c3 = (5 * n_cu // 6) * la["per"] + 500
    lane = np.zeros(n, np.uint8)
    for c in (c1, c2, c3):
        lane[c:] += 1
    return dict(n=n, n_cu=n_cu, lane=lane, changes=(c1, c2, c3), launch=la, seams=sm)


def step_batch(lay, seed=41):
    """Reads of 20 bases, eight a position: one in four aM bI cM, one in four aM bD cM, one in 64 a CIGAR of 12 operations (the wave
    path inside full steps), the rest 20M; a site every 50 bases, so that about half of the reads touch one."""
    n = lay["n"]
    rng = np.random.default_rng(seed)
    flag = (P | np.where(rng.random(n) < 0.5, REV, 0) | np.where(rng.random(n) < 0.5, FIRST, LAST)).astype(np.uint16)
    kind = np.arange(n) % 4
    longc = np.arange(n) % 64 == 7
    a = rng.integers(1, 15, n)
    b = rng.integers(1, 4, n)
    ncig = np.where(longc, 12, np.where(kind < 2, 3, 1))
    at = np.cumsum(ncig) - ncig
    w = np.zeros(int(ncig.sum()), np.int64)
    plain = ~longc & (kind >= 2)
    w[at[plain]] = 20 << 4
    i3, d3 = ~longc & (kind == 0), ~longc & (kind == 1)
    w[at[i3]] = a[i3] << 4
    w[at[i3] + 1] = (b[i3] << 4) | I
    w[at[i3] + 2] = (20 - a[i3] - b[i3]) << 4
    w[at[d3]] = a[d3] << 4
    w[at[d3] + 1] = (b[d3] << 4) | D
    w[at[d3] + 2] = (20 - a[d3]) << 4
    twelve = np.array([(2 << 4), (1 << 4) | I, (1 << 4), (1 << 4) | D, (2 << 4), (2 << 4) | I, (3 << 4), (70 << 4) | D, (1 << 4), (1 << 4) | I, (6 << 4), (1 << 4) | S], np.int64)
    for k in range(12):
        w[at[longc] + k] = twelve[k]
    pos = np.arange(n) // 8
    cols = cols_flat(np.full(n, 20), flag, ncig, w, pos, lane=lay["lane"], seed=seed)
    return cols, (np.zeros(len(range(3, n // 8 + 120, 50)), np.int32), np.arange(3, n // 8 + 120, 50, dtype=np.int32))


def groups_batch(seed=44):
    """Four read groups, alternating read by read and then in runs of 1, 2 and 700 reads, on two contigs with a site every 23 bases;
    CIGARs of 1 to 19 operations, some reads shorter than their CIGAR, one read in ten not examined, mapq of every kind."""
    rng = np.random.default_rng(seed)
    lane = [i % 4 for i in range(80)]
    for g, run in ((0, 1), (1, 2), (2, 700), (3, 2), (1, 700), (2, 1), (0, 700), (3, 1), (3, 300)):
        lane += [g] * run
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
    return cols_of(reads, seed), sites_of([(r, p) for r in (0, 1) for p in range(2, 3 * len(lane) + 600, 23)])
