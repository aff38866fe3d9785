"""Test infrastructure for the indel-by-cycle kernel (no GPU use): the constants and the launch arithmetic of k_ibc.hip restated — the
thread path's limit, the step, the tile's cycles, grid and shares — the builders of column dicts from reads given by their CIGARs, and
the shapes of tests/test_gpu_indel_by_cycle.py.  tests/test_indel_by_cycle_cpu.py holds the constants against the kernel's #define
lines.

k_ibc uses about one workgroup per CU; a workgroup walks its share ceil(n_reads / grid) of the processing order in steps of IB_STEP
reads, so a batch has a second step only when n_reads > IB_STEP * n_cu.  A read of at most IB_T operations is walked by its own
thread, a longer one by a wave, 64 operations a pass."""
import numpy as np

from tests.cycle_steps import ceil_div, seams, shares, steps

IB_T = 8             # operations up to which a thread walks the read
IB_STEP = 1024       # reads of a k_ibc step (IB_THREADS)
IB_C = 1024          # cycles of the LDS tile
PASS = 64            # operations of a wave's pass
WG_READS = 256       # a launch has no more workgroups than ceil(reads / 256)
K = 64               # length bins
OPMAX = (1 << 28) - 1
M, I, D, N_, S, H, P_, EQ, X = 0, 1, 2, 3, 4, 5, 6, 7, 8
P, REV, FIRST, LAST, MAIN = 0x1, 0x10, 0x40, 0x80, 0x1000
QUERY_OPS = (0, 1, 4, 7, 8)


def ibc_launch(n_reads, n_cu):
    """bqc_launch_ibc: dict(grid, per, shares, steps: the step count of every workgroup)."""
    grid = max(1, min(n_cu, ceil_div(n_reads, WG_READS)))
    per, sh = shares(n_reads, grid)
    return dict(grid=grid, per=per, shares=sh, steps=[len(steps(b, e, IB_STEP)) for b, e in sh])


def query_len(cigar):
    return sum(n for n, op in cigar if op in QUERY_OPS)


def cols_flat(L, flag, ncig, words, lane=None, rid=None):
    """Column dict of reads given by arrays: lengths, flags, operations per read and the CIGAR words back to back.  Every base is A,
    Phred 30, mapq 0 and no proper-pair flag (no read is triplet-eligible), no NM tag; positions non-decreasing, eight reads a
    position, on contig `rid` (0)."""
    L = np.asarray(L, np.int64)
    n = len(L)
    return dict(flag=np.asarray(flag, np.uint16), mapq=np.zeros(n, np.uint8), lane=np.zeros(n, np.uint8) if lane is None else np.asarray(lane, np.uint8),
                rid=np.zeros(n, np.int32) if rid is None else np.asarray(rid, np.int32), pos=(np.arange(n) // 8).astype(np.int32),
                tlen=np.zeros(n, np.int32), nm=np.full(n, -1, np.int32), as_=np.full(n, 100, np.int32), l_seq=L.astype(np.uint32),
                n_cigar=np.asarray(ncig, np.uint16), seq=np.full(int(((L + 1) // 2).sum()), 0x11, np.uint8),
                qual=np.full(int(L.sum()), 30, np.uint8), cigar=np.asarray(words, np.uint32))


def cols_of(reads):
    """cols_flat for reads given as dicts: cigar [(length, op), ...] and optionally L (default: the CIGAR's query length), flag
    (default: paired, first mate, mate on a main chromosome), lane (0), rid (0)."""
    words = [(n << 4) | op for r in reads for n, op in r["cigar"]]
    return cols_flat([r.get("L", query_len(r["cigar"])) for r in reads], [r.get("flag", P | FIRST | MAIN) for r in reads],
                     [len(r["cigar"]) for r in reads], words, [r.get("lane", 0) for r in reads], [r.get("rid", 0) for r in reads])


def ref_len_for(cols):
    """A contig length under which every read of cols_flat starts inside the contig."""
    return len(cols["flag"]) // 8 + 64


def seam_cigar(nc, salt=0):
    """A CIGAR of nc operations with an event in the first and the last operation, in the first and the last operation of every pass
    of 64 and so on both sides of every pass seam (where nc reaches that far): insertions and deletions in turn, lengths 1..5,
    between match operations of 1..3 bases.  An insertion in operation 0 lies at j = 0; a deletion there, or in the last operation,
    has no base on one side and is no event."""
    at = {k for k in (0, 1, nc - 2, nc - 1) if 0 <= k < nc}
    for seam in range(PASS, nc + 1, PASS):
        at |= {k for k in (seam - 2, seam - 1, seam, seam + 1) if 0 <= k < nc}
    out, seen = [], 0
    for k in range(nc):
        if k in at:
            out.append((1 + (k + salt) % 5, I if (seen + salt) % 2 == 0 else D))
            seen += 1
        else:
            out.append((1 + (k + salt) % 3, M))
    return out


PATH_NCIGARS = [IB_T - 1, IB_T, IB_T + 1, 63, 64, 65, 127, 128, 129, 1000, 65_535]


def path_reads():
    """Test 2's reads: per operation count of PATH_NCIGARS a forward first mate, a reverse second mate, and a forward read three
    bases shorter than its CIGAR (its last events run past L).  On contig 1, not main: the longest ones hold more inserted and
    deleted bases than hist_cap allows on a main chromosome."""
    reads = []
    for nc in PATH_NCIGARS:
        reads.append(dict(cigar=seam_cigar(nc, 0), flag=P | FIRST | MAIN, rid=1))
        reads.append(dict(cigar=seam_cigar(nc, 1), flag=P | LAST | MAIN | REV, rid=1))
        c = seam_cigar(nc, 2)
        reads.append(dict(cigar=c, flag=P | FIRST | MAIN, L=query_len(c) - 3, rid=1))
    return reads


def step_layout(n_cu):
    """The size and the read-group column of the step batch for a card of n_cu CUs: more than 2 * IB_STEP * n_cu reads, or as many
    more as it takes until the LAST workgroup makes three steps as well.  Read groups 0..3, non-decreasing (stream order is processing
    order); the changes lie exactly on a step seam of a workgroup near n_cu // 3, in the middle of a step, and in the middle of
    another workgroup's first step."""
    n = 2 * IB_STEP * n_cu + 977
    while min(ibc_launch(n, n_cu)["steps"]) < 3:
        n += 1
    la = ibc_launch(n, n_cu)
    sm = seams(n, la["grid"], IB_STEP)
    c1 = (n_cu // 3) * la["per"] + IB_STEP
    c2 = (2 * n_cu // 3) * la["per"] + IB_STEP + 333
    c3 = (5 * n_cu // 6) * la["per"] + 500
    lane = np.zeros(n, np.uint8)
    for c in (c1, c2, c3):
        lane[c:] += 1
    return dict(n=n, n_cu=n_cu, lane=lane, changes=(c1, c2, c3), launch=la, seams=sm)


def assert_step_layout(lay):
    la, (c1, c2, c3) = lay["launch"], lay["changes"]
    assert lay["n"] > 2 * IB_STEP * lay["n_cu"] and la["grid"] == lay["n_cu"] == len(la["steps"])
    assert min(la["steps"]) >= 3, la
    starts = {b for b, e in la["shares"]}
    assert 0 < c1 < c2 < c3 < lay["n"]
    assert c1 in lay["seams"] and c1 not in starts
    for c in (c2, c3):
        assert c not in lay["seams"] and c not in starts and min(abs(c - s) for s in list(lay["seams"]) + list(starts)) >= 100


def step_batch(lay, seed=31):
    """The step batch's columns: reads of 20 bases, both strands and mates; one in four aM bI cM, one in four aM bD cM, one in 64 a
    CIGAR of 12 operations (the wave path inside full steps), the rest 20M."""
    n = lay["n"]
    rng = np.random.default_rng(seed)
    flag = (P | MAIN | np.where(rng.random(n) < 0.5, REV, 0) | np.where(rng.random(n) < 0.5, FIRST, LAST)).astype(np.uint16)
    kind = np.arange(n) % 4  # 0 insertion, 1 deletion, 2 and 3 plain
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
    # 12 operations: 2M 1I 1M 1D 2M 2I 3M 70D 1M 1I 6M 1S = 20 bases
    twelve = np.array([(2 << 4), (1 << 4) | I, (1 << 4), (1 << 4) | D, (2 << 4), (2 << 4) | I, (3 << 4), (70 << 4) | D, (1 << 4), (1 << 4) | I, (6 << 4), (1 << 4) | S], np.int64)
    for k in range(12):
        w[at[longc] + k] = twelve[k]
    return cols_flat(np.full(n, 20), flag, ncig, w, lay["lane"])


# ---------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_indel_by_cycle.py (tests/test_indel_by_cycle_cpu.py runs both restatements over each of them)
# ---------------------------------------------------------------------------------------------------------------------------
def rule_reads():
    """Test 1's reads, three read groups: every branch of the rule on both strands and mates.  Reads whose indels are 60 bases or
    longer lie on contig 1, which the tests declare not main (the per-read kernels refuse inserted or deleted bases at or above
    hist_cap on a main chromosome)."""
    shapes = [
        [(3, I), (17, M)],                                  # an insertion at j = 0
        [(17, M), (3, I)],                                  # one ending exactly at L
        [(10, M), (2, D), (10, M)],                         # a deletion between two bases
        [(2, D), (20, M)],                                  # a deletion at j = 0: no base in front
        [(20, M), (2, D)],                                  # one at j = L: none behind
        [(5, S), (4, EQ), (1, I), (3, X), (1, D), (7, M)],  # S, = and X advance as M does
        [(4, H), (6, M), (9, N_), (2, P_), (3, I), (11, M), (7, H)],   # N, H and P do nothing: the insertion lies at j = 6
        [(6, M)] + [(4, op) for op in range(9, 16)] + [(1, D), (6, M)],  # codes 9 ... 15 do nothing
        [(5, M), (0, I), (0, D), (0, M), (1, I), (0, S), (6, M), (0, D)],  # zero-length operations are no events
        [(1, M), (1, I), (1, D), (1, I), (1, D), (1, M)],   # events side by side
        [(1, D), (1, I), (1, D), (4, M), (1, D), (1, I), (1, D)],
    ]
    long_shapes = [[(4, M), (n, I), (5, M), (n, D), (3, M)] for n in (63, 64, 65)] + [[(4, M), (OPMAX, D), (5, M), (64, D), (2, M)],
                                                                                     [(9, M), (OPMAX, N_), (2, I), (1000, D), (9, M)]]
    # events at cycles 15 / 16, 299 / 300 and 1023 / 1024, on either strand: reads of 1100 bases
    for c in (15, 16, 299, 300, 1023, 1024):
        shapes.append([(c, M), (1, I), (1100 - c - 1, M)])           # forward: insertion at cycle c; reverse: at 1100 - c - 1
        shapes.append([(c + 1, M), (2, D), (1100 - c - 1, M)])       # forward: deletion at cycle c
        shapes.append([(1100 - c - 2, M), (2, I), (c, M)])           # reverse: insertion at cycle c
        shapes.append([(1100 - 1 - c, M), (1, D), (c + 1, M)])       # reverse: deletion at cycle c
    reads = []
    for k, cig in enumerate(shapes + long_shapes):
        for rev in (0, REV):
            for mate in (FIRST, LAST):
                reads.append(dict(cigar=cig, flag=P | MAIN | rev | mate, lane=(k + (rev >> 4)) % 3, rid=1 if k >= len(shapes) else 0))
    # the read shorter and longer than its CIGAR's query length
    run_past = [(10, M), (5, I), (3, M), (1, D), (4, M)]
    for L in (12, 14, 15, 17, 18, 19, 22, 30):  # 12, 14: the insertion runs past L; 15: it ends at L; 18: the deletion lies at j = L
        for rev in (0, REV):
            reads.append(dict(cigar=run_past, L=L, flag=P | MAIN | rev | LAST, lane=L % 3))
    # reads that are not examined
    cig = [(5, M), (1, I), (2, M), (1, D), (5, M)]
    for extra in (0x100, 0x800, 0x4, 0x900, 0x104):
        reads.append(dict(cigar=cig, flag=P | MAIN | FIRST | extra, lane=1))
    reads.append(dict(cigar=cig, flag=P | MAIN | 0x100, lane=2))          # secondary without a mate flag
    reads.append(dict(cigar=[], L=13, flag=P | MAIN | FIRST, lane=0))     # n_cigar = 0
    reads.append(dict(cigar=cig, L=0, flag=P | MAIN | LAST, lane=0))      # l_seq = 0
    # examined whatever these say: duplicate, QC fail, mapq 0, no contig
    for extra in (0x400, 0x200, 0x20):
        reads.append(dict(cigar=cig, flag=P | MAIN | LAST | extra, lane=2))
    reads.append(dict(cigar=cig, flag=P | MAIN | FIRST, lane=1, rid=-1))
    order = np.random.default_rng(5).permutation(len(reads))
    return [reads[i] for i in order]


def wrap_reads():
    """Test 3's reads (contig 1, not main; 100 bases each): query-consuming lengths that add up past 2^32 inside one pass of 64
    operations, and through the carry of the pass before.  16 operations of 2^28 - 1 bases and one of 16 + 26 make 2^32 + 26: the
    events behind them would lie at stored index 26 and 27 of 100 were the sum taken in 32 bits."""
    before = [(3, M), (2, I), (4, M), (1, D), (1, M)]                     # events at j = 3 and j = 9
    after = [(1, I), (1, D), (1, M)]
    big = [(OPMAX, S if k % 2 else M) for k in range(16)] + [(16 + 26 - 10, M)]
    inside = before + big + after                                         # 25 operations: one pass
    fill = [(0, M), (7, P_), (0, I), (3, N_)] * 13                        # 52 operations that add nothing
    carry = before + big[:9] + fill + big[9:] + after                     # 77 operations: nine of the big ones in pass 0, the rest in pass 1
    assert len(inside) > IB_T and len(inside) <= PASS < len(carry) and query_len(inside) - 2 == (1 << 32) + 26
    reads = []
    for cig in (inside, carry):
        for rev in (0, REV):
            reads.append(dict(cigar=cig, L=100, flag=P | MAIN | FIRST | rev, rid=1))
    return reads


def tile_reads(N):
    """Test 4's reads: lengths IB_C and IB_C + 1 and long reads, with events at the cycles IB_C - 1 and IB_C and at N - 1 and N, on
    either strand, down the thread path and (padded with empty operations) down the wave path."""
    reads = []
    for L in (IB_C, IB_C + 1, 2000, N + 60):
        for c in (IB_C - 2, IB_C - 1, IB_C, N - 1, N):
            for rev in (0, REV):
                for pad in ([], [(0, M), (5, P_)] * 6):
                    if c + 1 <= L:  # (the inserted base is the read's last at c = L - 1)
                        j = L - c - 1 if rev else c
                        reads.append(dict(cigar=pad + [(j, M), (1, I), (L - j - 1, M)], flag=P | MAIN | FIRST | rev))
                    if c + 2 <= L:  # (a base behind the gap)
                        jd = L - 1 - c if rev else c + 1
                        reads.append(dict(cigar=pad + [(jd, M), (3, D), (L - jd, M)], flag=P | MAIN | LAST | rev))
    return reads


def hot_cols(n=70_000):
    """Test 5: n identical reads, 40M 1I 19M 1D 40M."""
    words = np.tile(np.array([(40 << 4), (1 << 4) | I, (19 << 4), (1 << 4) | D, (40 << 4)], np.int64), n)
    return cols_flat(np.full(n, 100), np.full(n, P | MAIN | FIRST), np.full(n, 5), words)


def group_reads(seed=14):
    """Test 6 and 7's reads: four read groups, alternating read by read and then in runs of 1, 2 and 700 reads; one read in ten is not
    examined; CIGARs of 1 to 20 operations with insertions and deletions of 1 to 3 bases, some reads shorter than their CIGAR."""
    rng = np.random.default_rng(seed)
    lane = [i % 4 for i in range(80)]
    for g, run in ((0, 1), (1, 2), (2, 700), (3, 2), (1, 700), (2, 1), (0, 700), (3, 1), (3, 300)):
        lane += [g] * run
    reads = []
    for g in lane:
        nev = int(rng.choice([0, 0, 1, 1, 2, 4, 9]))
        cig = [(int(rng.integers(1, 30)), M)]
        for _ in range(nev):
            cig += [(int(rng.integers(1, 4)), I if rng.random() < 0.5 else D), (int(rng.integers(1, 30)), M)]
        kind = rng.random()
        f = P | MAIN | (REV if rng.random() < 0.5 else 0) | (FIRST if rng.random() < 0.5 else LAST)
        f |= 0x100 if kind < 0.04 else 0x800 if kind < 0.08 else 0x4 if kind < 0.1 else 0x400 if kind < 0.15 else 0
        L = query_len(cig) - (int(rng.integers(1, 10)) if rng.random() < 0.1 and query_len(cig) > 12 else 0)
        reads.append(dict(cigar=cig, L=L, flag=f, lane=g))
    return reads


def cross_reads(seed=18):
    """Test 8's reads, on a main chromosome: every indel operation is an event (bases on both sides, L the CIGAR's query length) of
    fewer than 64 bases; two read groups."""
    rng = np.random.default_rng(seed)
    reads = []
    for i in range(3000):
        cig = [(int(rng.integers(1, 40)), M)]
        for _ in range(int(rng.choice([0, 1, 1, 2, 3, 12]))):
            cig += [(int(rng.choice([1, 1, 1, 2, 5, 63])), I if rng.random() < 0.5 else D), (int(rng.integers(1, 40)), M)]
        reads.append(dict(cigar=cig, flag=P | MAIN | (REV if rng.random() < 0.5 else 0) | (FIRST if rng.random() < 0.5 else LAST), lane=i % 2))
    return reads
