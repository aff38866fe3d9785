"""The batches of the duplicate-set tests (tests/test_gpu_duplicate_sets.py; tests/test_duplicate_sets_cpu.py asserts that each of them
crosses the edge it is named for).  Reads are dicts as tests/sac_steps.cols_of takes them, with `tlen` beside; no read lies on a main
chromosome and no contig is loaded: the genome is not read."""
import numpy as np

from tests import dup_ref
from tests.sac_steps import D, EQ, FIRST, H, I, LAST, M, N_, OPMAX, P, REV, S, X, cols_of, mixed_cigar  # noqa: F401

MREV, UNMAPPED, MUNMAPPED, SECONDARY, QCFAIL, DUP, SUPPL = 0x20, 0x4, 0x8, 0x100, 0x200, 0x400, 0x800
DP_T = 8          # k_dup.hip: operations a thread sums itself
PASS = 64         # operations of a wave's pass
POS_MAX = (1 << 31) - 2
PATH_NCIGARS = [1, DP_T, DP_T + 1, PASS, PASS + 1, 4000]


def cols_with_tlen(reads, seed=0):
    cols = cols_of(reads, seed)
    cols["tlen"] = np.array([r.get("tlen", 0) for r in reads], np.int32)
    return cols


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the rule
# ---------------------------------------------------------------------------------------------------------------------------
RULE_REFS, RULE_LANES = 3, 3


def rule_batch():
    """(cols, reads, marks): marks maps a name to (index a, index b, the sets the two reads make: 1 or 2), or to a list of indices of
    reads that are not examined / are second ends."""
    reads, marks = [], {}
    base = dict(flag=P | FIRST, rid=1, pos=5000, tlen=300, lane=0, cigar=[(50, M)])

    def add(**kw):
        reads.append(dict(base, **kw))
        return len(reads) - 1

    a = add()
    marks["lane only"] = (a, add(lane=2), 1)
    marks["strand"] = (a, add(flag=P | FIRST | REV, pos=5000 - 49), 2)            # (the same u5 = 5000: pos + 50 - 1)
    marks["mate strand"] = (a, add(flag=P | FIRST | MREV), 2)
    marks["class"] = (add(tlen=0, pos=6000), add(tlen=7, pos=6000), 2)             # single against pair; the single's tlen is no part
    marks["rid"] = (a, add(rid=2), 2)
    marks["u5"] = (a, add(pos=5001), 2)
    marks["tlen"] = (a, add(tlen=301), 2)
    marks["mate flag only"] = (a, add(flag=P | LAST), 1)                           # 0x40 / 0x80 are no part of the signature
    marks["mapq only"] = (a, add(mapq=0), 1)
    marks["flagged"] = (a, add(flag=P | FIRST | DUP, lane=1), 1)                   # 0x400: examined, counted in F
    marks["not examined"] = [add(flag=P | FIRST | b) for b in (UNMAPPED, SECONDARY, QCFAIL, SUPPL)]
    marks["second end"] = [add(tlen=-300), add(tlen=-300, flag=P | LAST | REV | DUP)]
    # singles: tlen = 0, the mate unmapped, unpaired (their tlen and mate strand are no part of the signature)
    s0 = add(tlen=0, pos=7000)
    marks["single: mate unmapped"] = (s0, add(flag=P | FIRST | MUNMAPPED | MREV, tlen=300, pos=7000), 1)
    marks["single: unpaired"] = (s0, add(flag=FIRST, tlen=-5, pos=7000), 1)
    marks["single: tlen"] = (s0, add(tlen=0, pos=7000, flag=P | LAST | MREV), 1)
    # clips on a forward read: u5 = pos - lead whatever lies behind
    f0 = add(pos=8000, cigar=[(40, M)])
    for name, cig, pos in (("S", [(5, S), (35, M)], 8005), ("H", [(7, H), (40, M)], 8007), ("H+S", [(2, H), (3, S), (35, M)], 8005),
                           ("trailing", [(30, M), (6, S), (9, H)], 8000), ("both", [(4, S), (20, M), (16, S)], 8004)):
        marks["forward clip " + name] = (f0, add(pos=pos, cigar=cig), 1)
    # ... and on a reverse read: u5 = pos + reflen - 1 + trail whatever lies in front
    r0 = add(flag=P | LAST | REV, pos=9000, cigar=[(40, M)])                       # u5 = 9039
    for name, cig, pos in (("S", [(35, M), (5, S)], 9000), ("H", [(33, M), (7, H)], 9000), ("S+H", [(30, M), (4, S), (6, H)], 9000),
                           ("leading", [(9, H), (6, S), (30, M)], 9010), ("both", [(4, S), (20, M), (3, D), (10, M), (7, S)], 9000),
                           ("D and N", [(10, M), (5, D), (10, EQ), (5, N_), (5, X), (2, I), (5, M)], 9000)):
        marks["reverse clip " + name] = (r0, add(flag=P | LAST | REV, pos=pos, cigar=cig), 1)
    marks["inner clip is no clip"] = (f0, add(pos=8002, cigar=[(2, S), (10, M), (3, S), (25, M)]), 1)  # lead is the PREFIX only
    marks["inner clip is no trail"] = (r0, add(flag=P | LAST | REV, pos=9000, cigar=[(10, M), (3, S), (27, M), (3, S)]), 1)  # 9000 + 37 - 1 + 3
    # the same u5 through different clips, forward and reverse
    marks["all clips forward"] = (add(pos=9995, cigar=[(10, M)], tlen=0), add(pos=10_000, cigar=[(2, H), (3, S)], tlen=0), 1)
    marks["all clips reverse"] = (add(flag=P | LAST | REV, pos=9990, cigar=[(10, M)], tlen=0), add(flag=P | LAST | REV, pos=10_000, cigar=[(5, S)], tlen=0), 1)  # trail is 0
    marks["negative u5"] = (add(pos=0, cigar=[(10, S), (30, M)]), add(pos=0, cigar=[(4, H), (6, S), (30, M)], lane=1), 1)
    marks["negative u5 against 0"] = (marks["negative u5"][0], add(pos=0, cigar=[(30, M)]), 2)
    far = dict(flag=P | LAST | REV, rid=2, pos=POS_MAX, tlen=0)
    marks["far end"] = (add(cigar=[(4, M), (OPMAX, H), (OPMAX, H), (OPMAX, H)], **far), add(cigar=[(4, M), (OPMAX, H), (OPMAX - 1, H), (OPMAX, H), (1, H)], **far), 1)
    marks["far end u5"] = (marks["far end"][0], add(cigar=[(4, M), (OPMAX, H), (OPMAX, H), (OPMAX - 1, H)], **far), 2)
    # a crowd: every read of the list above once more per read group, and a few hundred reads in all
    n = len(reads)
    for lane in (1, 2, 0, 1, 2):
        for i in range(n):
            reads.append(dict(reads[i], lane=lane))
    return cols_with_tlen(reads, 3), reads, marks


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the two-word race, 3. contention
# ---------------------------------------------------------------------------------------------------------------------------
def race_batch(shared):
    """4096 reads of 64 signatures, 64 reads each, interleaved.  shared = "k0": one k0 (class, strands, u5), 64 different k1 (rid 0 ... 7
    x 8 template lengths); shared = "k1": one k1 (rid, tlen), 64 different k0 (u5)."""
    reads = []
    for i in range(4096):
        s = i % 64
        if shared == "k0":
            reads.append(dict(flag=P | FIRST, rid=s % 8, pos=1000, tlen=200 + s // 8, cigar=[(20, M)]))
        else:
            reads.append(dict(flag=P | FIRST, rid=3, pos=1000 + 7 * s, tlen=250, cigar=[(20, M)]))
    return cols_with_tlen(reads, 5)


RACE_REFS = 8


def hot_batch(n=20_000):
    reads = [dict(flag=P | FIRST, rid=0, pos=500, tlen=180, lane=i & 1, cigar=[(16, M)]) for i in range(n)]
    return cols_with_tlen(reads, 6)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. probing: sets of exactly `n` different signatures for the smallest table (capacity 16: 32 slots)
# ---------------------------------------------------------------------------------------------------------------------------
PROBE_ROUNDS = 48


def probe_batch(seed, n=16):
    """n different signatures with 1 ... 3 reads each.  Nothing is known of the hash: PROBE_ROUNDS such batches with half of the 32 slots
    taken each make it all but certain that some probe sequence runs over the table's end (a run of taken slots covers the last slot
    in a good share of the rounds)."""
    rng = np.random.default_rng(seed)
    pos = rng.choice(1 << 20, n, replace=False)
    reads = []
    for k in range(n):
        for _ in range(1 + k % 3):
            reads.append(dict(flag=P | FIRST | (REV if k & 1 else 0), rid=k % 2, pos=int(pos[k]), tlen=int(100 + k) if k % 4 else 0, cigar=[(25, M)]))
    order = rng.permutation(len(reads))
    return cols_with_tlen([reads[i] for i in order], seed)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. CIGAR lengths: thread path against wave path
# ---------------------------------------------------------------------------------------------------------------------------
def clip_cigar(nc, salt):
    """nc operations with clips at both ends where there is room, and clips inside that are no part of either."""
    if nc == 1:
        return [(30 + salt, M)]
    assert nc >= 7
    body = mixed_cigar(nc - 5, salt)
    body[0], body[-1] = (5, M), (4, M)  # (a match on either side: the clips outside are the maximal runs)
    return [(3, H), (2 + salt, S)] + body + [(1 + salt, S), (2, H), (1, H)]


def path_batch():
    """(reads, twins): per operation count a reverse read and a forward read (second contig) with clips on both ends, and for each
    its twin: a read of ONE operation that the restatement places on the same signature.  Every set then has exactly two reads."""
    reads = []
    for nc in PATH_NCIGARS:
        reads.append(dict(flag=P | LAST | REV, rid=0, pos=100_000, tlen=0, cigar=clip_cigar(nc, 0)))
        reads.append(dict(flag=P | FIRST, rid=1, pos=100_000 + nc, tlen=0, cigar=clip_cigar(nc, 1)))
    reads.append(dict(flag=P | FIRST, rid=1, pos=300_000, tlen=0, cigar=[(1, S)] * (DP_T + 3) + [(20, M)]))  # a forward read whose clips outlast the thread's words
    twins = []
    for r in reads:
        rev = r["flag"] & REV
        u5 = dup_ref.u5_of(r["cigar"], r["pos"], bool(rev))
        twins.append(dict(flag=r["flag"], rid=r["rid"], tlen=0, pos=u5 if rev else u5, cigar=[(1, M)]))  # (reverse: pos + 1 - 1; forward: pos)
    return reads, twins


# ---------------------------------------------------------------------------------------------------------------------------
# 6. order, 7. life cycle
# ---------------------------------------------------------------------------------------------------------------------------
ORDER_REFS, ORDER_LANES = 2, 4


def order_batch(seed=11, n=3000):
    """n reads of about n / 3 fragments on two contigs in four read groups: sets of 1 to a few dozen reads, both classes, second ends,
    flagged reads and reads that are not examined."""
    rng = np.random.default_rng(seed)
    frag = [dict(rid=int(rng.integers(0, 2)), pos=int(rng.integers(0, 50_000)), tlen=int(rng.integers(150, 160)), rev=int(rng.integers(0, 2)),
                 mrev=int(rng.integers(0, 2)), lead=int(rng.integers(0, 3))) for _ in range(n // 3)]
    pick = np.minimum(rng.zipf(1.6, n) - 1, len(frag) - 1)
    reads = []
    for i in range(n):
        f = frag[int(pick[i])]
        kind = int(rng.integers(0, 10))
        flag = P | (FIRST if i & 1 else LAST) | (REV if f["rev"] else 0) | (MREV if f["mrev"] else 0) | (DUP if i % 7 == 0 else 0) | (SECONDARY if kind == 2 else 0)
        tlen = -f["tlen"] if kind == 3 else 0 if kind == 4 else f["tlen"]
        cig = ([(f["lead"], S)] if f["lead"] else []) + [(30, M), (1, D), (10, M)] + ([(f["lead"], S)] if f["lead"] and f["rev"] else [])
        reads.append(dict(flag=flag, rid=f["rid"], pos=f["pos"], tlen=tlen, lane=int(rng.integers(0, ORDER_LANES)), cigar=cig))
    return cols_with_tlen(reads, seed)
