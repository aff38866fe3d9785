"""The batches of the overrepresented-sequence tests (tests/test_gpu_overrepresented.py; tests/test_overrepresented_cpu.py asserts that
each of them crosses the edge it is named for).  Reads are (sequence AS SEQUENCED over adp_steps.CODES, reverse, flag bits beside the
strand, read group); `cols` stores a reverse read as its reverse complement (adp_steps.as_stored).  No read lies on a main
chromosome and no contig is loaded: the genome is not read."""
import numpy as np

from tests.adp_steps import CODES, FIRST, LAST, P, REV, as_stored, cols_of

UNMAPPED, SECONDARY, QCFAIL, DUP, SUPPL, NO_QUAL = 0x4, 0x100, 0x200, 0x400, 0x800, 0x8000
OTHER = [c for c in CODES if c not in "ACGT"]  # the twelve stored codes that are no base
UNI = "AGATCGGAAGAG"


def cols(reads, pad=None):
    """The column dict of reads (sequence as sequenced, reverse, flag bits, read group).  pad: the stored code (a letter) that fills the
    pad nibble of every read of odd length — what a kernel that read it would take for a base."""
    c, _ = cols_of([(as_stored(s, rev), f | (REV if rev else 0)) for s, rev, f, g in reads], [g for s, rev, f, g in reads])
    if pad is not None:
        L = c["l_seq"].astype(np.int64)
        nb = (L + 1) // 2
        last = (np.cumsum(nb) - 1)[(L & 1) == 1]
        c["seq"] = c["seq"].copy()
        c["seq"][last] |= CODES.index(pad)
    return c


def rand_seq(rng, L):
    return "".join(rng.choice(list("ACGT"), L))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the rule
# ---------------------------------------------------------------------------------------------------------------------------
RULE_LANES = 3


def rule_batch(K):
    """(cols, reads, marks): marks maps a name to (index a, index b, the sets the two reads make: 1 or 2), to ("skipped", index) /
    ("entered", index), or to a list of indices of reads that are not examined."""
    rng = np.random.default_rng(100 + K)
    reads, marks = [], {}

    def add(s, rev=False, f=P | FIRST, g=0):
        reads.append((s, rev, f, g))
        return len(reads) - 1

    S = rand_seq(rng, K + 10)
    a = add(S)
    marks["not examined"] = [add(S, f=P | FIRST | SECONDARY), add(S, f=P | FIRST | SUPPL), add(S, f=P | LAST | SECONDARY | SUPPL),
                             add(S, f=P | SECONDARY), add("", f=P | FIRST | UNMAPPED)]  # every bit of 0x900; secondary without a mate flag; l_seq 0
    for name, bit in (("unmapped", UNMAPPED), ("QC fail", QCFAIL), ("duplicate", DUP), ("no qualities", NO_QUAL)):
        marks["examined: " + name] = (a, add(S, f=P | FIRST | bit, g=1), 1)
    marks["read group only"] = (a, add(S, g=2), 1)
    marks["forward against reverse"] = (a, add(S, rev=True), 1)      # (stored as revcomp(S))
    marks["both mates"] = (a, add(S, f=P | LAST), 2)
    marks["ACGT against ACGTA"] = (add("ACGT"), add("ACGTA"), 2)
    marks["ACGT twice"] = (marks["ACGT against ACGTA"][0], add("ACGT", rev=True), 1)
    flip = lambda s, i: s[:i] + "ACGT"[("ACGT".index(s[i]) + 1) % 4] + s[i + 1:]
    marks["different at K"] = (a, add(flip(S, K)), 1)
    marks["different at K reverse"] = (a, add(flip(S, K), rev=True), 1)
    marks["different at K - 1"] = (a, add(flip(S, K - 1)), 2)
    marks["different at K - 1 reverse"] = (a, add(flip(S, K - 1), rev=True), 2)
    marks["different at 0"] = (a, add(flip(S, 0), rev=True), 2)
    marks["longer than K"] = (a, add(S[:K] + rand_seq(rng, 200), rev=True), 1)
    marks["exactly K"] = (a, add(S[:K]), 1)
    marks["K - 1 against K"] = (a, add(S[:K - 1]), 2)
    for x in OTHER:  # a code that is no base at the prefix's last position (skipped) and directly behind it (entered), on both strands
        for rev in (False, True):
            tag = "%s %s" % (x, "reverse" if rev else "forward")
            marks["skipped: " + tag] = ("skipped", add(S[:K - 1] + x + S[K:], rev=rev))
            marks["entered: " + tag] = ("entered", add(S[:K] + x + S[K + 1:], rev=rev, g=1))
            marks["skipped short: " + tag] = ("skipped", add(S[:K - 6] + x, rev=rev, f=P | LAST))  # n = L < K: the read's last base
    for x in "TA":
        p = add(x * K)
        marks["poly-%s" % x] = (p, add(x * K, rev=True), 1)
        marks["poly-%s against one more" % x] = (p, add(x * (K - 1)), 2)
        marks["poly-%s and a longer one" % x] = (p, add(x * (K + 3), rev=True, g=2), 1)
    marks["poly-T against poly-A"] = (marks["poly-T"][0], marks["poly-A"][0], 2)
    n = len(reads)
    for g in (1, 2, 0):  # a crowd: every read once more per read group
        for i in range(n):
            s, rev, f, _ = reads[i]
            reads.append((s, rev, f, g))
    return cols(reads), reads, marks


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the layout
# ---------------------------------------------------------------------------------------------------------------------------
LAYOUT_LENGTHS = list(range(1, 131)) + [255, 256, 300]
LONG_LENGTHS = [10_000, 70_000]


def layout_batch(K, seed=7):
    """(cols, reads, starts): every length of LAYOUT_LENGTHS on both strands with its first byte on each of the four alignments mod 4
    (short filler reads in front), the long reads, and for EVERY such read a twin on the other strand that holds just its n bases,
    somewhere else in the batch: every set of 16 and more bases has exactly two reads (shorter random sequences meet by chance), unless
    a key was made of anything but the read's own n bases.  The pad nibbles hold a T.  The last read is reverse and of odd length.
    starts: {(length, reverse): the set of its first bytes mod 4}."""
    rng = np.random.default_rng(seed * 1000 + K)
    main, twins, starts = [], [], {}
    off = 0  # bytes of the payload in front of the next read

    def put(s, rev):
        nonlocal off
        main.append((s, rev, P | (FIRST if len(main) & 1 else LAST), 0))
        off += (len(s) + 1) // 2

    for L in LAYOUT_LENGTHS + LONG_LENGTHS:
        for rev in (False, True):
            for a in range(4):
                if L in LONG_LENGTHS and a:
                    continue
                fill = (a - off) % 4
                if fill and L not in LONG_LENGTHS:
                    f = rand_seq(rng, 2 * (fill + 8) - 1)  # (fill + 8 bytes; a filler is a read like any other: it has a twin as well)
                    put(f, False)
                    twins.append((f[:K], True, main[-1][2], 0))
                s = rand_seq(rng, L)
                starts.setdefault((L, rev), set()).add(off % 4)
                put(s, rev)
                twins.append((s[:K], not rev, main[-1][2], 0))
    order = rng.permutation(len(twins))
    tail = rand_seq(rng, 77)
    reads = main + [twins[i] for i in order] + [(tail[:K], False, P | FIRST, 0), (tail, True, P | FIRST, 0)]
    return cols(reads, pad="T"), reads, starts


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the two-word race, 4. contention
# ---------------------------------------------------------------------------------------------------------------------------
def race_batch(shared, K=56):
    """4096 reads of 64 keys, 64 reads each, interleaved.  shared = "first": one first key word (bases 0 ... 27), 64 different second
    words; shared = "second": the other way round."""
    rng = np.random.default_rng(5)
    head, tail = rand_seq(rng, 28), rand_seq(rng, K - 28)
    var = ["".join("ACGT"[(s >> (2 * k)) & 3] for k in range(3)) for s in range(64)]
    reads = []
    for i in range(4096):
        v = var[i % 64]
        s = head + v + tail[3:] if shared == "first" else v + head[3:] + tail
        reads.append((s, bool(i & 64), P | FIRST, 0))
    return cols(reads)


OV_STEP = 1024       # reads of a k_ovr step (OV_THREADS)


def steps_batch(n_cu, seed=13):
    """More than 2 * OV_STEP * n_cu reads of 24 bases: every workgroup of a card of n_cu CUs makes three steps (the columns loaded
    ahead, the new-set counters' turn).  The reads are drawn from 40 000 sequences, half of them never repeated; three read groups,
    non-decreasing; both mates and strands."""
    from tests.adp_steps import cols_of_nibbles
    rng = np.random.default_rng(seed)
    n = 2 * OV_STEP * n_cu + 977
    pool = rng.choice(np.array([1, 2, 4, 8], np.uint8), (40_000, 24))
    pick = np.where(rng.integers(0, 2, n) == 1, rng.integers(0, 20_000, n), 20_000 + np.arange(n) % 20_000)
    flag = (P | np.where(rng.integers(0, 2, n) == 1, FIRST, LAST) | np.where(rng.integers(0, 2, n) == 1, REV, 0)).astype(np.uint16)
    lane = np.sort(rng.integers(0, 3, n)).astype(np.uint8)
    c, _ = cols_of_nibbles(pool[pick].ravel(), np.full(n, 24), flag, lane)
    return c


def hot_batch(n=20_000):
    s = rand_seq(np.random.default_rng(6), 60)
    return cols([(s, bool((i >> 1) & 1), P | FIRST, i & 1) for i in range(n)])


# ---------------------------------------------------------------------------------------------------------------------------
# 5. probing: exactly `n` different keys for the smallest table (capacity 16: 32 slots)
# ---------------------------------------------------------------------------------------------------------------------------
PROBE_ROUNDS = 48


def probe_batch(seed, n=16):
    """n different keys with 1 ... 3 reads each.  Nothing is known of the hash: PROBE_ROUNDS such batches with half of the 32 slots
    taken each make it all but certain that some probe sequence runs over the table's end."""
    rng = np.random.default_rng(seed)
    reads = []
    for k in range(n):
        s = rand_seq(rng, 40 + k)
        for _ in range(1 + k % 3):
            reads.append((s, bool(k & 1), P | (FIRST if k % 4 else LAST), 0))
    return cols([reads[i] for i in rng.permutation(len(reads))])


def many_keys(n=5000):
    rng = np.random.default_rng(8)
    return cols([(rand_seq(rng, 50), False, P | FIRST, 0) for _ in range(n)])


# ---------------------------------------------------------------------------------------------------------------------------
# 6. threshold and list
# ---------------------------------------------------------------------------------------------------------------------------
def sets_batch(counts, seed, fill_to=None, mate=FIRST, length=60):
    """A set of counts[k] reads for every k (strands alternating), then single reads up to fill_to entered reads.  -> (reads, the sets'
    sequences)"""
    rng = np.random.default_rng(seed)
    seqs = [rand_seq(rng, length) for _ in counts]
    reads = [(s, bool(i & 1), P | mate, 0) for s, c in zip(seqs, counts) for i in range(c)]
    while fill_to is not None and len(reads) < fill_to:
        reads.append((rand_seq(rng, length), False, P | mate, 0))
    return reads, seqs


def threshold_batches():
    """{name: (reads, ppm, {mate: the sequences that must be listed, in order})} (K = 50)."""
    out = {}
    r, s = sets_batch([3, 2], 21, 3000)                                   # ceil(3000 * 1000 / 10^6) = 3
    out["T = 3 at 3000 reads"] = (r, 1000, {0: [s[0][:50]], 1: []})
    r, s = sets_batch([4, 3], 22, 3001)                                   # ceil(3001 * 1000 / 10^6) = 4
    out["T = 4 at 3001 reads"] = (r, 1000, {0: [s[0][:50]], 1: []})
    r0, s0 = sets_batch([5], 23)
    r1, s1 = sets_batch([4, 1], 24, mate=LAST)
    out["ppm 10^6"] = (r0 + r1, 1_000_000, {0: [s0[0][:50]], 1: []})      # T = entered: only a mate of ONE sequence lists it
    r, s = sets_batch([2], 25, 100)                                       # ceil(100 * 1000 / 10^6) = 1 -> 2: no single read is listed
    out["never a single read"] = (r, 1000, {0: [s[0][:50]], 1: []})
    r, s = sets_batch([3, 3, 3, 5, 3], 26, 40)
    out["ties"] = (r, 1000, {0: [s[3][:50]] + sorted(x[:50] for x in s[:3] + s[4:]), 1: []})
    r, s = sets_batch([3] * 10, 27, mate=LAST)                            # ceil(30 * 10^5 / 10^6) = 3: all ten, the most a mate can list
    out["ten sets at ppm 10^5"] = (r, 100_000, {0: [], 1: sorted(x[:50] for x in s)})
    rng = np.random.default_rng(28)
    dimer = rand_seq(rng, 10) + UNI + rand_seq(rng, 40)
    plain = "ACGTTGCA" * 8
    src = [(dimer, False, P | FIRST, 0)] * 4 + [("G" * 70, True, P | FIRST, 0)] * 3 + [(plain, False, P | FIRST, 0)] * 2
    out["sources"] = (src, 1000, {0: [dimer[:50], "G" * 50, plain[:50]], 1: []})
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# 7. order, life cycle, 8. 256 read groups
# ---------------------------------------------------------------------------------------------------------------------------
ORDER_LANES = 4


def order_batch(seed=11, n=3000, n_lanes=ORDER_LANES):
    """n reads drawn from about n / 3 sequences (sets of 1 to a few hundred reads), both mates and strands, lengths around K, reads with
    an N, reads that are not examined."""
    rng = np.random.default_rng(seed)
    pool = [rand_seq(rng, int(rng.integers(30, 90))) for _ in range(n // 3)]
    pick = np.minimum(rng.zipf(1.5, n) - 1, len(pool) - 1)
    reads = []
    for i in range(n):
        s = pool[int(pick[i])]
        kind = int(rng.integers(0, 12))
        if kind == 0:
            at = int(rng.integers(0, len(s)))
            s = s[:at] + "N" + s[at + 1:]
        f = P | (FIRST if pick[i] & 1 else LAST) | (SECONDARY if kind == 1 else 0) | (UNMAPPED if kind == 2 else 0) | (DUP if kind == 3 else 0)
        reads.append((s, bool(rng.integers(0, 2)), f, int(rng.integers(0, n_lanes))))
    return cols(reads)
