"""Test infrastructure for the substitution tables (no GPU use): the constants of k_sbc.hip stated once (tests/test_substitutions_cpu.py
holds them against the kernel's #define lines) and the builders of the batches of tests/test_gpu_substitutions.py.  The launch
arithmetic is k_mbc's (tests/cycle_steps.py: the same grid, step and run list), so the step batch is that module's."""
import numpy as np

from tests.cycle_steps import MB_RUNS, MB_STEP, mbc_launch, mbc_runs, step_batch, step_layout  # noqa: F401  (k_sbc's launch is k_mbc's)
from tests.long_layout import records

SB_C = 1024      # cycles of Y the LDS tile holds: cycles at or behind it go to device memory
SB_STEP = 768
SB_RUNS = 768
PASS = 256       # stored positions of a run a wave takes per pass
P, PR, REV, FIRST, LAST, MAIN = 0x1, 0x2, 0x10, 0x40, 0x80, 0x1000
A, C, G, T, N_ = 0, 1, 2, 3, 4
QUALS = np.array([0, 2, 19, 20, 37, 63, 64, 93, 222], np.uint8)


def seq_offsets(cols):
    L = cols["l_seq"].astype(np.int64)
    return np.cumsum((L + 1) // 2) - (L + 1) // 2


def set_nib(cols, so, i, j, nib):
    k = so[i] + j // 2
    byte = int(cols["seq"][k])
    cols["seq"][k] = (byte & 0xF0) | nib if j & 1 else (byte & 0x0F) | (nib << 4)


def on_ref(ref, pos, ops, rng, L=None):
    """Codes (0..3) of a read that lies on the contig at `pos` with this CIGAR: M and = copy (a genome N: a drawn base), X takes
    another base, I and S draw, D and N skip, H and P do nothing; positions outside the contig draw.  L: cut or fill up to L bases."""
    out, rp = [], pos
    for n, op in ops:
        if op in "M=X":
            idx = rp + np.arange(n)
            inside = (idx >= 0) & (idx < len(ref))
            base = np.where(inside, ref[np.clip(idx, 0, len(ref) - 1)], 4)
            base = np.where(base > 3, rng.integers(0, 4, n), base).astype(np.uint8)
            out.append((base + 1) % 4 if op == "X" else base)
            rp += n
        elif op in "IS":
            out.append(rng.integers(0, 4, n).astype(np.uint8))
        elif op in "DN":
            rp += n
    codes = np.concatenate(out) if out else np.zeros(0, np.uint8)
    if L is not None:
        codes = np.concatenate([codes, rng.integers(0, 4, max(0, L - len(codes))).astype(np.uint8)])[:L]
    return codes


def build(ref_of, reads, rng, frac=0.06):
    """Column dict of reads given as dicts(ops, pos, flag, rid, lane, mapq, L, qual): the bases lie on the contig ref_of[rid] (a
    contig that is None: drawn), a fraction `frac` of them replaced by another base (substitutions of every kind), the qualities
    drawn from QUALS unless given."""
    recs = []
    for r in reads:
        ref = ref_of[r.get("rid", 0)] if 0 <= r.get("rid", 0) < len(ref_of) else None
        ref = np.zeros(1, np.uint8) if ref is None else ref
        codes = on_ref(ref, r["pos"], r["ops"], rng, r.get("L")).astype(np.int64)
        sub = rng.random(len(codes)) < frac
        codes = np.where(sub, (codes + rng.integers(1, 4, len(codes))) % 4, codes)
        qual = r.get("qual")
        if qual is None:
            qual = QUALS[rng.integers(0, len(QUALS), len(codes))]
        recs.append(dict(codes=codes, qual=np.asarray(qual, np.uint8), flag=r["flag"], pos=r["pos"], ops=r["ops"], lane=r.get("lane", 0),
                         nm=sum(n for n, op in r["ops"] if op in "ID")))
    cols = records(recs)
    cols["rid"] = np.array([r.get("rid", 0) for r in reads], np.int32)
    cols["mapq"] = np.array([r.get("mapq", 30) for r in reads], np.uint8)  # (30: no read is eligible for the triplet counters)
    return cols


def flag_of(rev, second, more=0):
    return P | PR | MAIN | (REV if rev else 0) | (LAST if second else FIRST) | more


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the rule
# ---------------------------------------------------------------------------------------------------------------------------
def rule_refs():
    """Two contigs: 96 bases with an N at 40 and at 60..61, and 3000 bases with a few N."""
    rng = np.random.default_rng(71)
    small = rng.integers(0, 4, 96).astype(np.uint8)
    small[[40, 60, 61]] = 4
    big = rng.integers(0, 4, 3000).astype(np.uint8)
    big[rng.choice(3000, 25, replace=False)] = 4
    return [small, big]


def rule_batch(Q=20, MQ=30):
    """The hand-made kinds of reads, each on both strands and as both mates, in three read groups: over the same stretch forward and
    reverse; at the contig's first and last base; over a genome N (as the base and as either neighbour); read codes N, = and an
    ambiguity code; qualities Q - 1, Q, 221 and 222; mapq MQ - 1 and MQ; and reads of 17 to 1030 bases on the second contig."""
    refs = rule_refs()
    rng = np.random.default_rng(72)
    reads, special = [], []
    for lane in range(3):
        for rev in (0, 1):
            for second in (0, 1):
                f = flag_of(rev, second)
                base = dict(flag=f, lane=lane, mapq=max(MQ, 1))
                reads.append(dict(base, ops=[(20, "M")], pos=10))                       # the same stretch on both strands
                reads.append(dict(base, ops=[(12, "M")], pos=0))                        # rr = 0
                reads.append(dict(base, ops=[(12, "M")], pos=96 - 12))                  # rr = len - 1
                reads.append(dict(base, ops=[(30, "M")], pos=35))                       # genome N at 40, 60 and 61
                reads.append(dict(base, ops=[(2, "S"), (1, "M"), (1, "I"), (1, "M"), (2, "D"), (1, "M"), (2, "S")], pos=70))  # runs of one
                special.append(len(reads))
                reads.append(dict(base, ops=[(16, "M")], pos=12))                       # read codes N, = and M at 3, 4, 5
                qs = np.full(16, 40, np.uint8)
                qs[:4] = [max(Q, 1) - 1, Q, 221, 222]  # (223 and more: the library refuses the batch; the restatement's side is in test_substitutions_cpu.py)
                reads.append(dict(base, ops=[(16, "M")], pos=14, qual=qs))              # the quality's edges
                reads.append(dict(base, ops=[(16, "M")], pos=16, mapq=max(MQ, 1) - 1))  # below MQ (MQ = 0: mapq 0, which counts)
                reads.append(dict(base, ops=[(16, "M")], pos=18, mapq=MQ))
                for L in (17, 299, 301, 1030):
                    reads.append(dict(base, ops=[(L, "M")], pos=100 + 7 * lane + L, rid=1, qual=np.full(L, 20 + L % 7, np.uint8)))
    cols = build(refs, reads, rng)
    so = seq_offsets(cols)
    for i in special:
        for j, nib in ((3, 15), (4, 0), (5, 3)):
            set_nib(cols, so, i, j, nib)
    return cols, refs


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the genome window
# ---------------------------------------------------------------------------------------------------------------------------
WINDOW_LENS = (61, 62, 63, 64)  # the contig's last byte at every place of its dword (the allocator starts every contig on 256 bytes)


def window_batch():
    """Runs of 1 to 9 positions behind a soft clip of 0 to 3 bases (the run's first stored position at every residue mod 4) at every
    residue of `pos` mod 4, on both strands, at the first and last 8 bases of four contigs whose lengths have every residue mod 4,
    and in their middle: 6912 reads."""
    rng = np.random.default_rng(73)
    refs = []
    for n in WINDOW_LENS:
        r = rng.integers(0, 4, n).astype(np.uint8)
        r[[20, 33]] = 4
        refs.append(r)
    reads = []
    for rid, n in enumerate(WINDOW_LENS):
        for rev in (0, 1):
            for clip in range(4):
                for run in range(1, 10):
                    for d in range(8):
                        for pos in (d, 24 + d, n - run - d):
                            ops = ([(clip, "S")] if clip else []) + [(run, "M"), (2, "S")]
                            reads.append(dict(ops=ops, pos=pos, flag=flag_of(rev, len(reads) & 1), rid=rid))
    return build(refs, reads, rng, frac=0.1), refs


# ---------------------------------------------------------------------------------------------------------------------------
# 3. CIGAR shapes
# ---------------------------------------------------------------------------------------------------------------------------
def shapes_batch():
    """k_mbc's list of shapes: runs of 1, 2, 3 and 5 positions at every alignment, reads of dozens of runs, runs of more than 256
    positions, a run that starts before 0 and one that ends behind the contig, reverse reads far longer than N, lengths around the
    LDS tile's SB_C cycles, and 300 reads of five runs."""
    rng = np.random.default_rng(74)
    ref = rng.integers(0, 4, 30_000).astype(np.uint8)
    ref[rng.choice(30_000, 200, replace=False)] = 4
    small = [(1, "M"), (1, "I"), (2, "M"), (1, "D"), (3, "M"), (2, "I"), (5, "M"), (3, "D")]
    alt = [(90, "M") if k % 2 == 0 else ((11, "I") if k % 4 == 1 else (7, "D")) for k in range(41)]
    nine = [(20, "M"), (3, "I"), (20, "M"), (2, "D"), (20, "M"), (3, "I"), (20, "M"), (2, "D"), (20, "M")]
    reads = []
    for rev in (0, 1):
        for second in (0, 1):
            f = flag_of(rev, second)
            for shift in range(8):
                reads.append(dict(ops=small * 12, pos=400 + shift, flag=f))
            reads.append(dict(ops=alt, pos=1001, flag=f))
            reads.append(dict(ops=[(5, "H"), (5, "S"), (140, "M")], pos=303, flag=f))
            reads.append(dict(ops=[(10, "="), (1, "X"), (139, "=")], pos=707, flag=f))
            reads.append(dict(ops=[(50, "M"), (1000, "N"), (100, "M"), (2, "P"), (30, "M")], pos=606, flag=f))
            reads.append(dict(ops=[(150, "M")], pos=len(ref) - 100, flag=f))   # ends behind the contig
            reads.append(dict(ops=[(150, "M")], pos=-3, flag=f))               # starts in front of it
            reads.append(dict(ops=[(100, "M")], pos=1500, flag=f, L=60))       # the CIGAR consumes more than l_seq
            for L in (257, 258, 600, 2000, 4000, SB_C - 1, SB_C, SB_C + 1, 1023, 1024, 1025):
                reads.append(dict(ops=[(L, "M")], pos=2000 + 3 * L + rev, flag=f))
            reads.append(dict(ops=[(700, "M"), (5, "I"), (1300, "M")], pos=9000, flag=f))
    for more, rid in ((0x4, 0), (0x100, 0), (0x800, 0), (0x8000, 0), (0, -1), (0, 1)):  # not examined; then duplicates and QC fail, which are
        reads.append(dict(ops=[(150, "M")], pos=1700, flag=flag_of(0, 0, more), rid=rid))
    reads.append(dict(ops=[(150, "M")], pos=2500, flag=flag_of(0, 0, 0x400)))
    reads.append(dict(ops=[(150, "M")], pos=2600, flag=flag_of(1, 1, 0x200)))
    reads.append(dict(ops=[], pos=1600, flag=flag_of(0, 1), L=80))
    reads += [dict(ops=nine, pos=3000 + 37 * k, flag=flag_of(k & 2, k & 1)) for k in range(300)]
    cols = build([ref, None], reads, rng)
    cols["qual"][cols["flag"].repeat(cols["l_seq"].astype(np.int64)) & 0x8000 != 0] = 0xFF
    return cols, [ref, None]


# ---------------------------------------------------------------------------------------------------------------------------
# 4. three read groups, alternating and in runs
# ---------------------------------------------------------------------------------------------------------------------------
def groups_batch():
    from tests.long_layout import reads_on_ref
    rng = np.random.default_rng(75)
    ref = rng.integers(0, 4, 20_000).astype(np.uint8)
    ref[rng.choice(20_000, 60, replace=False)] = 4
    lane = [i % 3 for i in range(60)]
    for g, run in ((0, 1), (1, 2), (2, 700), (0, 2), (1, 700), (2, 1), (0, 700), (1, 1)):
        lane += [g] * run
    n = len(lane)
    L = rng.choice([16, 40, 150, 255, 256, 300, 700], n)
    flag = (P | PR | MAIN | np.where(rng.random(n) < 0.5, REV, 0) | np.where(rng.random(n) < 0.5, FIRST, LAST)).astype(np.uint16)
    cols = reads_on_ref(ref, np.sort(rng.integers(0, 19_000, n)), L, flag, QUALS[rng.integers(0, len(QUALS), int(L.sum()))], lane=lane)
    cols["mapq"] = rng.choice(np.array([0, 29, 30, 60, 254, 255], np.uint8), n)
    plant(cols, rng, 0.05)
    return cols, ref


def plant(cols, rng, frac):
    """Substitutions by rewriting nibbles of cols["seq"]: a fraction `frac` of the bases A, C, G, T becomes another of them."""
    seq = cols["seq"]
    for shift in (0, 4):
        nib = (seq >> shift) & 15
        hit = (rng.random(len(seq)) < frac) & np.isin(nib, (1, 2, 4, 8))
        new = np.array([1, 2, 4, 8], np.uint8)[(np.log2(np.maximum(nib, 1)).astype(np.int64) + rng.integers(1, 4, len(seq))) % 4]
        seq[:] = np.where(hit, (seq & (0xF0 >> shift)) | (new << shift), seq)
    return cols


# ---------------------------------------------------------------------------------------------------------------------------
# 5. one bin
# ---------------------------------------------------------------------------------------------------------------------------
def hot_batch(n, mismatch):
    """n identical reads of 16 A (mismatch: 16 C) on a contig of A alone: every pair into X[forward][AAA][A] (or [C])."""
    from tests.long_layout import reads_on_ref
    ref = np.zeros(1000, np.uint8)
    flag = P | PR | MAIN | FIRST | 0x400  # (duplicates: identical reads, and out of the coverage windows' way)
    cols = reads_on_ref(ref + (1 if mismatch else 0), np.full(n, 500), np.full(n, 16), np.full(n, flag, np.uint16), np.full(n * 16, 37, np.uint8))
    cols["mapq"][:] = 30
    return cols, ref


def step_batch_of(n_cu, variant, N):
    """The step batch of tests/cycle_steps.py for a card of n_cu CUs: every workgroup makes three steps, each with more runs than the
    list holds, and a read-group change lies on a step seam."""
    return step_batch(step_layout(n_cu, variant, N))
