"""Test infrastructure for the per-read statistics (no GPU use): the directed batches of tests/test_gpu_read_stats.py, each at one
kind of seam of bamqc_amd/csrc/read_stats.h, and the chunk and grid rules of the two kernels that run it, restated
(tests/test_read_stats_cpu.py asserts that every batch reaches its seam and holds the constants against the sources).

read_stats keeps one read group's counters in LDS: mismatch / deletion / insertion bins below RS_HB = 64, insert sizes below
RS_INS = 1024, read lengths and clip lengths up to BQC_CT = 304; everything else goes to the state vector with global atomics.
k_short runs it for reads of at most BQC_FAST_MAXLEN = 255 bases, k_reads for longer ones and, under BQC_NO_FAST=1, for all.

A batch is (cols, refs, opts), built once and never changed.  Two contigs: 0 is a main chromosome, 1 is not; no reference is loaded
and every read carries an alignment score of 30, which keeps it out of the triplets (the only statistic that needs the genome).
Positions rise four reads a step.  BQC_FLAG_MATE_MAIN is set unless a case is about that gate."""
import functools

import numpy as np

from tests import lane_limit, synth
from tests.rs_ref import BQC_CT, BQC_FAST_MAXLEN, RS_HB, RS_INS

P, PR, UNM, MUNM, REV, MREV, FIRST, LAST, SEC, QCF, DUP, SUPP, MATE_MAIN = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x400, 0x800, 0x1000
BASE = P | MATE_MAIN
FLAGS4 = [BASE | FIRST, BASE | LAST, BASE | FIRST | REV, BASE | LAST | REV]  # both mates, both strands
AS = 30                      # below the triplets' threshold of 50
INT32_MIN = -(1 << 31)
REFS = [None, None]
OPTS = dict(n_refs=2, main_chrom=[1, 0], n_lanes=1, isize=2000, max_read_len=1024, hist_cap=4096)
ERR_NO_MATE_FLAG, ERR_RANGE = 3, 6

# the launch constants (device_types.h, k_short.hip, bqc_pipeline.cpp)
CHUNK_READS = 128            # BQC_CHUNK_READS: reads of a chunk of k_reads
SW_READS = 4096              # BQC_SW_READS: positions of the processing order whose reads k_short's groups are made of
FAST_WAVES = 16              # BQC_FAST_WAVES
LANE_CYCLES = 16             # 8 * BQC_FAST_NH: cycles a lane of k_short owns
READS_GRID_PER_CU = 8        # k_reads: min(chunk bound, 8 workgroups per CU)


def query_len(cigar):
    return sum(n for n, c in cigar if c in "MIS=X")


def rd(cigar, flag, L=None, rid=0, mapq=60, tlen=300, nm=0, lane=0):
    """One read: the CIGAR as stored, L its query length unless given (a record that contradicts itself)."""
    L = query_len(cigar) if L is None else L
    return synth.single_read(("ACGT" * (L // 4 + 1))[:L], [30] * L, list(cigar), flag, pos=0, rid=rid, mapq=mapq, tlen=tlen, nm=nm, as_=AS, lane=lane)


def oriented(ops, flag):
    """The stored CIGAR of a read whose operations are given in read orientation (5' end first): reversed on the reverse strand."""
    return list(ops)[::-1] if flag & REV else list(ops)


def finish(recs, **opts):
    cols = synth.concat(recs)
    cols["pos"] = (np.arange(len(cols["flag"])) // 4).astype(np.int32)
    return cols, REFS, dict(OPTS, **opts)


def ordinary(n, lane=0):
    """n plain reads of 30 bases, mates and strands in turn."""
    return [rd([(30, "M")], FLAGS4[i % 4], lane=lane, nm=i % 3, mapq=20 + i % 5) for i in range(n)]


# ---------------------------------------------------------------------------------------------------------------------------
# bins: mismatch, deletion and insertion counts around RS_HB
# ---------------------------------------------------------------------------------------------------------------------------
BIN_VALUES = [0, 1, RS_HB - 2, RS_HB - 1, RS_HB, RS_HB + 1, 200]


def indel_shapes(v, op):
    """CIGARs of 1, 2, 3 and 6 operations whose `op` lengths sum to v: in the only word, the first, the last and inner words."""
    a, b = v // 2, v - v // 2
    x, y, z = v // 3, v // 3, v - 2 * (v // 3)
    return [[(v, op)],
            [(v, op), (20, "M")], [(20, "M"), (v, op)],
            [(10, "M"), (v, op), (10, "M")], [(a, op), (20, "M"), (b, op)],
            [(5, "M"), (x, op), (5, "M"), (y, op), (5, "M"), (z, op)], [(x, op), (5, "M"), (y, op), (5, "M"), (z, op), (5, "M")]]


def bins():
    recs = []
    for v in BIN_VALUES:
        for f in FLAGS4:
            for k in range(3):  # mismatches alone: NM = v on 30M
                recs.append(rd([(30, "M")], f, nm=v))
            for op in "DI":     # NM = the indel's length: no mismatch
                for shape in indel_shapes(v, op):
                    recs.append(rd(shape, f, nm=v))
    for f in FLAGS4:            # all three next to the table's end at once
        for d, i, m in ((RS_HB - 1, RS_HB, RS_HB + 1), (RS_HB, RS_HB + 1, RS_HB - 1), (RS_HB + 1, RS_HB - 1, RS_HB)):
            recs.append(rd([(10, "M"), (d, "D"), (5, "M"), (i, "I"), (10, "M")], f, nm=d + i + m))
    return finish(recs)


# ---------------------------------------------------------------------------------------------------------------------------
# insert: |tlen| around RS_INS and around the cap
# ---------------------------------------------------------------------------------------------------------------------------
def insert_values(isize):
    return sorted({0, 1, RS_INS - 2, RS_INS - 1, RS_INS, RS_INS + 1, isize - 1, isize, isize + 1, (1 << 31) - 1})


def insert(isize):
    recs = []
    for v in insert_values(isize):
        for t in (v, -v):
            for f in (BASE | FIRST, BASE | FIRST | REV):
                recs.append(rd([(30, "M")], f, tlen=t))
    recs += [rd([(30, "M")], f, tlen=INT32_MIN) for f in (BASE | FIRST, BASE | FIRST | REV, BASE | FIRST)]  # |tlen| = 2^31
    for t in (RS_INS - 1, RS_INS, 7):  # reads that must not count
        recs.append(rd([(30, "M")], BASE | LAST, tlen=t))                # a second mate
        recs.append(rd([(30, "M")], BASE | FIRST | MUNM, tlen=t))        # the mate is unmapped
        recs.append(rd([(30, "M")], P | FIRST, tlen=t))                  # the mate lies off the main chromosomes
        recs.append(rd([(30, "M")], BASE | FIRST, rid=1, tlen=t))        # the read lies on a contig that is not main
        recs.append(rd([(30, "M")], BASE | FIRST | UNM, tlen=t))         # the read is unmapped
        recs.append(rd([(30, "M")], BASE | FIRST | SEC, tlen=t))
    return finish(recs, isize=isize)


# ---------------------------------------------------------------------------------------------------------------------------
# lengths: read lengths around BQC_FAST_MAXLEN, BQC_CT and 2^16 (totalbps is kept in two LDS words)
# ---------------------------------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, BQC_FAST_MAXLEN - 1, BQC_FAST_MAXLEN, BQC_FAST_MAXLEN + 1, BQC_CT - 1, BQC_CT, BQC_CT + 1, 1000, 65535, 65536, 65537]
LENGTHS_MAX = 70_000


def lengths():
    recs = []
    for L in LENGTHS:
        recs.append(rd([(L, "M")] if L else [], BASE | FIRST))   # (L = 0: a mapped read without a CIGAR)
        recs.append(rd([(L, "M")], BASE | LAST | REV))
    recs.append(rd([(LENGTHS_MAX, "M")], BASE | FIRST))
    return finish(recs, max_read_len=LENGTHS_MAX)


def lengths_over():
    recs = ordinary(10) + [rd([(LENGTHS_MAX + 1, "M")], BASE | FIRST)] + ordinary(10)
    return finish(recs, max_read_len=LENGTHS_MAX)


# ---------------------------------------------------------------------------------------------------------------------------
# clips: the soft-clip rules, and clip and read lengths around BQC_CT
# ---------------------------------------------------------------------------------------------------------------------------
def clipped(n5, n3, L, f, body=None, op="S", **kw):
    """A read of L bases with a soft clip of n5 at its 5' end and of n3 at its 3' end in read orientation (None: no such word; the
    match between them takes the rest, or `body`)."""
    m = max(L - (n5 or 0) - (n3 or 0), 0) if body is None else body
    ops = ([] if n5 is None else [(n5, op)]) + [(m, "M")] + ([] if n3 is None else [(n3, op)])
    return rd(oriented(ops, f), f, L=L, **kw)


def clips():
    recs = []
    L = 30
    for f in FLAGS4:
        for n5 in (0, 1, L - 1, L):                       # 0S: a clip that marks nothing (and still wins over the 3' end)
            recs.append(clipped(n5, None, L, f))
        recs.append(clipped(L + 5, None, L, f, body=5))   # longer than the read: the read's own cycles only
        for n3 in (0, 1, L - 1, L):
            recs.append(clipped(None, n3, L, f))
        recs.append(clipped(None, L + 1, L, f, body=5))   # longer than the read: nothing
        recs.append(clipped(3, 7, L, f))                  # both ends: the 5' clip wins
        recs.append(clipped(0, 7, L, f))
        recs.append(rd([(L, "S")], f))                    # a lone S word: the first and the last word at once
        for n5 in (BQC_CT - 1, BQC_CT, BQC_CT + 1):       # k_reads alone: 400 bases
            recs.append(clipped(n5, None, 400, f))
        for Lr in (BQC_CT - 1, BQC_CT, BQC_CT + 1):       # the difference array's words L - n3 and L, in LDS up to L = BQC_CT
            recs.append(clipped(None, 10, Lr, f))
            recs.append(clipped(None, Lr, Lr, f, body=0))
        recs.append(clipped(4, None, L, f | UNM))         # unmapped, or not on a main chromosome: nothing
        recs.append(clipped(None, 4, L, f | UNM))
        recs.append(clipped(4, None, L, f, rid=1))
        recs.append(clipped(None, 4, L, f, rid=1))
    return finish(recs)


CANCEL_K = 70


def clip_cancel(op="S"):
    """First mates: k reads of 100 bases and k of 110, each with a 3' clip of 10: word 100 of the difference array takes k times -1
    and k times +1.  Second mates: 2 k reads of 100 bases with a 3' clip of 30: word 100 nets -2 k.
    op = "I": the same reads with an insertion (and NM = its length) where the clip is: every count of the batch is the same but for
    the clips, which are gone, and the insertion histogram, where a read moves from one bin to another."""
    recs = []
    nm = (lambda n: 0) if op == "S" else (lambda n: n)
    for i in range(CANCEL_K):
        recs.append(clipped(None, 10, 100, BASE | FIRST, op=op, nm=nm(10)))
        recs.append(clipped(None, 30, 100, BASE | LAST, op=op, nm=nm(30)))
        recs.append(clipped(None, 10, 110, BASE | FIRST, op=op, nm=nm(10)))
        recs.append(clipped(None, 30, 100, BASE | LAST, op=op, nm=nm(30)))
    return finish(recs)


# ---------------------------------------------------------------------------------------------------------------------------
# caps: hist_cap = 128
# ---------------------------------------------------------------------------------------------------------------------------
CAP = 128
OVER = {"del": dict(cigar=[(10, "M"), (CAP, "D"), (10, "M")], nm=CAP), "ins": dict(cigar=[(10, "M"), (CAP, "I"), (10, "M")], nm=CAP),
        "mm": dict(cigar=[(30, "M")], nm=CAP), "wrap": dict(cigar=[(10, "M"), (2, "D"), (10, "M")], nm=1)}  # wrap: NM < D + I


def caps_over(kind, at=25):
    """One offending read between 50 ordinary ones."""
    recs = ordinary(at) + [rd(OVER[kind]["cigar"], BASE | FIRST | REV, nm=OVER[kind]["nm"])] + ordinary(50 - at)
    return finish(recs, hist_cap=CAP)


def caps_extra_over():
    """A second NM tag whose mismatch count is hist_cap (the first one's is fine)."""
    cols, refs, opts = finish(ordinary(25) + [rd([(30, "M")], BASE | LAST, nm=3)] + ordinary(25), hist_cap=CAP)
    cols["nm_extra_read"], cols["nm_extra_val"] = np.array([25], np.uint32), np.array([CAP], np.int32)
    return cols, refs, opts


def caps():
    """The offending values where nothing looks at them, the largest legal values, a read without NM, further NM tags."""
    recs = ordinary(20)
    for kind in OVER:
        for f in (BASE | FIRST | UNM, BASE | LAST | SEC, BASE | FIRST | SUPP):
            recs.append(rd(OVER[kind]["cigar"], f, nm=OVER[kind]["nm"]))
        recs.append(rd(OVER[kind]["cigar"], BASE | LAST, rid=1, nm=OVER[kind]["nm"]))
    for f in FLAGS4:
        recs.append(rd([(10, "M"), (CAP - 1, "D"), (10, "M")], f, nm=CAP - 1))
        recs.append(rd([(10, "M"), (CAP - 1, "I"), (10, "M")], f, nm=CAP - 1))
        recs.append(rd([(30, "M")], f, nm=CAP - 1))
        recs.append(rd([(10, "M"), (3, "D"), (10, "M")], f, nm=-1))  # no NM tag: no mismatch count, the indels count
    extra_at = len(recs)
    recs.append(rd([(10, "M"), (2, "I"), (10, "M")], BASE | FIRST, nm=5))          # NM 5, then 2 + 127 and 2 + 0
    recs.append(rd([(30, "M")], BASE | LAST | SEC, nm=0))                          # a secondary read's further tag is not looked at
    recs.append(rd([(30, "M")], BASE | LAST, nm=-1))                               # no first tag, one further tag
    recs += ordinary(20)
    cols, refs, opts = finish(recs, hist_cap=CAP)
    cols["nm_extra_read"] = np.array([extra_at, extra_at, extra_at + 1, extra_at + 2], np.uint32)
    cols["nm_extra_val"] = np.array([2 + CAP - 1, 2, CAP, 64], np.int32)
    return cols, refs, opts


# ---------------------------------------------------------------------------------------------------------------------------
# flags: every combination of the bits the cascade reads
# ---------------------------------------------------------------------------------------------------------------------------
FLAG_BITS = [PR, UNM, MUNM, REV, MREV, FIRST, LAST, SEC, QCF, DUP, SUPP]
MAPQS = [0, 1, 254, 255]


def flag_values(no_mate):
    """The 2048 combinations; no_mate: those that end the run (a primary read with neither mate flag), else the others."""
    out = []
    for k in range(1 << len(FLAG_BITS)):
        f = sum(b for j, b in enumerate(FLAG_BITS) if k >> j & 1)
        if (not f & (SEC | SUPP) and not f & (FIRST | LAST)) == no_mate:
            out.append(f)
    return out


def flags(no_mate=False):
    pick = np.random.default_rng(11).integers(0, len(MAPQS), 4096).tolist()  # (not in step with the bits)
    recs = [rd([(30, "M")], BASE | f, rid=rid, mapq=MAPQS[pick[2 * k + rid]], nm=k % 3) for k, f in enumerate(flag_values(no_mate)) for rid in (0, 1)]
    return finish(recs)


# ---------------------------------------------------------------------------------------------------------------------------
# flush_reuse: a workgroup that passes from one read group's chunks to the next one's
# ---------------------------------------------------------------------------------------------------------------------------
# The processing order of a batch is its reads grouped by read group, 0 first (bqc_pipeline.cpp: host_pass), and both chunk tables
# follow it (k_prep.hip: k_build_plan), one stretch per read group:
#   k_reads   a read group's generic reads (longer than BQC_FAST_MAXLEN, or all under BQC_NO_FAST) in chunks of BQC_CHUNK_READS;
#             grid = min(n_slow / 128 + stretches + 4, 8 * CUs) (enqueue_batch, layout_batch: cs_cap); workgroup x walks the chunks
#             x, x + grid, ...
#   k_short   fast_w = ceil(longest fast read / 16) lanes per read, rpw = 64 / fast_w read slots per group, the first h0 = ceil(rpw / 2)
#             for reads with 0x40, the other h1 for the rest; per super-window of 4096 positions of the processing order
#             max(ceil(n0 / h0), ceil(n1 / h1)) groups; a read group's groups in chunks of 16 * (64 / rpw) groups (then its chunks of triplet
#             segments: none here); grid = CUs; workgroup x walks the chunks x, x + grid, ...
# A workgroup therefore meets read groups in rising order only: it cannot return to one within a launch.  What the batch does instead:
# read groups 0, 1, 2 whose reads fill even, odd and even bins again, sized so that one workgroup walks a chunk of each in one launch
# (rs_flush between them, twice), and the test submits the batch twice, which adds every group's second part on top of its first.
def chunk_lanes_reads(cols, no_fast):
    """The read group of every chunk of k_reads' table, in order."""
    slow = np.ones(len(cols["flag"]), bool) if no_fast else cols["l_seq"] > BQC_FAST_MAXLEN
    out = []
    for g in np.unique(cols["lane"]).tolist():
        out += [g] * -(-int((slow & (cols["lane"] == g)).sum()) // CHUNK_READS)
    return out


def grid_reads(cols, no_fast, n_cu):
    n_slow = len(cols["flag"]) if no_fast else int((cols["l_seq"] > BQC_FAST_MAXLEN).sum())
    return min(n_slow // CHUNK_READS + len(np.unique(cols["lane"])) + 4, READS_GRID_PER_CU * n_cu) if n_slow else 0


def chunk_lanes_short(cols):
    """The read group of every chunk of k_short's table, in order (no read has triplet segments)."""
    fast = cols["l_seq"] <= BQC_FAST_MAXLEN
    if not fast.any():
        return []
    fast_w = max(1, -(-int(cols["l_seq"][fast].max()) // LANE_CYCLES))
    rpw = 64 // fast_w
    h0, h1 = (rpw + 1) // 2, rpw // 2
    assert h1 > 0
    groups_cap = FAST_WAVES * (64 // rpw)
    out = []
    for g in np.unique(cols["lane"]).tolist():
        idx = np.flatnonzero(cols["lane"] == g)  # (stable: the group's reads in stream order)
        groups = 0
        for at in range(0, len(idx), SW_READS):
            sw = idx[at:at + SW_READS]
            n0 = int((fast[sw] & ((cols["flag"][sw] & FIRST) != 0)).sum())
            n1 = int(fast[sw].sum()) - n0
            groups += max(-(-n0 // h0), -(-n1 // h1))
        out += [g] * -(-groups // groups_cap)
    return out


def walks(chunk_lanes, grid):
    """Per workgroup the read groups it meets, in order, without repeats of the one it is in."""
    out = []
    for x in range(min(grid, len(chunk_lanes))):
        seq = []
        for g in chunk_lanes[x::grid]:
            if not seq or seq[-1] != g:
                seq.append(g)
        out.append(seq)
    return out


def flush_pattern(odd):
    """16 reads, first and second mates in turn, whose every LDS word has an even (odd = 0) or an odd index: read length, mapping quality,
    mismatches, deletions, insertions, the 5' clip's length, both words of the 3' clip's difference array, |tlen|."""
    e = odd
    kinds = [([(20, "M")], [(8, "M"), (1, "I"), (4, "M"), (1, "D"), (8, "M")]),
             ([(2, "S"), (8, "M"), (2, "I"), (4, "M"), (2, "D"), (6, "M")], [(1, "S"), (8, "M"), (3, "I"), (4, "M"), (1, "D"), (5, "M")]),
             ([(18, "M"), (2, "S")], [(6, "M"), (1, "I"), (4, "M"), (3, "D"), (8, "M"), (2, "S")])]
    recs = []
    for k, pair in enumerate(kinds):
        ops = pair[e]
        indel = sum(n for n, c in ops if c in "DI")
        for f in FLAGS4:
            recs.append(rd(oriented(ops, f), f, mapq=40 + 2 * k + e, nm=indel + 2 * k + e, tlen=(100, RS_INS - 2, RS_INS)[k] + e))
    for f in FLAGS4:
        recs.append(rd([], f | UNM, L=20 + e, mapq=0, tlen=0))
    cols = synth.concat(recs)
    assert ((cols["l_seq"] & 1) == e).all() and ((cols["flag"][0::2] & FIRST) != 0).all() and ((cols["flag"][1::2] & LAST) != 0).all()
    return cols


def flush_sizes(n_cu):
    """Reads of the read groups 0, 1, 2: an eighth of a round of k_short's workgroups, then a whole round twice (1024 reads fill a chunk
    of k_short and eight chunks of k_reads)."""
    return [1024 * max(1, n_cu // 8), 1024 * n_cu, 1024 * n_cu]


def flush_reuse(n_cu, shuffled=False):
    pat = synth.concat([flush_pattern(0), flush_pattern(1)])
    sizes = flush_sizes(n_cu)
    idx = np.concatenate([np.arange(n) % 16 + 16 * (g & 1) for g, n in enumerate(sizes)])
    lane = np.concatenate([np.full(n, g, np.uint8) for g, n in enumerate(sizes)])
    if shuffled:  # mates still in turn: pairs of reads are permuted
        perm = np.random.default_rng(5).permutation(len(idx) // 2)
        perm = (2 * perm[:, None] + np.arange(2)[None, :]).reshape(-1)
        idx, lane = idx[perm], lane[perm]
    cols = lane_limit.take(pat, idx)
    cols["lane"] = lane
    cols["pos"] = (np.arange(len(idx)) // 8).astype(np.int32)
    return cols, REFS, dict(OPTS, n_lanes=3)


def flush_crossings(cols, n_cu):
    """(workgroups of k_short, workgroups of k_reads under BQC_NO_FAST) that walk chunks of read group 0, then 1, then 2 in one launch."""
    short = [x for x, seq in enumerate(walks(chunk_lanes_short(cols), n_cu)) if seq == [0, 1, 2]]
    reads = [x for x, seq in enumerate(walks(chunk_lanes_reads(cols, True), grid_reads(cols, True, n_cu))) if seq == [0, 1, 2]]
    return short, reads


# ---------------------------------------------------------------------------------------------------------------------------
# the batches by name: (maker, the error code the run must end with)
# ---------------------------------------------------------------------------------------------------------------------------
BATCHES = {
    "bins": (bins, 0),
    "insert_2000": (lambda: insert(2000), 0),     # the clamp bin lies outside the LDS table
    "insert_500": (lambda: insert(500), 0),       # ... inside it
    "insert_1023": (lambda: insert(1023), 0),     # ... is its last word
    "lengths": (lengths, 0),
    "lengths_over": (lengths_over, ERR_RANGE),
    "clips": (clips, 0),
    "clip_cancel": (clip_cancel, 0),
    "caps": (caps, 0),
    "caps_del": (lambda: caps_over("del"), ERR_RANGE),
    "caps_ins": (lambda: caps_over("ins"), ERR_RANGE),
    "caps_mm": (lambda: caps_over("mm"), ERR_RANGE),
    "caps_wrap": (lambda: caps_over("wrap"), ERR_RANGE),
    "caps_extra": (caps_extra_over, ERR_RANGE),
    "flags": (flags, 0),
    "flags_no_mate": (lambda: flags(True), ERR_NO_MATE_FLAG),
}
SPLIT = ["bins", "insert_2000", "clips"]  # also in two submits, cut at an odd read


@functools.lru_cache(maxsize=None)
def made(name):
    cols, refs, opts = BATCHES[name][0]()
    for v in cols.values():
        v.setflags(write=False)
    return cols, refs, opts


@functools.lru_cache(maxsize=None)
def made_flush(n_cu, shuffled=False):
    cols, refs, opts = flush_reuse(n_cu, shuffled)
    for v in cols.values():
        v.setflags(write=False)
    return cols, refs, opts


@functools.lru_cache(maxsize=None)
def clean():
    """The batch a context takes after an error and a reset."""
    return finish(ordinary(97))
