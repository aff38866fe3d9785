"""Test infrastructure for the GC bias kernels (no GPU use): a plain restatement of the launch arithmetic of k_gcb.hip — the shares of
k_gcb_genome, the grid, a workgroup's share and its steps of k_gcb_reads — the reciprocals the kernels divide with, and the builder of
column dicts from reads given one by one.  tests/test_gc_bias_cpu.py holds the constants against the kernel's #define lines.

k_gcb_genome: a share is GG_SHARE consecutive window starts of one contig; thread t of a workgroup scans the dwords GG_ITEMS t ...
of the share's bytes, and takes the starts t, t + GG_THREADS, ... of the share.  k_gcb_reads: about one workgroup per CU; a
workgroup walks its share ceil(n_reads / grid) of the processing order in steps of GR_STEP reads."""
import numpy as np

from tests.cycle_steps import ceil_div, shares, steps

GG_THREADS = 256
GG_ITEMS = 9
GG_SHARE = 8192
GR_STEP = 1024       # reads of a k_gcb_reads step (GR_THREADS)
WG_READS = 256       # a launch has no more workgroups than ceil(reads / 256)
W_MIN, W_MAX = 20, 1000
P, REV, FIRST, LAST, MAIN = 0x1, 0x10, 0x40, 0x80, 0x1000


def reads_launch(n_reads, n_cu):
    """bqc_launch_gcb_reads: dict(grid, per, shares, steps: the step count of every workgroup)."""
    grid = max(1, min(n_cu, ceil_div(n_reads, WG_READS)))
    per, sh = shares(n_reads, grid)
    return dict(grid=grid, per=per, shares=sh, steps=[len(steps(b, e, GR_STEP)) for b, e in sh])


def genome_shares(lens, W):
    """The shares of a genome table's launch: [(rid, first start, starts)] over the contigs of at least W bases (None: not given)."""
    out = []
    for rid, n in enumerate(lens):
        if n is None or n < W:
            continue
        for s0 in range(0, n - W + 1, GG_SHARE):
            out.append((rid, s0, min(GG_SHARE, n - W + 1 - s0)))
    return out


def reciprocals(W):
    """ceil(2^32 / (W - n)) for n = 0..4: the kernels take floor(100 gc / (W - n)) as the high word of 100 gc times this."""
    return [((1 << 32) + (W - n) - 1) // (W - n) for n in range(5)]


def cols_of(reads):
    """Column dict of reads given as dicts: pos, cigar [(length, op), ...] and optionally flag (default: paired, first mate, mate on a
    main chromosome), rid (0), lane (0), L (the CIGAR's query length), qual (an array of L bytes, a number for all of them, or None:
    no qualities — 0x8000 and bytes of 0xFF).  Every base is A; mapq 0 and no proper-pair flag (no read is triplet-eligible)."""
    n = len(reads)
    L, flag, ncig, cig, qual = [], [], [], [], []
    for r in reads:
        words = [(ln << 4) | op for ln, op in r.get("cigar", [])]
        l = r.get("L", sum(ln for ln, op in r.get("cigar", []) if op in (0, 1, 4, 7, 8)))
        q = r.get("qual", 30)
        f = r.get("flag", P | FIRST | MAIN)
        if q is None:
            f |= 0x8000
            q = 0xFF
        q = np.full(l, q, np.uint8) if np.isscalar(q) else np.asarray(q, np.uint8)
        assert len(q) == l
        L.append(l); flag.append(f); ncig.append(len(words)); cig += words; qual.append(q)
    L = np.array(L, np.int64)
    return dict(flag=np.array(flag, np.uint16), mapq=np.zeros(n, np.uint8), lane=np.array([r.get("lane", 0) for r in reads], np.uint8),
                rid=np.array([r.get("rid", 0) for r in reads], np.int32), pos=np.array([r["pos"] for r in reads], np.int32),
                tlen=np.zeros(n, np.int32), nm=np.full(n, -1, np.int32), as_=np.full(n, 100, np.int32), l_seq=L.astype(np.uint32),
                n_cigar=np.array(ncig, np.uint16), seq=np.full(int(((L + 1) // 2).sum()), 0x11, np.uint8),
                qual=np.concatenate(qual + [np.zeros(0, np.uint8)]), cigar=np.array(cig, np.uint32))


def cols_flat(pos, flag, L, lane=None, rid=None, qual=30):
    """cols_of for many reads with the CIGAR LM each (arrays; qual: one byte value for all, or the flat array of sum(L) bytes)."""
    pos, L = np.asarray(pos, np.int64), np.asarray(L, np.int64)
    n = len(pos)
    q = np.full(int(L.sum()), qual, np.uint8) if np.isscalar(qual) else np.asarray(qual, np.uint8)
    return dict(flag=np.asarray(flag, np.uint16), mapq=np.zeros(n, np.uint8), lane=np.zeros(n, np.uint8) if lane is None else np.asarray(lane, np.uint8),
                rid=np.zeros(n, np.int32) if rid is None else np.asarray(rid, np.int32), pos=pos.astype(np.int32), tlen=np.zeros(n, np.int32),
                nm=np.full(n, -1, np.int32), as_=np.full(n, 100, np.int32), l_seq=L.astype(np.uint32), n_cigar=np.ones(n, np.uint16),
                seq=np.full(int(((L + 1) // 2).sum()), 0x11, np.uint8), qual=q, cigar=(L << 4).astype(np.uint32))
