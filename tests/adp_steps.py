"""Test infrastructure for the adapter-by-cycle kernel (no GPU use): a plain restatement of the launch arithmetic of k_adp.hip — grid,
a workgroup's share and its steps — the builder of column dicts from reads given as strings or as flat nibble arrays, and the step
batch of tests/test_gpu_adapter_by_cycle.py.

k_adp uses about one workgroup per CU; a workgroup walks its share ceil(n_reads / grid) of the processing order in steps of AD_STEP
reads, so a batch has a second step only when n_reads > AD_STEP * n_cu.  tests/test_adapter_by_cycle_cpu.py holds the constants
against the kernel's #define lines."""
import numpy as np

from tests.cycle_steps import ceil_div, seams, shares, steps

AD_STEP = 1024       # reads of a k_adp step (AD_THREADS)
AD_C = 1024          # cycles of the LDS tile
WG_READS = 256       # a launch has no more workgroups than ceil(reads / 256)
CODES = "=ACMGRSVTWYHKDBN"
COMPLEMENT = str.maketrans("ACGT", "TGCA")
P, REV, FIRST, LAST, MAIN = 0x1, 0x10, 0x40, 0x80, 0x1000


def adp_launch(n_reads, n_cu):
    """bqc_launch_adp: dict(grid, per, shares, steps: the step count of every workgroup)."""
    grid = max(1, min(n_cu, ceil_div(n_reads, WG_READS)))
    per, sh = shares(n_reads, grid)
    return dict(grid=grid, per=per, shares=sh, steps=[len(steps(b, e, AD_STEP)) for b, e in sh])


def as_stored(cycles, rev):
    """A read given in sequencing orientation as it is stored: itself, or its reverse complement with 0x10."""
    return cycles[::-1].translate(COMPLEMENT) if rev else cycles


def cols_of_nibbles(nib, L, flag, lane=None):
    """Column dict of reads whose 4-bit codes lie back to back in `nib` (sum(L) entries): every read mapped at a position of its own
    on contig 0 (non-decreasing, eight reads a position), CIGAR LM, Phred 30, not a proper pair (no read is triplet-eligible).
    -> (cols, the length a contig must have)."""
    L = np.asarray(L, np.int64)
    n = len(L)
    lp = L + (L & 1)
    padded = np.zeros(int(lp.sum()), np.uint8)
    padded[np.arange(int(L.sum())) + np.repeat((np.cumsum(lp) - lp) - (np.cumsum(L) - L), L)] = nib
    has = L > 0
    cols = dict(flag=np.asarray(flag, np.uint16), mapq=np.full(n, 60, np.uint8), lane=np.zeros(n, np.uint8) if lane is None else np.asarray(lane, np.uint8),
                rid=np.zeros(n, np.int32), pos=(np.arange(n) // 8).astype(np.int32), tlen=np.full(n, 300, np.int32), nm=np.zeros(n, np.int32),
                as_=np.full(n, 100, np.int32), l_seq=L.astype(np.uint32), n_cigar=has.astype(np.uint16), seq=(padded[0::2] << 4) | padded[1::2],
                qual=np.full(int(L.sum()), 30, np.uint8), cigar=(L[has] << 4).astype(np.uint32))
    return cols, n // 8 + int(L.max() if n else 0) + 64


def cols_of(reads, lane=None):
    """cols_of_nibbles for reads given as [(stored string over CODES, flag), ...]."""
    lut = np.zeros(256, np.uint8)
    for i, ch in enumerate(CODES):
        lut[ord(ch)] = i
    text = "".join(s for s, f in reads)
    return cols_of_nibbles(lut[np.frombuffer(text.encode(), np.uint8)], [len(s) for s, f in reads], [f for s, f in reads], lane)


def step_layout(n_cu):
    """The size and the read-group column of the step batch of 20-base reads for a card of n_cu CUs: more than 2 * AD_STEP * n_cu
    reads, or as many more as it takes until the LAST workgroup makes three steps as well.  Read groups 0..2, non-decreasing (stream
    order is processing order); the changes lie exactly on a step seam of a workgroup near n_cu // 3 and in the middle of a step."""
    n = 2 * AD_STEP * n_cu + 977
    while min(adp_launch(n, n_cu)["steps"]) < 3:
        n += 1
    la = adp_launch(n, n_cu)
    sm = seams(n, la["grid"], AD_STEP)
    c1 = (n_cu // 3) * la["per"] + AD_STEP
    c2 = (2 * n_cu // 3) * la["per"] + AD_STEP + 333
    lane = np.zeros(n, np.uint8)
    lane[c1:] += 1
    lane[c2:] += 1
    return dict(n=n, n_cu=n_cu, lane=lane, changes=(c1, c2), launch=la, seams=sm)


def assert_step_layout(lay):
    la, (c1, c2) = lay["launch"], lay["changes"]
    assert lay["n"] > 2 * AD_STEP * lay["n_cu"] and la["grid"] == lay["n_cu"] == len(la["steps"])
    assert min(la["steps"]) >= 3, la
    starts = {b for b, e in la["shares"]}
    assert 0 < c1 < c2 < lay["n"]
    assert c1 in lay["seams"] and c1 not in starts
    assert c2 not in lay["seams"] and c2 not in starts and min(abs(c2 - s) for s in lay["seams"]) >= 100
