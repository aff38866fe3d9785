"""Test infrastructure for the launch shapes of the two per-cycle kernels (no GPU use): a plain restatement of the launch arithmetic
of k_qcyc.hip and k_mbc.hip — grid, rows, a workgroup's share and its steps, the runs a read leaves in k_mbc's list and the rounds
of a step — and the builder of the step batch of tests/test_gpu_cycle_steps.py and tests/test_cycle_steps_cpu.py.

Both kernels use about one workgroup per CU; a workgroup walks its share ceil(n_reads / grid) of the processing order in steps of
MB_STEP (k_mbc) or QC_STEP (k_qcyc) reads, so a batch has a second step only when n_reads > STEP * n_cu.  The constants below are
stated once; test_cycle_steps_cpu.py holds them against the kernels' #define lines."""
import numpy as np

from tests.long_layout import reads_on_ref

MB_STEP = 768        # reads of a k_mbc step
QC_STEP = 960        # reads of a k_qcyc step
WG_READS = 256       # a launch has no more workgroups than ceil(reads / 256)
ROW_CYCLES = 256     # cycles of a k_qcyc row (QC_C; MB_C is k_mbc's tile width)
MAX_ROWS = 64        # rows of k_qcyc at the most: the last one takes whatever lies behind it
MB_RUNS = 768        # runs k_mbc's list holds
MB_U = 4             # runs whose loads a wave of k_mbc requests together
QC_U = 6             # reads whose loads a wave of k_qcyc requests together
FAST_MAXLEN = 255    # longer reads are the launcher's "long" ones (BQC_FAST_MAXLEN)

P, PR, REV, FIRST, LAST, MAIN = 0x1, 0x2, 0x10, 0x40, 0x80, 0x1000
QUALS = np.array([0, 2, 37, 63, 64, 93, 222], np.uint8)
SHORT_LENGTHS = np.array([1, 2, 3, 4, 5, 7, 8, 13, 31, 40])
N_LONG_VARIANT = 300  # reads of 300 bases in the variant "long"


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------
# the launch arithmetic, restated
# ---------------------------------------------------------------------------------------------------------------------------
def processing_order(lane):
    """The order in which the kernels take the reads: grouped by read group, stable (bqc_pipeline.cpp host_pass); a batch of one
    read group as it is."""
    return np.argsort(np.asarray(lane), kind="stable")


def shares(n_reads, grid):
    """[(begin, end)] of the workgroups 0..grid-1 of a row (begin >= n_reads: the workgroup has nothing and returns)."""
    per = ceil_div(n_reads, grid)
    return per, [(x * per, min(n_reads, x * per + per)) for x in range(grid) if x * per < n_reads]


def steps(begin, end, step):
    """The `base` of every step a workgroup makes over [begin, end)."""
    return list(range(begin, end, step))


def seams(n_reads, grid, step):
    """Positions in the processing order at which some workgroup of the row begins a step that is not its first."""
    return [b for begin, end in shares(n_reads, grid)[1] for b in steps(begin, end, step)[1:]]


def mbc_launch(n_reads, n_cu):
    """bqc_launch_mbc: dict(grid, per, shares, steps: the step count of every workgroup)."""
    grid = max(1, min(n_cu, ceil_div(n_reads, WG_READS)))
    per, sh = shares(n_reads, grid)
    return dict(grid=grid, per=per, shares=sh, steps=[len(steps(b, e, MB_STEP)) for b, e in sh])


def qcyc_launch(L, N, n_cu):
    """bqc_launch_qcyc for a batch with the read lengths L and the capacity N (qcyc_launch_counts)."""
    L = np.asarray(L, np.int64)
    long_ = L > FAST_MAXLEN
    return qcyc_launch_counts(len(L), int(long_.sum()), int(L[long_].max()) if long_.any() else 0, N, n_cu)


def qcyc_launch_counts(n, n_long, longest, N, n_cu):
    """bqc_launch_qcyc for n reads of which n_long are longer than 255 bases, the longest of them `longest`: dict(rows, g0, g1, per0,
    per1, last_width: the cycles of the last row, steps0 / steps1: the step count of every workgroup of row 0 / of a further row)."""
    top = min(N, max(longest, ROW_CYCLES) if n_long else ROW_CYCLES - 1)
    rows = min(ceil_div(top, ROW_CYCLES), MAX_ROWS)
    wsum = n + (rows - 1) * n_long
    g1 = max(1, n_cu * n_long // wsum) if rows > 1 else 1
    g0 = max(1, n_cu * n // wsum)
    g0 = max(1, min(g0, ceil_div(n, WG_READS)))
    g1 = max(1, min(g1, ceil_div(n_long, WG_READS)))
    per0, sh0 = shares(n, g0)
    per1, sh1 = shares(n, g1)
    return dict(rows=rows, g0=g0, g1=g1, per0=per0, per1=per1, last_width=top - (rows - 1) * ROW_CYCLES,
                steps0=[len(steps(b, e, QC_STEP)) for b, e in sh0], steps1=[len(steps(b, e, QC_STEP)) for b, e in sh1] if rows > 1 else [])


def mbc_runs(cols, ref_lens, N):
    """Runs per read as k_mbc's walk leaves them: one per match-like operation (M, =, X) of a counted read whose stored positions,
    cut to the read, to [0, len) of the contig and to the cycles below N, are not empty.  ref_lens: by rid, 0 for a contig not set."""
    L = cols["l_seq"].astype(np.int64)
    f = cols["flag"].astype(np.int64)
    nc = cols["n_cigar"].astype(np.int64)
    rid = cols["rid"].astype(np.int64)
    lens = np.array(list(ref_lens) + [0], np.int64)
    rid_in = np.where((rid >= 0) & (rid < len(ref_lens)), rid, len(ref_lens))
    counted = ((f & 0x900) == 0) & ((f & 0xC0) != 0) & ((f & 0x8000) == 0) & ((f & 0x4) == 0) & (L > 0) & (nc > 0) & (lens[rid_in] > 0)
    w = cols["cigar"].astype(np.int64)
    op, n = w & 15, w >> 4
    read = np.repeat(np.arange(len(L)), nc)
    first = (np.cumsum(nc) - nc)[read]
    dq = np.where(np.isin(op, (0, 1, 4, 7, 8)), n, 0)
    dr = np.where(np.isin(op, (0, 2, 3, 7, 8)), n, 0)
    j = (np.cumsum(dq) - dq) - (np.cumsum(dq) - dq)[first]
    g = cols["pos"].astype(np.int64)[read] + (np.cumsum(dr) - dr) - (np.cumsum(dr) - dr)[first]
    posv = g - j
    lo = np.maximum(j, np.maximum(-posv, 0))
    hi = np.minimum(np.minimum(j + n, L[read]), np.maximum(lens[rid_in[read]] - posv, 0))
    rev = (f[read] & 0x10) != 0
    lo = np.where(rev, np.maximum(lo, L[read] - N), lo)
    hi = np.where(rev, hi, np.minimum(hi, N))
    run = np.isin(op, (0, 7, 8)) & counted[read] & (lo < hi)
    return np.bincount(read[run], minlength=len(L))


def mbc_rounds(runs, lane):
    """The rounds of one k_mbc step whose threads hold `runs` runs each, of the read groups `lane`: a lower bound of their number
    that holds however the slots of the list are handed out — every round takes at most MB_RUNS runs, and at most MB_RUNS of one
    thread — and the read groups of each round when the threads that still have runs take their slots in turn (the waves of a
    workgroup run the filling loop side by side).  -> (lower bound, [set of read groups per round])."""
    left = np.asarray(runs, np.int64).copy()
    lane = np.asarray(lane)
    bound = max(ceil_div(int(left.sum()), MB_RUNS), ceil_div(int(left.max()), MB_RUNS)) if len(left) and left.sum() else 0
    rounds = []
    while left.sum():
        free, groups = MB_RUNS, set()
        while free and left.sum():
            have = np.flatnonzero(left)[:free]  # one slot each, in thread order, until the list is full
            k = min(int(left[have].min()), max(1, free // len(have)))
            left[have] -= k
            free -= k * len(have)
            groups |= set(lane[have].tolist())
        rounds.append(groups)
    return bound, rounds


# ---------------------------------------------------------------------------------------------------------------------------
# the step batch
# ---------------------------------------------------------------------------------------------------------------------------
def _lengths(n, variant, seed):
    rng = np.random.default_rng(seed)
    L = SHORT_LENGTHS[rng.integers(0, len(SHORT_LENGTHS), n)]
    rare = np.arange(n) % 64 == 17
    L[rare] = np.where(rng.random(int(rare.sum())) < 0.5, 150, 255)
    if variant == "long":
        L[np.linspace(0, n - 1, N_LONG_VARIANT + 2).astype(np.int64)[1:-1]] = 300
    return L


def step_layout(n_cu, variant, N):
    """The size, the lengths and the read-group column of the step batch for a card of n_cu CUs, and the launches it gets at the
    capacity N (which enters k_qcyc's grid where it cuts the rows: N = 64 leaves the variant "long" one row).
    n: 2 * 960 * n_cu + 977, or as many more as it takes until the LAST workgroup of both kernels makes three steps as well (the
    last share is the shortest: per * grid - n reads short of the others').  Read groups 0..3, non-decreasing; the changes lie on
    a k_mbc step seam of a workgroup near n_cu // 3, on a k_qcyc row-0 step seam of a workgroup near 2 * n_cu // 3, and in the
    middle of a step of both kernels."""
    assert variant in ("short", "long")
    n = 2 * QC_STEP * n_cu + 977
    n_long, longest = (N_LONG_VARIANT, 300) if variant == "long" else (0, 0)
    while True:
        mb, qc = mbc_launch(n, n_cu), qcyc_launch_counts(n, n_long, longest, N, n_cu)
        if min(mb["steps"]) >= 3 and min(qc["steps0"]) >= 3:
            break
        n += 1
    L = _lengths(n, variant, 4100 + n_cu)
    assert qcyc_launch(L, N, n_cu) == qc
    mb_seams, qc_seams = seams(n, mb["grid"], MB_STEP), seams(n, qc["g0"], QC_STEP)
    c1 = (n_cu // 3) * mb["per"] + MB_STEP
    c2 = (2 * qc["g0"] // 3) * qc["per0"] + QC_STEP
    if c2 <= c1:
        c2 += QC_STEP
    near = np.array(sorted(set(mb_seams) | set(qc_seams) | {b for b, e in mb["shares"]} | {b for b, e in shares(n, qc["g0"])[1]}))
    c3 = (c2 + n) // 2
    while np.abs(near - c3).min() < 100:
        c3 += 1
    assert 0 < c1 < c2 < c3 < n
    lane = np.zeros(n, np.uint8)
    for c in (c1, c2, c3):
        lane[c:] += 1
    return dict(n=n, n_cu=n_cu, variant=variant, N=N, L=L, lane=lane, changes=(c1, c2, c3), mbc=mb, qcyc=qc, mbc_seams=mb_seams, qcyc_seams=qc_seams)


def step_batch(lay):
    """The batch of a step_layout -> (cols, ref); its content depends on the layout's n_cu, variant, n and changes alone.  Reads copied from one contig of about 2 M bases at sorted positions, both strands and both mates,
    qualities of QUALS, mapq 30 (no read is eligible for the triplet counters).  Every read of 8 bases and more carries the CIGAR
    aM 1I bM — two runs — while its bases are the contig's as they lie: behind the insertion they are shifted by one against the
    genome, which fills M."""
    n, L = lay["n"], lay["L"]
    rng = np.random.default_rng(4200 + lay["n_cu"])
    ref = rng.integers(0, 4, 2_000_000).astype(np.uint8)
    pos = np.sort(rng.integers(0, len(ref) - 400, n))
    flag = (P | PR | MAIN | np.where(rng.random(n) < 0.5, REV, 0) | np.where(rng.random(n) < 0.5, FIRST, LAST)).astype(np.uint16)
    qual = QUALS[rng.integers(0, len(QUALS), int(L.sum()))]
    cols = reads_on_ref(ref, pos, L, flag, qual, lane=lay["lane"])
    ins = L >= 8
    a = 1 + (rng.random(n) * (L - 2)).astype(np.int64)  # 1 <= a <= L - 2
    ncig = np.where(ins, 3, 1)
    cig = np.zeros(int(ncig.sum()), np.int64)
    at = np.cumsum(ncig) - ncig
    cig[at[~ins]] = L[~ins] << 4
    cig[at[ins]] = a[ins] << 4
    cig[at[ins] + 1] = (1 << 4) | 1
    cig[at[ins] + 2] = (L[ins] - 1 - a[ins]) << 4
    cols["cigar"], cols["n_cigar"] = cig.astype(np.uint32), ncig.astype(np.uint16)
    cols["nm"] = ins.astype(np.int32)
    cols["mapq"][:] = 30
    return cols, ref


def assert_step_layout(lay, cols, ref_len):
    """The layout the step batch was built for, from the restated arithmetic: at least 3 steps for every workgroup of both kernels
    (every row of k_qcyc), more than MB_RUNS runs in each full step of k_mbc, the read-group changes where intended.  -> the fewest
    runs of a full k_mbc step."""
    mb, qc = lay["mbc"], lay["qcyc"]
    assert len(mb["steps"]) == mb["grid"] and len(qc["steps0"]) == qc["g0"]  # (no workgroup without reads)
    assert min(mb["steps"]) >= 3 and min(qc["steps0"]) >= 3 and (not qc["steps1"] or min(qc["steps1"]) >= 3), describe(lay)
    assert qc["rows"] == (2 if lay["variant"] == "long" and lay["N"] > ROW_CYCLES else 1) and qc["g1"] <= 2
    assert np.array_equal(cols["l_seq"], lay["L"]) and np.array_equal(cols["lane"], lay["lane"])
    runs = np.concatenate([[0], np.cumsum(mbc_runs(cols, [ref_len], lay["N"]))])
    full = [b for begin, end in mb["shares"] for b in steps(begin, end, MB_STEP) if b + MB_STEP <= end]
    assert len(full) >= 2 * mb["grid"]
    fewest = int(min(runs[b + MB_STEP] - runs[b] for b in full))
    assert fewest > MB_RUNS, fewest
    c1, c2, c3 = lay["changes"]
    assert np.array_equal(np.flatnonzero(np.diff(cols["lane"].astype(np.int64))) + 1, [c1, c2, c3])  # non-decreasing: stream order is processing order
    assert np.array_equal(processing_order(cols["lane"]), np.arange(lay["n"]))
    starts = {b for b, e in mb["shares"]} | {b for b, e in shares(lay["n"], qc["g0"])[1]}
    assert c1 in lay["mbc_seams"] and c1 not in starts and c1 // mb["per"] == lay["n_cu"] // 3
    assert c2 in lay["qcyc_seams"] and c2 not in starts and c2 // qc["per0"] == 2 * qc["g0"] // 3
    assert c3 not in lay["mbc_seams"] and c3 not in lay["qcyc_seams"] and c3 not in starts
    return fewest


def describe(lay):
    mb, qc = lay["mbc"], lay["qcyc"]
    return ("n %d; k_mbc grid %d per %d steps %d..%d; k_qcyc rows %d g0 %d per %d steps %d..%d, g1 %d per %d steps %s; read-group changes at %s" % (
        lay["n"], mb["grid"], mb["per"], min(mb["steps"]), max(mb["steps"]), qc["rows"], qc["g0"], qc["per0"], min(qc["steps0"]), max(qc["steps0"]),
        qc["g1"], qc["per1"], ("%d..%d" % (min(qc["steps1"]), max(qc["steps1"])) if qc["steps1"] else "-"), list(lay["changes"])))
