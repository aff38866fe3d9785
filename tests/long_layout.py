"""Test infrastructure for k_long's layout limits (no GPU use): closed forms of the per-cycle counters from the input columns,
a plain restatement of which wave of which workgroup gets which read, and the batch builders of tests/test_gpu_long_layout.py
and tests/test_long_layout_cpu.py.

k_long (bamqc_amd/csrc/k_long.hip) handles every read longer than 255 bases, and every read with BQC_NO_FAST=1.  A row owns
992 cycles; a workgroup has 12 waves, wave w takes the reads w, w + 12, ... of a chunk of at most 128 reads; workgroup x of a
row takes the chunks x, x + gx, ...; a wave keeps 4-bit base counters spilled every 15 rows and 16-bit quality sums flushed
every 255 rows, per mate, and both are spilled at a read-group change whatever they hold.  The closed forms are written from the
column definitions of include/bamqc.h, not from the oracle: the two statements have to agree (test_long_layout_cpu.py) before
either is held against the kernel."""
import numpy as np

from tests import synth

KL_ROW = 992          # cycles a row of k_long owns
KL_WAVES = 12         # waves of a workgroup: wave w takes the reads w, w + 12, ... of a chunk
CHUNK_READS = 128     # reads of a generic chunk at the most (BQC_CHUNK_READS)
FAST_MAXLEN = 255     # longer reads take k_long (BQC_FAST_MAXLEN)
SPILL_ROWS = 15       # rows of a mate after which a wave spills its 4-bit base counters
QFLUSH_ROWS = 255     # ... and flushes its 16-bit quality sums
T8_SPW = 8            # 8-mer scratch rows of a workgroup; further read groups of a launch go out with atomics (BQC_T8_SPW)
WRAP_ROWS = 296       # 296 * 222 > 65535 >= 295 * 222: rows of Phred 222 a 16-bit quality sum cannot hold

P, PR, REV, FIRST, LAST, MATE_MAIN = 0x1, 0x2, 0x10, 0x40, 0x80, 0x1000
OPTS = dict(max_read_len=65536, hist_cap=4096, isize=2000)


# ---------------------------------------------------------------------------------------------------------------------------
# reads on a contig
# ---------------------------------------------------------------------------------------------------------------------------
def dna_ref(seed, n):
    return np.random.default_rng(seed).integers(0, 4, n).astype(np.uint8)  # no N: every base of a read on it is A/C/G/T


def reads_on_ref(ref, pos, L, flag, qual, cigar=None, nm=None, as_=None, lane=None):
    """Reads copied from the reference at `pos` (BAM orientation).  qual: flat uint8 (sum(L) bytes); cigar: list of
    [(n, op), ...] per read (default all-M); as_: the AS tag (default: the read's length); lane: read group (default 0)."""
    pos = np.asarray(pos, np.int64)
    L = np.asarray(L, np.int64)
    n = len(pos)
    seqs = []
    for lo in range(0, n, 100_000):  # (in slices: the index arrays stay small)
        p, l = pos[lo:lo + 100_000], L[lo:lo + 100_000]
        lp = l + (l & 1)
        k = np.arange(int(lp.sum()), dtype=np.int64) - np.repeat(np.cumsum(lp) - lp, lp)
        idx = np.minimum(np.repeat(p, lp) + k, len(ref) - 1)
        nib = np.where(k < np.repeat(l, lp), synth.NIB[ref[idx]], 0).astype(np.uint8)
        seqs.append((nib[0::2] << 4) | nib[1::2])
    if cigar is None:
        cig = (L.astype(np.uint32) << 4)  # M
        ncig = np.ones(n, np.uint16)
    else:
        cig = np.concatenate([synth.cigar_words(c) for c in cigar])
        ncig = np.array([len(c) for c in cigar], np.uint16)
    return dict(flag=np.asarray(flag, np.uint16), mapq=np.full(n, 60, np.uint8),
                lane=np.zeros(n, np.uint8) if lane is None else np.asarray(lane, np.uint8),
                rid=np.zeros(n, np.int32), pos=pos.astype(np.int32), tlen=np.full(n, 400, np.int32),
                nm=np.zeros(n, np.int32) if nm is None else np.asarray(nm, np.int32),
                as_=np.minimum(L, 1 << 30).astype(np.int32) if as_ is None else np.full(n, as_, np.int32),
                l_seq=L.astype(np.uint32), n_cigar=ncig, seq=np.concatenate(seqs), qual=np.asarray(qual, np.uint8),
                cigar=cig.astype(np.uint32))


def records(recs):
    """Column dict of hand-made reads: dicts of codes (0..4 = A C G T N, BAM orientation), qual, flag, pos, ops, nm."""
    parts = []
    for r in recs:
        L = len(r["codes"])
        parts.append(dict(flag=np.array([r["flag"]], np.uint16), mapq=np.array([60], np.uint8), lane=np.array([r.get("lane", 0)], np.uint8),
                          rid=np.zeros(1, np.int32), pos=np.array([r["pos"]], np.int32), tlen=np.array([400], np.int32),
                          nm=np.array([r.get("nm", 0)], np.int32), as_=np.array([max(L, 100)], np.int32), l_seq=np.array([L], np.uint32),
                          n_cigar=np.array([len(r["ops"])], np.uint16), seq=synth.pack_nibbles(synth.NIB[np.asarray(r["codes"], np.int64)]),
                          qual=np.asarray(r["qual"], np.uint8), cigar=synth.cigar_words(r["ops"])))
    return synth.concat(parts)


def aligned_codes(ref, pos, ops, rng):
    """The bases (BAM orientation) of a read that lies on the reference at `pos` with this CIGAR: M copies, I draws, D / N skip."""
    out, rp = [], pos
    for n, op in ops:
        if op == "M":
            out.append(ref[rp:rp + n])
            rp += n
        elif op == "I":
            out.append(rng.integers(0, 4, n).astype(np.uint8))
        else:
            assert op in "DN"
            rp += n
    assert rp <= len(ref)
    return np.concatenate(out)


def flags(rev, second):
    rev, second = np.asarray(rev, bool), np.asarray(second, bool)
    return (P | PR | MATE_MAIN | np.where(rev, REV, 0) | np.where(second, LAST, FIRST)).astype(np.uint16)


# ---------------------------------------------------------------------------------------------------------------------------
# (a) closed forms
# ---------------------------------------------------------------------------------------------------------------------------
def expected_triplets(ref, cols, phred):
    """TripletCounting.hpp:195-236 for eligible all-M reads on an N-free contig, copied from it: every position 1..L-2 of the
    read (chromPos = pos + readPos lies in [1, len - 2]) counts iff (signed char)(phred + 33) >= '5', into context
    ref[p-1] ref[p] ref[p+1], group forward / reverse x first / second, base ref[p]."""
    t = np.zeros(64 * 16, np.uint64)
    if not (20 <= phred <= 94):
        return t
    L = int(cols["l_seq"][0])
    p = cols["pos"].astype(np.int64)[:, None] + np.arange(1, L - 1)[None, :]
    ctx = ref[p - 1].astype(np.int64) * 16 + ref[p] * 4 + ref[p + 1]
    fl = cols["flag"].astype(np.int64)
    grp = np.where(fl & 0x10, 2, 0) + np.where(fl & 0x40, 0, 1)
    np.add.at(t, (ctx * 16 + grp[:, None] * 4 + ref[p]).ravel(), 1)
    return t


def triplets_all_m(ref, cols, lane=None):
    """expected_triplets for reads of several lengths (of read group `lane`): eligible, all-M, copied from the N-free contig, every
    quality in 20..94 or every quality outside (the callers' batches: asserted)."""
    L = cols["l_seq"].astype(np.int64)
    assert (cols["n_cigar"] == 1).all() and ((cols["cigar"] & 15) == 0).all() and (cols["as_"] >= 50).all()
    q = cols["qual"]
    counted = bool(((q >= 20) & (q <= 94)).all())
    assert counted or bool(((q < 20) | (q > 94)).all())
    t = np.zeros(64 * 16, np.uint64)
    sel = np.ones(len(L), bool) if lane is None else cols["lane"] == lane
    for l in np.unique(L[sel]):
        m = sel & (L == l)
        t += expected_triplets(ref, dict(l_seq=cols["l_seq"][m], pos=cols["pos"][m], flag=cols["flag"][m]), 30 if counted else 222)
    return t


_CODE_OF_NIB = np.full(16, -1, np.int64)
_CODE_OF_NIB[[1, 2, 4, 8, 15]] = np.arange(5)


def closed_forms(cols_list, n_lanes=1):
    """Per read group, from the columns alone, in int64: dnacount[0..4][cycle], qualcount[cycle], readLength, Ncount, GCcount and
    qualcount_readnr of both mates, and the read group's eightmer[65536].  Sequencing orientation: cycle j of a reverse read is
    BAM index L - 1 - j, complemented; primary records (!(flag & 0x900)) with a mate flag; an 8-mer is a window of 8 consecutive
    A/C/G/T, the first base most significant.  Array lengths as bamqc.h gives them: the mate's longest read for the per-cycle
    arrays, one more for the histograms, 0 without a read.  -> [ {name: value} per read group ], names as _abi.counts_to_dict's."""
    if isinstance(cols_list, dict):
        cols_list = [cols_list]
    cap = max(int(c["l_seq"].max()) for c in cols_list)
    dna = np.zeros((n_lanes, 2, 5, cap), np.int64)
    qual = np.zeros((n_lanes, 2, cap), np.int64)
    hist = np.zeros((3, n_lanes, 2, cap + 1), np.int64)  # readLength, Ncount, GCcount
    nr = np.zeros((n_lanes, 2), np.int64)
    longest = np.zeros((n_lanes, 2), np.int64)
    e8 = np.zeros((n_lanes, 65536), np.int64)
    for cols in cols_list:
        fl = cols["flag"].astype(np.int64)
        L = cols["l_seq"].astype(np.int64)
        lane = cols["lane"].astype(np.int64)
        n = len(L)
        assert (lane < n_lanes).all() and (L > 0).all()
        so, qo = np.cumsum((L + 1) // 2) - (L + 1) // 2, np.cumsum(L) - L
        assert not ((fl & 0x8000) != 0).any() and (cols["qual"][qo] != 0xFF).all()  # (every read has qualities)
        rid = np.repeat(np.arange(n), L)
        k = np.arange(int(L.sum()), dtype=np.int64) - qo[rid]  # BAM index
        byte = cols["seq"][so[rid] + k // 2].astype(np.int64)
        code = _CODE_OF_NIB[np.where(k & 1, byte & 15, byte >> 4)]
        assert (code >= 0).all()  # A C G T N only
        rev = (fl[rid] & REV) != 0
        cyc = np.where(rev, L[rid] - 1 - k, k)
        base = np.where(rev & (code < 4), 3 - code, code)
        use_r = ((fl & 0x900) == 0) & ((fl & 0xC0) != 0)
        mate_r = np.where(fl & FIRST, 0, 1)
        use, gl, gm = use_r[rid], lane[rid], mate_r[rid]
        np.add.at(dna, (gl[use], gm[use], base[use], cyc[use]), 1)
        np.add.at(qual, (gl[use], gm[use], cyc[use]), cols["qual"].astype(np.int64)[use])
        n_n = np.bincount(rid[use & (base == 4)], minlength=n)
        n_gc = np.bincount(rid[use & ((base == 1) | (base == 2))], minlength=n)
        for h, v in enumerate((L, n_n, n_gc)):
            np.add.at(hist[h], (lane[use_r], mate_r[use_r], v[use_r]), 1)
        np.add.at(nr, (lane[use_r], mate_r[use_r]), 1)
        np.maximum.at(longest, (lane[use_r], mate_r[use_r]), L[use_r])
        # 8-mers: the reads' bases in sequencing order, one after another (read r at qo[r] .. qo[r] + L[r])
        T = int(L.sum())
        S = np.zeros(T + 8, np.int64)
        S[qo[rid] + cyc] = base
        h8 = np.zeros(T, np.int64)
        n_in = np.zeros(T, np.int64)
        for i in range(8):
            w = S[i:i + T]
            h8 += np.where(w == 4, 0, w) << (2 * (7 - i))
            n_in += w == 4
        ok = use & (k + 8 <= L[rid]) & (n_in == 0)  # (position t of S: read rid[t], cycle k[t])
        np.add.at(e8, (gl[ok], h8[ok]), 1)
    out = []
    for l in range(n_lanes):
        d = {"eightmer": e8[l]}
        for m in range(2):
            p, nc, any_ = "r%d." % (m + 1), int(longest[l, m]), nr[l, m] > 0
            for b in range(5):
                d[p + "dnacount%d" % b] = dna[l, m, b, :nc]
            d[p + "qualcount"] = qual[l, m, :nc]
            d[p + "qualcount_readnr"] = int(nr[l, m])
            for h, name in enumerate(("readLength", "Ncount", "GCcount")):
                d[p + name] = hist[h, l, m, :nc + 1 if any_ else 0]
        out.append(d)
    return out


def diff_closed_forms(forms, counts):
    """Differences between closed_forms() and a counts dict (the oracle's or the library's), as _abi.diff_counts words them."""
    diffs = []
    if len(forms) != len(counts):
        return ["read groups: %d != %d" % (len(forms), len(counts))]
    for li, (f, c) in enumerate(zip(forms, counts)):
        for name, want in f.items():
            got = c[name]
            if isinstance(want, np.ndarray):
                got = np.asarray(got).astype(np.int64)
                if want.shape != got.shape:
                    diffs.append("lane %d %s: length %d (closed form) != %d" % (li, name, len(want), len(got)))
                elif not np.array_equal(want, got):
                    idx = np.nonzero(want != got)[0]
                    diffs.append("lane %d %s: %d bins differ, first at %d: %d (closed form) != %d" % (
                        li, name, len(idx), idx[0], int(want[idx[0]]), int(got[idx[0]])))
            elif want != got:
                diffs.append("lane %d %s: %r (closed form) != %r" % (li, name, want, got))
    return diffs


# ---------------------------------------------------------------------------------------------------------------------------
# (b) the work assignment, restated
# ---------------------------------------------------------------------------------------------------------------------------
def kl_grid(longest_slow, max_read_len, n_chunks_ub, n_cu):
    """kl_grid of k_long.hip: (gx, rows)."""
    ln = min(longest_slow, max_read_len)
    rows = -(-ln // KL_ROW) if ln else 1
    return min(max(1, n_cu // rows), n_chunks_ub), rows


def chunk_plan(cols, n_lanes=1, no_fast=False):
    """The generic chunks of a batch as the pre-pass cuts them (host_pass / plan_read_groups of bqc_pipeline.cpp, k_build_plan of
    k_prep.hip): the reads are taken read group by read group (stable; a batch of one read group as it is), every read group
    present is one stretch; a stretch's generic reads (longer than 255 bases; all with no_fast), in order, are cut every 128.
    A chunk never spans two stretches.  -> ([(read group, read indices)], the host's upper bound of the chunk count, the longest
    generic read)."""
    L = np.asarray(cols["l_seq"], np.int64)
    lane = np.asarray(cols["lane"], np.int64)
    assert (lane < n_lanes).all()
    slow = np.ones(len(L), bool) if no_fast else L > FAST_MAXLEN
    present = [l for l in range(n_lanes) if (lane == l).any()]
    if len(present) == 1:
        stretches = [(present[0], np.arange(len(L)))]
    else:
        stretches = [(l, np.nonzero(lane == l)[0]) for l in present]
    chunks = []
    for l, idx in stretches:
        s = idx[slow[idx]]
        chunks += [(l, s[k:k + CHUNK_READS]) for k in range(0, len(s), CHUNK_READS)]
    n_slow = int(slow.sum())
    return chunks, n_slow // CHUNK_READS + len(stretches) + 4, int(L[slow].max()) if n_slow else 0


def row0_runs(cols, n_cu, n_lanes=1, no_fast=False, max_read_len=65536):
    """What the waves of row 0 add between two read-group changes: workgroup x of gx takes the chunks x, x + gx, ...; wave w the
    reads w, w + 12, ... of a chunk; a read adds a row of its mate when it is primary and has a mate flag (row 0: any length);
    the accumulators are spilled, and the row counts start again, where the chunk's read group differs from the one before, and
    at the end.  -> (gx, rows, [(x, wave, mate, read group, rows added)]) — every wave and mate, zero rows included."""
    chunks, n_ub, longest = chunk_plan(cols, n_lanes, no_fast)
    gx, rows = kl_grid(longest, max_read_len, n_ub, n_cu)
    fl = np.asarray(cols["flag"], np.int64)
    use = ((fl & 0x900) == 0) & ((fl & 0xC0) != 0) & (np.asarray(cols["l_seq"], np.int64) > 0)
    first = (fl & FIRST) != 0
    runs = []
    for x in range(gx):
        cur, cnt = None, np.zeros((KL_WAVES, 2), np.int64)

        def change():
            runs.extend((x, w, m, cur, int(cnt[w, m])) for w in range(KL_WAVES) for m in range(2))
            cnt[:] = 0
        for ci in range(x, len(chunks), gx):
            lane, reads = chunks[ci]
            if lane != cur:
                if cur is not None:
                    change()
                cur = lane
            for w in range(KL_WAVES):
                r = reads[w::KL_WAVES]
                u = use[r]
                cnt[w, 0] += int((u & first[r]).sum())
                cnt[w, 1] += int((u & ~first[r]).sum())
        if cur is not None:
            change()
    return gx, rows, runs


# ---------------------------------------------------------------------------------------------------------------------------
# (c) the batches
# ---------------------------------------------------------------------------------------------------------------------------
def long_rows(n_cu):
    """Rows of the long read that shapes the grid of cases 1 and 2: 65, so that gx = n_cu // 65 is small — or fewer, until gx is no
    multiple of 3.  (Case 1 B gives the mates in the pattern 1, 1, 2 by read index; 128 = 2 and 12 = 0 modulo 3, so the reads a
    wave takes of one chunk are all of one mate, and which one moves on by 2 * gx from one chunk of the workgroup to its next:
    with gx a multiple of 3 — 256 // 65 — a wave would meet one mate only, ever.)"""
    rows = 65
    while rows > 1 and (n_cu // rows) % 3 == 0 and n_cu // rows > 0:
        rows -= 1
    return rows


def long_len(n_cu):
    return (long_rows(n_cu) - 1) * KL_ROW + 1


def _a_first(ref, pos, L, rev):
    """Positions moved on to the next one at which the read's FIRST CYCLE is an A (forward: ref[pos]; reverse: the complement of
    ref[pos + L - 1]): a wave's 4-bit counter of A at cycle 0 then counts every row, and a spill that comes a row late wraps it.
    (On random bases sixteen rows with one base at one cycle do not happen: 4^-15.)"""
    n = len(ref)

    def nxt(code, i):  # the next index >= i holding `code` (n: none)
        at = np.append(np.nonzero(ref == code)[0], n)
        return at[np.searchsorted(at, i)]
    p = np.where(rev, nxt(3, pos + L - 1) - (L - 1), nxt(0, pos))
    assert (p >= 0).all() and (p + L <= n).all()
    return p


def _long_read(ref, n_cu, phred_of):
    L = long_len(n_cu)
    return reads_on_ref(ref, [0], [L], flags([False], [False]), phred_of(L))


def case1_layout(n_cu, variant, factor):
    """Flags and lengths of case 1 (the long read first), enough for row0_runs."""
    gx = max(1, n_cu // long_rows(n_cu))
    n = CHUNK_READS * gx * factor
    rng = np.random.default_rng(1100 + (variant == "B"))
    rev = rng.random(n) < 0.5
    second = (np.arange(n) % 3 == 2) if variant == "B" else np.zeros(n, bool)  # B: 1, 1, 2, 1, 1, 2, ...
    return rev, second, dict(flag=np.concatenate([flags([False], [False]), flags(rev, second)]),
                             l_seq=np.concatenate([[long_len(n_cu)], np.full(n, 16)]), lane=np.zeros(n + 1, np.uint8))


def case1_rows(n_cu, variant, factor):
    """(gx, rows, the fewest rows of a mate that a wave of a row-0 workgroup adds) — over the mates the variant has."""
    gx, rows, runs = row0_runs(case1_layout(n_cu, variant, factor)[2], n_cu, no_fast=True)
    mates = (0, 1) if variant == "B" else (0,)
    assert len(runs) == gx * KL_WAVES * 2  # (one read group: one run per workgroup, wave and mate)
    return gx, rows, min(r[4] for r in runs if r[2] in mates)


def case1_factor(n_cu, variant):
    """60 chunks per row-0 workgroup, or as many more as it takes until every wave adds 2 * 296 rows of each mate."""
    factor = 60
    while case1_rows(n_cu, variant, factor)[2] < 2 * WRAP_ROWS:
        factor += 20
        assert factor <= 400, "case 1 does not reach the quality flush on a card with %d CUs" % n_cu
    return factor


def case1(n_cu, variant):
    """Flush cadences: one all-M read of long_len(n_cu) bases and 128 * gx * factor reads of 16 bases, all Phred 222, one read
    group, half on the reverse strand, every short read's first cycle an A.  A: first mates; B: mates 1, 1, 2 by read index."""
    ref = dna_ref(1001, 80_000)
    rev, second, lay = case1_layout(n_cu, variant, case1_factor(n_cu, variant))
    n = len(rev)
    pos = np.sort(np.random.default_rng(1002).integers(0, len(ref) - 64, n))
    pos = _a_first(ref, pos, np.full(n, 16), rev)
    short = reads_on_ref(ref, pos, np.full(n, 16), flags(rev, second), np.full(16 * n, 222, np.uint8), as_=100)
    cols = synth.concat([_long_read(ref, n_cu, lambda L: np.full(L, 222, np.uint8)), short])
    assert np.array_equal(cols["flag"], lay["flag"]) and np.array_equal(cols["l_seq"], lay["l_seq"])
    return cols, ref


CASE2_GROUPS = 24


def case2(n_cu):
    """Fill level at a read-group change: 24 read groups, group g with 150 + 3 g reads FOR THE WORKGROUP THAT TAKES ITS FIRST CHUNK
    — that is 128 * (gx - 1) + 150 + 3 g reads, so that this workgroup also takes the group's last chunk (a group of 150 reads is
    two chunks, which two workgroups would share: no wave would hold more than 11 rows) —, 16..40 bases, Phred 30..41, both
    strands, one read in seven a second mate, first cycle an A; the long read of case 1 in read group 0."""
    ref = dna_ref(1201, 80_000)
    gx = max(1, n_cu // long_rows(n_cu))
    rng = np.random.default_rng(1202)
    parts = [_long_read(ref, n_cu, lambda L: rng.integers(30, 42, L).astype(np.uint8))]
    for g in range(CASE2_GROUPS):
        n = CHUNK_READS * (gx - 1) + 150 + 3 * g
        L = rng.integers(16, 41, n)
        rev = rng.random(n) < 0.5
        second = rng.random(n) < 1 / 7
        pos = _a_first(ref, np.sort(rng.integers(0, len(ref) - 128, n)), L, rev)
        parts.append(reads_on_ref(ref, pos, L, flags(rev, second), rng.integers(30, 42, int(L.sum())).astype(np.uint8), as_=100,
                                  lane=np.full(n, g)))
    return synth.concat(parts), ref


def case2_levels(n_cu, cols):
    """(gx, the set of row counts a wave of row 0 holds of a mate at a read-group change, the changes a workgroup meets at the least)"""
    gx, rows, runs = row0_runs(cols, n_cu, n_lanes=CASE2_GROUPS, no_fast=True)
    per_wg = [len({r[3] for r in runs if r[0] == x}) for x in range(gx)]
    return gx, {r[4] for r in runs}, min(per_wg)


SEAM_LENGTHS = [KL_ROW * r + d for r in (1, 2) for d in range(-17, 18)] + [256, 257, 258]


def _seam_of(L, r):
    """The seam of the highest row <= r that lies at least 6 cycles inside the read, or None."""
    for s in range(KL_ROW * r, 0, -KL_ROW):
        if 6 <= s <= L - 6:
            return s
    return None


def case3(sub):
    """Row seams: four reads (forward / reverse x first / second mate) of each length 992 r + d, r in (1, 2), d in -17..17, and of
    256, 257, 258 bases.  a: N-free, all-M.  b: one N per read at cycle 992 r + e (sequencing orientation), e cycling through
    -9..8 by read index — where the read ends before that cycle, the same at the seam below, and without one among the last 18
    cycles —, the four cycles around every seam with qualities of {19, 20, 94, 95}.  c: a 2D, 3I or 5N after `a` bases, a within
    +-2 of the seam (of the mirrored seam L - 992 r for a reverse read; the middle of a read that has no seam inside)."""
    ref = dna_ref(1301, 60_000)
    rng = np.random.default_rng(1302 + "abc".index(sub))
    recs = []
    for li, L in enumerate(SEAM_LENGTHS):
        r = max(1, min(2, (L + 17) // KL_ROW))
        for v in range(4):
            i = 4 * li + v
            rev, second = bool(v & 1), bool(v & 2)
            qual = rng.integers(30, 42, L).astype(np.uint8)
            ops, nm = [(L, "M")], 0
            if sub == "c":
                s, off = _seam_of(L, r), i % 5 - 2
                a = L // 2 + off if s is None else (L - s if rev else s) + off
                kind = (i // 5) % 3
                ops = [[(a, "M"), (2, "D"), (L - a, "M")], [(a, "M"), (3, "I"), (L - a - 3, "M")], [(a, "M"), (5, "N"), (L - a, "M")]][kind]
                nm = (2, 3, 0)[kind]
            pos = int(rng.integers(1, len(ref) - L - 16))
            codes = aligned_codes(ref, pos, ops, rng).astype(np.int64)
            assert len(codes) == L
            if sub == "b":
                e = i % 18 - 9
                c = KL_ROW * r + e
                if c >= L:
                    c = KL_ROW * (r - 1) + e if r > 1 else L - 1 - (e + 9)
                codes[L - 1 - c if rev else c] = 4
                for s in range(KL_ROW, L + 2, KL_ROW):
                    for c in range(s - 2, min(s + 2, L)):
                        qual[L - 1 - c if rev else c] = (19, 20, 94, 95)[int(rng.integers(0, 4))]
            recs.append(dict(codes=codes, qual=qual, flag=int(flags([rev], [second])[0]), pos=pos, ops=ops, nm=nm))
    return records(recs), ref


def case3_two_batches(parts):
    """The three sub-cases (the (cols, ref) pairs of case3) one after another, cut into two batches in the middle."""
    cols = synth.concat([c for c, _ in parts])
    n = len(cols["flag"])
    return [synth.slice_batch(cols, 0, n // 2), synth.slice_batch(cols, n // 2, n)]


CHUNK_NS = [1, 2, 11, 12, 13, 23, 24, 25, 35, 36, 37, 127, 128, 129, 257]


def case4(n):
    """Chunk sizes: n reads, lengths 300 / 1100 in turn (row 1 skips every other read of a chunk), strands and mates mixed, all-M
    with a 2D in every third read."""
    ref = dna_ref(1401, 40_000)
    rng = np.random.default_rng(1402 + n)
    pos = np.sort(rng.integers(1, len(ref) - 1200, n))
    recs = []
    for i in range(n):
        L = 1100 if i & 1 else 300
        ops = [(L // 3, "M"), (2, "D"), (L - L // 3, "M")] if i % 3 == 2 else [(L, "M")]
        recs.append(dict(codes=aligned_codes(ref, int(pos[i]), ops, rng), qual=rng.integers(30, 42, L).astype(np.uint8),
                         flag=int(flags([rng.random() < 0.5], [rng.random() < 0.5])[0]), pos=int(pos[i]), ops=ops, nm=2 if i % 3 == 2 else 0))
    return records(recs), ref
