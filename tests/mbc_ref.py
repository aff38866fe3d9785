"""The mismatches by cycle and base quality (--mismatch-by-cycle) restated in numpy from their definition in include/bamqc.h: a
loop over the reads of a column dict and over their CIGAR operations.  Shares nothing with the kernel (bamqc_amd/csrc/k_mbc.hip)."""
import numpy as np

QPAD = 224  # Phred 0..222, rows padded
_CODE = np.full(16, -1, np.int64)  # the read's 4-bit code -> Dna5; A C G T only, everything else -1
_CODE[[1, 2, 4, 8]] = np.arange(4)


def table(cols_list, refs, n_lanes, N):
    """T[lane][mate][0: A, 1: M][cycle][q] over the batches.  refs: the contigs as the context holds them, a list by rid of Dna5
    arrays (its length is n_refs), None for a contig that was never set."""
    T = np.zeros((n_lanes, 2, 2, N, QPAD), np.uint64)
    n_refs = len(refs)
    for cols in ([cols_list] if isinstance(cols_list, dict) else cols_list):
        L = cols["l_seq"].astype(np.int64)
        qo = np.cumsum(L) - L
        so = np.cumsum((L + 1) // 2) - (L + 1) // 2
        nc = cols["n_cigar"].astype(np.int64)
        co = np.cumsum(nc) - nc
        for i, f in enumerate(cols["flag"].astype(np.int64)):
            rid = int(cols["rid"][i])
            if f & 0x900 or not f & 0xC0 or f & 0x8000 or f & 0x4 or rid < 0 or rid >= n_refs or refs[rid] is None or nc[i] == 0:
                continue
            ref = refs[rid]
            Li = int(L[i])
            mate = 0 if f & 0x40 else 1
            lane = int(cols["lane"][i])
            j, r = 0, int(cols["pos"][i])
            for w in cols["cigar"][co[i]:co[i] + nc[i]]:
                op, n = int(w) & 15, int(w) >> 4
                if op in (0, 7, 8):
                    jj = j + np.arange(max(0, min(n, Li - j)), dtype=np.int64)  # jj < l_seq
                    rr = jj - j + r
                    on = (rr >= 0) & (rr < len(ref))
                    jj, rr = jj[on], rr[on]
                    byte = cols["seq"][so[i] + jj // 2].astype(np.int64)
                    nib = np.where(jj & 1, byte & 15, byte >> 4)
                    g = ref[rr].astype(np.int64)
                    q = cols["qual"][qo[i] + jj].astype(np.int64)
                    c = Li - 1 - jj if f & 0x10 else jj
                    ok = (_CODE[nib] >= 0) & (g <= 3) & (q <= 222) & (c < N)
                    np.add.at(T[lane, mate, 0], (c[ok], q[ok]), 1)
                    mm = ok & (_CODE[nib] != g)
                    np.add.at(T[lane, mate, 1], (c[mm], q[mm]), 1)
                    j += n
                    r += n
                elif op in (1, 4):
                    j += n
                elif op in (2, 3):
                    r += n
    return T


def table_fast(cols_list, refs, n_lanes, N):
    """table(), vectorised for batches of hundreds of thousands of reads.  One entry per CIGAR operation with the exclusive running
    sums of its read's query-consuming (M I S = X) and reference-consuming (M D N = X) lengths; the match-like operations, cut to
    l_seq, become one entry per base; then the rules of table() and one np.bincount per table.  Written from the same definition;
    tests/test_cycle_steps_cpu.py holds the two against each other bit for bit."""
    size = n_lanes * 2 * 2 * N * QPAD
    T = np.zeros(size, np.int64)
    n_refs = len(refs)
    ref_len = np.array([0 if r is None else len(r) for r in refs] + [0], np.int64)
    ref_set = np.array([r is not None for r in refs] + [False])
    ref_at = np.cumsum(ref_len) - ref_len  # where a contig starts in `genome`
    genome = np.concatenate([np.zeros(0, np.int64)] + [np.asarray(r, np.int64) for r in refs if r is not None])
    for cols in ([cols_list] if isinstance(cols_list, dict) else cols_list):
        L = cols["l_seq"].astype(np.int64)
        f = cols["flag"].astype(np.int64)
        nc = cols["n_cigar"].astype(np.int64)
        rid = cols["rid"].astype(np.int64)
        rid_in = np.where((rid >= 0) & (rid < n_refs), rid, n_refs)  # (n_refs: the entry of no contig)
        counted = ((f & 0x900) == 0) & ((f & 0xC0) != 0) & ((f & 0x8000) == 0) & ((f & 0x4) == 0) & ref_set[rid_in] & (nc > 0)
        qo = np.cumsum(L) - L
        so = np.cumsum((L + 1) // 2) - (L + 1) // 2
        co = np.cumsum(nc) - nc
        # one entry per operation
        w = cols["cigar"][:int(nc.sum())].astype(np.int64)
        op, n = w & 15, w >> 4
        o_read = np.repeat(np.arange(len(L)), nc)
        in_q = np.where(np.isin(op, (0, 1, 4, 7, 8)), n, 0)
        in_r = np.where(np.isin(op, (0, 2, 3, 7, 8)), n, 0)
        ex_q, ex_r = np.cumsum(in_q) - in_q, np.cumsum(in_r) - in_r
        j0 = ex_q - ex_q[co[o_read]]                                          # stored index of the operation's first base
        r0 = cols["pos"].astype(np.int64)[o_read] + ex_r - ex_r[co[o_read]]   # its genome position
        take = np.where(np.isin(op, (0, 7, 8)) & counted[o_read], np.clip(np.minimum(n, L[o_read] - j0), 0, None), 0)  # jj < l_seq
        # one entry per base of a match-like operation
        b_op = np.repeat(np.arange(len(w)), take)
        t = np.arange(int(take.sum()), dtype=np.int64) - np.repeat(np.cumsum(take) - take, take)
        b_read = o_read[b_op]
        jj, rr = j0[b_op] + t, r0[b_op] + t
        on = (rr >= 0) & (rr < ref_len[rid_in[b_read]])
        b_read, jj, rr = b_read[on], jj[on], rr[on]
        byte = cols["seq"][so[b_read] + jj // 2].astype(np.int64)
        code = _CODE[np.where(jj & 1, byte & 15, byte >> 4)]
        g = genome[ref_at[rid_in[b_read]] + rr]
        q = cols["qual"][qo[b_read] + jj].astype(np.int64)
        c = np.where((f[b_read] & 0x10) != 0, L[b_read] - 1 - jj, jj)
        ok = (code >= 0) & (g <= 3) & (q <= 222) & (c < N)
        mate = np.where((f & 0x40) != 0, 0, 1)
        bins = (((cols["lane"].astype(np.int64)[b_read] * 2 + mate[b_read]) * 2) * N + c) * QPAD + q  # table A; M lies N * QPAD behind
        T += np.bincount(bins[ok], minlength=size)
        T += np.bincount(bins[ok & (code != g)] + N * QPAD, minlength=size)
    return T.reshape(n_lanes, 2, 2, N, QPAD).astype(np.uint64)


def sizes(T_lm, mate_cycles):
    """(n_cycles, n_q) of one lane and mate: min(N, the mate's n_cycles in bqc_mate_counts), 1 + the highest q with a non-zero A."""
    nz = np.nonzero(T_lm[0].sum(axis=0))[0]
    return min(T_lm.shape[1], mate_cycles), (int(nz[-1]) + 1 if len(nz) else 0)


def text(T, cycles, sample_id, lane_names, lane_index=None):
    """The `.mbc` text: lanes in the order given, per mate the table A then the table M, each a key line with the sizes and one line
    of n_q counts per cycle.  cycles[lane][mate]: the mate's n_cycles in bqc_mate_counts."""
    out = []
    for k, name in enumerate(lane_names):
        l = k if lane_index is None else lane_index[k]
        out += ["sample_id " + sample_id, "lane " + name]
        for m, mate in enumerate(("first", "second")):
            nc, nq = sizes(T[l, m], int(cycles[l, m]))
            for t, key in enumerate(("aligned_bases_by_position_and_qual_", "mismatches_by_position_and_qual_")):
                out.append("%s%s %d %d" % (key, mate, nc, nq))
                if nq:
                    out += [" ".join(str(int(v)) for v in T[l, m, t, c, :nq]) for c in range(nc)]
    return "\n".join(out) + "\n"
