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
