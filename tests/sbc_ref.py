"""The substitutions by sequence context and by cycle (--substitutions) restated from their definition in include/bamqc.h: table()
is plain Python loops over the reads, their CIGAR operations and their bases; table_fast() is the same definition vectorised in numpy
for batches of hundreds of thousands of reads.  tests/test_substitutions_cpu.py holds the two against each other on every fixture
both can handle.  Shares nothing with the kernel (bamqc_amd/csrc/k_sbc.hip)."""
import numpy as np

XW = 512  # words of X of a lane and mate: [2 strands][64 contexts][4 read bases]
_CODE = {1: 0, 2: 1, 4: 2, 8: 3}  # the read's 4-bit code -> A C G T; everything else is not examined
_CODE_NP = np.full(16, -1, np.int64)
_CODE_NP[[1, 2, 4, 8]] = np.arange(4)


def mate_words(N):
    return XW + 16 * N


def _lists(cols_list):
    return [cols_list] if isinstance(cols_list, dict) else cols_list


def table(cols_list, refs, n_lanes, N, Q=20, MQ=30):
    """(T, no_context): T[lane][mate][512 + 16 N] as the state vector holds it — X [s][ctx][b'] then Y [c][t'][b'] — and
    no_context[lane][mate], the examined pairs that enter Y and not X.  refs: the contigs as the context holds them, a list by rid of
    Dna5 arrays (its length is n_refs), None for a contig that was never set."""
    T = np.zeros((n_lanes, 2, mate_words(N)), np.uint64)
    miss = np.zeros((n_lanes, 2), np.int64)
    n_refs = len(refs)
    for cols in _lists(cols_list):
        L = cols["l_seq"].astype(np.int64)
        qo = np.cumsum(L) - L
        so = np.cumsum((L + 1) // 2) - (L + 1) // 2
        nc = cols["n_cigar"].astype(np.int64)
        co = np.cumsum(nc) - nc
        for i in range(len(L)):
            f, rid, lane, l_seq = int(cols["flag"][i]), int(cols["rid"][i]), int(cols["lane"][i]), int(L[i])
            if f & 0x900 or not f & 0xC0 or f & 0x8000 or f & 0x4 or l_seq == 0 or nc[i] == 0 or lane >= n_lanes:
                continue
            if rid < 0 or rid >= n_refs or refs[rid] is None or int(cols["mapq"][i]) < MQ:
                continue
            g = refs[rid]
            glen = len(g)
            mate = 0 if f & 0x40 else 1
            rev = (f >> 4) & 1
            row = T[lane, mate]
            j, r = 0, int(cols["pos"][i])
            for w in cols["cigar"][co[i]:co[i] + nc[i]]:
                op, n = int(w) & 15, int(w) >> 4
                if op in (0, 7, 8):
                    for t in range(max(0, min(n, l_seq - j))):  # jj < l_seq
                        jj, rr = j + t, r + t
                        if rr < 0 or rr >= glen:
                            continue
                        byte = int(cols["seq"][so[i] + jj // 2])
                        code = _CODE.get(byte & 15 if jj & 1 else byte >> 4)
                        tt = int(g[rr])
                        q = int(cols["qual"][qo[i] + jj])
                        c = l_seq - 1 - jj if rev else jj
                        if code is None or tt > 3 or q < Q or q > 222 or c >= N:
                            continue
                        b = 3 - code if rev else code
                        t_ = 3 - tt if rev else tt
                        row[XW + c * 16 + t_ * 4 + b] += 1
                        if rr < 1 or rr + 1 >= glen or g[rr - 1] > 3 or g[rr + 1] > 3:
                            miss[lane, mate] += 1
                            continue
                        before, behind = int(g[rr - 1]), int(g[rr + 1])
                        ctx = 16 * (3 - behind) + 4 * (3 - tt) + (3 - before) if rev else 16 * before + 4 * tt + behind
                        row[(rev * 64 + ctx) * 4 + b] += 1
                    j += n
                    r += n
                elif op in (1, 4):
                    j += n
                elif op in (2, 3):
                    r += n
    return T, miss


def table_fast(cols_list, refs, n_lanes, N, Q=20, MQ=30):
    """table(), vectorised: one entry per CIGAR operation with the exclusive running sums of its read's query-consuming (M I S = X)
    and reference-consuming (M D N = X) lengths; the match-like operations, cut to l_seq, become one entry per base; then the rules
    of the definition and one np.bincount per table."""
    mw = mate_words(N)
    size = n_lanes * 2 * mw
    T = np.zeros(size, np.int64)
    miss = np.zeros(n_lanes * 2, np.int64)
    n_refs = len(refs)
    ref_len = np.array([0 if r is None else len(r) for r in refs] + [0], np.int64)
    ref_set = np.array([r is not None for r in refs] + [False])
    ref_at = np.cumsum(ref_len) - ref_len + 1  # where a contig starts in `genome` (one pad entry in front, one behind)
    genome = np.concatenate([np.full(1, 4, np.int64)] + [np.asarray(r, np.int64) for r in refs if r is not None] + [np.full(1, 4, np.int64)])
    for cols in _lists(cols_list):
        L = cols["l_seq"].astype(np.int64)
        f = cols["flag"].astype(np.int64)
        nc = cols["n_cigar"].astype(np.int64)
        rid = cols["rid"].astype(np.int64)
        lane = cols["lane"].astype(np.int64)
        rid_in = np.where((rid >= 0) & (rid < n_refs), rid, n_refs)
        counted = (((f & 0x900) == 0) & ((f & 0xC0) != 0) & ((f & 0x8000) == 0) & ((f & 0x4) == 0) & ref_set[rid_in] & (nc > 0) & (L > 0) &
                   (lane < n_lanes) & (cols["mapq"].astype(np.int64) >= MQ))
        qo = np.cumsum(L) - L
        so = np.cumsum((L + 1) // 2) - (L + 1) // 2
        co = np.cumsum(nc) - nc
        w = cols["cigar"][:int(nc.sum())].astype(np.int64)
        if not len(w):
            continue
        op, n = w & 15, w >> 4
        o_read = np.repeat(np.arange(len(L)), nc)
        in_q = np.where(np.isin(op, (0, 1, 4, 7, 8)), n, 0)
        in_r = np.where(np.isin(op, (0, 2, 3, 7, 8)), n, 0)
        ex_q, ex_r = np.cumsum(in_q) - in_q, np.cumsum(in_r) - in_r
        j0 = ex_q - ex_q[co[o_read]]
        r0 = cols["pos"].astype(np.int64)[o_read] + ex_r - ex_r[co[o_read]]
        take = np.where(np.isin(op, (0, 7, 8)) & counted[o_read], np.clip(np.minimum(n, L[o_read] - j0), 0, None), 0)
        b_op = np.repeat(np.arange(len(w)), take)
        t = np.arange(int(take.sum()), dtype=np.int64) - np.repeat(np.cumsum(take) - take, take)
        b_read = o_read[b_op]
        jj, rr = j0[b_op] + t, r0[b_op] + t
        glen = ref_len[rid_in[b_read]]
        on = (rr >= 0) & (rr < glen)
        b_read, jj, rr, glen = b_read[on], jj[on], rr[on], glen[on]
        byte = cols["seq"][so[b_read] + jj // 2].astype(np.int64)
        code = _CODE_NP[np.where(jj & 1, byte & 15, byte >> 4)]
        at = ref_at[rid_in[b_read]] + rr
        g = genome[at]
        q = cols["qual"][qo[b_read] + jj].astype(np.int64)
        rev = (f[b_read] >> 4) & 1
        c = np.where(rev == 1, L[b_read] - 1 - jj, jj)
        ok = (code >= 0) & (g <= 3) & (q >= Q) & (q <= 222) & (c < N)
        b_read, rr, glen, code, at, g, rev, c = b_read[ok], rr[ok], glen[ok], code[ok], at[ok], g[ok], rev[ok], c[ok]
        lm = lane[b_read] * 2 + np.where((f[b_read] & 0x40) != 0, 0, 1)
        b = np.where(rev == 1, 3 - code, code)
        t_ = np.where(rev == 1, 3 - g, g)
        T += np.bincount(lm * mw + XW + c * 16 + t_ * 4 + b, minlength=size)
        before, behind = genome[at - 1], genome[at + 1]  # (the pad entries and a neighbouring contig are never used: rr is checked)
        has = (rr >= 1) & (rr + 1 < glen) & (before <= 3) & (behind <= 3)
        ctx = np.where(rev == 1, 16 * (3 - behind) + 4 * (3 - g) + (3 - before), 16 * before + 4 * g + behind)
        T += np.bincount((lm * mw + (rev * 64 + ctx) * 4 + b)[has], minlength=size)
        miss += np.bincount(lm[~has], minlength=n_lanes * 2)
    return T.reshape(n_lanes, 2, mw).astype(np.uint64), miss.reshape(n_lanes, 2)


def views(T_lm, N):
    """(by_context[2][64][4], by_cycle[n_cycles][4][4]) of one lane and mate, n_cycles = 1 + the highest cycle with a non-zero bin."""
    Y = T_lm[XW:].reshape(N, 16)
    nz = np.flatnonzero(Y.any(axis=1))
    nc = int(nz[-1]) + 1 if len(nz) else 0
    return T_lm[:XW].reshape(2, 64, 4), Y[:nc].reshape(nc, 4, 4)


def text(T, N, Q, MQ, sample_id, lane_names, lane_index=None):
    """The `.sbc` text: lanes in the order given; the two thresholds; per mate 64 lines of contexts for the forward and 64 for the
    reverse strand, then the base pairs by cycle, a key line with the sizes and one line of 16 counts per cycle."""
    out = []
    for k, name in enumerate(lane_names):
        l = k if lane_index is None else lane_index[k]
        out += ["sample_id " + sample_id, "lane " + name, "substitution_min_base_qual %d" % Q, "substitution_min_mapq %d" % MQ]
        for m, mate in enumerate(("first", "second")):
            X, Y = views(T[l, m], N)
            for s, strand in enumerate(("forward", "reverse")):
                for ctx in range(64):
                    name3 = "ACGT"[ctx >> 4] + "ACGT"[(ctx >> 2) & 3] + "ACGT"[ctx & 3]
                    out.append("substitutions_by_context_%s_%s %s %s" % (mate, strand, name3, " ".join(str(int(v)) for v in X[s, ctx])))
            out.append("substitutions_by_position_%s %d 16" % (mate, len(Y)))
            out += [" ".join(str(int(v)) for v in y.reshape(16)) for y in Y]
    return "\n".join(out) + "\n"
