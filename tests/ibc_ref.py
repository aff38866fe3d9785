"""The indels by cycle and by length, restated from include/bamqc.h (section "indels by cycle and by length"), not from the kernel:
`table` is the plain loop — read by read, operation by operation, in Python integers — and `table_fast` its vectorised twin for the
larger cases.  Both give the module's words of the state vector as an (n_lanes, 2, 3 N + 128) uint64 array: per read group and mate
the rows E, IC, DC of N cycles, then IL and DL of 64 length bins."""
import numpy as np

K = 64
E_ROW, IC_ROW, DC_ROW = 0, 1, 2
QUERY_OPS = (0, 1, 4, 7, 8)  # M, I, S, =, X consume bases of the read; of these I is the event


def mate_words(N):
    return 3 * N + 2 * K


def examined(flag, lane, L, nc, n_lanes):
    return (flag & 0x900) == 0 and (flag & 0xC0) != 0 and (flag & 0x4) == 0 and nc > 0 and L > 0 and lane < n_lanes


def events(L, rev, cigar):
    """The events of one read of L bases with the CIGAR words `cigar` (stored order): [(kind, cycle, length)], kind 0 insertion,
    1 deletion — before the capacity is applied."""
    out, j = [], 0
    for wd in cigar:
        op, n = int(wd) & 15, int(wd) >> 4
        if op in (0, 7, 8, 4):
            j += n
        elif op == 1:
            if n >= 1 and j + n <= L:
                out.append((0, L - j - n if rev else j, n))
            j += n
        elif op == 2:
            if n >= 1 and 0 < j < L:
                out.append((1, L - 1 - j if rev else j - 1, n))
    return out


def table(cols, n_lanes, N):
    T = np.zeros((n_lanes, 2, mate_words(N)), np.uint64)
    first = 0
    for i in range(len(cols["flag"])):
        f, g, L, nc = int(cols["flag"][i]), int(cols["lane"][i]), int(cols["l_seq"][i]), int(cols["n_cigar"][i])
        cig = cols["cigar"][first:first + nc]
        first += nc
        if not examined(f, g, L, nc, n_lanes):
            continue
        m = 0 if f & 0x40 else 1
        T[g, m, E_ROW * N + min(L, N) - 1] += 1
        for kind, c, n in events(L, bool(f & 0x10), cig):
            if c >= N:
                continue
            T[g, m, (IC_ROW + kind) * N + c] += 1
            T[g, m, 3 * N + kind * K + min(n, K) - 1] += 1
    return T


def table_fast(cols, n_lanes, N):
    f = cols["flag"].astype(np.int64)
    g = cols["lane"].astype(np.int64)
    L = cols["l_seq"].astype(np.int64)
    nc = cols["n_cigar"].astype(np.int64)
    ok = ((f & 0x900) == 0) & ((f & 0xC0) != 0) & ((f & 0x4) == 0) & (nc > 0) & (L > 0) & (g < n_lanes)
    mate = np.where(f & 0x40, 0, 1)
    rev = (f & 0x10) != 0
    mw = mate_words(N)
    T = np.zeros(n_lanes * 2 * mw, np.int64)
    base = (np.where(ok, g, 0) * 2 + mate) * mw
    np.add.at(T, (base + np.minimum(L, N) - 1)[ok], 1)
    w = cols["cigar"].astype(np.int64)
    op, n = w & 15, w >> 4
    read = np.repeat(np.arange(len(L)), nc)
    q = np.where(np.isin(op, QUERY_OPS), n, 0)
    excl = np.cumsum(q) - q  # (int64: 2^32 words of 2^28 stay below 2^63)
    j = excl - excl[(np.cumsum(nc) - nc)[read]]
    Lr, rv = L[read], rev[read]
    ins = (op == 1) & (n >= 1) & (j + n <= Lr)
    dele = (op == 2) & (n >= 1) & (j > 0) & (j < Lr)
    c = np.where(op == 1, np.where(rv, Lr - j - n, j), np.where(rv, Lr - 1 - j, j - 1))
    ev = (ins | dele) & ok[read] & (c < N)
    kind = (op == 2).astype(np.int64)
    np.add.at(T, (base[read] + (IC_ROW + kind) * N + c)[ev], 1)
    np.add.at(T, (base[read] + 3 * N + kind * K + np.minimum(n, K) - 1)[ev], 1)
    return T.astype(np.uint64).reshape(n_lanes, 2, mw)


def views(T, lane, mate):
    """What bqc_indel_by_cycle gives for the (lane, mate): (reads_by_length, insertions, deletions, insertion_lengths,
    deletion_lengths), the first three n_cycles long."""
    w = T[lane, mate]
    N = (len(w) - 2 * K) // 3
    nz = np.flatnonzero(w[:N])
    nc = int(nz[-1]) + 1 if len(nz) else 0
    return w[:nc], w[N:N + nc], w[2 * N:2 * N + nc], w[3 * N:3 * N + K], w[3 * N + K:]


def text(T, sample, names, lane_index):
    """The `.ibc` of bqc_write_indel_by_cycle for the table T, lanes `lane_index` under the names `names`."""
    out = []
    for name, l in zip(names, lane_index):
        out += ["sample_id %s" % sample, "lane %s" % name]
        for m, sfx in enumerate(("first", "second")):
            e, ic, dc, il, dl = views(T, l, m)
            for key, v in (("indel_reads_by_length", e), ("insertions_by_position", ic), ("deletions_by_position", dc),
                           ("insertion_length_histogram", il), ("deletion_length_histogram", dl)):
                out.append(" ".join(["%s_%s" % (key, sfx)] + [str(int(x)) for x in v]))
    return "\n".join(out) + "\n"
