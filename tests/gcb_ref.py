"""The GC bias (--gc-bias) restated from its definition in include/bamqc.h, in two forms: table(), a plain loop per window and per
read, and table_fast(), vectorised with prefix sums.  Shares nothing with the kernels' arithmetic (bamqc_amd/csrc/k_gcb.hip).

The statistic.  Window length W, 20 <= W <= 1000; 101 bins.  A window [s, s+W) of a contig, 0 <= s, s + W <= len, has gc = the bases
with Dna5 code 1 or 2 and n = those with code 4; with n > 4 it has no bin, otherwise g = floor(100 gc / (W - n)).  G[g] counts every
window start s in [0, len - W] of every contig given whose window has a bin.  A read is examined iff flag & 0x904 == 0, n_cigar > 0,
0 <= rid < n_refs and the contig is given (and its read group is below n_lanes: the pre-pass refuses a batch that holds another).
Its window starts at s = pos (forward) or pos + the lengths of its CIGAR operations M, D, N, =, X - W (0x10 set); it is counted iff
0 <= s, s + W <= len and the window has a bin g.  R[lane][g] += 1; without BQC_FLAG_NO_QUAL (0x8000) also B[lane][g] += l_seq and
Q[lane][g] += the sum of its quality bytes.  T is [n_lanes][3 rows: R, B, Q][101]."""
import numpy as np

BINS = 101
ROWS = 3
R_ROW, B_ROW, Q_ROW = 0, 1, 2
REF_OPS = (0, 2, 3, 7, 8)


def _batches(cols_list):
    return [cols_list] if isinstance(cols_list, dict) else cols_list


def window_bin(window, W):
    """The bin of one window of W Dna5 codes, None when it has none."""
    gc = sum(1 for c in window if c in (1, 2))
    n = sum(1 for c in window if c == 4)
    return None if n > 4 else (100 * gc) // (W - n)


def genome(refs, W):
    """G over the contigs of `refs` (a list by rid; None: not given)."""
    G = np.zeros(BINS, np.uint64)
    for ref in refs:
        if ref is None:
            continue
        codes = [int(c) for c in ref]
        for s in range(len(codes) - W + 1):
            g = window_bin(codes[s:s + W], W)
            if g is not None:
                G[g] += 1
    return G


def table(cols_list, refs, n_lanes, W):
    """(G, T) by plain loops."""
    T = np.zeros((n_lanes, ROWS, BINS), np.uint64)
    for cols in _batches(cols_list):
        L = cols["l_seq"].astype(np.int64)
        nc = cols["n_cigar"].astype(np.int64)
        qoff = np.cumsum(L) - L
        coff = np.cumsum(nc) - nc
        for i, f in enumerate(cols["flag"].astype(np.int64)):
            rid, lane = int(cols["rid"][i]), int(cols["lane"][i])
            if f & 0x904 or nc[i] == 0 or rid < 0 or rid >= len(refs) or refs[rid] is None or lane >= n_lanes:
                continue
            s = int(cols["pos"][i])
            if f & 0x10:
                words = [int(w) for w in cols["cigar"][coff[i]:coff[i] + nc[i]]]
                s += sum(w >> 4 for w in words if (w & 15) in REF_OPS) - W
            if s < 0 or s + W > len(refs[rid]):
                continue
            g = window_bin([int(c) for c in refs[rid][s:s + W]], W)
            if g is None:
                continue
            T[lane, R_ROW, g] += 1
            if not f & 0x8000:
                T[lane, B_ROW, g] += int(L[i])
                T[lane, Q_ROW, g] += sum(int(q) for q in cols["qual"][qoff[i]:qoff[i] + L[i]])
    return genome(refs, W), T


def _bins_fast(ref, W):
    """Per window start of a contig the bin, -1 where the window has none (len - W + 1 entries; none for a shorter contig)."""
    ref = np.asarray(ref, np.int64)
    if len(ref) < W:
        return np.zeros(0, np.int64)
    cg = np.concatenate([[0], np.cumsum((ref == 1) | (ref == 2))])
    cn = np.concatenate([[0], np.cumsum(ref == 4)])
    gc, n = cg[W:] - cg[:-W], cn[W:] - cn[:-W]
    return np.where(n > 4, -1, (100 * gc) // (W - np.minimum(n, 4)))


def table_fast(cols_list, refs, n_lanes, W):
    """table(), vectorised: the bins of every window start of every contig from prefix sums, np.bincount over the counted reads."""
    bins = [None if r is None else _bins_fast(r, W) for r in refs]
    G = np.zeros(BINS, np.int64)
    for b in bins:
        if b is not None:
            G += np.bincount(b[b >= 0], minlength=BINS)
    T = np.zeros((n_lanes, ROWS, BINS), np.int64)
    given = np.array([b is not None for b in bins] + [False])
    nstarts = np.array([0 if b is None else len(b) for b in bins] + [0], np.int64)
    flat = np.concatenate([np.zeros(0, np.int64) if b is None else b for b in bins] + [np.zeros(1, np.int64)])
    first = np.cumsum(nstarts) - nstarts
    for cols in _batches(cols_list):
        f = cols["flag"].astype(np.int64)
        L = cols["l_seq"].astype(np.int64)
        nc = cols["n_cigar"].astype(np.int64)
        lane = cols["lane"].astype(np.int64)
        rid = cols["rid"].astype(np.int64)
        rid_in = np.where((rid >= 0) & (rid < len(refs)), rid, len(refs))
        w = cols["cigar"].astype(np.int64)
        read = np.repeat(np.arange(len(L)), nc)
        span = np.bincount(read, weights=np.where(np.isin(w & 15, REF_OPS), w >> 4, 0), minlength=len(L)).astype(np.int64)
        s = cols["pos"].astype(np.int64) + np.where((f & 0x10) != 0, span - W, 0)
        ok = ((f & 0x904) == 0) & (nc > 0) & given[rid_in] & (lane < n_lanes) & (s >= 0) & (s < nstarts[rid_in])
        g = np.where(ok, flat[np.where(ok, first[rid_in] + s, 0)], -1)
        ok &= g >= 0
        qsum = np.bincount(np.repeat(np.arange(len(L)), L), weights=cols["qual"][:int(L.sum())].astype(np.float64), minlength=len(L)).astype(np.int64)
        hasq = ok & ((f & 0x8000) == 0)
        at = lane * ROWS * BINS + g
        flatT = T.reshape(-1)
        flatT += np.bincount(at[ok], minlength=flatT.size)
        flatT += np.bincount(at[hasq] + B_ROW * BINS, weights=L[hasq].astype(np.float64), minlength=flatT.size).astype(np.int64)
        flatT += np.bincount(at[hasq] + Q_ROW * BINS, weights=qsum[hasq].astype(np.float64), minlength=flatT.size).astype(np.int64)
    return G.astype(np.uint64), T.astype(np.uint64)


def text(G, T, W, sample_id, lane_names, lane_index=None):
    """The `.gcb` text: lanes in the order given; the genome's line is the same for every lane."""
    out = []
    for k, name in enumerate(lane_names):
        l = k if lane_index is None else lane_index[k]
        out += ["sample_id " + sample_id, "lane " + name, "gc_bias_window %d" % W]
        for key, row in (("genome_windows_by_gc", G), ("read_starts_by_gc", T[l, R_ROW]), ("bases_by_gc", T[l, B_ROW]), ("base_qual_sum_by_gc", T[l, Q_ROW])):
            out.append(" ".join([key] + [str(int(v)) for v in row]))
    return "\n".join(out) + "\n"
