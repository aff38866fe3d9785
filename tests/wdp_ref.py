"""The depth in fixed genome windows (include/bamqc.h: bqc_enable_window_depth) restated in plain Python / numpy, no GPU use: a loop
form that follows the header's text operation by operation in Python integers, and a vectorised form for the larger batches (asserted
equal on the step batches by tests/test_window_depth_cpu.py).  The state: S[lane] = [E, E_low, X, 0] and then the planes reads, bases
and bases_low of NW words each, uint64 modulo 2^64.  Also the finalize products and the `.wdp` text."""
import numpy as np

MATCH_OPS, QUERY_OPS, GENOME_OPS = (0, 7, 8), (0, 1, 4, 7, 8), (0, 2, 3, 7, 8)
MASK = (1 << 64) - 1
HIST_BINS = 1001
W_MIN, W_MAX = 100, 1 << 24
WORDS_MAX = 1 << 28


def examined(cols, n_lanes, n_refs):
    f = cols["flag"].astype(np.int64)
    return ((f & 0xF04) == 0) & (cols["n_cigar"] > 0) & (cols["l_seq"] > 0) & (cols["lane"].astype(np.int64) < n_lanes) & (cols["rid"] >= 0) & \
        (cols["rid"].astype(np.int64) < n_refs)


def layout(W, ref_len, n_lanes=1):
    """(len, nw, woff, NW): int64 arrays; woff has n_refs + 1 entries."""
    ln = np.asarray(ref_len, np.int64)
    assert W_MIN <= W <= W_MAX and (ln >= 0).all() and (ln < 1 << 31).all()
    nw = (ln + W - 1) // W
    woff = np.concatenate([[0], np.cumsum(nw)]).astype(np.int64)
    NW = int(woff[-1])
    assert n_lanes * (4 + 3 * NW) <= WORDS_MAX
    return ln, nw, woff, NW


def state(cols, W, ref_len, n_lanes, MQ=20):
    """The loop form."""
    ln, nw, woff, NW = layout(W, ref_len, n_lanes)
    S = [[0] * (4 + 3 * NW) for _ in range(n_lanes)]
    nc = cols["n_cigar"].astype(np.int64)
    co = np.cumsum(nc) - nc
    for r in np.flatnonzero(examined(cols, n_lanes, len(ln))):
        L, rid, lane, pos = int(cols["l_seq"][r]), int(cols["rid"][r]), int(cols["lane"][r]), int(cols["pos"][r])
        good = int(cols["mapq"][r]) >= MQ
        length, first = int(ln[rid]), int(woff[rid])
        row = S[lane]
        plane = 4 + (NW if good else 2 * NW) + first
        j, g = 0, pos
        for w in cols["cigar"][co[r]:co[r] + int(nc[r])].tolist():
            op, n = w & 15, w >> 4
            if op in MATCH_OPS:
                m = min(n, max(0, L - j))
                p = g
                while p < g + m:  # the covered positions [g, g + m), a window (or a stretch off the contig) at a time
                    if 0 <= p < length:
                        k = p // W
                        e = min((k + 1) * W, length, g + m)
                        row[plane + k] = (row[plane + k] + e - p) & MASK
                    else:
                        e = min(0, g + m) if p < 0 else g + m
                        row[2] = (row[2] + e - p) & MASK
                    p = e
                j += n
                g += n
            elif op in (1, 4):
                j += n
            elif op in (2, 3):
                g += n
        row[0 if good else 1] = (row[0 if good else 1] + 1) & MASK
        if good and 0 <= pos < length:
            row[4 + first + pos // W] = (row[4 + first + pos // W] + 1) & MASK
    return np.array(S, np.uint64).reshape(n_lanes, 4 + 3 * NW)


def state_fast(cols, W, ref_len, n_lanes, MQ=20):
    """The vectorised form: every match operation of every examined read at once, then every (operation, window) pair."""
    ln, nw, woff, NW = layout(W, ref_len, n_lanes)
    S = np.zeros((n_lanes, 4 + 3 * NW), np.uint64)
    ok = examined(cols, n_lanes, len(ln))
    good_r = cols["mapq"].astype(np.int64) >= MQ
    nc = cols["n_cigar"].astype(np.int64)
    co = np.cumsum(nc) - nc
    lane_r = cols["lane"].astype(np.int64)
    rid_r = np.where(ok, cols["rid"].astype(np.int64), 0)
    pos_r = cols["pos"].astype(np.int64)
    np.add.at(S[:, 0], lane_r[ok & good_r], np.uint64(1))
    np.add.at(S[:, 1], lane_r[ok & ~good_r], np.uint64(1))
    st = np.flatnonzero(ok & good_r & (pos_r >= 0) & (pos_r < ln[rid_r]))
    np.add.at(S, (lane_r[st], 4 + woff[rid_r[st]] + pos_r[st] // W), np.uint64(1))
    read_of = np.repeat(np.arange(len(nc)), nc)
    w = cols["cigar"].astype(np.int64)
    op, n = w & 15, w >> 4
    ql = np.where(np.isin(op, QUERY_OPS), n, 0)
    gl = np.where(np.isin(op, GENOME_OPS), n, 0)
    cq, cg_ = np.cumsum(ql), np.cumsum(gl)
    first = co[read_of]
    base_q = np.where(first > 0, cq[np.maximum(first, 1) - 1], 0)
    base_g = np.where(first > 0, cg_[np.maximum(first, 1) - 1], 0)
    j = cq - ql - base_q
    g = pos_r[read_of] + cg_ - gl - base_g
    L = cols["l_seq"].astype(np.int64)[read_of]
    sel = np.flatnonzero(np.isin(op, MATCH_OPS) & ok[read_of] & (n > 0) & (j < L))
    m = np.minimum(n[sel], L[sel] - j[sel])
    rd = read_of[sel]
    length = ln[rid_r[rd]]
    a0 = np.clip(g[sel], 0, length)
    a1 = np.clip(g[sel] + m, 0, length)
    cov = np.maximum(a1 - a0, 0)
    np.add.at(S[:, 2], lane_r[rd], (m - cov).astype(np.uint64))
    on = np.flatnonzero(cov > 0)
    k0, k1 = a0[on] // W, (a1[on] - 1) // W
    cnt = k1 - k0 + 1
    o = np.repeat(on, cnt)
    k = np.repeat(k0, cnt) + np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    lo = np.maximum(a0[o], k * W)
    hi = np.minimum(a1[o], (k + 1) * W)
    assert (lo < hi).all()
    plane = np.where(good_r[rd[o]], NW, 2 * NW)
    np.add.at(S, (lane_r[rd[o]], 4 + plane + woff[rid_r[rd[o]]] + k), (hi - lo).astype(np.uint64))
    return S


def products(S, W, ref_len, main_chrom):
    """The finalize products: per lane dict(reads_examined, reads_low_mapq, bases_outside, reads, bases, bases_low (NW,), contigs
    (n_refs, 3), hist (1001,))."""
    ln, nw, woff, NW = layout(W, ref_len)
    wlen = np.concatenate([np.minimum((np.arange(int(nw[r])) + 1) * W, ln[r]) - np.arange(int(nw[r])) * W for r in range(len(ln))] + [np.zeros(0, np.int64)]).astype(np.uint64)
    in_main = np.repeat(np.asarray(main_chrom)[:len(ln)] == 1, nw) if len(ln) else np.zeros(0, bool)
    out = []
    for l in range(S.shape[0]):
        planes = [S[l, 4 + q * NW:4 + (q + 1) * NW] for q in range(3)]
        contigs = np.array([[int(p[int(woff[r]):int(woff[r + 1])].sum(dtype=np.uint64)) for p in planes] for r in range(len(ln))], np.uint64).reshape(len(ln), 3)
        depth = planes[1][in_main] // wlen[in_main]
        hist = np.bincount(np.minimum(depth, np.uint64(HIST_BINS - 1)).astype(np.int64), minlength=HIST_BINS).astype(np.uint64)
        out.append(dict(reads_examined=int(S[l, 0]), reads_low_mapq=int(S[l, 1]), bases_outside=int(S[l, 2]), reads=planes[0], bases=planes[1], bases_low=planes[2],
                        contigs=contigs, hist=hist))
    return out


def products_loops(S, W, ref_len, main_chrom):
    """The same by loops over contigs and windows in Python integers."""
    ln, nw, woff, NW = layout(W, ref_len)
    out = []
    for l in range(S.shape[0]):
        row = [int(x) for x in S[l]]
        contigs, hist = [], [0] * HIST_BINS
        for r in range(len(ln)):
            sums = [0, 0, 0]
            for k in range(int(nw[r])):
                at = 4 + int(woff[r]) + k
                for q in range(3):
                    sums[q] = (sums[q] + row[at + q * NW]) & MASK
                if main_chrom[r] == 1:
                    length = min((k + 1) * W, int(ln[r])) - k * W
                    hist[min(row[at + NW] // length, HIST_BINS - 1)] += 1
            contigs.append(sums)
        out.append(dict(reads_examined=row[0], reads_low_mapq=row[1], bases_outside=row[2], reads=S[l, 4:4 + NW], bases=S[l, 4 + NW:4 + 2 * NW],
                        bases_low=S[l, 4 + 2 * NW:4 + 3 * NW], contigs=np.array(contigs, np.uint64).reshape(len(ln), 3), hist=np.array(hist, np.uint64)))
    return out


def text(prod, W, MQ, ref_names, ref_len, sample, lane_names, lane_index):
    """The `.wdp` file (include/bamqc.h: bqc_write_window_depth)."""
    ln, nw, woff, NW = layout(W, ref_len)
    out = []
    for name, l in zip(lane_names, lane_index):
        p = prod[l]
        out += ["sample_id %s" % sample, "lane %s" % name, "window_depth_window %d" % W, "window_depth_min_mapq %d" % MQ,
                "window_depth_reads_examined %d" % p["reads_examined"], "window_depth_reads_low_mapq %d" % p["reads_low_mapq"],
                "window_depth_bases_outside_contigs %d" % p["bases_outside"],
                " ".join(["window_depth_histogram", str(HIST_BINS)] + [str(int(x)) for x in p["hist"]]), "contigs %d" % len(ln)]
        for r in range(len(ln)):
            out.append("%s %d %d %s" % (ref_names[r], int(ln[r]), int(nw[r]), " ".join(str(int(x)) for x in p["contigs"][r])))
        lines = []
        for r in range(len(ln)):
            for k in range(int(nw[r])):
                w = int(woff[r]) + k
                v = (int(p["reads"][w]), int(p["bases"][w]), int(p["bases_low"][w]))
                if any(v):
                    lines.append("%s %d %d %d %d %d" % ((ref_names[r], k * W, min((k + 1) * W, int(ln[r]))) + v))
        out.append("windows %d %d" % (len(lines), NW))
        out += lines
    return "\n".join(out) + "\n"


def reciprocal(W):
    """The kernel's multiply-shift for floor(g / W): (mul, shift) with shift = 31 + ceil(log2 W), mul = ceil(2^shift / W)."""
    shift = 31 + (W - 1).bit_length()
    return ((1 << shift) + W - 1) // W, shift
