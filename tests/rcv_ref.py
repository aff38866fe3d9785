"""The depth over given regions (include/bamqc.h: bqc_enable_region_coverage) restated in plain Python / numpy, no GPU use: a loop form
that follows the header's text operation by operation and takes the depth by a loop over positions, and a vectorised form for the
larger batches (asserted equal on the step batches by tests/test_region_coverage_cpu.py).  The state: S[lane] = [E, T, A, 0] and
then the B + R difference words, uint64 modulo 2^64."""
import numpy as np

MATCH_OPS, QUERY_OPS, GENOME_OPS = (0, 7, 8), (0, 1, 4, 7, 8), (0, 2, 3, 7, 8)
END_MAX = (1 << 31) - 1
MASK = (1 << 64) - 1
DEFAULT_THRESHOLDS = (1, 10, 20, 30, 50, 100)


def examined(cols, n_lanes, n_refs, MQ):
    f = cols["flag"].astype(np.int64)
    return ((f & 0xF04) == 0) & (cols["mapq"].astype(np.int64) >= MQ) & (cols["n_cigar"] > 0) & (cols["l_seq"] > 0) & \
        (cols["lane"].astype(np.int64) < n_lanes) & (cols["rid"] >= 0) & (cols["rid"].astype(np.int64) < n_refs)


def layout(regions, n_refs, n_lanes=1):
    """The checked list: (rid, start, end, len, off, B), all int64; off has R + 1 entries."""
    rid, start, end = (np.asarray(a, np.int64) for a in regions)
    assert len(rid) == len(start) == len(end) >= 1 and (rid >= 0).all() and (rid < n_refs).all() and (start >= 0).all() and (end > start).all() and (end <= END_MAX).all()
    same = rid[1:] == rid[:-1]
    assert (np.diff(rid) >= 0).all() and (start[1:][same] >= end[:-1][same]).all()
    ln = end - start
    off = np.concatenate([[0], np.cumsum(ln + 1)])
    B = int(ln.sum())
    assert n_lanes * (B + len(rid) + 4) <= 1 << 28
    return rid, start, end, ln, off, B


def state(cols, regions, n_lanes, n_refs, MQ=20):
    """The loop form."""
    rid_s, start, end, ln, off, B = layout(regions, n_refs, n_lanes)
    S = [[0] * (4 + B + len(rid_s)) for _ in range(n_lanes)]
    nc = cols["n_cigar"].astype(np.int64)
    co = np.cumsum(nc) - nc
    for r in np.flatnonzero(examined(cols, n_lanes, n_refs, MQ)):
        L, rid, lane = int(cols["l_seq"][r]), int(cols["rid"][r]), int(cols["lane"][r])
        j, g, hit = 0, int(cols["pos"][r]), False
        row = S[lane]
        for w in cols["cigar"][co[r]:co[r] + int(nc[r])].tolist():
            op, n = w & 15, w >> 4
            if op in MATCH_OPS:
                m = min(n, max(0, L - j))
                row[2] = (row[2] + m) & MASK
                for k in np.flatnonzero((rid_s == rid) & (start < g + m) & (end > g)).tolist():
                    lo, hi = max(g, int(start[k])), min(g + m, int(end[k]))
                    a, b = 4 + int(off[k]) + lo - int(start[k]), 4 + int(off[k]) + hi - int(start[k])
                    row[a] = (row[a] + 1) & MASK
                    row[b] = (row[b] - 1) & MASK
                    hit = True
                j += n
                g += n
            elif op in (1, 4):
                j += n
            elif op in (2, 3):
                g += n
        row[0] = (row[0] + 1) & MASK
        if hit:
            row[1] = (row[1] + 1) & MASK
    return np.array(S, np.uint64)


def state_fast(cols, regions, n_lanes, n_refs, MQ=20):
    """The vectorised form: every match operation of every examined read at once."""
    rid_s, start, end, ln, off, B = layout(regions, n_refs, n_lanes)
    S = np.zeros((n_lanes, 4 + B + len(rid_s)), np.uint64)
    ok = examined(cols, n_lanes, n_refs, MQ)
    nc = cols["n_cigar"].astype(np.int64)
    co = np.cumsum(nc) - nc
    lane_r = cols["lane"].astype(np.int64)
    np.add.at(S[:, 0], lane_r[ok], np.uint64(1))
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
    g = cols["pos"].astype(np.int64)[read_of] + cg_ - gl - base_g
    L = cols["l_seq"].astype(np.int64)[read_of]
    rid = cols["rid"].astype(np.int64)[read_of]
    sel = np.flatnonzero(np.isin(op, MATCH_OPS) & ok[read_of] & (n > 0) & (j < L))
    m = np.minimum(n[sel], L[sel] - j[sel])
    np.add.at(S[:, 2], lane_r[read_of[sel]], m.astype(np.uint64))
    g0, g1 = g[sel], g[sel] + m
    clip = lambda x: np.minimum(np.maximum(x, 0), END_MAX + 1)
    lo = np.searchsorted(rid_s << 32 | end, rid[sel] << 32 | clip(g0), side="right")   # the first region with end > g
    hi = np.searchsorted(rid_s << 32 | start, rid[sel] << 32 | clip(g1), side="left")  # behind the last region with start < g + m
    cnt = np.maximum(hi - lo, 0)
    o = np.repeat(np.arange(len(sel)), cnt)
    k = np.repeat(lo, cnt) + np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    a = np.maximum(g0[o], start[k])
    b = np.minimum(g1[o], end[k])
    assert (a < b).all()
    lane_o = lane_r[read_of[sel[o]]]
    np.add.at(S, (lane_o, 4 + off[k] + a - start[k]), np.uint64(1))
    np.add.at(S, (lane_o, 4 + off[k] + b - start[k]), np.uint64(MASK))
    hit_reads = np.unique(read_of[sel[o]])
    np.add.at(S[:, 1], lane_r[hit_reads], np.uint64(1))
    return S


class NotADifferenceArray(Exception):
    def __init__(self, region):
        Exception.__init__(self, "region %d does not close at depth 0" % region)
        self.region = region


def products(S, regions, n_refs, thresholds=DEFAULT_THRESHOLDS, D=1000):
    """The finalize products by a loop over positions: per lane dict(reads_examined, reads_on_target, aligned_bases, bases_on_target,
    target_bases, regions (R, 3 + n), hist (D + 1,)).  NotADifferenceArray with the first region (over all lanes) that does not close."""
    rid_s, start, end, ln, off, B = layout(regions, n_refs)
    out, bad = [], []
    for l in range(S.shape[0]):
        row = [int(x) for x in S[l]]
        tab = np.zeros((len(rid_s), 3 + len(thresholds)), np.uint64)
        hist = [0] * (D + 1)
        depth = 0
        for k in range(len(rid_s)):
            total, mn, mx, ge = 0, MASK, 0, [0] * len(thresholds)
            for p in range(int(ln[k])):
                depth = (depth + row[4 + int(off[k]) + p]) & MASK
                total = (total + depth) & MASK
                mn, mx = min(mn, depth), max(mx, depth)
                for t, thr in enumerate(thresholds):
                    ge[t] += depth >= thr
                hist[min(depth, D)] += 1
            depth = (depth + row[4 + int(off[k]) + int(ln[k])]) & MASK
            if depth:
                bad.append(k)
            tab[k] = [total, mn, mx] + ge
        out.append(dict(reads_examined=row[0], reads_on_target=row[1], aligned_bases=row[2], bases_on_target=int(tab[:, 0].sum(dtype=np.uint64)), target_bases=B,
                        regions=tab, hist=np.array(hist, np.uint64)))
    if bad:
        raise NotADifferenceArray(min(bad))
    return out


def products_fast(S, regions, n_refs, thresholds=DEFAULT_THRESHOLDS, D=1000):
    """The same by cumsum and reduceat."""
    rid_s, start, end, ln, off, B = layout(regions, n_refs)
    out, bad = [], []
    closing = off[1:] - 1
    inside = np.ones(B + len(rid_s), bool)
    inside[closing] = False
    first = off[:-1]
    for l in range(S.shape[0]):
        depth = np.cumsum(S[l, 4:], dtype=np.uint64)
        bad += np.flatnonzero(depth[closing] != 0).tolist()
        cols = [np.add.reduceat(depth * inside.astype(np.uint64), first, dtype=np.uint64), np.minimum.reduceat(np.where(inside, depth, np.uint64(MASK)), first),
                np.maximum.reduceat(depth * inside.astype(np.uint64), first)]
        cols += [np.add.reduceat((inside & (depth >= np.uint64(t))).astype(np.uint64), first) for t in thresholds]
        tab = np.stack(cols, axis=1).astype(np.uint64)
        hist = np.bincount(np.minimum(depth[inside], np.uint64(D)).astype(np.int64), minlength=D + 1).astype(np.uint64)
        out.append(dict(reads_examined=int(S[l, 0]), reads_on_target=int(S[l, 1]), aligned_bases=int(S[l, 2]), bases_on_target=int(tab[:, 0].sum(dtype=np.uint64)),
                        target_bases=B, regions=tab, hist=hist))
    if bad:
        raise NotADifferenceArray(min(bad))
    return out


def text(prod, regions, ref_names, MQ, thresholds, sample, lane_names, lane_index):
    """The `.rcv` file (include/bamqc.h: bqc_write_region_coverage)."""
    out = []
    for name, l in zip(lane_names, lane_index):
        p = prod[l]
        out += ["sample_id %s" % sample, "lane %s" % name, "region_min_mapq %d" % MQ, "region_reads_examined %d" % p["reads_examined"],
                "region_reads_on_target %d" % p["reads_on_target"], "region_aligned_bases %d" % p["aligned_bases"], "region_bases_on_target %d" % p["bases_on_target"],
                "region_target_bases %d" % p["target_bases"], " ".join(["region_depth_thresholds"] + [str(int(t)) for t in thresholds]),
                " ".join(["region_depth_histogram", str(len(p["hist"]))] + [str(int(x)) for x in p["hist"]]), "regions %d" % len(regions[0])]
        for k in range(len(regions[0])):
            out.append("%s %d %d %s" % (ref_names[int(regions[0][k])], int(regions[1][k]), int(regions[2][k]), " ".join(str(int(x)) for x in p["regions"][k])))
    return "\n".join(out) + "\n"
