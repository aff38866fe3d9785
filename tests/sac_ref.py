"""The allele counts at given sites (include/bamqc.h: bqc_enable_site_alleles) restated in plain Python / numpy, no GPU use: a loop
form that follows the header's text operation by operation, and a vectorised form for the large batches (asserted equal on the small
ones by tests/test_site_alleles_cpu.py).  The table: T[lane][site][4 * strand + base], uint64."""
import numpy as np

MATCH_OPS, QUERY_OPS, GENOME_OPS = (0, 7, 8), (0, 1, 4, 7, 8), (0, 2, 3, 7, 8)
BASE_OF = {1: 0, 2: 1, 4: 2, 8: 3}
POS_MAX = (1 << 31) - 2


def examined(cols, n_lanes, n_refs, MQ):
    f = cols["flag"].astype(np.int64)
    return ((f & 0xF04) == 0) & ((f & 0x8000) == 0) & (cols["mapq"].astype(np.int64) >= MQ) & (cols["n_cigar"] > 0) & (cols["l_seq"] > 0) & \
        (cols["lane"].astype(np.int64) < n_lanes) & (cols["rid"] >= 0) & (cols["rid"].astype(np.int64) < n_refs)


def offsets(cols):
    L = cols["l_seq"].astype(np.int64)
    nc = cols["n_cigar"].astype(np.int64)
    return np.cumsum((L + 1) // 2) - (L + 1) // 2, np.cumsum(L) - L, np.cumsum(nc) - nc


def check_sites(rid, pos, n_refs):
    rid, pos = np.asarray(rid, np.int64), np.asarray(pos, np.int64)
    assert len(rid) == len(pos) >= 1 and (rid >= 0).all() and (rid < n_refs).all() and (pos >= 0).all() and (pos <= POS_MAX).all()
    key = rid << 32 | pos
    assert (np.diff(key) > 0).all()
    return rid, pos, key


def table(cols, sites, n_lanes, n_refs, Q=20, MQ=20):
    """The loop form."""
    rid_s, pos_s, key = check_sites(sites[0], sites[1], n_refs)
    T = np.zeros((n_lanes, len(rid_s), 8), np.uint64)
    so, qo, co = offsets(cols)
    ok = examined(cols, n_lanes, n_refs, MQ)
    for r in np.flatnonzero(ok):
        L, rid, lane = int(cols["l_seq"][r]), int(cols["rid"][r]), int(cols["lane"][r])
        s = (int(cols["flag"][r]) >> 4) & 1
        j, g = 0, int(cols["pos"][r])
        for w in cols["cigar"][co[r]:co[r] + int(cols["n_cigar"][r])].tolist():
            op, n = w & 15, w >> 4
            if op in MATCH_OPS:
                lo = np.searchsorted(key, rid << 32 | min(max(g, 0), POS_MAX + 1))
                hi = np.searchsorted(key, rid << 32 | min(max(g + n, 0), POS_MAX + 1))
                for k in range(lo, hi):
                    i = j + int(pos_s[k]) - g
                    if i >= L:
                        break
                    byte = int(cols["seq"][so[r] + i // 2])
                    code = byte & 15 if i & 1 else byte >> 4
                    q = int(cols["qual"][qo[r] + i])
                    if code in BASE_OF and Q <= q <= 222:
                        T[lane, k, 4 * s + BASE_OF[code]] += 1
                j += n
                g += n
            elif op in (1, 4):
                j += n
            elif op in (2, 3):
                g += n
    return T


def table_fast(cols, sites, n_lanes, n_refs, Q=20, MQ=20):
    """The vectorised form: every match operation of every examined read at once."""
    rid_s, pos_s, key = check_sites(sites[0], sites[1], n_refs)
    T = np.zeros((n_lanes, len(rid_s), 8), np.uint64)
    so, qo, co = offsets(cols)
    ok = examined(cols, n_lanes, n_refs, MQ)
    nc = cols["n_cigar"].astype(np.int64)
    read_of = np.repeat(np.arange(len(nc)), nc)
    w = cols["cigar"].astype(np.int64)
    op, n = w & 15, w >> 4
    ql = np.where(np.isin(op, QUERY_OPS), n, 0)
    gl = np.where(np.isin(op, GENOME_OPS), n, 0)
    cq, cg_ = np.cumsum(ql), np.cumsum(gl)
    first = co[read_of]  # the read's first operation
    base_q = np.where(first > 0, cq[np.maximum(first, 1) - 1], 0)
    base_g = np.where(first > 0, cg_[np.maximum(first, 1) - 1], 0)
    j = cq - ql - base_q
    g = cols["pos"].astype(np.int64)[read_of] + cg_ - gl - base_g
    L = cols["l_seq"].astype(np.int64)[read_of]
    rid = cols["rid"].astype(np.int64)[read_of]
    m = np.isin(op, MATCH_OPS) & ok[read_of] & (n > 0) & (j < L)
    idx = np.flatnonzero(m)
    lo = np.searchsorted(key, rid[idx] << 32 | np.minimum(np.maximum(g[idx], 0), POS_MAX + 1))
    hi = np.searchsorted(key, rid[idx] << 32 | np.minimum(np.maximum(g[idx] + n[idx], 0), POS_MAX + 1))
    cnt = np.maximum(hi - lo, 0)
    o = np.repeat(idx, cnt)                    # the operation of every (operation, site) pair
    k = np.repeat(lo, cnt) + np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)  # its site
    i = j[o] + pos_s[k] - g[o]
    keep = i < L[o]
    o, k, i = o[keep], k[keep], i[keep]
    r = read_of[o]
    byte = cols["seq"][so[r] + i // 2].astype(np.int64)
    code = np.where(i & 1, byte & 15, byte >> 4)
    q = cols["qual"][qo[r] + i].astype(np.int64)
    base = np.full(16, -1, np.int64)
    for c, b in BASE_OF.items():
        base[c] = b
    b = base[code]
    good = (b >= 0) & (q >= Q) & (q <= 222)
    s = (cols["flag"].astype(np.int64)[r] >> 4) & 1
    np.add.at(T, (cols["lane"].astype(np.int64)[r][good], k[good], (4 * s + b)[good]), 1)
    return T


def text(T, sites, ref_names, Q, MQ, sample, lane_names, lane_index):
    """The `.sac` file (include/bamqc.h: bqc_write_site_alleles)."""
    out = []
    for name, l in zip(lane_names, lane_index):
        out += ["sample_id %s" % sample, "lane %s" % name, "site_allele_min_base_qual %d" % Q, "site_allele_min_mapq %d" % MQ, "site_alleles %d" % T.shape[1]]
        for k in range(T.shape[1]):
            out.append("%s %d %s" % (ref_names[int(sites[0][k])], int(sites[1][k]) + 1, " ".join(str(int(x)) for x in T[l, k])))
    return "\n".join(out) + "\n"
