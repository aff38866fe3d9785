"""The duplicate sets by alignment signature (include/bamqc.h, bqc_enable_duplicate_sets) restated in plain Python: the checker of
k_dup.hip.  `view` is the rule as loops over a dict from signature to count; `view_fast` is the same in numpy and is held against it on
the CPU (tests/test_duplicate_sets_cpu.py).  Both return what Aggregator.duplicate_sets() returns.  Also the library-size estimate and
the `.dup` text."""
import math

import numpy as np

BINS = 256
CAP_MIN, CAP_MAX = 16, 1 << 31
CLIPS = (4, 5)
GENOME_OPS = (0, 2, 3, 7, 8)
SINGLE, PAIR, SECOND = 0, 1, 2


class Overflow(Exception):
    """More signatures than the capacity: the stream fails with BQC_ERR_RANGE."""


def slots(capacity):
    C = 32
    while C < 2 * capacity:
        C *= 2
    return C


def examined(flag, l_seq, n_cigar, rid, lane, n_lanes, n_refs):
    return (flag & 0xB04) == 0 and n_cigar > 0 and l_seq > 0 and 0 <= rid < n_refs and lane < n_lanes


def read_class(flag, tlen):
    both = (flag & 0x1) and not (flag & 0x8)
    return PAIR if both and tlen > 0 else SECOND if both and tlen < 0 else SINGLE


def clips(cigar):
    """(lead, trail, reflen) of a CIGAR [(length, op), ...] in stored order."""
    k = 0
    while k < len(cigar) and cigar[k][1] in CLIPS:
        k += 1
    lead = sum(n for n, _ in cigar[:k])
    e = len(cigar)
    while e > k and cigar[e - 1][1] in CLIPS:
        e -= 1
    trail = sum(n for n, _ in cigar[e:])
    return lead, trail, sum(n for n, op in cigar if op in GENOME_OPS)


def u5_of(cigar, pos, reverse):
    lead, trail, reflen = clips(cigar)
    u5 = pos + reflen - 1 + trail if reverse else pos - lead
    assert abs(u5) < 1 << 45
    return u5


def signature(flag, rid, pos, tlen, cigar):
    """The tuple of an examined read of class single or pair."""
    cls = read_class(flag, tlen)
    assert cls != SECOND
    return (cls, flag >> 4 & 1, (flag >> 5 & 1) if cls == PAIR else 0, rid, u5_of(cigar, pos, flag >> 4 & 1), tlen if cls == PAIR else 0)


def cigars_of(cols):
    off = np.concatenate([[0], np.cumsum(cols["n_cigar"].astype(np.int64))])
    w = cols["cigar"]
    return [[(int(x) >> 4, int(x) & 15) for x in w[off[i]:off[i + 1]]] for i in range(len(cols["flag"]))]


def estimate(n, c):
    """Picard's estimateLibrarySize."""
    if c == 0 or c >= n:
        return 0
    n, c = float(n), float(c)
    f = lambda x: c / x - 1 + math.exp(-n / x)
    m, M = 1.0, 100.0
    while f(M * c) > 0:
        M *= 10
    for _ in range(40):
        r = (m + M) / 2
        u = f(r * c)
        if u == 0:
            break
        if u > 0:
            m = r
        else:
            M = r
    return int(c * (m + M) / 2)


def products(sets, lanes, capacity):
    """sets: dict signature -> count; lanes: (n_lanes, 5)."""
    if len(sets) > capacity:
        raise Overflow(len(sets))
    hist = np.zeros((2, BINS), np.uint64)
    largest = np.zeros(2, np.uint64)
    for sig, n in sets.items():
        hist[sig[0], min(n, BINS) - 1] += 1
        largest[sig[0]] = max(int(largest[sig[0]]), n)
    U = hist.sum(axis=1)
    for c in range(2):
        assert int(lanes[:, c].sum()) == sum(n for s, n in sets.items() if s[0] == c)
    return dict(capacity=capacity, sets=U, largest=largest, hist=hist, estimated_library_size=estimate(int(lanes[:, 1].sum()), int(U[1])), lanes=lanes)


def count_sets(cols, n_lanes, n_refs):
    """The loops: (dict signature -> count, lanes (n_lanes, 5), the signature of every read or None)."""
    sets, per_read = {}, []
    lanes = np.zeros((n_lanes, 5), np.uint64)
    cig = cigars_of(cols)
    for i in range(len(cols["flag"])):
        flag, rid, pos, tlen, lane = int(cols["flag"][i]), int(cols["rid"][i]), int(cols["pos"][i]), int(cols["tlen"][i]), int(cols["lane"][i])
        per_read.append(None)
        if not examined(flag, int(cols["l_seq"][i]), len(cig[i]), rid, lane, n_lanes, n_refs):
            continue
        cls = read_class(flag, tlen)
        if cls == SECOND:
            lanes[lane, 4] += 1
            continue
        lanes[lane, cls] += 1
        if flag & 0x400:
            lanes[lane, 2 + cls] += 1
        sig = signature(flag, rid, pos, tlen, cig[i])
        sets[sig] = sets.get(sig, 0) + 1
        per_read[-1] = sig
    return sets, lanes, per_read


def view(cols, n_lanes, n_refs, capacity=1 << 26):
    sets, lanes, _ = count_sets(cols, n_lanes, n_refs)
    return products(sets, lanes, capacity)


def keys_fast(cols, n_lanes, n_refs):
    """numpy: (cls per read with -1 for a read that is not examined, k0, k1 of every read: the two words of include/bamqc.h)."""
    flag = cols["flag"].astype(np.int64)
    n = len(flag)
    nc = cols["n_cigar"].astype(np.int64)
    rid, pos, tlen = cols["rid"].astype(np.int64), cols["pos"].astype(np.int64), cols["tlen"].astype(np.int64)
    ex = ((flag & 0xB04) == 0) & (nc > 0) & (cols["l_seq"] > 0) & (rid >= 0) & (rid < n_refs) & (cols["lane"] < n_lanes)
    both = ((flag & 1) != 0) & ((flag & 8) == 0)
    cls = np.where(both & (tlen > 0), PAIR, np.where(both & (tlen < 0), SECOND, SINGLE))
    cls = np.where(ex, cls, -1)
    w = cols["cigar"].astype(np.int64)
    op, ln = w & 15, w >> 4
    owner = np.repeat(np.arange(n), nc)
    k = np.arange(len(w)) - np.repeat(np.cumsum(nc) - nc, nc)
    clip = (op == 4) | (op == 5)
    first, last = nc.copy(), np.full(n, -1, np.int64)
    np.minimum.at(first, owner[~clip], k[~clip])
    np.maximum.at(last, owner[~clip], k[~clip])
    tot = lambda m: np.bincount(owner[m], weights=ln[m].astype(np.float64), minlength=n).astype(np.int64)  # (sums below 2^44: exact)
    lead = tot(clip & (k < first[owner]))
    trail = tot(clip & (k > last[owner]) & (last[owner] >= 0))
    reflen = tot(np.isin(op, GENOME_OPS))
    rev = flag >> 4 & 1
    u5 = np.where(rev == 1, pos + reflen - 1 + trail, pos - lead)
    pair = cls == PAIR
    k0 = (u5 + (1 << 45)) | (pair.astype(np.int64) << 46) | (rev << 47) | (np.where(pair, flag >> 5 & 1, 0) << 48)
    k1 = rid | ((np.where(pair, tlen, 0) & 0xFFFFFFFF) << 32)
    return cls, k0.astype(np.uint64), k1.astype(np.uint64)


def view_fast(cols, n_lanes, n_refs, capacity=1 << 26):
    cls, k0, k1 = keys_fast(cols, n_lanes, n_refs)
    lane = cols["lane"].astype(np.int64)
    fl = (cols["flag"] & 0x400) != 0
    lanes = np.zeros((n_lanes, 5), np.uint64)
    for c, m in ((0, cls == SINGLE), (1, cls == PAIR), (2, (cls == SINGLE) & fl), (3, (cls == PAIR) & fl), (4, cls == SECOND)):
        lanes[:, c] = np.bincount(lane[m], minlength=n_lanes)[:n_lanes]
    m = (cls == SINGLE) | (cls == PAIR)
    keys = np.stack([k0[m], k1[m]], axis=1)
    uniq, counts = np.unique(keys, axis=0, return_counts=True) if len(keys) else (np.zeros((0, 2), np.uint64), np.zeros(0, np.int64))
    if len(uniq) > capacity:
        raise Overflow(len(uniq))
    ucls = (uniq[:, 0] >> np.uint64(46)).astype(np.int64) & 1
    hist = np.zeros((2, BINS), np.uint64)
    largest = np.zeros(2, np.uint64)
    for c in range(2):
        n = counts[ucls == c]
        hist[c] = np.bincount(np.minimum(n, BINS) - 1, minlength=BINS)
        largest[c] = n.max() if len(n) else 0
    U = hist.sum(axis=1)
    return dict(capacity=capacity, sets=U, largest=largest, hist=hist, estimated_library_size=estimate(int(lanes[:, 1].sum()), int(U[1])), lanes=lanes)


def same_view(a, b):
    """None, or the first key in which two views differ."""
    for key in ("capacity", "estimated_library_size"):
        if int(a[key]) != int(b[key]):
            return key
    for key in ("sets", "largest", "hist", "lanes"):
        if np.asarray(a[key]).shape != np.asarray(b[key]).shape or not np.array_equal(np.asarray(a[key], np.uint64), np.asarray(b[key], np.uint64)):
            return key
    return None


def text(v, sample_id="", lane_names=("",), lane_index=None):
    idx = list(range(len(lane_names))) if lane_index is None else list(lane_index)
    out = ["sample_id %s" % sample_id, "duplicate_sets_capacity %d" % v["capacity"]]
    for name, l in zip(lane_names, idx):
        s = v["lanes"][l]
        out += ["lane %s" % name, "duplicate_reads_examined_single %d" % s[0], "duplicate_reads_examined_pair %d" % s[1],
                "duplicate_reads_flagged_single %d" % s[2], "duplicate_reads_flagged_pair %d" % s[3], "duplicate_reads_second_end %d" % s[4]]
    out += ["all_lanes", "duplicate_sets_single %d" % v["sets"][0], "duplicate_sets_pair %d" % v["sets"][1],
            "duplicate_set_largest_single %d" % v["largest"][0], "duplicate_set_largest_pair %d" % v["largest"][1],
            "duplicate_set_size_histogram_single " + " ".join(str(int(x)) for x in v["hist"][0]),
            "duplicate_set_size_histogram_pair " + " ".join(str(int(x)) for x in v["hist"][1]),
            "duplicate_estimated_library_size %d" % v["estimated_library_size"]]
    return "\n".join(out) + "\n"
