"""The overrepresented sequences (include/bamqc.h, bqc_enable_overrepresented) restated in plain Python: the checker of k_ovr.hip.
`view` is the rule as loops over a dict from (mate, sequence) to count, on reads decoded to strings; `view_fast` is the same in numpy
on a matrix of codes and is held against it on the CPU (tests/test_overrepresented_cpu.py).  Both take a column dict or a list of them
and return what Aggregator.overrepresented() returns.  Also the `.ovr` text.  Shares nothing with the kernel's arithmetic: no key words."""
import numpy as np

from tests.adp_ref import BUILTIN, COMPLEMENT, stored

BINS = 256
K_MIN, K_MAX = 20, 56
PPM_MIN, PPM_MAX = 10, 1_000_000
CAP_MIN, CAP_MAX = 16, 1 << 31


class Overflow(Exception):
    """More keys than the capacity: the stream fails with BQC_ERR_RANGE."""


def _batches(cols_list):
    return [cols_list] if isinstance(cols_list, dict) else cols_list


def examined(flag, l_seq, lane, n_lanes):
    return (flag & 0x900) == 0 and (flag & 0xC0) != 0 and l_seq > 0 and lane < n_lanes


def sequenced(s, reverse):
    """A stored read as sequenced."""
    return s[::-1].translate(COMPLEMENT) if reverse else s


def threshold(entered, ppm):
    return max(2, -(-entered * ppm // 1_000_000))


def source(seq):
    for name, ad in BUILTIN:
        if ad in seq:
            return name
    return "-"


def products(sets, lanes, K, ppm, capacity):
    """sets: dict (mate, sequence) -> count; lanes: (n_lanes, 4)."""
    if len(sets) > capacity:
        raise Overflow(len(sets))
    hist = np.zeros((2, BINS), np.uint64)
    largest = np.zeros(2, np.uint64)
    for (m, s), n in sets.items():
        hist[m, min(n, BINS) - 1] += 1
        largest[m] = max(int(largest[m]), n)
    entered = [int(lanes[:, m].sum()) - int(lanes[:, 2 + m].sum()) for m in range(2)]
    for m in range(2):
        assert entered[m] == sum(n for (mm, s), n in sets.items() if mm == m)
    thr = [threshold(entered[m], ppm) for m in range(2)]
    listed = [sorted(((s, n, source(s)) for (mm, s), n in sets.items() if mm == m and n >= thr[m]), key=lambda x: (-x[1], x[0])) for m in range(2)]
    return dict(K=K, ppm=ppm, capacity=capacity, lanes=lanes, distinct=hist.sum(axis=1), largest=largest, hist=hist, threshold=np.array(thr, np.uint64), listed=listed)


def count_sets(cols_list, n_lanes, K):
    """The loops: (dict (mate, sequence) -> count, lanes (n_lanes, 4), per batch the key of every read: a tuple, "skipped" or None)."""
    sets, per_read = {}, []
    lanes = np.zeros((n_lanes, 4), np.uint64)
    for cols in _batches(cols_list):
        L = cols["l_seq"].astype(np.int64)
        soff = np.cumsum((L + 1) // 2) - (L + 1) // 2
        keys = []
        for i, f in enumerate(cols["flag"].astype(np.int64)):
            lane = int(cols["lane"][i])
            keys.append(None)
            if not examined(int(f), int(L[i]), lane, n_lanes):
                continue
            mate = 0 if f & 0x40 else 1
            lanes[lane, mate] += 1
            s = sequenced(stored(cols, i, int(soff[i])), bool(f & 0x10))[:K]
            if any(ch not in "ACGT" for ch in s):
                lanes[lane, 2 + mate] += 1
                keys[-1] = "skipped"
                continue
            sets[(mate, s)] = sets.get((mate, s), 0) + 1
            keys[-1] = (mate, s)
        per_read.append(keys)
    return sets, lanes, per_read


def view(cols_list, n_lanes, K=50, ppm=1000, capacity=1 << 26):
    sets, lanes, _ = count_sets(cols_list, n_lanes, K)
    return products(sets, lanes, K, ppm, capacity)


def view_fast(cols_list, n_lanes, K=50, ppm=1000, capacity=1 << 26):
    """numpy: a row per examined read — mate, n and K codes (A 0 ... T 3, 4 every other stored code, 5 behind the read's n bases) — and
    np.unique over the rows without a 4."""
    code_of = np.full(16, 4, np.int8)
    code_of[[1, 2, 4, 8]] = [0, 1, 2, 3]
    lanes = np.zeros((n_lanes, 4), np.uint64)
    rows = []
    for cols in _batches(cols_list):
        L = cols["l_seq"].astype(np.int64)
        f = cols["flag"].astype(np.int64)
        lane = cols["lane"].astype(np.int64)
        ok = ((f & 0x900) == 0) & ((f & 0xC0) != 0) & (L > 0) & (lane < n_lanes)
        nb = (L + 1) // 2
        soff = (np.cumsum(nb) - nb)[ok]
        L, f, lane = L[ok], f[ok], lane[ok]
        mate = np.where((f & 0x40) != 0, 0, 1)
        n = np.minimum(L, K)
        j = np.arange(K)[None, :]
        inside = j < n[:, None]
        rev = ((f & 0x10) != 0)[:, None]
        at = np.where(inside, np.where(rev, L[:, None] - 1 - j, j), 0)  # the stored index of sequenced base j
        byte = cols["seq"][soff[:, None] + (at >> 1)].astype(np.int64) if len(L) else np.zeros((0, K), np.int64)
        code = code_of[np.where(at & 1, byte & 15, byte >> 4)]
        code = np.where(rev & (code < 4), 3 - code, code)
        code = np.where(inside, code, 5).astype(np.int8)
        bad = (code == 4).any(axis=1)
        for m in range(2):
            lanes[:, m] += np.bincount(lane[mate == m], minlength=n_lanes)[:n_lanes].astype(np.uint64)
            lanes[:, 2 + m] += np.bincount(lane[(mate == m) & bad], minlength=n_lanes)[:n_lanes].astype(np.uint64)
        rows.append(np.concatenate([mate[~bad, None].astype(np.int8), code[~bad]], axis=1))
    rows = np.concatenate(rows) if rows else np.zeros((0, K + 1), np.int8)
    uniq, counts = np.unique(rows, axis=0, return_counts=True) if len(rows) else (np.zeros((0, K + 1), np.int8), np.zeros(0, np.int64))
    if len(uniq) > capacity:
        raise Overflow(len(uniq))
    hist = np.zeros((2, BINS), np.uint64)
    largest = np.zeros(2, np.uint64)
    thr, listed = [], []
    for m in range(2):
        mine = uniq[:, 0] == m
        cn = counts[mine]
        hist[m] = np.bincount(np.minimum(cn, BINS) - 1, minlength=BINS)
        largest[m] = cn.max() if len(cn) else 0
        t = threshold(int(cn.sum()), ppm)
        thr.append(t)
        out = []
        for row, c in zip(uniq[mine][cn >= t], cn[cn >= t]):
            s = "".join("ACGT"[x] for x in row[1:] if x < 4)
            out.append((s, int(c), source(s)))
        listed.append(sorted(out, key=lambda x: (-x[1], x[0])))
    return dict(K=K, ppm=ppm, capacity=capacity, lanes=lanes, distinct=hist.sum(axis=1), largest=largest, hist=hist, threshold=np.array(thr, np.uint64), listed=listed)


def same_view(a, b):
    """None, or the first key in which two views differ."""
    for key in ("K", "ppm", "capacity"):
        if int(a[key]) != int(b[key]):
            return key
    for key in ("lanes", "distinct", "largest", "hist", "threshold"):
        if np.asarray(a[key]).shape != np.asarray(b[key]).shape or not np.array_equal(np.asarray(a[key], np.uint64), np.asarray(b[key], np.uint64)):
            return key
    if [[tuple(x) for x in l] for l in a["listed"]] != [[tuple(x) for x in l] for l in b["listed"]]:
        return "listed"
    return None


def text(v, sample_id="", lane_names=("",), lane_index=None):
    idx = list(range(len(lane_names))) if lane_index is None else list(lane_index)
    out = ["sample_id %s" % sample_id, "overrepresented_len %d" % v["K"], "overrepresented_ppm %d" % v["ppm"], "overrepresented_capacity %d" % v["capacity"]]
    for name, l in zip(lane_names, idx):
        s = v["lanes"][l]
        out += ["lane %s" % name, "sequence_reads_examined_first %d" % s[0], "sequence_reads_examined_second %d" % s[1],
                "sequence_reads_skipped_first %d" % s[2], "sequence_reads_skipped_second %d" % s[3]]
    out.append("all_lanes")
    for m, mate in enumerate(("first", "second")):
        out += ["sequences_distinct_%s %d" % (mate, v["distinct"][m]), "sequence_set_largest_%s %d" % (mate, v["largest"][m]),
                "sequence_set_size_histogram_%s " % mate + " ".join(str(int(x)) for x in v["hist"][m]),
                "overrepresented_threshold_%s %d" % (mate, v["threshold"][m]), "overrepresented_sequences_%s %d" % (mate, len(v["listed"][m]))]
        out += ["%s %d %s" % x for x in v["listed"][m]]
    return "\n".join(out) + "\n"
