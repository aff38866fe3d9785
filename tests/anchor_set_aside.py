"""The set-aside rule of a shard that starts inside the stream (bqc_options.shard_tail), restated in Python one read at a time with one
state per read group — next to tests/anchor_recurrence.py's per_group_anchors, which it extends: while a read group is PENDING its
reads that enter coverage() are set aside, up to the group's first read that resets the windows whatever their state (another
chromosome than the group's read before, or more than 2000 positions from it in unsigned 32-bit arithmetic); from that read on the
group runs as a stream of its own would from there.  What the card's kernels (csrc/k_anchor.hip, the several-read-groups instances) and
the host's pass (csrc/bqc_pipeline.cpp: host_pass) are compared with."""
import numpy as np

from tests.anchor_recurrence import NO_WIN

M = 1 << 32


def fresh_group_states(n_lanes):
    """every read group as a shard_tail context finds it: pending, no read seen, a window state that has not started"""
    return [dict(pending=True, has_prev=False, prev_rid=0, prev_bp=0, first=True, sid=0, shift=0, w=0) for _ in range(n_lanes)]


def enters_coverage(cols, i, n_lanes, n_refs):
    f, rid = int(cols["flag"][i]), int(cols["rid"][i])
    return not ((f & 0xD04) or not (f & 0xC0) or not (0 <= rid < n_refs) or int(cols["lane"][i]) >= n_lanes)


def per_group_set_aside(cols, states, n_lanes, n_refs):
    """one batch, one read at a time: returns
        aside[i]   the read is set aside (its anchor is BQC_COV_PENDING)
        win[i]     otherwise its window relative to ITS group's window at batch entry (NO_WIN: the read does not enter coverage(), or
                   is set aside)
        off[i]     and its position in the two live windows
    and the states behind the batch (`states` itself is left alone)"""
    n = len(cols["flag"])
    aside = np.zeros(n, bool)
    win = np.full(n, NO_WIN, np.uint64)
    off = np.zeros(n, np.uint32)
    states = [dict(s) for s in states]
    base = [s["w"] for s in states]
    for i in range(n):
        if not enters_coverage(cols, i, n_lanes, n_refs):
            continue
        s = states[int(cols["lane"][i])]
        rid, b = int(cols["rid"][i]), int(cols["pos"][i]) % M
        if s["pending"]:
            d = (b - s["prev_bp"]) % M
            certain = s["has_prev"] and (rid != s["prev_rid"] or 2000 < d <= 0xFFFFFFFF - 2000)
            s["has_prev"], s["prev_rid"], s["prev_bp"] = True, rid, b
            if not certain:
                aside[i] = True
                continue
            s["pending"] = False
        if s["first"]:
            s["first"], s["sid"], s["shift"] = False, rid, b
        if s["sid"] != rid or (b - s["shift"]) % M > 2000:
            s["sid"], s["shift"], s["w"] = rid, b, s["w"] + 2
        p = (b - s["shift"]) % M
        if 1000 < p < 2000:
            s["w"], s["shift"], p = s["w"] + 1, (s["shift"] + 1000) % M, p - 1000
        win[i], off[i] = s["w"] - base[int(cols["lane"][i])], p
    return aside, win, off, states


def count_breaks(cols, n_lanes, n_refs):
    """the batch's breaks as the card's chain counts them (the limit is AN_MAX_BREAKS over the whole batch, reads set aside included):
    a read group's first read of the batch that enters coverage(), and every such read that is not less than 1000 positions behind
    its group's read before it on the same chromosome"""
    last = {}
    k = 0
    for i in range(len(cols["flag"])):
        if not enters_coverage(cols, i, n_lanes, n_refs):
            continue
        g, rid, b = int(cols["lane"][i]), int(cols["rid"][i]), int(cols["pos"][i]) % M
        if g not in last or last[g][0] != rid or (b - last[g][1]) % M >= 1000:
            k += 1
        last[g] = (rid, b)
    return k
