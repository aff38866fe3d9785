"""The window state machine of OverallNumbers::coverage (OverallNumbers.hpp:84-110) restated in Python, one read at a time: what the
anchor tests compare the library with (the card's kernels in test_gpu_anchor*.py and test_gpu_async_submit.py, the rule's one C++
statement in test_anchor_rule.py)."""
import numpy as np

NO_WIN = 0xFFFFFFFF


def reference_anchors(cols, state, n_refs, main):
    """the recurrence itself, one read at a time: returns (win relative to the batch's first window or 0xFFFFFFFF, offset) per read"""
    n = len(cols["flag"])
    win = np.full(n, 0xFFFFFFFF, np.uint64)
    off = np.zeros(n, np.uint32)
    first, sid, shift, w = state
    base = w
    M = 1 << 32
    for i in range(n):
        f, rid = int(cols["flag"][i]), int(cols["rid"][i])
        if (f & 0xD04) or not (f & 0xC0) or not (0 <= rid < n_refs) or not main[rid] or int(cols["lane"][i]) >= 1:
            continue
        b = int(cols["pos"][i]) % M
        if first:
            first, sid, shift = False, rid, b
        if sid != rid or (b - shift) % M > 2000:
            sid, shift, w = rid, b, w + 2
        p = (b - shift) % M
        if 1000 < p < 2000:
            w, shift, p = w + 1, (shift + 1000) % M, p - 1000
        win[i], off[i] = w - base, p
    return win, off, (first, sid, shift, w)


def per_group_anchors(cols, states, n_lanes, n_refs):
    """the recurrence one read at a time, a state (first, chromosome, shift, window) per read group: returns (window relative to the
    read's group's window at batch entry, or NO_WIN; offset) per read, and the states behind the batch"""
    n = len(cols["flag"])
    win = np.full(n, NO_WIN, np.uint64)
    off = np.zeros(n, np.uint32)
    states = [list(s) for s in states]
    base = [s[3] for s in states]
    M = 1 << 32
    for i in range(n):
        f, rid, lane = int(cols["flag"][i]), int(cols["rid"][i]), int(cols["lane"][i])
        if (f & 0xD04) or not (f & 0xC0) or not (0 <= rid < n_refs) or lane >= n_lanes:
            continue
        first, sid, shift, w = states[lane]
        b = int(cols["pos"][i]) % M
        if first:
            first, sid, shift = False, rid, b
        if sid != rid or (b - shift) % M > 2000:
            sid, shift, w = rid, b, w + 2
        p = (b - shift) % M
        if 1000 < p < 2000:
            w, shift, p = w + 1, (shift + 1000) % M, p - 1000
        states[lane] = [first, sid, shift, w]
        win[i], off[i] = w - base[lane], p
    return win, off, states
