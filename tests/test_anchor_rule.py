"""CPU: the one C++ statement of the coverage rule (csrc/anchor.h: which reads enter coverage(), and the step of the window state
machine, OverallNumbers.hpp:84-110) — the functions the host's pass and the card's chain both call — against the Python
restatements the GPU tests use (tests/anchor_recurrence.py), read by read and state by state.  Through the library's host-only
entry point bqc_anchor_rule: no GPU call."""
import ctypes as C

import numpy as np
import pytest

from bamqc_amd import _lib
from tests import synth as tsynth
from tests.anchor_recurrence import NO_WIN, per_group_anchors, reference_anchors
from tests.test_gpu_anchor import dense, make_case, with_positions

LENS = [4_000_000, 3_000_000]


class AnchorState(C.Structure):  # csrc/anchor.h
    _fields_ = [("first", C.c_uint32), ("id", C.c_int32), ("shift", C.c_uint32), ("pad", C.c_uint32), ("win", C.c_uint64),
                ("pending", C.c_uint32), ("has_prev", C.c_uint32), ("prev_rid", C.c_int32), ("prev_bp", C.c_uint32)]


def fresh_states(n_lanes):
    st = (AnchorState * n_lanes)()
    for s in st:
        s.first = 1
    return st


def rule(cols, states, n_refs, main):
    """bqc_anchor_rule over a batch: (window relative to the read's group's window at batch entry or NO_WIN, offset) per read; `states`
    move on"""
    fn = _lib.load().bqc_anchor_rule
    fn.restype = None
    fn.argtypes = [C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    n = len(cols["flag"])
    col = {k: np.ascontiguousarray(cols[k], dt) for k, dt in (("flag", np.uint16), ("rid", np.int32), ("pos", np.int32), ("lane", np.uint8))}
    main = np.ascontiguousarray(main, np.uint8)
    base = np.array([s.win for s in states], np.uint64)
    win, off = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    fn(n, col["flag"].ctypes.data, col["rid"].ctypes.data, col["pos"].ctypes.data, col["lane"].ctypes.data, n_refs, main.ctypes.data,
       len(states), C.addressof(states), win.ctypes.data, off.ctypes.data)
    cand = win != np.uint64(0xFFFFFFFFFFFFFFFF)
    lane = col["lane"].astype(np.int64)
    rel = np.full(n, NO_WIN, np.uint64)
    rel[cand] = win[cand] - base[lane[cand]]
    return rel, off


def state_tuple(s):
    return (bool(s.first), s.id, s.shift, s.win)


def check_one_group(batches, n_refs, main):
    states, want_state = fresh_states(1), (True, 0, 0, 0)
    n_cand = 0
    for cols in batches:
        win, off = rule(cols, states, n_refs, main)
        want_win, want_off, want_state = reference_anchors(cols, want_state, n_refs, main)
        assert np.array_equal(win, want_win), np.flatnonzero(win != want_win)[:10]
        assert np.array_equal(off, want_off), np.flatnonzero(off != want_off)[:10]  # (0 for a read that does not enter coverage(), both sides)
        if not want_state[0]:
            assert state_tuple(states[0]) == tuple(want_state)
        n_cand += int((want_win != NO_WIN).sum())
    return n_cand


@pytest.fixture(scope="module")
def base_cols():
    cols, _ = dense(5, 60_000, LENS)
    cols = dict(cols)
    cols["flag"] = ((np.asarray(cols["flag"]) & ~np.uint16(0xD04)) | np.uint16(0x40)).astype(np.uint16)  # (every read with a chromosome a candidate)
    return cols


def with_chromosome(batches):
    return sum(int((np.asarray(b["rid"]) >= 0).sum()) for b in batches)


@pytest.mark.parametrize("kind", ["thresholds", "stuck", "sparse", "unsorted"])
def test_the_rule_equals_the_restatement_on_the_position_lists_of_the_gpu_tests(kind, base_cols):
    batches = make_case(kind, np.random.default_rng(7), base_cols, LENS)
    assert check_one_group(batches, len(LENS), [1] * len(LENS)) == with_chromosome(batches) > 10


def test_positions_that_wrap_32_bits(base_cols):
    """negative `pos` (beginPos is unsigned: just below 2^32) and reads in front of `shift` (the difference wraps: a reset), over a
    batch end"""
    top = 1 << 31
    a = [5000, 4000, 4999, 6100, 3, -5, -3, -1, 0, 100, 1200, -1, 2200, top - 1, -top, -top + 999, -top + 1001, -top + 3001, top - 1]
    b = [top - 1, -top + 2000, -2001, -1001, -1, 999, 1000, 1001, -1, -2000, -3001, 7, 7]
    zeros = np.zeros(len(a), np.int32)
    batches = [with_positions(base_cols, a, zeros), with_positions(base_cols, b, zeros[:len(b)])]
    assert check_one_group(batches, len(LENS), [1] * len(LENS)) == len(a) + len(b)


def test_reads_that_fail_each_term_of_the_candidate_test(base_cols):
    """one term at a time — unmapped, secondary, duplicate, supplementary, neither first nor last, chromosome out of range either way,
    not a main chromosome, read group out of range — between reads that enter coverage() 900 positions apart (a read wrongly let in
    or left out moves every window behind it)"""
    flags = [0x40, 0x44, 0x80, 0x140, 0x440, 0x41, 0x840, 0x01, 0x00, 0xC0, 0x40, 0x40, 0x40, 0x40, 0x80, 0xD44, 0x40]
    rid = [0] * len(flags)
    lane = [0] * len(flags)
    rid[10], rid[11], rid[12], lane[13] = -1, 3, 1, 1  # (three chromosomes, chromosome 1 not a main one; one read group)
    n = len(flags)
    cols = with_positions(base_cols, np.arange(n) * 900 + 50, rid)
    cols["flag"] = np.array(flags, np.uint16)
    cols["lane"] = np.array(lane, np.uint8)
    cols2 = dict(cols, rid=np.where(np.array(rid) == 0, 2, rid).astype(np.int32))  # (the same on chromosome 2: a reset, state carried)
    assert check_one_group([cols, cols2], 3, [1, 0, 1]) == 2 * 6


def test_three_interleaved_read_groups_over_consecutive_batches(base_cols):
    """a state per read group, carried over four batches: group 0 dense and sorted, group 1 with gaps around the thresholds, group 2
    unsorted over both chromosomes; some reads of a fourth group the context does not have"""
    rng = np.random.default_rng(21)
    n = 24_000
    i = np.arange(n)
    lane = (i % 3).astype(np.uint8)
    lane[rng.integers(0, n, size=40)] = 3
    pos = np.sort(rng.integers(0, 2_900_000, size=n))
    k1 = np.flatnonzero(lane == 1)
    pos[k1] = np.cumsum(rng.choice([3, 400, 999, 1000, 1001, 1500, 1999, 2000, 2001, 2600], size=len(k1)))
    k2 = np.flatnonzero(lane == 2)
    pos[k2] = rng.integers(0, 2_900_000, size=len(k2))
    rid = np.zeros(n, np.int32)
    rid[k2] = np.sort(rng.integers(0, 2, size=len(k2)))
    cols = with_positions(base_cols, pos, rid)
    cols["lane"] = lane
    states, want_states = fresh_states(3), [(True, 0, 0, 0)] * 3
    for lo in range(0, n, 6_000):
        part = tsynth.slice_batch(cols, lo, lo + 6_000)
        win, off = rule(part, states, 2, [1, 1])
        want_win, want_off, want_states = per_group_anchors(part, want_states, 3, 2)
        assert np.array_equal(win, want_win), np.flatnonzero(win != want_win)[:10]
        assert np.array_equal(off, want_off), np.flatnonzero(off != want_off)[:10]
        assert [state_tuple(s) for s in states] == [tuple(s) for s in want_states]
        assert (want_win == NO_WIN).sum() == (part["lane"] == 3).sum() > 0
