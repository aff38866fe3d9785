"""CPU: the Python restatement of the per-read-group set-aside rule (tests/anchor_set_aside.py) the GPU tests compare the card with:
where nothing is pending it is the per-group recurrence of tests/anchor_recurrence.py, and on a hand-made stream it sets aside what
the rule says — per read group, up to the group's own first certain reset, with the thresholds in unsigned 32-bit arithmetic."""
import numpy as np

from tests.anchor_recurrence import NO_WIN, per_group_anchors
from tests.anchor_set_aside import count_breaks, fresh_group_states, per_group_set_aside


def reads(lane, rid, pos, flag=None):
    n = len(lane)
    return dict(flag=np.array(flag if flag is not None else [0x40] * n, np.uint16), lane=np.array(lane, np.uint8), rid=np.array(rid, np.int32),
                pos=np.array(pos, np.int64).astype(np.int32))


def test_without_a_pending_group_it_is_the_per_group_recurrence():
    rng = np.random.default_rng(3)
    n = 5_000
    lane = rng.integers(0, 4, size=n)  # (group 3: not one of the context's three)
    rid = np.sort(rng.integers(0, 2, size=n))
    pos = np.cumsum(rng.choice([0, 3, 400, 999, 1000, 1001, 1999, 2000, 2001, 2600], size=n)) % 3_000_000
    flag = rng.choice([0x40, 0x80, 0x44, 0x140, 0x01], size=n, p=[0.4, 0.4, 0.1, 0.05, 0.05])
    cols = reads(lane, rid, pos, flag)
    states = fresh_group_states(3)
    for s in states:
        s["pending"] = False
    want_states = [(True, 0, 0, 0)] * 3
    for lo in range(0, n, 1_000):
        part = {k: v[lo:lo + 1_000] for k, v in cols.items()}
        aside, win, off, states = per_group_set_aside(part, states, 3, 2)
        want_win, want_off, want_states = per_group_anchors(part, want_states, 3, 2)
        assert not aside.any()
        assert np.array_equal(win, want_win) and np.array_equal(off, want_off)
        assert [[s["first"], s["sid"], s["shift"], s["w"]] for s in states] == [list(s) for s in want_states]


def test_each_group_is_set_aside_up_to_its_own_first_certain_reset():
    #            0     1     2     3     4      5      6     7     8      9     10     11
    lane = [0,    1,    0,    1,    0,     1,     2,    0,    1,     0,    1,     0]
    rid = [0,     0,    0,    0,    0,     0,     0,    0,    1,     0,    1,     0]
    pos = [5000,  5100, 7000, 4800, 9001,  2799,  100,  9500, 50,    9900, 60,    13000]
    # group 0: 5000 (no read before: aside), 7000 (d = 2000: aside), 9001 (d = 2001: certain) -> anchored from read 4 on
    # group 1: 5100 (aside), 4800 (d wraps to 2^32 - 300: aside), 2799 (d wraps to 2^32 - 2001: certain) -> anchored from read 5 on
    # group 2: one read, nothing before it: aside, pending to the end
    aside, win, off, states = per_group_set_aside(reads(lane, rid, pos), fresh_group_states(3), 3, 2)
    assert aside.tolist() == [True, True, True, True, False, False, True, False, False, False, False, False]
    assert [s["pending"] for s in states] == [False, False, True]
    # group 0 as a stream that begins at read 4: 9001 first (window 0, offset 0), 9500 (499), 9900 (899), 13000 resets (window 2)
    assert [int(win[i]) for i in (4, 7, 9, 11)] == [0, 0, 0, 2] and [int(off[i]) for i in (4, 7, 9, 11)] == [0, 499, 899, 0]
    # group 1 from read 5: 2799 first, then the other chromosome resets (window 2), 60 stays (offset 10)
    assert [int(win[i]) for i in (5, 8, 10)] == [0, 2, 2] and [int(off[i]) for i in (5, 8, 10)] == [0, 0, 10]
    assert all(int(win[i]) == NO_WIN for i in np.flatnonzero(aside))
    assert (states[0]["prev_bp"], states[1]["prev_bp"], states[2]["prev_bp"]) == (9001, 2799, 100)  # the reset read's, or the last one set aside


def test_pending_state_is_carried_over_batches_and_breaks_are_counted_per_group():
    a = reads([0, 1, 0, 1], [0, 0, 0, 0], [100, 150, 300, 350])
    b = reads([0, 1, 0, 1], [0, 0, 0, 0], [500, 2351, 1400, 2400])
    states = fresh_group_states(2)
    aside, _, _, states = per_group_set_aside(a, states, 2, 1)
    assert aside.all() and all(s["pending"] and s["has_prev"] for s in states)
    aside, win, off, states = per_group_set_aside(b, states, 2, 1)
    assert aside.tolist() == [True, False, True, False]  # group 1: 2351 - 350 = 2001 behind the batch before's last read
    assert [s["pending"] for s in states] == [True, False]
    assert (int(win[1]), int(off[1]), int(win[3]), int(off[3])) == (0, 0, 0, 49)
    assert count_breaks(a, 2, 1) == 2 and count_breaks(b, 2, 1) == 2  # each group's first read of the batch; 1400 - 500 and 2400 - 2351 < 1000
