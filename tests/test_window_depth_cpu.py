"""No GPU: the two forms of tests/wdp_ref.py agree on every batch of tests/wdp_steps.py, the batches really cross the edges that
tests/test_gpu_window_depth.py names them for, and the kernel's multiply-shift reciprocal is exact where the kernel uses it."""
import numpy as np
import pytest

from tests import lane_limit, wdp_ref, wdp_steps
from tests.wdp_steps import LEN_MAX, OPMAX, WAVE, WD_T


def both(cols, W, lens, n_lanes, MQ=20):
    St = wdp_ref.state(cols, W, lens, n_lanes, MQ)
    fast = wdp_ref.state_fast(cols, W, lens, n_lanes, MQ)
    assert St.shape == fast.shape == (n_lanes, 4 + 3 * wdp_ref.layout(W, lens)[3])
    bad = np.argwhere(St != fast)
    assert not len(bad), (len(bad), bad[:3].tolist())
    main = [1] * len(lens)
    a, b = wdp_ref.products(St, W, lens, main), wdp_ref.products_loops(St, W, lens, main)
    for x, y in zip(a, b):
        assert all(np.array_equal(x[k], y[k]) for k in x)
        assert int(x["hist"].sum()) == wdp_ref.layout(W, lens)[3]
    return St


def planes(St, W, lens):
    NW = wdp_ref.layout(W, lens)[3]
    return St[:, 4:4 + NW], St[:, 4 + NW:4 + 2 * NW], St[:, 4 + 2 * NW:]


@pytest.mark.parametrize("MQ", [0, 20, 255])
def test_rule_batch(MQ):
    cols = wdp_steps.rule_batch(MQ)
    lens, W = wdp_steps.RULE_LENS, wdp_steps.RULE_W
    St = both(cols, W, lens, 3, MQ)
    reads, bases, low = planes(St, W, lens)
    assert set(range(16)) <= set((cols["cigar"] & 15).tolist())  # every operation code
    f = cols["flag"].astype(np.int64)
    assert all(((f & bit) != 0).any() for bit in (0x4, 0x100, 0x200, 0x400, 0x800, 0x8000))
    assert (cols["pos"] == 0).any() and (cols["pos"] < 0).any()
    nc = cols["n_cigar"].astype(np.int64)
    one = np.flatnonzero(nc == 1)
    end = cols["pos"][one].astype(np.int64) + (cols["cigar"][np.cumsum(nc)[one] - 1] >> 4)
    assert ((end == lens[0]) & (cols["rid"][one] == 0)).any() and ((end > lens[0]) & (cols["rid"][one] == 0)).any()  # ends on the last base; runs past it
    assert lens[1] == 0 and (cols["rid"] == 1).any() and (St[:, 2] > 0).all()
    assert (cols["l_seq"] < 10).any()
    for l in range(3):
        assert St[l, 3] == 0 and St[l, 0] > 0
        if MQ:  # good and low reads in one window (MQ = 0: every read is good)
            assert bases[l, 1] > 0 and low[l, 1] > 0 and St[l, 1] > 0
        else:
            assert St[l, 1] == 0 and not low[l].any()
        total = int(bases[l].sum()) + int(low[l].sum()) + int(St[l, 2])
        assert total > 0


@pytest.mark.parametrize("W", wdp_steps.BORDER_WS)
def test_border_batch(W):
    cols, lens = wdp_steps.border_batch(W)
    assert lens == [1, W - 1, W, W + 1, 3 * W, 2 * W + 37]
    St = both(cols, W, lens, 2, 20)
    nc = cols["n_cigar"].astype(np.int64)
    one = nc == 1
    first = np.cumsum(nc) - nc
    n0 = (cols["cigar"][first] >> 4).astype(np.int64)
    pos = cols["pos"].astype(np.int64)
    for b in (W, 2 * W):
        for d in (-1, 0, 1):  # runs that begin and that end on a border and one base to either side
            assert (one & (pos == b + d)).any() and (one & (pos + n0 == b + d)).any(), (b, d)
    if W <= wdp_steps.EXACT_M_MAX:
        for k in (1, 2, 3):
            assert (one & (n0 == k * W) & (pos % W == 0)).any() and (one & (n0 == k * W) & (pos % W != 0)).any()
    nw = wdp_ref.layout(W, lens)[1]
    assert nw.tolist() == [1, 1, 1, 2, 3, 3]
    reads, bases, low = planes(St, W, lens)
    assert (bases + low)[:, -1].any()  # the short last window of the last contig
    assert St[:, 2].all()


@pytest.mark.parametrize("W", wdp_steps.COORD_WS)
def test_coord_batch(W):
    cols = wdp_steps.coord_batch(W)
    St = both(cols, W, wdp_steps.COORD_LENS, 2, 20)
    assert wdp_steps.COORD_LENS[0] == (1 << 31) - 1
    pos = cols["pos"].astype(np.int64)
    assert (pos == LEN_MAX - 1).any()
    assert ((cols["cigar"] >> 4) == OPMAX).any()
    last = (LEN_MAX - 1) // W
    for d in (-1, 0, 1):
        assert (pos == last * W + d).any() and (pos == (last - 1) * W + d).any()
    reads, bases, low = planes(St, W, wdp_steps.COORD_LENS)
    nw0 = int(wdp_ref.layout(W, wdp_steps.COORD_LENS)[1][0])
    assert bases[0, nw0 - 1] > 0 and reads[0, nw0 - 1] > 0 and St[:, 2].all()
    assert (cols["n_cigar"] > WD_T).any()  # the far deletion goes down the wave path


def test_reciprocal_is_exact():
    """(g * mul) >> shift == g // W at every border and one base to either side, for the window sizes of the tests and the range's ends,
    and mul < 2^32 and g * mul < 2^64."""
    rng = np.random.default_rng(5)
    for W in sorted(set(wdp_steps.BORDER_WS + wdp_steps.COORD_WS + [100, 101, 127, 128, 129, 1000, (1 << 24) - 1, 1 << 24] + rng.integers(100, 1 << 24, 40).tolist())):
        mul, shift = wdp_ref.reciprocal(W)
        assert mul < 1 << 32 and shift <= 55 and (LEN_MAX * mul) < 1 << 64
        k = np.unique(np.concatenate([np.arange(0, min(LEN_MAX // W + 1, 3000)), np.array([LEN_MAX // W, LEN_MAX // W - 1]), rng.integers(0, LEN_MAX // W + 1, 3000)]))
        g = np.unique(np.concatenate([k * W - 1, k * W, k * W + 1, k * W + W - 1, np.array([0, LEN_MAX - 1, LEN_MAX])]))
        g = g[(g >= 0) & (g <= LEN_MAX)]
        for x in g.tolist():
            assert (x * mul) >> shift == x // W, (W, x)


def test_path_batch():
    reads, lens = wdp_steps.path_batch()
    cols = wdp_steps.cols_of(reads, 4)
    St = both(cols, wdp_steps.PATH_W, lens, 1, 20)
    nc = sorted(set(cols["n_cigar"].tolist()))
    assert set(wdp_steps.PATH_NCIGARS) <= set(nc) and WD_T in nc and WD_T + 1 in nc
    reads_p, bases, low = planes(St, wdp_steps.PATH_W, lens)
    assert St[0, 2] > 4000                                      # the 10 kb runs are clipped at contig 1's end, on both paths
    assert (bases[0, 10:100] >= 100).all()                      # one M over a hundred windows
    assert low[0].any()
    for k in range(len(reads)):                                 # each read alone is a batch of its own
        wdp_ref.state(wdp_steps.cols_of(reads[k:k + 1], 100 + k), wdp_steps.PATH_W, lens, 1, 20)


def test_combining_batches():
    cols = wdp_steps.hot_batch()
    St = both(cols, wdp_steps.HOT_W, wdp_steps.HOT_LENS, 2)
    assert St[:, 0].tolist() == [10_000, 10_000] and St[:, 4 + 5 + 1].tolist() == [600_000, 600_000] and St[:, 4 + 1].tolist() == [10_000, 10_000]
    cols = wdp_steps.runs_batch()
    both(cols, wdp_steps.RUN_W, wdp_steps.RUN_LENS, 1)
    keys = wdp_steps.keys_in_order(cols, wdp_steps.RUN_W, wdp_steps.RUN_LENS, 1, 20)
    runs = wdp_steps.run_lengths(keys).tolist()
    assert runs == wdp_steps.RUNS and {1, 2, 63, 64, 65} <= set(runs)
    starts = np.cumsum([0] + runs[:-1])
    assert sum(s // WAVE != (s + n - 1) // WAVE for s, n in zip(starts, runs)) >= 5  # runs that cross a wave's border
    # alternating read groups: grouped by the processing order, the seam inside a wave, the same plane and window on both sides
    cols = wdp_steps.alternating_batch("group")
    both(cols, wdp_steps.RUN_W, wdp_steps.RUN_LENS, 2)
    assert (np.diff(cols["lane"].astype(np.int64)) != 0).all()
    keys = wdp_steps.keys_in_order(cols, wdp_steps.RUN_W, wdp_steps.RUN_LENS, 2, 20)
    seam = np.flatnonzero(keys[1:, 0] != keys[:-1, 0]) + 1
    assert seam.tolist() == [100] and 100 % WAVE and (keys[:, 1:] == keys[0, 1:]).all()
    # alternating classes: side by side in every wave
    cols = wdp_steps.alternating_batch("class")
    St = both(cols, wdp_steps.RUN_W, wdp_steps.RUN_LENS, 1)
    keys = wdp_steps.keys_in_order(cols, wdp_steps.RUN_W, wdp_steps.RUN_LENS, 1, 20)
    assert (np.diff(keys[:, 1]) != 0).all() and (keys[:, 2] == keys[0, 2]).all()
    assert St[0, 0] == St[0, 1] == 100


def test_group_and_lane_limit_batches():
    cols = wdp_steps.groups_batch()
    St = both(cols, wdp_steps.GROUP_W, wdp_steps.GROUP_LENS, 4)
    assert St[:, :2].all() and St[:, 2].any() and (cols["n_cigar"] > WD_T).any()
    pos = cols["pos"][cols["rid"] == 0]
    assert (np.diff(pos.astype(np.int64)) >= 0).all()  # a sorted file
    keys = wdp_steps.keys_in_order(cols, wdp_steps.GROUP_W, wdp_steps.GROUP_LENS, 4, 20)
    assert wdp_steps.run_lengths(keys).max() >= 2
    N = 256
    lens = [lane_limit.REF_LEN] * 2
    for cols in (lane_limit.sprinkled(N), lane_limit.ends(N), lane_limit.solo(N, 63), lane_limit.solo(N, 64), lane_limit.solo(N, 255)):
        St = wdp_ref.state_fast(cols, 1000, lens, N)
        assert St[:, 0].sum() > 0
    St = wdp_ref.state_fast(lane_limit.sprinkled(N), 1000, lens, N)
    assert St[63, 0] and St[64, 0] and St[255, 0] and wdp_steps.WD_ETA_LANES == 64
