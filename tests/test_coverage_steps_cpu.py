"""CPU: what the coverage depth tests on the card stand on (tests/test_gpu_coverage_steps.py).

1. The restatement tests/cov_ref.py equals the oracle's genome coverage histogram on every batch of tests/cov_steps.py and on two
   random streams: the GPU test may trust it as far as this goes.
2. Every batch of cov_steps crosses the edge it is named for, by the restatement's model of the plan (CovPlanner::finish): conditions
   on the inputs, checked here so that a GPU test cannot pass on a batch that misses its edge.
3. The constants the batches are built around are the kernels' (#define lines and the launcher's literals)."""
import os
import re

import numpy as np
import pytest

from tests import cov_ref, cov_steps as cs, synth
from tests.parity import run_oracle, split

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bamqc_amd", "csrc")


def oracle_poscov(c, batches=None):
    rc, want, _ = run_oracle(batches or c.batches, cs.refs_of(c.n_refs), n_refs=c.n_refs, n_lanes=c.n_lanes, **c.opts)
    assert rc == 0
    return np.stack([want[l]["poscov"] for l in range(c.n_lanes)])


def all_tiles(exp):
    return [t for tiles in exp.tiles for t in tiles]


def zero_complete_windows(exp, lane=0):
    """complete windows (flushed before the end of the stream) in which no position is covered"""
    return [w for w in range(exp.last[lane]) if not exp.window_depth(lane, w).any()]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the restatement is the oracle's
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cs.CASES))
def test_restatement_equals_the_oracle_on_every_directed_batch(name):
    c, exp = cs.get(name), cs.expected(name)
    got = oracle_poscov(c)
    assert np.array_equal(exp.poscov, got), [(l, np.flatnonzero(exp.poscov[l] != got[l])[:10]) for l in range(c.n_lanes)]
    assert all(int(exp.poscov[l].sum()) == (exp.last[l] + 2) * cov_ref.VSIZE for l in range(c.n_lanes))  # every window once


@pytest.mark.parametrize("kind", ["dense", "sparse three groups"])
def test_restatement_equals_the_oracle_on_random_streams(kind):
    if kind == "dense":  # ~150-fold depth: the clamp, slides only
        cols, refs = synth.synth(seed=31, n_reads=3000, n_refs=1, ref_len=4000, p_clip=0.3, p_indel=0.3, hardclip=True)
        n_lanes, batches = 1, [cols]
    else:  # resets, three read groups, two contigs, long CIGARs with N, three batches
        cols, refs = synth.synth(seed=32, n_reads=1500, n_refs=2, ref_len=400_000, n_lanes=3, long_cigar=True, p_clip=0.3)
        n_lanes, batches = 3, split(cols, [400, 1100])
    exp = cov_ref.coverage(batches, n_lanes, len(refs))
    rc, want, _ = run_oracle(batches, refs, n_refs=len(refs), n_lanes=n_lanes)
    assert rc == 0
    for l in range(n_lanes):
        assert np.array_equal(exp.poscov[l], want[l]["poscov"]), (l, np.flatnonzero(exp.poscov[l] != want[l]["poscov"])[:10])
    if kind == "dense":
        assert exp.poscov[0][cov_ref.COVSIZE] > 0
    else:
        assert len(exp.tiles) == 3 and all(r > 10 for r in exp.last)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. every batch crosses its edge
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", cs.CLAMP_K)
def test_clamp_stacks_sit_where_they_claim_and_count_as_computed_by_hand(K):
    exp = cs.expected("clamp_%d" % K)
    assert np.array_equal(exp.poscov[0], cs.clamp_by_hand(K))
    assert int(exp.poscov[0][99]) == (150 if K == 99 else 0) and int(exp.poscov[0][100]) == (150 if K >= 100 else 0)
    [tiles] = exp.tiles
    for where, w in cs.CLAMP_STACK_WINDOWS.items():
        d = exp.window_depth(0, w)
        assert int(d.max()) == K and int((d == K).sum()) == 50, where
        [t] = [t for t in tiles if t["win_lo"] <= w < t["win_lo"] + cov_ref.TILE_WINDOWS]
        assert t["common"] == (where == "common"), (where, t)
    assert exp.last[0] == cs.CLAMP_STACK_WINDOWS["live at the end"]  # that stack is histogrammed by the flush at the end of the stream
    common = [t for t in tiles if t["common"]]
    assert tiles[-1]["win_lo"] >= common[0]["win_lo"] + 2 * cov_ref.TILE_WINDOWS  # the reads go on two tiles beyond the common one


def test_clamp_split_reaches_101_only_with_the_carry():
    exp = cs.expected("clamp_split")
    per_batch = [sum(1 for r in reads if r.win == 0 and r.off == 200) for reads in exp.reads]
    assert per_batch == [60, 41]
    assert int(exp.window_depth(0, 0).max()) == 101 and int(exp.poscov[0][100]) == 50 and int(exp.poscov[0][99]) == 0


def test_thresholds_batch_sits_on_every_threshold():
    exp = cs.expected("thresholds")
    [reads] = exp.reads
    offs = {r.off for r in reads}
    assert {0, 1, 999, 1000, 2000} <= offs and 1001 not in offs and 1999 not in offs and 2001 not in offs
    ends = {(r.off, hi) for r in reads for lo, hi in r.runs}
    for off in (0, 999, 1000):
        assert {(off, 1999), (off, 2000), (off, 2001)} <= ends, off
    at_2000 = [r for r in reads if r.off == 2000]
    assert len(at_2000) == 2 and all(r.runs and r.covered == 0 for r in at_2000)  # a read at p = 2000 covers nothing
    assert any(r.runs == [(0, 2500)] and r.covered == 2000 for r in reads)
    assert any(r.runs == [(10, 2710)] and r.covered == 1990 for r in reads)  # 100M 2500D 100M: one run
    wins = [r.win for r in reads]
    steps = set(np.diff(wins).tolist())
    assert steps == {0, 1, 2}  # stays, slides and resets


def test_seams_batch_crosses_every_tile_seam():
    exp = cs.expected("seams")
    r1, r2 = exp.reads
    t1, t2 = exp.tiles
    T = cov_ref.TILE_WINDOWS
    # a read whose first window is a tile's last and that covers up to the cut at 2000
    assert [r for r in r1 if r.win == 3 and r.counted == [(500, 2000)]]
    assert [r for r in r1 if r.win == 7 and r.runs == [(500, 3120)] and r.counted == [(500, 2000)]]
    assert [r for r in r1 if r.win == 7 and r.counted == [(1000, 1300)]]  # covers window 8 only
    # tile 1's read range begins at the read of window 3, which is not a read of the tile's own windows
    tile1 = [t for t in t1 if t["win_lo"] == T][0]
    first = [r for r in r1 if r.index == tile1["list_begin"]][0]
    assert first.win == T - 1 and [r for r in r1 if r.win == T][0].index > first.index
    # a tile that receives only spill: no read of batch 1 has a first window in tile 2, yet windows 8 holds depth
    tile2 = [t for t in t1 if t["win_lo"] == 2 * T][0]
    assert not [r for r in r1 if r.win >= 2 * T] and not tile2["common"] and exp.window_depth(0, 2 * T).any()
    # batch 2: numbered from window 7; resets across tile edges leave complete windows nobody covers
    assert [r.rel for r in r2][:5] == [0, 2, 4, 6, 8] and r2[0].win == 7
    zero = zero_complete_windows(exp)
    assert {7 + 3, 7 + 7} <= set(zero)  # the last windows of relative tiles 0 and 1
    assert [r for r in r2 if r.rel == 8 and r.counted == [(900, 1100)]]
    assert int(exp.window_depth(0, 7).max()) == 2  # batch 2's first read over carried-in depth


def test_no_batch_has_a_complete_window_outside_every_tile():
    """A reset advances the window index by 2 and a slide by 1, and the planner gives every read's window and the one behind it a
    tile: no window below the last one is ever outside every tile.  The host-side add for "complete windows nobody touched" is
    therefore 0 for every batch here — and for any batch."""
    for name in cs.CASES:
        exp = cs.expected(name)
        assert all(v == 0 for u in exp.untouched for v in u.values()), name


@pytest.mark.parametrize("n_lanes", [1, 2])
@pytest.mark.parametrize("N", cs.RANGE_N)
def test_read_range_lengths_are_exact(N, n_lanes):
    c = cs.get("range_%d_%s" % (N, "one_group" if n_lanes == 1 else "two_groups"))
    exp = cs.expected("range_%d_%s" % (N, "one_group" if n_lanes == 1 else "two_groups"))
    [tiles], [reads] = exp.tiles, exp.reads
    [t] = [t for t in tiles if t["lane"] == 0 and t["win_lo"] == cov_ref.TILE_WINDOWS]
    assert t["length"] == N and t["common"] and t["mixed"] == (n_lanes == 2)
    if n_lanes == 2:  # the range holds reads of the other group that cover positions of the tile's windows (same window numbers)
        lanes = np.asarray(c.batches[0]["lane"])[t["list_begin"]:t["list_end"]]
        assert (lanes == 1).sum() >= N // 2 - 3
        other = [r for r in reads if r.lane == 1 and t["list_begin"] <= r.index < t["list_end"] and r.rel == cov_ref.TILE_WINDOWS and r.covered]
        assert len(other) >= N // 2 - 3
        assert not np.array_equal(exp.poscov[0], exp.poscov[1])


def test_two_groups_share_window_numbers_with_different_depths_and_one_sided_extras():
    c, exp = cs.get("same_coordinates"), cs.expected("same_coordinates")
    reads = [r for b in exp.reads for r in b]
    assert {r.win for r in reads if r.lane == 0} == {r.win for r in reads if r.lane == 1} == set(range(7))
    assert all(len(r.counted) == 1 for r in reads if r.lane == 0)
    assert sum(len(r.counted) - 1 for r in reads if r.lane == 1) == sum(exp.n_extra) == 2 * 13
    assert exp.n_extra[1] == 24 and all(t["mixed"] for t in exp.tiles[1])
    assert not np.array_equal(exp.poscov[0], exp.poscov[1])
    for w in range(1, 7):
        assert not np.array_equal(exp.window_depth(0, w), exp.window_depth(1, w))


def test_many_tiles_exceed_the_grid_in_both_groups():
    exp = cs.expected("many_tiles")
    [tiles] = exp.tiles
    assert len(tiles) >= cs.K_COV_GRID + 1
    per_group = [sum(1 for t in tiles if t["lane"] == l) for l in (0, 1)]
    assert min(per_group) >= 1200, per_group
    switching = [i for i in range(len(tiles) - cs.K_COV_GRID) if tiles[i]["lane"] != tiles[i + cs.K_COV_GRID]["lane"]]
    assert len(switching) > 400  # workgroups whose second tile is another read group's: the LDS histogram is flushed inside the loop
    assert {tiles[i + cs.K_COV_GRID]["lane"] for i in switching} == {1} and {tiles[i]["lane"] for i in switching} == {0}
    assert [tiles[i]["lane"] for i in range(len(tiles))] == sorted(tiles[i]["lane"] for i in range(len(tiles)))
    cols = cs.get("many_tiles").batches[0]
    assert len(cols["flag"]) <= 16_384  # (at most one position break per read: the card-anchored path takes the batch)


def test_carry_streams():
    for name, whole in (("clamp_101_read_by_read", "clamp_101"), ("thresholds_read_by_read", "thresholds"), ("seams_read_by_read", "seams")):
        c = cs.get(name)
        assert all(len(b["flag"]) == 1 for b in c.batches) and len(c.batches) < 400, name
        assert np.array_equal(cs.expected(name).poscov, cs.expected(whole).poscov), name
    c, exp = cs.get("absent_group"), cs.expected("absent_group")
    assert [sorted(set(b["lane"].tolist())) for b in c.batches] == [[0], [1], [0, 1]]
    assert not [t for t in exp.tiles[1] if t["lane"] == 0]  # batch 2 owns no tile of group 0
    before = sum(r.covered for r in exp.reads[0])
    assert exp.reads[2][0].lane == 0 and exp.reads[2][0].rel == 0 and before > 0  # batch 3 goes on inside group 0's live windows
    assert exp.window_depth(0, 0).max() >= 3 and exp.window_depth(0, 1).any()
    c, exp = cs.get("unmapped_between"), cs.expected("unmapped_between")
    assert exp.reads[1] == [] and exp.tiles[1] == [] and len(c.batches[1]["flag"]) == 5
    assert exp.reads[2][0].rel == 0 and exp.window_depth(0, 0).max() >= 3 and exp.window_depth(0, 1).any()


def test_clipped_batches():
    exp = cs.expected("clipped")
    body = exp.reads[1]
    assert len(body) == 4 * len(cs.CLIPPED) and {r.off for r in body} == {500, 1000}
    ops = cov_ref.read_ops(cs.get("clipped").batches[1])
    rev = (np.asarray(cs.get("clipped").batches[1]["flag"]) & 0x10) != 0
    for k in range(len(cs.CLIPPED)):  # each CIGAR on both strands at both offsets
        four = body[4 * k:4 * k + 4]
        assert all(ops[r.index] == [tuple(o) for o in cs.CLIPPED[k]] for r in four)
        assert sorted((r.off, bool(rev[r.index])) for r in four) == [(500, False), (500, True), (1000, False), (1000, True)]
    runs_of = lambda k, off, strand: [r for r in body[4 * k:4 * k + 4] if r.off == off and bool(rev[r.index]) == strand][0].runs
    assert runs_of(0, 500, False) == [(510, 600)] and runs_of(0, 500, True) == [(500, 590)]   # the leading clip shifts the interval
    assert len(runs_of(1, 1000, False)) == 4                                                  # three extras
    assert runs_of(2, 500, False) == [(505, 555), (575, 605)] and runs_of(2, 500, True) == [(500, 530), (550, 600)]
    assert runs_of(3, 500, False) == [(500, 660)]                                             # M D M: one run
    for k in range(5, 11):                                                                    # = X N I P H
        assert runs_of(k, 1000, True) == [(1000, 1060)]
    every = [run for r in body for run in r.runs]
    assert [1 for lo, hi in every if lo < 2000 < hi] and [1 for lo, hi in every if lo == 2000] and [1 for lo, hi in every if lo > 2000]
    assert [r for r in body if len(r.runs) == 2 and r.runs[0][1] < 2000 and r.runs[1][0] < 2000 < r.runs[1][1]]  # a SECOND run crosses
    assert exp.n_extra[1] > 40
    exp = cs.expected("extras_200")
    c = cs.get("extras_200")
    assert exp.n_extra == [0, 200, 0] and len(c.batches[1]["flag"]) == 1
    assert len(c.batches[1]["cigar"]) // 2 + 1 == 201  # the capacity of cov_extra[] for that batch
    exp = cs.expected("all_clipped")
    c = cs.get("all_clipped")
    assert exp.n_extra[1] == len(c.batches[1]["flag"]) == 600 and all(o == [(1, "M"), (1, "S"), (1, "M")] for o in cov_ref.read_ops(c.batches[1]))


def test_shard_tails_have_no_certain_reset():
    """the cases that run as a shard's tail: the head leaves live windows, and no read of the tail is more than 2000 behind the
    read before it of its read group — every candidate is set aside and takes the pending route"""
    for name in cs.SHARD_TAILS:
        c, exp = cs.get(name), cs.expected(name)
        assert all(exp.reads[k] for k in range(c.head)), name
        for l in range(c.n_lanes):
            pos = np.concatenate([np.asarray(b["pos"])[np.asarray(b["lane"]) == l] for b in c.batches])
            assert len(pos) > 1 and np.all(np.abs(np.diff(pos)) <= 2000), (name, l)
        assert all(len(set(b["rid"].tolist())) == 1 for b in c.batches)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the kernels' constants
# ---------------------------------------------------------------------------------------------------------------------------
def test_constants_are_the_kernels():
    text = lambda name: open(os.path.join(CSRC, name)).read()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(CSRC)), "include", "bamqc.h")).read() + text("device_types.h")
    define = lambda name: int(re.search(r"#define\s+%s\s+\(?(\d+)" % name, hdr).group(1))
    assert define("BQC_VSIZE") == cov_ref.VSIZE and define("BQC_COVSIZE") == cov_ref.COVSIZE
    assert define("BQC_COV_TILE_WINDOWS") == cov_ref.TILE_WINDOWS
    cov = text("k_cov.hip")
    assert re.search(r"b\.n_cov_tiles < %du \? b\.n_cov_tiles : %du" % (cs.K_COV_GRID, cs.K_COV_GRID), cov)
    assert "dim3(grid), dim3(256)" in cov and "2 * blockDim.x" in cov  # two prefetched entries per thread of 256: 512
    assert "cx_cap = H.cigar_words / 2 + 1" in text("bqc_pipeline.cpp")
