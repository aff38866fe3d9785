"""CPU: the batches of tests/lane_limit.py cross the edges they are named for (no GPU use): the ballot counts of stable_slot on both
sides of every power of two, steps of the processing order with hundreds of read groups, workgroups with empty columns, all four words
of the read-group mask, and reads of read groups 63, 64 and N - 1 that every module's rule examines."""
import re
import os

import numpy as np
import pytest

from tests import cycle_steps, dup_ref, ibc_ref, rcv_ref, sac_ref, synth
from tests import lane_limit as ll

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bamqc_amd", "csrc")


def test_bits_for_on_both_sides_of_every_power_of_two():
    """lane_bits = bits_for(n_lanes - 1) in k_an_scatter_g, bits_for(n_lanes) in k_lo_scatter (keys lane + 1)"""
    assert [(ll.bits_for(N - 1), ll.bits_for(N)) for N in ll.COUNTS] == [(6, 7), (7, 7), (7, 8), (8, 8), (8, 8), (8, 9)]
    assert [ll.bits_for(v) for v in (0, 1, 2, 3, 4)] == [0, 1, 2, 2, 3]
    src = open(os.path.join(CSRC, "k_anchor.hip")).read()
    assert "bits_for(uint32_t max_key) { return max_key ? 32u - (uint32_t)__builtin_clz(max_key) : 0u; }" in src, \
        "bits_for of k_anchor.hip is no longer what tests/lane_limit.py restates"
    assert "a.lane_bits = bits_for(a.n_lanes - 1u)" in src and "nl, bits_for(nl), tmp, order)" in src


def test_the_constants_the_layouts_lean_on():
    """the 64 read groups of rc_eta's LDS copy, the 256 rows of k_dup's sums, the four mask words"""
    assert re.search(r"^#define RC_ETA_LANES\s+64\b", open(os.path.join(CSRC, "k_rcv.hip")).read(), re.M)
    assert re.search(r"^#define DP_LANES\s+256\b", open(os.path.join(CSRC, "k_dup.hip")).read(), re.M)
    assert re.search(r"lane_bits\[4\]", open(os.path.join(CSRC, "bqc_pipeline.cpp")).read() + open(os.path.join(CSRC, "bqc_ctx.h")).read() + open(os.path.join(CSRC, "gpu_batch.h")).read())


def groups_per_step(lane, step=ll.STEP):
    order = cycle_steps.processing_order(lane)
    by = np.asarray(lane)[order]
    return [len(np.unique(by[b:b + step])) for b in range(0, len(by), step)]


def test_sprinkled_256_has_a_step_with_200_groups():
    lane = ll.sprinkled(256)["lane"]
    assert max(groups_per_step(lane)) >= 200
    assert len(np.unique(lane)) >= 240
    assert max(groups_per_step(ll.one_each(256)["lane"], 256)) == 256  # (a workgroup's share of a small batch is 256 reads)


@pytest.mark.parametrize("N", ll.COUNTS)
def test_layouts(N):
    sp = ll.sprinkled(N)
    assert int(sp["lane"].max()) <= N - 1 and len(sp["flag"]) == 4 * N + 37
    assert sorted(np.unique(ll.ends(N)["lane"]).tolist()) == [0, N - 1]
    assert sorted(ll.one_each(N)["lane"].tolist()) == list(range(N))
    for g in ll.SOLO_GROUPS:
        if g < N:
            lane = ll.solo(N, g)["lane"]
            assert (lane == g).all() and np.array_equal(cycle_steps.processing_order(lane), np.arange(len(lane)))
    # runs: a 1024-read block of the stream order with fewer than N / 4 groups, and groups without a read
    lane = ll.runs(N)["lane"].astype(np.int64)
    blocks = [len(np.unique(lane[b:b + ll.STEP])) for b in range(0, len(lane), ll.STEP)]
    assert min(blocks) < N / 4, blocks
    seen = set(lane.tolist())
    missing = [g for g in range(N) if g not in seen]
    assert N // 4 <= len(missing) <= N // 3 + 1 and N - 1 in seen
    lengths = [n for _, n in ll.runs_plan(N)]
    assert len(set(lengths)) >= 8 and max(lengths) >= 300 and min(lengths) == 1


@pytest.mark.parametrize("N", ll.COUNTS)
def test_stream(N):
    batches = ll.stream(N)
    assert 5 <= len(batches) <= 7
    sizes = [len(b["flag"]) for b in batches]
    assert sizes[:4] == [1, 1023, 1024, 1025] and max(sizes) <= 20_000
    whole = synth.concat(batches)
    lane = whole["lane"].astype(np.int64)
    assert lane.max() == N - 1 and int(whole["l_seq"].max()) > 256 and int(np.median(whole["l_seq"])) == 150
    # read groups on both sides of every multiple of 64 below N, so every word of the mask that N reaches is set
    for g in ll.edge_groups(N):
        assert (lane == g).any(), g
    words = ll.lane_words(lane)
    assert all(words[w] for w in range((N + 63) // 64)) and not any(words[(N + 63) // 64:])
    # reads of more than 256 bases in read groups of 64 and above (k_long and the slow chunks)
    if N > 64:
        assert (lane[whole["l_seq"] > 256] >= 64).any()
    # positions run forward within every read group (the whole stream is in coordinate order)
    key = whole["rid"].astype(np.int64) << 32 | whole["pos"].astype(np.int64)
    assert (np.diff(key) >= 0).all()
    # batches with several read groups and batches with one
    multi = [len(np.unique(b["lane"])) > 1 for b in batches]
    assert any(multi) and not all(multi)


def test_all_four_mask_words():
    assert all(ll.lane_words(synth.concat(ll.stream(256))["lane"]))
    assert ll.lane_words(ll.solo(256, 64)["lane"]) == [0, 1, 0, 0]
    assert ll.lane_words(ll.solo(256, 63)["lane"]) == [1 << 63, 0, 0, 0]
    assert ll.lane_words(ll.solo(256, 255)["lane"]) == [0, 0, 0, 1 << 63]
    assert [w != 0 for w in ll.lane_words(ll.ends(256)["lane"])] == [True, False, False, True]


@pytest.fixture(scope="module")
def module_batches():
    return ll.module_batches()


@pytest.mark.parametrize("name", ll.MODULES)
def test_every_module_examines_reads_of_groups_63_64_and_255(module_batches, name):
    """by the module's own restatement: its table of the batches holds something of each of these read groups (and of group 200, the
    solo batch's), in the first batch alone too"""
    for batches in (module_batches, module_batches[:1]):
        rows = ll.group_rows(name, ll.module_table(name, batches, 256))
        assert rows.shape == (256,)
        for g in (63, 64, 255):
            assert rows[g], (name, g)
    assert rows.sum() >= 200  # (the sprinkled batch alone reaches most groups)


def test_the_examined_rules_that_the_restatements_state_by_name():
    """sac_ref.examined, rcv_ref.examined, dup_ref.examined and ibc_ref.examined, read by read, on the sprinkled batch"""
    cols = ll.sprinkled(256)
    lane = cols["lane"].astype(np.int64)
    ok = {"sac": sac_ref.examined(cols, 256, 2, 20), "rcv": rcv_ref.examined(cols, 256, 2, 20),
          "dup": np.array([dup_ref.examined(int(cols["flag"][i]), int(cols["l_seq"][i]), int(cols["n_cigar"][i]), int(cols["rid"][i]), int(lane[i]), 256, 2)
                           for i in range(len(lane))]),
          "ibc": np.array([ibc_ref.examined(int(cols["flag"][i]), int(lane[i]), int(cols["l_seq"][i]), int(cols["n_cigar"][i]), 256) for i in range(len(lane))])}
    for name, m in ok.items():
        for g in (63, 64, 255):
            assert (m & (lane == g)).any(), (name, g)
        assert (m >= ll.clean(cols)).all(), name  # (a clean read is examined by every one of them)


def test_module_lists():
    rid, pos = ll.sites()
    sac_ref.check_sites(rid, pos, 2)
    rcv_ref.layout(ll.regions(), 2, 256)
    ln = ll.regions()[2] - ll.regions()[1]
    assert ln.min() == 1 and ln.max() == 400
