"""GPU: a shard that starts inside the stream (bqc_options.shard_tail) with SEVERAL read groups anchors its batches on the card
(csrc/k_anchor.hip, the several-read-groups instances; include/bamqc.h: bqc_anchor_*): every read group's reads are set aside there up
to the group's own first certain reset, exactly as the host's pass sets them aside per read group.  Against a restatement of the rule
one read at a time (tests/anchor_set_aside.py), against the host's pass on the same batches (bqc_submit: the exported state vector
word for word) and against the oracle on the whole stream; then the program with --gpus 2 and 3 on a file with three read groups."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bamqc_amd import Aggregator, _abi, _lib, hostio, synth
from tests.anchor_recurrence import NO_WIN
from tests.anchor_set_aside import count_breaks, enters_coverage, fresh_group_states, per_group_set_aside
from tests.cli_oracle import oracle_bamqualcheck
from tests.hipmem import Hip
from tests.parity import run_oracle, split
from tests.test_gpu_anchor import device_batch
from tests.test_gpu_anchor_read_groups import with_lanes_positions
from tests.test_gpu_sharded import EXE, run_ranks, same

pytestmark = pytest.mark.gpu

PENDING = 0xFFFFFFFE   # BQC_COV_PENDING
AN_MAX_BREAKS = 16_384  # csrc/anchor.h
LENS = [2_000_000, 1_000_000]


def ctx(refs, n_lanes, **opts):
    a = Aggregator(n_refs=len(refs), n_lanes=n_lanes, **opts)
    for i, r in enumerate(refs):
        a.set_reference(i, r)
    return a


def anchor_err(lib, agg):
    return (lib.bqc_anchor_error(agg.h) or b"").decode()


def check_anchors(cols, cov, aside, win, off, n_lanes):
    """the anchors the card wrote for one batch against the restatement: BQC_COV_PENDING exactly for the reads set aside, their log
    indices a permutation of 0 .. n_pending - 1 that ascends inside a read group; the others {window, offset}"""
    got_aside = cov[:, 0] == PENDING
    assert np.array_equal(got_aside, aside), np.flatnonzero(got_aside != aside)[:10]
    idx = cov[aside, 1].astype(np.int64)
    assert np.array_equal(np.sort(idx), np.arange(len(idx))), (len(idx), np.sort(idx)[:10])
    lane = np.asarray(cols["lane"])[aside]
    for g in range(n_lanes):
        assert np.all(np.diff(idx[lane == g]) > 0), g
    rest = ~aside
    got = cov[rest, 0].astype(np.uint64)
    assert np.array_equal(got, win[rest]), np.flatnonzero(got != win[rest])[:10]
    cand = rest & (win != NO_WIN)
    assert np.array_equal(cov[cand, 1], off[cand]), np.flatnonzero(cov[cand, 1] != off[cand])[:10]


def run_shard(head, tail, refs, n_lanes, leaves_at=None):
    """head through bqc_submit of a plain context; tail through a shard_tail context, every batch anchored on the card and checked read
    by read (from batch `leaves_at` on: bqc_anchor_complete says 1 for that one, bqc_anchor_enqueue says 1 for the rest, and they go
    through bqc_submit), and through a second shard_tail context by bqc_submit alone (the host's pass).  Both resolved from the head's
    exported state: the same state vector word for word, and head + tail finalize to the oracle's counts for the whole stream.
    Returns (reads set aside per read group, groups still pending at the end of the shard), by the restatement."""
    lib = _lib.load()
    n_refs = len(refs)
    rc, want, _ = run_oracle(head + tail, refs, n_refs=n_refs, n_lanes=n_lanes)
    assert rc == 0
    hip = Hip()
    pred, card, host, total = ctx(refs, n_lanes), ctx(refs, n_lanes, shard_tail=1), ctx(refs, n_lanes, shard_tail=1), ctx(refs, n_lanes)
    try:
        for c in head:
            pred.submit(c)
        states = fresh_group_states(n_lanes)
        set_aside = np.zeros(n_lanes, np.int64)
        for k, c in enumerate(tail):
            assert count_breaks(c, n_lanes, n_refs) <= AN_MAX_BREAKS or k == leaves_at, k  # (a condition on the input, not on the card)
            pending_before = [s["pending"] for s in states]
            aside, win, off, states = per_group_set_aside(c, states, n_lanes, n_refs)
            set_aside += np.bincount(np.asarray(c["lane"])[aside], minlength=n_lanes)[:n_lanes]
            b, d_cov = device_batch(hip, c)
            h = C.c_void_p()
            rc = lib.bqc_anchor_enqueue(card.h, C.byref(b), d_cov, None, C.byref(h))
            if leaves_at is not None and k > leaves_at:
                assert rc == 1, (k, rc)
                card.submit(c)
                continue
            assert rc == 0, (k, rc, anchor_err(lib, card))
            assert hip.rt.hipDeviceSynchronize() == 0
            rc = lib.bqc_anchor_complete(card.h, h, None)
            if k == leaves_at:
                assert any(pending_before), k  # (the card is left in the middle of the pending phase)
                assert count_breaks(c, n_lanes, n_refs) > AN_MAX_BREAKS
                assert rc == 1, (k, rc, anchor_err(lib, card))
                card.submit(c)  # no group's state has moved: the host's pass sets aside from where the batch before left every group
                continue
            assert rc == 0, (k, rc, anchor_err(lib, card))
            cov = hip.get(d_cov, 8 * len(c["flag"]), np.uint32).reshape(-1, 2)
            check_anchors(c, cov, aside, win, off, n_lanes)
            assert lib.bqc_submit_anchored(card.h, C.byref(b), h, None) == 0, (lib.bqc_last_error(card.h) or b"").decode()
            card.sync()  # (the columns' device buffers are released after the test: the batch must be through)
        for c in tail:
            host.submit(c)
        buf = np.zeros(int(lib.bqc_shard_state_bytes(pred.h)), np.uint8)
        assert lib.bqc_shard_export(pred.h, buf.ctypes.data_as(C.c_void_p)) == 0, (lib.bqc_last_error(pred.h) or b"").decode()
        for a in (card, host):
            assert lib.bqc_shard_resolve(a.h, buf.ctypes.data_as(C.c_void_p)) == 0, (lib.bqc_last_error(a.h) or b"").decode()
        v_card, v_host = card.state_export_host(), host.state_export_host()
        assert np.array_equal(v_card, v_host), np.flatnonzero(v_card != v_host)[:10]
        total.state_import_host(pred.state_export_host() + v_card)
        d = _abi.diff_counts(want, total.finalize())
        assert not d, "\n".join(d[:20])
        return set_aside, [s["pending"] for s in states]
    finally:
        for a in (pred, card, host, total):
            a.close()
        hip.free()


def stream(n_lanes, lanes_made=None):
    """60 000 reads over two contigs; head = the first 30 000, the tail's four batches: two on the first contig, one across the contigs'
    border, one on the second"""
    refs = [synth.reference(37, i, n) for i, n in enumerate(LENS)]
    cols = synth.batch(37, 60_000, LENS, refs, n_lanes=lanes_made or n_lanes)
    c1 = int(np.searchsorted(cols["rid"], 1))
    assert c1 == 40_000
    parts = split(cols, [12_000, 30_000, 33_000, c1 + 500, 52_000])
    return parts[:2], parts[2:], refs


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_lanes", [3, 12])
def test_shard_with_several_read_groups_sets_aside_on_the_card(n_lanes):
    """Every tail batch of a shard_tail context with 3 / 12 read groups is anchored on the card (bqc_anchor_enqueue says 0).  By the
    restatement: 3 groups — 3236 / 3321 / 3175 reads set aside (every read of the tail on the first contig: the data has no gap
    above 2000 there), at most 10 breaks per batch; 12 groups — 1 .. 55 reads set aside per group (a group's reads lie 12 times
    further apart: the groups leave the pending state at different reads of the first contig), at most 2118 breaks per batch."""
    head, tail, refs = stream(n_lanes)
    set_aside, pending = run_shard(head, tail, refs, n_lanes)
    assert np.all(set_aside > 0), set_aside  # every group has reads set aside
    assert not any(pending)
    if n_lanes == 12:
        assert len(set(set_aside.tolist())) > 6 and set_aside.max() < 200, set_aside  # (they left at different reads, early)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. groups that do not behave alike
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_group_that_stays_pending_to_the_end_of_the_shard():
    """group 2's reads on the second contig relabelled to group 0: every candidate of group 2 in the tail is set aside, and resolve
    continues it from the state that came in (no trajectory of its own)"""
    head, tail, refs = stream(3)
    tail = [with_lanes_positions(c, lane=np.where((c["rid"] == 1) & (c["lane"] == 2), 0, c["lane"])) for c in tail]
    n2 = sum(sum(1 for i in np.flatnonzero(c["lane"] == 2) if enters_coverage(c, i, 3, 2)) for c in tail)
    set_aside, pending = run_shard(head, tail, refs, 3)
    assert pending == [False, False, True]
    assert set_aside[2] == n2 > 1000, (set_aside, n2)


def test_a_group_absent_from_the_shard():
    head, tail, refs = stream(3)
    tail = [with_lanes_positions(c, lane=np.where(c["lane"] == 1, 0, c["lane"])) for c in tail]
    set_aside, pending = run_shard(head, tail, refs, 3)
    assert pending == [False, True, False] and set_aside[1] == 0 and set_aside[0] > 0 and set_aside[2] > 0, (pending, set_aside)


def test_a_group_that_first_appears_in_the_shards_last_batch():
    head, tail, refs = stream(4, lanes_made=3)
    last = tail[-1]
    tail[-1] = with_lanes_positions(last, lane=np.where(np.arange(len(last["flag"])) % 5 == 0, 3, last["lane"]))
    set_aside, pending = run_shard(head, tail, refs, 4)
    assert set_aside[3] > 100 and pending[3] and not any(pending[:3]), (set_aside, pending)


def test_a_pending_group_with_reads_in_front_of_their_predecessor():
    """group 1, while pending: a read 300 positions in front of the group's read before it (the difference wraps to just below 2^32:
    no certain reset, the read is set aside), later one 5000 in front (wraps too, but by more than 2000: a certain reset — group 1 leaves
    the pending state there, in the middle of the first contig and of a batch, the others at the second contig)"""
    head, tail, refs = stream(3)
    c = tail[0]
    k1 = [int(i) for i in np.flatnonzero(c["lane"] == 1) if enters_coverage(c, i, 3, 2)]
    pos = np.array(c["pos"], np.int64)
    pos[k1[40]] = pos[k1[39]] - 300
    pos[k1[200]] = pos[k1[199]] - 5000
    assert pos[k1[200]] >= 0
    tail[0] = with_lanes_positions(c, pos=pos)
    set_aside, pending = run_shard(head, tail, refs, 3)
    assert set_aside[1] == 200 and set_aside[0] > 1000 and set_aside[2] > 1000 and not any(pending), (set_aside, pending)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. leaving the card in the middle of the pending phase
# ---------------------------------------------------------------------------------------------------------------------------------
def test_too_many_breaks_while_groups_are_pending():
    """The tail's second batch has 20 000 reads of group 2 that lie 1200 apart (2400 where a record in between does not enter
    coverage(): group 2 leaves the pending state early in that batch): more breaks than the card's chain takes, while groups 0 and 1,
    dense, stay pending through the whole batch.  bqc_anchor_complete says 1; that batch and the rest go through bqc_submit, whose
    pass finds every group's set-aside state where the first (anchored) batch left it."""
    lens = [30_000_000]
    refs = [synth.reference(14, 0, lens[0])]
    rng = np.random.default_rng(4)
    dense_at = lambda cols, lo, span: with_lanes_positions(cols, pos=np.sort(rng.integers(lo, lo + span, size=len(cols["flag"]))))
    head = [dense_at(synth.batch(14, 40_000, lens, refs, n_lanes=3), 0, 2_000_000)]
    first = dense_at(synth.batch(17, 6_000, lens, refs, n_lanes=3), 2_000_000, 300_000)
    base = synth.batch(15, 60_000, lens, refs, n_lanes=1)
    n = len(base["flag"])
    lane = np.where(np.arange(n) % 3 == 2, 2, np.arange(n) % 2).astype(np.uint8)
    pos = np.sort(rng.integers(2_300_000, 4_300_000, size=n))
    k2 = np.flatnonzero(lane == 2)
    pos[k2] = np.arange(len(k2)) * 1200 + 2_300_007
    sparse = with_lanes_positions(base, lane=lane, pos=pos)
    after = dense_at(synth.batch(16, 30_000, lens, refs, n_lanes=3), 27_000_000, 2_000_000)
    set_aside, pending = run_shard(head, [first, sparse, after], refs, 3, leaves_at=1)
    assert set_aside[0] > 20_000 and set_aside[1] > 20_000 and set_aside[2] >= 1_000 and not any(pending), (set_aside, pending)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the program
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,batch", [(2, "1000000"), (3, "20011")])
def test_three_read_group_shards_set_aside_on_the_card(tmp_path, world, batch):
    """THREE read groups and the reader on the card: every worker's coverage anchors are made on the card, also those of the workers
    that start inside the stream.  Same bytes as the single-process run, the host's pass (BQC_DEVICE_ANCHORS=0) and the oracle
    program."""
    import subprocess
    bam, fa = str(tmp_path / "rg3.bam"), str(tmp_path / "rg3.fa")
    hostio.synth_write(bam, fa, seed=78, n_reads=250_000, ref_names=["chr1", "chr2", "chrM"], ref_lens=[2_000_000, 400_000, 20_000], n_lanes=3)
    single = str(tmp_path / "single.bamqc")
    r = subprocess.run([EXE, "-r", fa, "-o", single, "-c", "chr1,chr2", bam], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, BQC_GPU_DECODE="1", BQC_TIMING="1"))
    assert r.returncode == 0, r.stderr
    want = str(tmp_path / "oracle.bamqc")
    assert oracle_bamqualcheck(bam, fa, want, chroms="chr1,chr2") == 0
    assert same(want, single)
    seen = {}
    for anchors in ("1", "0"):
        out = str(tmp_path / ("sharded_%s.bamqc" % anchors))
        rcs, outs = run_ranks(world, ["-r", fa, "-o", out, "-c", "chr1,chr2", "--batch-reads", batch, bam],
                              env_extra={"BQC_GPU_DECODE": "1", "BQC_TIMING": "1", "BQC_DEVICE_ANCHORS": anchors}, launcher="cxx")
        assert rcs == [0] * world, outs
        assert same(single, out)
        seen[anchors] = [int(x) for x in re.findall(r"\[timing\] (\d+) batches anchored on the card", outs[0])]
    assert len(seen["1"]) == world and all(k > 0 for k in seen["1"]), seen  # every worker, those inside the stream too
    assert len(seen["0"]) == world and all(k == 0 for k in seen["0"]), seen
