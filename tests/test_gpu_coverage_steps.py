"""GPU: the coverage depth histogram at the seams of its three pieces — the host's CovPlanner (tiles of 4 windows, read ranges), the
interval code of k_prep.hip (prep_walk's emit; k_pend_cov / pend_interval for a shard's set-aside reads) and k_cov (LDS difference
array, two prefetched entries per thread and a loop over the rest, read-group filter, common and boundary tiles, carry-in and
carry-out, the per-read-group LDS histogram of a persistent workgroup) — on the hand-built batches of tests/cov_steps.py, each named
for its edge (tests/test_coverage_steps_cpu.py proves that it crosses it).

Every case through the host's pass (bqc_submit) against the oracle with the whole count set and against the restatement
tests/cov_ref.py for the histogram of every read group; some also through the card-anchored path (the same exported state vector
word for word as the host's pass) and as the tail of a shard (PendRun / PendExtra / k_pend_cov).  Integer counts, exact."""
import ctypes as C

import numpy as np
import pytest

from bamqc_amd import Aggregator, _abi, _lib
from tests import cov_steps as cs
from tests.anchor_recurrence import NO_WIN, per_group_anchors
from tests.hipmem import Hip
from tests.parity import assert_parity
from tests.test_gpu_anchor import device_batch
from tests.test_gpu_anchor_shard_read_groups import run_shard

pytestmark = pytest.mark.gpu


def assert_poscov(name, counts):
    exp = cs.expected(name)
    for l in range(cs.get(name).n_lanes):
        got, want = counts[l]["poscov"], exp.poscov[l]
        assert np.array_equal(got, want), "%s, read group %d: bins %s: got %s, want %s" % (
            name, l, np.flatnonzero(got != want)[:10], got[got != want][:10], want[got != want][:10])


@pytest.mark.parametrize("name", list(cs.CASES))
def test_host_pass_equals_the_oracle_and_the_restatement(name):
    c = cs.get(name)
    _, got, _, agg = assert_parity(c.batches, cs.refs_of(c.n_refs), n_refs=c.n_refs, n_lanes=c.n_lanes, **c.opts)
    agg.close()
    assert_poscov(name, got)


@pytest.mark.parametrize("name", cs.ANCHORED)
def test_card_anchored_path_equals_the_host_pass_word_for_word(name):
    """every batch anchored on the card (bqc_anchor_enqueue / bqc_anchor_complete, the anchors checked read by read against the
    recurrence) and submitted with bqc_submit_anchored; a second context gets the batches through bqc_submit"""
    c = cs.get(name)
    lib = _lib.load()
    refs = cs.refs_of(c.n_refs)
    hip = Hip()
    dev = Aggregator(n_refs=c.n_refs, n_lanes=c.n_lanes, **c.opts)
    host = Aggregator(n_refs=c.n_refs, n_lanes=c.n_lanes, **c.opts)
    try:
        for i, r in enumerate(refs):
            dev.set_reference(i, r)
            host.set_reference(i, r)
        states = [(True, 0, 0, 0)] * c.n_lanes
        for cols in c.batches:
            b, d_cov = device_batch(hip, cols)
            h = C.c_void_p()
            assert lib.bqc_anchor_enqueue(dev.h, C.byref(b), d_cov, None, C.byref(h)) == 0, (lib.bqc_anchor_error(dev.h) or b"").decode()
            assert hip.rt.hipDeviceSynchronize() == 0
            assert lib.bqc_anchor_complete(dev.h, h, None) == 0, (lib.bqc_anchor_error(dev.h) or b"").decode()
            cov = hip.get(d_cov, 8 * len(cols["flag"]), np.uint32).reshape(-1, 2)
            win, off, states = per_group_anchors(cols, states, c.n_lanes, c.n_refs)
            assert np.array_equal(cov[:, 0].astype(np.uint64), win), np.flatnonzero(cov[:, 0].astype(np.uint64) != win)[:10]
            cand = win != NO_WIN
            assert np.array_equal(cov[cand, 1], off[cand]), np.flatnonzero(cov[cand, 1] != off[cand])[:10]
            assert lib.bqc_submit_anchored(dev.h, C.byref(b), h, None) == 0, (lib.bqc_last_error(dev.h) or b"").decode()
            dev.sync()  # (the columns' device buffers are released after the test: the batch must be through)
            host.submit(cols)
        v_dev, v_host = dev.state_export_host(), host.state_export_host()
        assert np.array_equal(v_dev, v_host), np.flatnonzero(v_dev != v_host)[:10]
        got = dev.finalize()
        assert not _abi.diff_counts(host.finalize(), got)
        assert_poscov(name, got)
    finally:
        dev.close()
        host.close()
        hip.free()


@pytest.mark.parametrize("name", cs.SHARD_TAILS)
def test_shard_tail_takes_the_pending_route_to_the_same_counts(name):
    """the case's first batch as the head of the stream, the rest as the tail of a shard (run_shard: anchored on the card and through
    the host's pass, resolved from the head's state, the whole against the oracle): every candidate of the tail is set aside, its
    intervals come from PendRun / PendExtra through k_pend_cov"""
    c = cs.get(name)
    assert c.opts == {}
    head, tail = c.batches[:c.head], c.batches[c.head:]
    set_aside, pending = run_shard(head, tail, cs.refs_of(c.n_refs), c.n_lanes)
    entering = np.zeros(c.n_lanes, np.int64)
    for reads in cs.expected(name).reads[c.head:]:
        entering += np.bincount([r.lane for r in reads], minlength=c.n_lanes)
    assert np.array_equal(set_aside, entering) and all(pending), (set_aside, entering, pending)
